"""DC optimal power flow without a device: the model rows against the dense restatement, the restatement against MATPOWER's goldens and the KKT
certificate, K from the library's term lists against the dense formula, the loader's new fields.

Measured here (tests/dcopf_reference.py, rho = 0.1 adapted and rho = 1, tolerance 1e-9, the worse of the two):
  case14test   angles 9.4e-9, outputs 3.4e-8 from the goldens; certificate: bound 3.5e-6, stationarity 7.1e-6, complementarity 7.6e-5
  case30test   angles 2.3e-8, outputs 6.0e-8;                  certificate: bound 6.5e-8, stationarity 1.8e-6, complementarity 1.7e-5
               over the 130 scaled-demand lanes of the device tests: 8.0e-8, 2.4e-7, 2.2e-5
The certificate is taken on the unscaled problem, whose multipliers are of the order of the prices (4e3 and 3e2 per unit), while the iteration
stops on the scaled one (OSQP's rule, relative to norms of up to 1e3 in the piecewise rows): hence 1e-6 rather than 1e-9.  KKT_BOUND is these x 10.
A multiplier on the side where the row has no bound is 0 in exact arithmetic; measured 3e-18; bounded by the rounding of one multiplier step,
2^-52 x the largest multiplier (4e3) x 10 = 1e-11.
"""
import importlib
import os

import numpy as np
import pytest

import dcopf_reference as R

jg = importlib.import_module("juliagrid.jl_amd")
opf = importlib.import_module("juliagrid.jl_amd.dcoptimalpowerflow")
sysmod = importlib.import_module("juliagrid.jl_amd.system")

CASES = ("case14test", "case30test")
KKT_BOUND = {"case14test": (3.6e-5, 7.2e-5, 7.7e-4, 1e-11), "case30test": (8.1e-7, 1.9e-5, 2.2e-4, 1e-11)}
ATOL = 1e-6                                                             # the reference's own tolerance against these goldens


def system_of(case):
    s = jg.powerSystem(R.tables(case))
    jg.dcModel_(s)
    return s


_solved = {}


def solved(case, rho):
    if (case, rho) not in _solved:
        s = system_of(case)
        md = R.model(s)
        _solved[case, rho] = (s, md, R.admm(md, rho=rho))
    return _solved[case, rho]


def within(cert, bound):
    return all(c <= b for c, b in zip(cert, bound))


@pytest.mark.parametrize("case", CASES)
def test_model_rows_equal_the_restatement(case):
    s = system_of(case)
    md, pm = R.model(s), opf.modelRows(s)
    assert (pm.n, pm.m) == (md.n, md.m)
    assert np.array_equal(opf.denseRows(pm), md.A)
    assert np.array_equal(pm.l, md.l) and np.array_equal(pm.u, md.u)
    assert np.array_equal(pm.P, md.P) and np.array_equal(pm.q, md.q) and pm.constant == md.constant
    assert list(pm.kind) == list(md.kind) and np.array_equal(pm.equality == 1, md.eq)


def test_case14_leaves_out_what_is_out_of_service():
    s = system_of("case14test")
    pm = opf.modelRows(s)
    assert s.branch.layout.status[2] == 0 and s.generator.layout.status[2] == 0
    assert 2 not in pm.var_pg and len(pm.var_pg) == 7
    A = opf.denseRows(pm)
    f, t = s.branch.layout.from_[2] - 1, s.branch.layout.to[2] - 1     # branch 3 is the only tie between its two buses
    assert A[pm.rows["balance"][f], t] == 0.0 and A[pm.rows["balance"][t], f] == 0.0
    # generator 5 has a piecewise cost of two points: linear, no helper, no piecewise row
    assert s.generator.cost.active.model[4] == 1 and 4 not in pm.helper and sorted(pm.helper) == [1, 7]
    pts = s.generator.cost.active.piecewise[5]
    assert pm.q[pm.var_pg[4]] == (pts[1, 1] - pts[0, 1]) / (pts[1, 0] - pts[0, 0])
    assert [r[0] for r in (pm.ref[i] for i in pm.rows["piecewise"])] == [2, 2, 8, 8, 8]
    assert [pm.ref[i] for i in pm.rows["flow"]] == [5, 9] and [pm.ref[i] for i in pm.rows["angle"]] == [6, 12, 14]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("rho", (0.1, 1.0))
def test_restatement_reaches_the_goldens(case, rho):
    s, md, r = solved(case, rho)
    g = R.golden(case)
    assert r.status == 0
    an = opf.DcOptimalPowerFlow.__new__(opf.DcOptimalPowerFlow)        # power_ alone: host code
    an.system, an.model, an.batch, an._x, an._demand, an._h = s, opf.modelRows(s), 1, r.x[None, :], s.bus.demand.active[None, :], None
    an.power = R.NS()
    opf.power_(an)
    th, gp, _ = R.parts(md, s, r.x)
    dev = dict(voltage=th - g["voltage"], generator=gp - g["generator"], injection=an.power.injection.active - g["injection"],
               supply=an.power.supply.active - g["supply"])
    dev["from"] = an.power.from_.active - g["from"]
    print(case, rho, r.iterations, r.refactorisations, {k: float(np.abs(v).max()) for k, v in dev.items()})
    for k, v in dev.items():
        assert np.abs(v).max() <= ATOL, k


@pytest.mark.parametrize("case", CASES)
def test_certificate(case):
    g = R.golden(case)
    for rho in (0.1, 1.0):
        s, md, r = solved(case, rho)
        th, gp, h = R.parts(md, s, r.x)
        cert = R.kkt(md, md.l, md.u, th, gp, h, R.duals(md, s, r.y))
        print(case, rho, cert)
        assert within(cert, KKT_BOUND[case])
    # the goldens carry no multipliers: the golden point with the restatement's multipliers.  Its helpers lie on their costs' curves
    s, md, r = solved(case, 1.0)
    h = np.array([np.interp(g["generator"][k], *s.generator.cost.active.piecewise[k + 1].T) for k in md.hv])
    cert = R.kkt(md, md.l, md.u, g["voltage"], g["generator"], h, R.duals(md, s, r.y))
    print(case, "golden", cert)
    assert cert[0] <= ATOL * np.abs(md.A).sum(axis=1).max()             # rows of A applied to a point within ATOL of feasible
    assert cert[3] <= KKT_BOUND[case][3]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("rho", (0.1, 7.0))
def test_K_from_the_term_lists(case, rho):
    s = system_of(case)
    pm, md = opf.modelRows(s), R.model(s)
    K, c, E = opf.hostModel(pm, rho, 1e-6)
    assert c == 1.0 / max(md.P.max(), np.abs(md.q).max())
    assert np.allclose(E, 1.0 / np.sqrt((md.A ** 2).sum(axis=1)), rtol=1e-15, atol=0)
    A = md.A * E[:, None]
    dense = np.diag(c * md.P + 1e-6) + A.T @ (np.where(md.eq, 1e3 * rho, rho)[:, None] * A)
    assert np.abs(K - dense).max() <= 1e-12 * np.abs(dense).max()
    assert np.array_equal(K != 0, (A.T @ A != 0) | np.eye(pm.n, dtype=bool))


def test_loader_fields_round_trip(tmp_path):
    t = R.tables("case14test")
    a = jg.powerSystem(t)
    np.savez(tmp_path / "c.npz", **t)
    b = jg.powerSystem(str(tmp_path / "c.npz"))
    F = lambda v: repr(float(v))
    lines = ["function mpc = c", "mpc.baseMVA = 100;", "mpc.bus = ["]
    lines += [f" {i + 1} {int(a.bus.layout.type[i])} {F(a.bus.demand.active[i] * 100)} 0 0 0 1 1 0 138 1 1.06 0.94" for i in range(a.bus.number)]
    lines += ["];", "mpc.gen = ["]
    g = a.generator
    lines += [f" {int(g.layout.bus[k])} 0 0 0 0 1 100 {int(g.layout.status[k])} {F(g.capability.maxActive[k] * 100)} {F(g.capability.minActive[k] * 100)}" for k in range(g.number)]
    lines += ["];", "mpc.branch = ["]
    br = a.branch
    lines += [f" {int(br.layout.from_[k])} {int(br.layout.to[k])} 0 {F(br.parameter.reactance[k])} 0 {F(br.flow.maxFromBus[k] * 100)} 0 0 0 0 {int(br.layout.status[k])} "
              f"{F(np.rad2deg(br.voltage.minDiffAngle[k]))} {F(np.rad2deg(br.voltage.maxDiffAngle[k]))}" for k in range(br.number)]
    lines += ["];", "mpc.gencost = ["]
    for k in range(g.number):
        if g.cost.active.model[k] == 2:
            c = g.cost.active.polynomial[k + 1]
            lines.append(f" 2 0 0 {c.size} " + " ".join(repr(float(v / 100.0 ** (c.size - 1 - j))) for j, v in enumerate(c)) + ";")
        else:
            p = g.cost.active.piecewise[k + 1]
            lines.append(f" 1 0 0 {len(p)} " + " ".join(f"{F(x * 100)} {F(y)}" for x, y in p) + ";")
    lines += ["];"]
    (tmp_path / "c.m").write_text("\n".join(lines) + "\n")
    m = jg.powerSystem(str(tmp_path / "c.m"))
    for other, tol in ((b, 0.0), (m, 1e-12)):
        assert np.allclose(other.generator.capability.minActive, g.capability.minActive, rtol=tol, atol=0)
        assert np.allclose(other.generator.capability.maxActive, g.capability.maxActive, rtol=tol, atol=0)
        assert np.allclose(other.branch.flow.maxFromBus, br.flow.maxFromBus, rtol=tol, atol=0) and np.array_equal(other.branch.flow.minFromBus, -other.branch.flow.maxFromBus)
        assert np.allclose(other.branch.voltage.minDiffAngle, br.voltage.minDiffAngle, rtol=tol, atol=0)
        assert np.allclose(other.branch.voltage.maxDiffAngle, br.voltage.maxDiffAngle, rtol=tol, atol=0)
        assert np.array_equal(other.generator.cost.active.model, g.cost.active.model)
        for k in range(g.number):
            name = "polynomial" if g.cost.active.model[k] == 2 else "piecewise"
            assert np.allclose(getattr(other.generator.cost.active, name)[k + 1], getattr(g.cost.active, name)[k + 1], rtol=tol, atol=0)
    # the dict made from a system reads back; fields that are absent: no cost, no limit
    again = jg.powerSystem({**t, **sysmod.costTables(a)})
    assert all(np.array_equal(again.generator.cost.active.piecewise[k], v) for k, v in g.cost.active.piecewise.items())
    plain = jg.powerSystem("case14test")
    assert not plain.generator.cost.active.model.any() and np.all(plain.generator.capability.minActive == -np.inf)
    assert not plain.branch.flow.maxFromBus.any() and np.all(plain.branch.voltage.maxDiffAngle == 2 * np.pi)
    assert opf.modelRows(plain).rows["flow"].size == 0 and opf.modelRows(plain).rows["angle"].size == 0


def test_setters():
    s = system_of("case30test")
    sysmod.cost_(s, 1, polynomial=[10.0, 20.0, 5.0])
    sysmod.cost_(s, 2, piecewise=[[0.0, 0.0], [1.0, 30.0]])
    jg.updateGeneratorSystem_(s, 1, minActive=0.1, maxActive=0.7)
    jg.updateBranchSystem_(s, 1, rating=0.3, minDiffAngle=-0.2, maxDiffAngle=0.25)
    pm = opf.modelRows(s)
    assert pm.P[pm.var_pg[0]] == 20.0 and pm.q[pm.var_pg[0]] == 20.0 and pm.q[pm.var_pg[1]] == 30.0
    r = pm.rows["capability"][0]
    assert (pm.l[r], pm.u[r]) == (0.1, 0.7)
    assert pm.ref[pm.rows["flow"][0]] == 1 and pm.u[pm.rows["flow"][0]] == 0.3 and pm.ref[pm.rows["angle"][0]] == 1
    with pytest.raises(ValueError):
        sysmod.cost_(s, 1)


def test_degree_three_is_refused():
    s = system_of("case14test")
    sysmod.cost_(s, 1, polynomial=[1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match="degree"):
        opf.modelRows(s)
