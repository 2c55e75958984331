"""Batched DC optimal power flow on the device against MATPOWER's goldens, the dense restatement (tests/dcopf_reference.py) and its KKT certificate.

Every solve here runs at tolerance 1e-9 (case14test too: about 16 450 iterations of a 23-variable problem).  The certificate's bounds are the host
test's (tests/test_dcopf_host.py: the restatement's values x 10).  The nodal prices are held to 2.4e-4: the restatement's own deviation between
tolerance 1e-9 and 1e-10 over the first 20 lanes is 2.4e-5 (prices of about 260 per unit), x 10.
"""
import importlib

import numpy as np
import pytest

import dcopf_reference as R
from test_dcopf_host import ATOL, KKT_BOUND, system_of, within

jg = importlib.import_module("juliagrid.jl_amd")
opf = importlib.import_module("juliagrid.jl_amd.dcoptimalpowerflow")

pytestmark = pytest.mark.gpu

PRICE_BOUND = 2.4e-4
SEED, LANES = 30, 130


def lane(an, j):
    """x, y of lane j and its results as 1-D arrays."""
    one = an.batch == 1
    pick = (lambda a: a) if one else (lambda a: a[j])
    dual = R.NS(balance=pick(an.dual.balance), slack=pick(an.dual.slack), capability=pick(an.dual.capability),
                flow={k: pick(v) for k, v in an.dual.flow.items()}, angle={k: pick(v) for k, v in an.dual.angle.items()},
                piecewise={k: pick(v) for k, v in an.dual.piecewise.items()})
    return R.NS(x=an._x[j], y=an._y[j], angle=pick(an.voltage.angle), pg=pick(an.power.generator.active), dual=dual,
                objective=float(np.atleast_1d(an.objective)[j]), status=int(np.atleast_1d(an.status)[j]), iterations=int(np.atleast_1d(an.iterations)[j]))


def certificate(an, md, j, l=None, u=None):
    r = lane(an, j)
    h = np.array([r.x[v] for v in md.hv.values()])
    return R.kkt(md, md.l if l is None else l, md.u if u is None else u, r.angle, r.pg, h, r.dual)


_profiles = {}


def profiles():
    """The scaled-demand lanes of case30test and the restatement's solution of each (rho = 0.1, not adapted), computed once."""
    if not _profiles:
        s = system_of("case30test")
        f = np.random.default_rng(SEED).uniform(0.8, 1.1, size=LANES)
        demand = s.bus.demand.active[None, :] * f[:, None]
        ref = []
        for j in range(LANES):
            md = R.model(s, demand=demand[j])
            ref.append((md, R.admm(md, adapt_every=0)))
        assert all(r.status == 0 for _, r in ref)
        _profiles.update(system=s, demand=demand, ref=ref)
    return _profiles


def solve_lanes(s, demand, **kw):
    an = jg.dcOptimalPowerFlow(s, batch=demand.shape[0], **kw)
    opf.setInjection_(an, demand)
    opf.solve_(an)
    return an


@pytest.mark.parametrize("case", ("case14test", "case30test"))
def test_goldens(case):
    s = system_of(case)
    an = jg.dcOptimalPowerFlow(s)
    opf.powerFlow_(an, power=True)
    g = R.golden(case)
    dev = dict(voltage=an.voltage.angle - g["voltage"], generator=an.power.generator.active - g["generator"], injection=an.power.injection.active - g["injection"],
               supply=an.power.supply.active - g["supply"])
    dev["from"] = an.power.from_.active - g["from"]
    cert = certificate(an, R.model(s), 0)
    print(case, "iterations", an.iterations, "refactorisations", an.refactorisations, {k: float(np.abs(v).max()) for k, v in dev.items()}, "certificate", cert)
    assert an.status == 0
    for k, v in dev.items():
        assert np.abs(v).max() <= ATOL, k
    assert np.allclose(an.power.to.active, -an.power.from_.active, rtol=0, atol=0)
    assert within(cert, KKT_BOUND[case])


@pytest.mark.parametrize("batch", (1, 5, 64, 70, 130))
def test_lane_edges(batch):
    p = profiles()
    an = solve_lanes(p["system"], p["demand"][:batch], adapt=False)
    worst = np.zeros(4)
    for j in range(batch):
        md, ref = p["ref"][j]
        r = lane(an, j)
        th, gp, _ = R.parts(md, p["system"], ref.x)
        d = (np.abs(r.angle - th).max(), np.abs(r.pg - gp).max(), abs(r.objective - ref.objective) / abs(ref.objective),
             np.abs(r.dual.balance - ref.y[md.kind == "balance"]).max())
        worst = np.maximum(worst, d)
        assert r.status == 0, j
        assert d[0] <= 1e-6 and d[1] <= 1e-6 and d[2] <= 1e-6 and d[3] <= PRICE_BOUND, (j, d)
        assert within(certificate(an, md, j), KKT_BOUND["case30test"]), j
    print("batch", batch, "worst deviation (angle, pg, objective, price)", worst, "iterations", np.min(an.iterations), np.max(an.iterations))


def test_lane_independence():
    p = profiles()
    an = solve_lanes(p["system"], p["demand"][:70], adapt=False)
    for j in (0, 37, 63, 64, 69):
        one = solve_lanes(p["system"], p["demand"][j:j + 1], adapt=False)
        assert np.array_equal(one._x[0], an._x[j]) and np.array_equal(one._y[0], an._y[j]), j
        assert int(one.iterations) == int(an.iterations[j]), j


def test_rho_adaptation():
    """case14test from rho = 0.1: the restatement needs 16 450 iterations and 4 refactorisations with adaptation and is not done after 20 000 without."""
    s = system_of("case14test")
    g = R.golden("case14test")
    an = jg.dcOptimalPowerFlow(s, rho=0.1, iteration=20000)
    opf.solve_(an)
    print("adapted: iterations", an.iterations, "refactorisations", an.refactorisations, "rho", an.rho)
    assert an.status == 0 and an.refactorisations >= 1 and an.rho != 0.1
    assert np.abs(an.voltage.angle - g["voltage"]).max() <= ATOL and np.abs(an.power.generator.active - g["generator"]).max() <= ATOL
    fixed = jg.dcOptimalPowerFlow(s, rho=0.1, iteration=20000, adapt=False)
    opf.solve_(fixed)
    assert fixed.status == 5 and fixed.iterations == 20000 and fixed.refactorisations == 0 and fixed.rho == 0.1


def test_generator_outage_in_one_lane():
    s = system_of("case30test")
    demand = np.tile(s.bus.demand.active, (5, 1)) * np.array([1.0, 0.95, 1.05, 0.9, 1.0])[:, None]
    base = solve_lanes(s, demand, adapt=False)
    an = jg.dcOptimalPowerFlow(s, batch=5, adapt=False)
    opf.setInjection_(an, demand)
    opf.setOutages_(an, generators=[0, 0, 1, 0, 0])
    opf.solve_(an)
    md = R.model(s, demand=demand[2], out_generator=1)
    ref = R.admm(md, adapt_every=0)
    th, gp, _ = R.parts(md, s, ref.x)
    r = lane(an, 2)
    assert r.status == 0 and ref.status == 0 and abs(r.pg[0]) <= 1e-6
    assert np.abs(r.angle - th).max() <= 1e-6 and np.abs(r.pg - gp).max() <= 1e-6 and abs(r.objective - ref.objective) <= 1e-6 * abs(ref.objective)
    assert within(certificate(an, md, 2), KKT_BOUND["case30test"])
    for j in (0, 1, 3, 4):
        assert np.array_equal(an._x[j], base._x[j]) and np.array_equal(an._y[j], base._y[j]) and an.iterations[j] == base.iterations[j], j
    with pytest.raises(ValueError, match="changes the constraint matrix"):
        opf.setOutages_(an, branches=[0, 0, 1, 0, 0])


def test_infeasible_lane():
    s = system_of("case30test")
    f = np.array([1.0, 0.95, 10.0, 0.9, 1.05])
    demand = np.tile(s.bus.demand.active, (5, 1)) * f[:, None]
    an = solve_lanes(s, demand, adapt=False, iteration=20000)
    assert R.admm(R.model(s, demand=demand[2]), adapt_every=0, iteration=20000).status == 2
    print("status", an.status, "iterations", an.iterations)
    assert list(an.status) == [0, 0, 2, 0, 0] and an.iterations.max() < 20000
    keep = [0, 1, 3, 4]
    other = solve_lanes(s, demand[keep], adapt=False, iteration=20000)
    for a, b in enumerate(keep):
        assert np.array_equal(other._x[a], an._x[b]) and np.array_equal(other._y[a], an._y[b]) and other.iterations[a] == an.iterations[b]


def test_warm_start():
    s = system_of("case30test")
    md = R.model(s, demand=s.bus.demand.active * 1.01)
    an = jg.dcOptimalPowerFlow(s, adapt=False)
    opf.solve_(an)
    cold = jg.dcOptimalPowerFlow(s, adapt=False)
    opf.setInjection_(cold, s.bus.demand.active * 1.01)
    opf.solve_(cold)
    opf.setInjection_(an, s.bus.demand.active * 1.01)
    opf.solve_(an)                                                      # goes on from the first solution
    print("cold", cold.iterations, "warm", an.iterations)
    assert an.status == 0 and cold.status == 0 and an.iterations < cold.iterations
    assert np.abs(an.voltage.angle - cold.voltage.angle).max() <= 1e-6 and np.abs(an.power.generator.active - cold.power.generator.active).max() <= 1e-6
    assert within(certificate(an, md, 0), KKT_BOUND["case30test"])
    # the same through setInitialPoint_ on a new analysis
    again = jg.dcOptimalPowerFlow(s, adapt=False)
    opf.setInjection_(again, s.bus.demand.active * 1.01)
    first = jg.dcOptimalPowerFlow(s, adapt=False)
    opf.solve_(first)
    opf.setInitialPoint_(again, first)
    opf.solve_(again)
    assert again.status == 0 and again.iterations < cold.iterations


def test_island_is_singular():
    t = R.tables("case14test")
    t["br_status"] = t["br_status"].copy()
    t["br_status"][13] = 0                                              # branch 14 is the only tie of its to-bus
    s = jg.powerSystem(t)
    an = jg.dcOptimalPowerFlow(s, batch=3)
    opf.solve_(an)
    assert list(an.status) == [3, 3, 3] and np.all(np.isnan(an.voltage.angle))
