"""Per-lane branch outages of the DC optimal power flow without a device: the dense restatement of an outaged lane (tests/dcopf_outage_reference.py:
the base rows and scaling, A_s = A + p d', free rows) against the rebuilt route (dcopf_reference.model of the system without the branch), the
rebuilt model's KKT certificate on the restatement's solution, the bridges, and setBranchOutages_'s bookkeeping on an analysis without a handle.

Measured here on case30test, rho = 0.1 not adapted, over its 38 non-bridge in-service branches (every lane status 0 on both routes):
  the rebuilt route's own move between tolerance 1e-9 and 1e-10:  angles and outputs 5.53e-8, nodal prices 1.914e-5
  ANGLE_BOUND = 5.6e-7 and PRICE_BOUND = 2.0e-4 are these x 10 (the rule of test_dcopf_gpu.PRICE_BOUND), rounded up
  the restatement against the rebuilt route:                      angles and outputs 3.98e-8, nodal prices 1.38e-5
  the restatement with its solves on the base factor and the rank-2 correction (`woodbury=`, the device's way) against the dense K_s: equal
  iteration counts; x 3.5e-14 x max|x|, y 4.7e-13 x max|y|, objective 3.1e-15 relative.  LANE_BOUND, the device tests' parity bound, is these x 10
On case14test, rho = 0.1 adapted (the device test of the adaptation): see CASE14_ANGLE_BOUND / CASE14_PRICE_BOUND below.
"""
import importlib

import numpy as np
import pytest

import dcopf_outage_reference as O
import dcopf_reference as R
from test_dcopf_host import KKT_BOUND, system_of, within

jg = importlib.import_module("juliagrid.jl_amd")
opf = importlib.import_module("juliagrid.jl_amd.dcoptimalpowerflow")

ANGLE_BOUND, PRICE_BOUND = 5.6e-7, 2.0e-4
# case14test, rho = 0.1 adapted every 200, branches 2 and 9 out: the rebuilt route's move between tolerance 1e-9 and 1e-10 is 4.74e-5 in angles and
# outputs (2.91e-5 and 4.74e-5) and 2.48e-5 in the nodal prices (2.48e-5 and 2.12e-5); x 10, rounded up.  The restatement is 8.0e-5 and 4.4e-5 from the
# rebuilt route there: the two end at different rho, and this case's outputs are held loosely by its piecewise-linear costs
CASE14_ANGLE_BOUND, CASE14_PRICE_BOUND = 4.8e-4, 2.5e-4
LANE_BOUND = (3.5e-13, 4.7e-12, 3.1e-14)                                # x / max|x|, y / max|y|, objective relative
BRIDGES = {"case14test": [6, 11, 14, 16], "case30test": [1, 15, 18, 38]}

_lanes = {}


def candidates(system, case):
    return [k + 1 for k in range(system.branch.number) if system.branch.layout.status[k] == 1 and k + 1 not in BRIDGES[case]]


def lanes30():
    """Per non-bridge branch of case30test: the rebuilt model, its solutions at 1e-9 and 1e-10, the base model, the lane and the restatement's solution."""
    if not _lanes:
        s, t = system_of("case30test"), R.tables("case30test")
        for k in candidates(s, "case30test"):
            s2, md2 = O.rebuilt(t, k)
            md, ln, r = O.solve(s, k, adapt_every=0)
            _lanes[k] = R.NS(system=s, rebuilt_system=s2, md2=md2, a=R.admm(md2, adapt_every=0), b=R.admm(md2, adapt_every=0, tolerance=1e-10), md=md, lane=ln, r=r)
    return _lanes


def deviation(md, x, y, md2, x2, y2):
    """Largest difference in (angles and outputs, nodal prices) between a solution on the base rows and one on the rebuilt rows (the same variables)."""
    return np.abs(x - x2).max(), np.abs(y[md.kind == "balance"] - y2[md2.kind == "balance"]).max()


def test_restatement_equals_the_rebuilt_route():
    L = lanes30()
    assert len(L) == 38
    move, dev = np.zeros(2), np.zeros(2)
    for k, e in L.items():
        assert e.a.status == e.b.status == e.r.status == 0, k
        move = np.maximum(move, deviation(e.md2, e.a.x, e.a.y, e.md2, e.b.x, e.b.y))
        d = deviation(e.md, e.r.x, e.r.y, e.md2, e.a.x, e.a.y)
        dev = np.maximum(dev, d)
        assert d[0] <= ANGLE_BOUND and d[1] <= PRICE_BOUND, (k, d)
    print("rebuilt route's move 1e-9 -> 1e-10", move, "restatement against rebuilt", dev)
    assert 10 * move[0] <= ANGLE_BOUND and 10 * move[1] <= PRICE_BOUND     # the bounds are the measured moves x 10, not less


def test_rebuilt_certificate_on_the_restatement():
    for k, e in lanes30().items():
        assert np.all(e.r.y[e.lane.free] == 0.0), k                     # free rows: the multiplier never leaves 0
        th, gp, h = R.parts(e.md, e.system, e.r.x)
        cert = R.kkt(e.md2, e.md2.l, e.md2.u, th, gp, h, R.duals(e.md, e.system, e.r.y))
        assert within(cert, KKT_BOUND["case30test"]), (k, cert)


def test_woodbury_equals_the_dense_solve():
    """The rank-2 correction on the base factor, iterated to the end, against K_s factorised densely: what LANE_BOUND is measured from."""
    worst = np.zeros(3)
    for k, e in lanes30().items():
        w = O.admm(e.md, e.lane.A, e.lane.l, e.lane.u, adapt_every=0, woodbury=e.lane)
        assert w.status == 0 and w.iterations == e.r.iterations, k
        worst = np.maximum(worst, (np.abs(w.x - e.r.x).max() / np.abs(e.r.x).max(), np.abs(w.y - e.r.y).max() / np.abs(e.r.y).max(),
                                   abs(w.objective - e.r.objective) / abs(e.r.objective)))
    print("woodbury against dense (x, y, objective; relative)", worst)
    assert all(10 * a <= b for a, b in zip(worst, LANE_BOUND))


@pytest.mark.parametrize("case", ("case14test", "case30test"))
def test_bridges(case):
    s = system_of(case)
    tb = jg.islandTable(s)
    found = [k + 1 for k in range(s.branch.number) if tb.lo[k] <= tb.hi[k]]
    assert found == BRIDGES[case] == O.bridges(s)


def hostOnly(s, batch):
    return opf.DcOptimalPowerFlow(s, opf.modelRows(s), batch, None, False, 25, 200)


def shifted(t):
    t["br_shift"] = t["br_shift"].copy()
    t["br_shift"][9] = 3.0                                              # branch 10 of case30test: no bridge, rated (a flow row)


def test_bookkeeping():
    t = R.tables("case30test")
    shifted(t)
    s = jg.powerSystem(t)
    jg.dcModel_(s)
    an = hostOnly(s, 4)
    md = an.model
    assert 10 in [md.ref[i] for i in md.rows["flow"]] and s.branch.parameter.shiftAngle[9] != 0.0
    l0, u0 = an._l.copy(), an._u.copy()
    opf.setBranchOutages_(an, [0, 10, 15, None])
    assert list(an.outage) == [0, 10, 15, 0] and list(an._outage_state) == [0, 1, 3, 0] and an._outage_dirty
    own = [i for i in np.concatenate((md.rows["flow"], md.rows["angle"])) if md.ref[i] == 10]
    assert own and np.all(an._l[1, own] == -np.inf) and np.all(an._u[1, own] == np.inf)
    for j in (0, 2, 3):                                                 # a bridge lane is not run: its bounds stay
        assert np.array_equal(an._l[j], l0[j]) and np.array_equal(an._u[j], u0[j])
    other = np.setdiff1d(np.arange(md.m), own)
    s2, md2 = O.rebuilt(t, 10, edit=shifted)
    pm2 = opf.modelRows(s2)
    bal, bal2 = md.rows["balance"], pm2.rows["balance"]
    assert np.allclose(an._l[1, bal], pm2.l[bal2], rtol=0, atol=1e-14) and np.array_equal(an._l[1, bal], an._u[1, bal])
    f, tt = s.branch.layout.from_[9] - 1, s.branch.layout.to[9] - 1
    assert an._l[1, bal[f]] != l0[1, bal[f]] and an._l[1, bal[tt]] != l0[1, bal[tt]]
    rest = np.setdiff1d(other, bal)
    assert np.array_equal(an._l[1, rest], l0[1, rest]) and np.array_equal(an._u[1, rest], u0[1, rest])
    # a later setInjection_ rewrites the balance rows: the shift change stays
    demand = s.bus.demand.active * 1.1
    opf.setInjection_(an, demand)
    assert np.allclose(an._l[1, bal], R.model(s2, demand=demand).l[md2.kind == "balance"], rtol=0, atol=1e-14)
    assert np.array_equal(an._l[0, bal], -(demand + s.bus.shunt.conductance + s.model.dc.shiftPower))
    # generator outage and capability in the same lane
    opf.setOutages_(an, generators=[0, 1, 0, 0])
    assert an._l[1, md.rows["capability"][0]] == an._u[1, md.rows["capability"][0]] == 0.0 and np.all(an._l[1, own] == -np.inf)
    # replacing the set, then clearing it
    opf.setBranchOutages_(an, 12)
    assert list(an.outage) == [12] * 4 and np.array_equal(an._l[1, own], l0[1, own]) and np.array_equal(an._u[1, own], u0[1, own])
    opf.setBranchOutages_(an, None)
    opf.setOutages_(an, generators=None)
    opf.setInjection_(an, s.bus.demand.active)
    an._l[1, md.rows["capability"][0]], an._u[1, md.rows["capability"][0]] = l0[1, md.rows["capability"][0]], u0[1, md.rows["capability"][0]]
    assert not an.outage.any() and not an._outage_state.any() and not an._shift.any()
    assert np.array_equal(an._l, l0) and np.array_equal(an._u, u0)
    with pytest.raises(IndexError):
        opf.setBranchOutages_(an, [0, 0, 0, s.branch.number + 1])
    with pytest.raises(ValueError):
        opf.setBranchOutages_(an, [0, 0])
    with pytest.raises(ValueError, match="changes the constraint matrix"):
        opf.setOutages_(an, branches=[0, 10, 0, 0])


def test_a_branch_out_of_service_is_no_outage():
    s = system_of("case14test")
    assert s.branch.layout.status[2] == 0
    an = hostOnly(s, 2)
    l0 = an._l.copy()
    opf.setBranchOutages_(an, [3, 14])
    assert list(an.outage) == [0, 14] and list(an._outage_state) == [0, 3] and np.array_equal(an._l, l0)


def test_power_of_an_outaged_lane():
    s = system_of("case30test")
    an = hostOnly(s, 2)
    opf.setBranchOutages_(an, [0, 10])
    an._x = np.tile(np.linspace(0.0, 0.3, an.model.n), (2, 1))
    opf.power_(an)
    assert an.power.from_.active[1, 9] == 0.0 and an.power.to.active[1, 9] == 0.0 and an.power.from_.active[0, 9] != 0.0
    f, t = s.branch.layout.from_[9] - 1, s.branch.layout.to[9] - 1
    d = an.power.injection.active[0] - an.power.injection.active[1]
    assert d[f] == pytest.approx(an.power.from_.active[0, 9]) and d[t] == pytest.approx(-an.power.from_.active[0, 9])
    assert np.count_nonzero(np.abs(d) > 1e-15) == 2
