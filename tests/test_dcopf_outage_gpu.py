"""Per-lane branch outages of the batched DC optimal power flow on the device (setBranchOutages_, csrc/jg_dcopf.hip) against the dense restatement of an
outaged lane (tests/dcopf_outage_reference.py), the rebuilt route on the device (a dcOptimalPowerFlow of the system without the branch) and the rebuilt
model's KKT certificate.

Bounds.  Against the restatement (the same iteration, K_s factorised densely): the restatement run with its solves on the base factor and the rank-2
correction (`woodbury=`) ends, over the 38 non-bridge outages of case30test and the lanes used here, at most 3.5e-14 x max|x| from the dense one in x,
4.7e-13 x max|y| in y and 3.1e-15 relative in the objective, with equal iteration counts; LANE_BOUND is these x 10.  An MI355X showed, over both
batches: 1.5e-14, 2.3e-13, 3.0e-15, equal iteration counts.  Against the rebuilt route: tests/test_dcopf_outage_host.py's
measured bounds.
"""
import importlib

import numpy as np
import pytest

import dcopf_outage_reference as O
import dcopf_reference as R
from test_dcopf_gpu import certificate, lane
from test_dcopf_host import KKT_BOUND, system_of, within
from test_dcopf_outage_host import ANGLE_BOUND, CASE14_ANGLE_BOUND, CASE14_PRICE_BOUND, LANE_BOUND, PRICE_BOUND, shifted

jg = importlib.import_module("juliagrid.jl_amd")
opf = importlib.import_module("juliagrid.jl_amd.dcoptimalpowerflow")

pytestmark = pytest.mark.gpu

OBJECTIVE_BOUND = 1e-6                                                  # relative: test_dcopf_gpu's bound on a lane's objective
# (branch out, generator out, demand factor): no outage, outages, the bridges 15 and 38, a generator outage beside a branch outage, scaled demand
SPECS = ((0, 0, 1.0), (10, 0, 1.0), (15, 0, 1.0), (5, 1, 1.0), (29, 0, 0.9), (0, 0, 1.05), (44, 0, 1.0), (7, 0, 0.95), (38, 0, 0.9), (22, 1, 1.05))
BRIDGES = (15, 38)

_ref = {}


def reference(spec):
    """The restatement's solution of one lane of case30test (rho = 0.1, not adapted), computed once per spec."""
    if spec not in _ref:
        s = system_of("case30test")
        k, g, f = spec
        _ref[spec] = O.solve(s, k, demand=s.bus.demand.active * f, out_generator=g, adapt_every=0)
    return _ref[spec]


def handle(s, specs, branches=True, **kw):
    an = jg.dcOptimalPowerFlow(s, batch=len(specs), **kw)
    opf.setInjection_(an, s.bus.demand.active[None, :] * np.array([f for _, _, f in specs])[:, None])
    opf.setOutages_(an, generators=[g for _, g, _ in specs])
    if branches:
        opf.setBranchOutages_(an, [k for k, _, _ in specs])
    return an


_solved = {}


def solved(batch):
    """The batch of `batch` lanes cycling through SPECS, solved once (adapt=False)."""
    if batch not in _solved:
        specs = [SPECS[j % len(SPECS)] for j in range(batch)]
        an = handle(system_of("case30test"), specs, adapt=False)
        opf.solve_(an)
        _solved[batch] = (specs, an)
    return _solved[batch]


@pytest.mark.parametrize("batch", (5, 70))
def test_lanes_equal_the_restatement(batch):
    specs, an = solved(batch)
    worst = np.zeros(3)
    for j, spec in enumerate(specs):
        if spec[0] in BRIDGES:
            assert an.status[j] == 3 and np.all(np.isnan(an._x[j])) and np.all(np.isnan(an._y[j])) and np.isnan(an.objective[j]) and an.iterations[j] == 0, j
            continue
        md, ln, ref = reference(spec)
        d = (np.abs(an._x[j] - ref.x).max() / np.abs(ref.x).max(), np.abs(an._y[j] - ref.y).max() / np.abs(ref.y).max(),
             abs(an.objective[j] - ref.objective) / abs(ref.objective))
        worst = np.maximum(worst, d)
        assert an.status[j] == ref.status == 0 and an.iterations[j] == ref.iterations, (j, spec, an.status[j], an.iterations[j], ref.iterations)
        assert all(a <= b for a, b in zip(d, LANE_BOUND)), (j, spec, d)
    print("batch", batch, "worst deviation from the restatement (x, y, objective; relative)", worst, "iterations", an.iterations.min(), an.iterations.max())


def test_untouched_lanes_are_bitwise_the_plain_handle():
    specs, an = solved(70)
    s = system_of("case30test")
    plain = handle(s, specs, branches=False, adapt=False)
    opf.solve_(plain)
    free = [j for j, spec in enumerate(specs) if spec[0] == 0]
    assert len(free) == 14 and any(j >= 64 for j in free)
    for j in free:
        assert np.array_equal(plain._x[j], an._x[j]) and np.array_equal(plain._y[j], an._y[j]) and plain.iterations[j] == an.iterations[j], j
    cleared = handle(s, specs, adapt=False)
    opf.solve_(cleared, iteration=50)                                   # the tables are on the device and W is built ...
    opf.setBranchOutages_(cleared, None)
    md = cleared.model                                                  # ... and the iterates back at zero
    opf._lib.check(opf._lib.lib().jg_dcopf_set_start(cleared._h, np.zeros(70 * md.n), np.zeros(70 * md.m)))
    opf.solve_(cleared)
    for j in range(70):
        assert np.array_equal(plain._x[j], cleared._x[j]) and np.array_equal(plain._y[j], cleared._y[j]) and plain.iterations[j] == cleared.iterations[j], j


def against_rebuilt(an, j, s, k, tables, demand=None, edit=None, bounds=(ANGLE_BOUND, PRICE_BOUND), kkt="case30test", **kw):
    """Lane j of `an` (branch k out) against a device solve of the system rebuilt without k; returns the deviations (angles, outputs, prices)."""
    s2, md2 = O.rebuilt(tables, k, demand=demand, edit=edit)
    other = jg.dcOptimalPowerFlow(s2, **kw)
    if demand is not None:
        opf.setInjection_(other, demand)
    opf.solve_(other)
    r = lane(an, j)
    d = (np.abs(r.angle - other.voltage.angle).max(), np.abs(r.pg - other.power.generator.active).max(), np.abs(r.dual.balance - other.dual.balance).max())
    assert r.status == 0 and other.status == 0, (k, r.status, other.status)
    assert d[0] <= bounds[0] and d[1] <= bounds[0] and d[2] <= bounds[1], (k, d)
    if kkt:
        assert within(certificate(an, md2, j), KKT_BOUND[kkt]), (k, certificate(an, md2, j))
    return d


def test_lanes_equal_the_rebuilt_route():
    s, t = system_of("case30test"), R.tables("case30test")
    an = handle(s, [(0, 0, 1.0), (10, 0, 1.0), (29, 0, 1.0), (44, 0, 1.0)], adapt=False)
    opf.solve_(an)
    for j, k in ((1, 10), (2, 29), (3, 44)):
        print("branch", k, "deviation from the rebuilt route (angles, outputs, prices)", against_rebuilt(an, j, s, k, t, adapt=False))


def test_rho_adaptation_rebuilds_w():
    """case14test from rho = 0.1: the factor changes with rho, and with it W and the lanes' 2 x 2 inverses."""
    s, t = system_of("case14test"), R.tables("case14test")
    an = jg.dcOptimalPowerFlow(s, batch=3, rho=0.1, iteration=60000)
    opf.setBranchOutages_(an, [0, 9, 2])
    opf.solve_(an)
    print("iterations", an.iterations, "refactorisations", an.refactorisations, "rho", an.rho)
    assert list(an.status) == [0, 0, 0] and an.refactorisations >= 1 and an.rho != 0.1
    bounds = (CASE14_ANGLE_BOUND, CASE14_PRICE_BOUND)
    for j, k in ((1, 9), (2, 2)):
        s2, md2 = O.rebuilt(t, k)
        ref = R.admm(md2, rho=0.1)
        th, gp, _ = R.parts(md2, s2, ref.x)
        r = lane(an, j)
        d = (np.abs(r.angle - th).max(), np.abs(r.pg - gp).max(), np.abs(r.dual.balance - ref.y[md2.kind == "balance"]).max())
        print("branch", k, "deviation from the rebuilt restatement (angles, outputs, prices)", d, "its iterations", ref.iterations)
        assert ref.status == 0 and d[0] <= bounds[0] and d[1] <= bounds[0] and d[2] <= bounds[1], (k, d)
    g, r = R.golden("case14test"), lane(an, 0)                          # the lane without an outage: MATPOWER's solution of the case
    assert np.abs(r.angle - g["voltage"]).max() <= bounds[0] and np.abs(r.pg - g["generator"]).max() <= bounds[0]


def test_infeasible_and_bridge_lanes():
    s = system_of("case14test")
    an = jg.dcOptimalPowerFlow(s, batch=4, rho=0.1, iteration=60000)
    opf.setBranchOutages_(an, [0, 13, 14, 9])
    opf.solve_(an)
    print("status", an.status, "iterations", an.iterations)
    assert s.branch.parameter.shiftAngle[13] != 0.0
    assert list(an.status) == [0, 2, 3, 0] and an.iterations[2] == 0 and an.iterations.max() < 60000
    assert np.all(np.isnan(an.voltage.angle[2])) and np.all(np.isfinite(an.voltage.angle[[0, 1, 3]]))


def test_phase_shift():
    t = R.tables("case30test")
    shifted(t)
    s = jg.powerSystem(t)
    jg.dcModel_(s)
    an = jg.dcOptimalPowerFlow(s, batch=2, adapt=False)
    opf.setBranchOutages_(an, [10, 10])
    opf.solve_(an)
    d = against_rebuilt(an, 1, s, 10, R.tables("case30test"), edit=shifted, adapt=False)
    demand = s.bus.demand.active * 1.05
    opf.setInjection_(an, np.stack((s.bus.demand.active, demand)))      # rewrites the balance rows: the shift change stays
    opf.solve_(an)
    e = against_rebuilt(an, 1, s, 10, R.tables("case30test"), demand=demand, edit=shifted, adapt=False)
    print("deviation from the rebuilt route before / after setInjection_", d, e)
    # the shift power matters: the same lane without the change of the balance rows is somewhere else
    f, tt = s.branch.layout.from_[9] - 1, s.branch.layout.to[9] - 1
    assert abs(an._shift[1, f]) > 1e-3 and an._shift[1, f] == -an._shift[1, tt]


def test_warm_start_and_replacing_the_set():
    s = system_of("case30test")
    an = jg.dcOptimalPowerFlow(s, batch=2, adapt=False)
    opf.solve_(an)
    opf.setBranchOutages_(an, [10, 0])
    opf.solve_(an)
    cold = jg.dcOptimalPowerFlow(s, batch=2, adapt=False)
    opf.setBranchOutages_(cold, [10, 0])
    opf.solve_(cold)
    print("cold", cold.iterations, "warm", an.iterations)
    assert list(an.status) == [0, 0] and list(cold.status) == [0, 0] and an.iterations[0] < cold.iterations[0]
    assert np.abs(an._x[0] - cold._x[0]).max() <= ANGLE_BOUND and np.abs(an.dual.balance[0] - cold.dual.balance[0]).max() <= PRICE_BOUND
    opf.setBranchOutages_(an, [29, 44])                                 # another set: nothing of the first one is left
    opf.solve_(an)
    fresh = jg.dcOptimalPowerFlow(s, batch=2, adapt=False)
    opf.setBranchOutages_(fresh, [29, 44])
    opf.solve_(fresh)
    assert list(an.outage) == [29, 44] and list(an.status) == [0, 0]
    for j in (0, 1):
        assert np.abs(an._x[j] - fresh._x[j]).max() <= ANGLE_BOUND and np.abs(an.dual.balance[j] - fresh.dual.balance[j]).max() <= PRICE_BOUND, j


def test_results_and_outage_costs():
    specs, an = solved(5)
    opf.power_(an)
    md = an.model
    assert 10 in [md.ref[i] for i in md.rows["flow"]]
    assert an.power.from_.active[1, 9] == 0.0 and an.power.to.active[1, 9] == 0.0 and an.power.from_.active[0, 9] != 0.0
    assert an.dual.flow[10][1] == 0.0 and np.all(np.isnan(an.power.from_.active[2]))
    # the injections are those of the remaining flows: supply - demand sums to the losses of a DC grid, none
    assert abs(an.power.injection.active[1].sum() - system_of("case30test").bus.shunt.conductance.sum()) <= 1e-9
    s = system_of("case30test")
    branches = [10, 29, 15, 44]
    c = jg.outageCosts(s, branches, adapt=False)
    print("outage costs", c.cost, "status", c.status, "price", c.price)
    assert c.base.status == 0 and list(c.status) == [0, 0, 3, 0] and np.isnan(c.cost[2])
    ok = c.status == 0
    assert np.all(c.cost[ok] >= -OBJECTIVE_BOUND * abs(c.base.objective)) and np.all(c.iterations[ok] > 0) and np.all(np.isfinite(c.price[ok]))


def test_set_outages_still_refuses_branches():
    specs, an = solved(5)
    with pytest.raises(ValueError, match="changes the constraint matrix"):
        opf.setOutages_(an, branches=[0, 10, 0, 0, 0])
