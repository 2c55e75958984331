"""What the Newton-Raphson and the Gauss-Newton handle own (csrc/jg_lanes.hpp: Lanes::alloc / upload / pin / arena / release_all, jg::Graph): a handle that fails
half-way through its creation goes cleanly, every block a handle allocates on first use goes with it, and a dropped iteration graph is captured again.
Shapes: case14 with 3 scenarios (one lane group: the one-launch verdict) and case118 with 70 (128 lanes: check + compaction, lanes move).  Nothing here is
computed differently from one pass to the next, so every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_case
from test_lanes_gpu import _monitoring
from test_oracle_se import se_case14
from test_se_gpu import _all_families, _mirror, _system_like

pytestmark = pytest.mark.gpu

SHAPES = [("case14", 3), ("case118", 70)]
# Free device memory after the destroys of the second pass may be lower than after the first pass's by this much (bytes): twice the largest pass-to-pass
# difference of this test body on the commit before the handles had an owner.  Three runs there read the same figures each time: 109 051 904 bytes for the
# case14 shape (the first in the process: the driver's own pools still grow), 0 for the case118 shape.
LEAK_MARGIN = 2 * 109051904


def _create_args(jg, s, batch=1, max_patch=0):
    Y, YT = s.model.ac.nodalMatrix, s.model.ac.nodalMatrixTranspose
    reim = jg.powerflow._reim
    return [s.bus.number, np.array(Y.colptr), np.array(Y.rowval), reim(Y.nzval).copy(), reim(YT.nzval).copy(),
            np.ascontiguousarray(s.bus.layout.type, dtype=np.int8), int(s.bus.layout.slack), batch, max_patch, 0]


def _solve(jg, s):
    an = jg.newtonRaphson(s)
    jg.powerFlow_(an)
    out = (int(an.method.iteration), int(an.status), an.voltage.magnitude.copy(), an.voltage.angle.copy())
    an.close()
    return out


def test_a_half_built_nr_handle_goes_cleanly(jg):
    """Both failures leave jg_nr_create after its analysis thread has started: the one exit path joins the thread and destroys what was built."""
    s = jg.powerSystem(load_case("case14"))
    L = jg._lib.lib()
    it0, st0, vm0, va0 = _solve(jg, s)
    assert st0 == 0 and it0 > 0
    n, colptr, rowval, y, yt, typ, slack, batch, mp, dev = _create_args(jg, s)
    p = next(q for q in range(int(colptr[1]) - 1) if rowval[q] != 1)          # an off-diagonal entry of column 1
    colptr2 = colptr.copy()
    colptr2[1:] -= 1
    h = jg._lib.VP()
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_nr_create(C.byref(h), n, colptr2, np.delete(rowval, p), np.delete(y, [2 * p, 2 * p + 1]), np.delete(yt, [2 * p, 2 * p + 1]),
                                     typ, slack, batch, mp, dev))
    assert e.value.code == 1 and "Ybus pattern is not structurally symmetric" in str(e.value) and not h.value
    assert _solve(jg, s)[:2] == (it0, st0)
    stale = yt.copy()
    stale[2] += 1.0
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_nr_create(C.byref(h), n, colptr, rowval, y, stale, typ, slack, batch, mp, dev))
    assert e.value.code == 4 and "nodalMatrix and nodalMatrixTranspose disagree (stale model)" in str(e.value) and not h.value
    it, st, vm, va = _solve(jg, s)
    assert (it, st) == (it0, st0) and np.array_equal(vm, vm0) and np.array_equal(va, va0)


def _state(an, tag, out):
    an._pull_voltage()
    out[tag + ".vm"], out[tag + ".va"] = np.array(an.voltage.magnitude), np.array(an.voltage.angle)
    out[tag + ".it"], out[tag + ".st"] = np.array(an.method.iteration), np.array(an.status)


def nr_sequence(jg, name, batch):
    """Every export of jg_nr that allocates on first use, on ONE handle: fast Newton-Raphson is for the rest of a handle's life, so it comes last (and finds the
    vectors the refined steps allocated).  The base case is a handle of one scenario and the stragglers move into a second handle.  Returns every result array
    by name."""
    out = {}
    L = jg._lib.lib()
    s = jg.powerSystem(load_case(name))
    n, nb = s.bus.number, s.branch.number
    labels = [int(x) for x in jg.outageList(s, batch - 1, seed=3)] + [0]
    an = jg.newtonRaphson(s, batch=batch)
    jg.setOutages_(an, labels)
    rng = np.random.default_rng(5)
    amp = np.linspace(0.0, 1.0, batch)[:, None]                          # starts further from the flat one the higher the lane: iteration counts differ by lane
    vm0, va0 = np.atleast_2d(an.voltage.magnitude)[:1], np.atleast_2d(an.voltage.angle)[:1]
    jg.powerflow._push_voltage(an, vm0 * (1.0 + 0.03 * amp * rng.uniform(-1, 1, (batch, n))), va0 + 0.1 * amp * rng.uniform(-1, 1, (batch, n)))
    an.snapshot_voltage()
    jg.setRefinement_(an, True)                                           # refined steps
    jg.powerFlow_(an)
    _state(an, "refined", out)
    jg.setRefinement_(an, False)
    an.restore_voltage()
    jg.powerFlow_(an)
    _state(an, "plain", out)
    jg.powerflow._upload_branches(an)                                     # branches; the staging of the branch quantities grows with the second call
    jg._lib.check(L.jg_nr_set_outage_labels(an._h, np.ascontiguousarray(an._outage_labels, dtype=np.int64)))
    out["from.small"], = jg.powerflow._pairs(an, lambda h, a: L.jg_nr_branch_quantities(h, a, None, None, None, None, None, None), nb, True)
    for k, b in enumerate(jg.powerflow._pairs(an, L.jg_nr_branch_quantities, nb, *[True] * 7)):
        out[f"branch.{k}"] = b
    assert np.array_equal(out["from.small"], out["branch.0"])
    for k, v in vars(jg.screenSummary_(an, rating=np.full(nb, 0.5))).items():
        out["screen." + k] = np.array(v)
    tp = s.bus.layout.type.copy()                                         # bus types per scenario, then a reactive-limit pass
    tp[int(np.flatnonzero(tp == 2)[0])] = 1
    jg.setBusType_(an, tp, [batch - 1])
    jg.powerFlow_(an)
    _state(an, "typed", out)
    out["violate"] = jg.reactiveLimit_(an)
    out["limitCount"] = np.array(an.method.limitCount)
    jg.powerFlow_(an)
    _state(an, "limited", out)
    jg.setBusType_(an, None)
    jg.setInjection_(an)
    jg._lib.check(L.jg_nr_adjust_angle(an._h, 2, 0.125))
    _state(an, "shifted", out)
    single = jg.newtonRaphson(s)                                          # a base case: attached, a compensated start, detached, attached again
    jg.powerFlow_(single)
    base = jg.BaseCase(single)
    for tag in ("comp1", "comp2"):
        base.attach(an)
        jg.startFromBase_(an)
        jg.powerFlow_(an)
        _state(an, tag, out)
        jg._lib.check(L.jg_nr_attach_base(an._h, None))
    out["first"] = np.array(jg.firstIterationCounts(an))
    base.close()
    single.close()
    an.restore_voltage()                                                  # the stragglers of a deferred run finish in a second handle
    pool = jg.newtonRaphson(s, batch=batch)
    left = an.run_defer(defer_at=64)
    home = pool.take_lanes(an, 0) if left else np.zeros(0, dtype=np.int32)
    an.finish()
    _state(an, "deferred", out)
    out["left"], out["home"] = np.array(left), home
    if home.size:
        out["pool.it"], out["pool.st"] = pool.resume(home.size)
        pool._pull_voltage()
        out["pool.vm"], out["pool.va"] = np.array(pool.voltage.magnitude[:home.size]), np.array(pool.voltage.angle[:home.size])
    pool.close()
    an.restore_voltage()                                                  # fast setup, one patch batch, a fast run
    _, _, _, _, bp, bq = jg.powerflow._fast_model(s, True)
    jg._lib.check(L.jg_nr_fast_setup(an._h, np.ascontiguousarray(bp), np.ascontiguousarray(bq)))
    an.method.fast, an.method.bx = True, True
    jg.setOutages_(an, labels)
    jg.powerFlow_(an)
    _state(an, "fast", out)
    an.close()
    return out


_MON14 = {}


def _monitoring_plain(jg, oracle, name):
    """The sets of tests/test_lanes_gpu.py; on case14 without the correlated PMUs, which the correction pass of the orthogonal method does not take."""
    if name != "case14":
        return _monitoring(jg, oracle, name)
    if not _MON14:
        t, osys, vm, va = se_case14(oracle)
        _MON14[0] = _mirror(jg, _system_like(jg, t, osys), _all_families(oracle, osys, vm, va, dict()))
    return _MON14[0]


def gn_sequence(jg, oracle, name, batch):
    """The correction pass (jg_gn_set_method), readings + noise on the device, a run, the objective, the residual test.  On case14 once more with the normal
    equations on the set with correlated PMUs: the objective then uploads a pair table that is not empty."""
    out = {}
    sets = [("se", _monitoring_plain(jg, oracle, name), jg.Orthogonal)] + ([("sec", _monitoring(jg, oracle, name), jg.LU)] if name == "case14" else [])
    for tag, mon, method in sets:
        an = jg.gaussNewton(mon, method, batch=batch)
        jg.drawNoise_(an, seed=9, scale=0.1)
        jg.stateEstimation_(an)
        _state(an, tag, out)
        out[tag + ".objective"] = np.array(an.objectiveDevice())
        r = jg.residualTest_(an)
        out[tag + ".maxres"], out[tag + ".index"] = np.array(r.maxNormalizedResidual), np.array(r.index)
        an.close()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name,batch", SHAPES)
def test_every_first_use_block_has_an_owner(jg, oracle, name, batch):
    """Two passes over every first-use allocation of both handles give the same bits, and the second pass's destroys give back what the first pass's did: free
    device memory after pass 2 is at most LEAK_MARGIN = 218 103 808 bytes below the reading after pass 1 (twice the 109 051 904 bytes measured on the parent)."""
    import torch
    free = []
    passes = []
    for _ in range(2):
        res = nr_sequence(jg, name, batch)
        res.update(gn_sequence(jg, oracle, name, batch))
        passes.append(res)
        free.append(torch.cuda.mem_get_info()[0])
    _same(*passes)
    assert name != "case118" or passes[0]["home"].size > 0               # the 128-lane shape does hand stragglers over
    print(f"[lifetime {name} x {batch}] {len(passes[0])} arrays; free device memory after pass 1 / 2: {free[0]} / {free[1]} (difference {free[0] - free[1]} bytes)")
    assert free[0] - free[1] <= LEAK_MARGIN


@pytest.mark.parametrize("name,batch", SHAPES)
def test_dropped_graphs_are_captured_again(jg, name, batch):
    s = jg.powerSystem(load_case(name))
    an = jg.newtonRaphson(s, batch=batch)
    jg.setOutages_(an, [int(x) for x in jg.outageList(s, batch, seed=4)])
    an.snapshot_voltage()
    a, b = {}, {}
    jg.powerFlow_(an)
    _state(an, "run", a)
    jg.setRefinement_(an, True)                                           # each change of the mode drops A, B, Bm, J and M
    jg.setRefinement_(an, False)
    an.restore_voltage()
    jg.powerFlow_(an)
    _state(an, "run", b)
    _same(a, b)
    an.close()


def test_the_whole_solve_graph_follows_the_stop_hint(jg):
    """ONE scenario: the second solve runs as one graph of as many iterations as the first took; a solve from the solution shrinks the hint, and the next solve from
    the start runs a shorter graph, then the loop.  The graph is captured again for every new length -- and, after a drop, for the same one."""
    an = jg.newtonRaphson(jg.powerSystem(load_case("case14")))
    an.snapshot_voltage()
    runs = []

    def run(restore=True):
        if restore:
            an.restore_voltage()
        res = {}
        jg.powerFlow_(an)
        _state(an, "run", res)
        runs.append(res)

    run(False)                                                            # iteration graphs; the hint becomes k
    assert runs[0]["run.it"] > 1 and runs[0]["run.st"] == 0
    run()                                                                 # one graph of k iterations
    jg.setRefinement_(an, True)
    jg.setRefinement_(an, False)
    run()                                                                 # ... captured again after the drop
    run(False)                                                            # from the solution: the hint shrinks
    assert runs[3]["run.it"] < runs[0]["run.it"]
    run()                                                                 # a shorter graph, the Jacobian alone, the loop
    run()                                                                 # the hint is k again
    for r in (runs[1], runs[2], runs[4], runs[5]):
        _same(runs[0], r)
    an.close()
