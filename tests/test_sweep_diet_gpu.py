"""The bus-order increment is optional per handle (jg_nr_set_keep_increment; the null `out` of the backward sweeps, of the shared-factor backward rows and
of the dense top's epilogue), and the pivot-order store of a row nothing reads back is skipped (jg_symbolic.hpp: bwd_dead, CompTables::dead; JG_SWEEP_DEAD=0
keeps it).  No arithmetic changes, so a batch gives the SAME BITS -- iteration counts, status, V, theta -- in the three forms keep-increment 0, keep-increment 1
and JG_SWEEP_DEAD=0, and what the oracle gives (V, theta within 1e-8, equal iteration counts, the project's bound of tests/test_nr_gpu.py).

Shapes: case118 at 1 lane (the single-instance sweep, which stores as before), 64 (a full lane group), 65 (a group and one clamped lane) and 130 (three groups
with padding; the batch compacts to one group for its last iteration); case1354pegase at 70 lanes, the smallest shipped grid whose plan has chain tasks and a
multi-level top.  The rest of the path: a ContingencyPipeline with a straggler pool (lane compaction and hand-off without the increment rows), the first step
on a shared base factor with the default dense top and with none, and the fall-back to a refactorising first iteration."""
import numpy as np
import pytest

from conftest import load_case

pytestmark = pytest.mark.gpu

ITERATION, TOLERANCE = 20, 1e-8


def _keep(jg, an, on):
    jg._lib.check(jg._lib.lib().jg_nr_set_keep_increment(an._h, 1 if on else 0))


def _labels(jg, s, batch):
    ok = [int(x) for x in jg.outageList(s, max(batch, 3), seed=11)]
    if batch == 1:
        return ok[:1]
    return [0] + ok[:batch - 2] + [ok[0]]                           # the base case (converged at the start), outages, a duplicate


@pytest.fixture(scope="module")
def grids(jg, oracle):
    """per grid: system, base-case solution, oracle system and the oracle's N-1 runs by label (computed once, shared, never changed)"""
    out = {}
    for name in ("case118", "case1354pegase"):
        t = load_case(name)
        s = jg.powerSystem(t)
        single = jg.newtonRaphson(s)
        jg.powerFlow_(single)
        assert single.status == 0
        start = (single.voltage.magnitude.copy(), single.voltage.angle.copy())
        single.close()
        out[name] = dict(s=s, start=start, osys=oracle.OracleSystem(t), runs={})
    return out


def _oracle_run(oracle, jg, d, label):
    if label not in d["runs"]:
        o = oracle.OracleNR(d["osys"])
        if label:
            ptr, dy = jg.outagePatch(d["s"], label)
            for p, v in zip(ptr, dy):
                o.add_ybus(p - 1, v)
        o.set_voltage(*d["start"])
        rc = o.power_flow()
        vm, va = o.voltage()
        d["runs"][label] = (rc, o.iteration, np.array(vm), np.array(va))
    return d["runs"][label]


def _result(an):
    return dict(vm=np.atleast_2d(an.voltage.magnitude).copy(), va=np.atleast_2d(an.voltage.angle).copy(),
                it=np.atleast_1d(an.method.iteration).copy(), status=np.atleast_1d(an.status).copy())


def _run_refactorising(jg, d, labels, keep):
    an = jg.contingencyAnalysis(d["s"], labels)
    _keep(jg, an, keep)
    jg.setFirstIteration_(an, False)
    jg.powerflow._push_voltage(an, *d["start"])
    jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
    res = _result(an)
    res["counts"] = jg.firstIterationCounts(an)
    res["inc"] = np.atleast_2d(an.increment).copy() if keep else None
    an.close()
    return res


def _same_bits(a, b):
    for k in ("it", "status", "vm", "va"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name,batch", [("case118", 1), ("case118", 64), ("case118", 65), ("case118", 130), ("case1354pegase", 70)])
def test_batch_without_the_increment_is_bitwise_the_batch_with_it_and_matches_the_oracle(jg, oracle, grids, monkeypatch, name, batch):
    d = grids[name]
    labels = _labels(jg, d["s"], batch)
    monkeypatch.delenv("JG_SWEEP_DEAD", raising=False)
    off = _run_refactorising(jg, d, labels, False)
    on = _run_refactorising(jg, d, labels, True)
    monkeypatch.setenv("JG_SWEEP_DEAD", "0")
    stored = _run_refactorising(jg, d, labels, False)
    stored_on = _run_refactorising(jg, d, labels, True)
    monkeypatch.delenv("JG_SWEEP_DEAD")
    assert off["counts"] == (0, 1) and on["counts"] == (0, 1) and stored["counts"] == (0, 1)
    _same_bits(off, on)
    _same_bits(off, stored)
    _same_bits(off, stored_on)
    assert np.array_equal(on["inc"], stored_on["inc"])
    good = off["status"] == 0
    worst = 0.0
    for sc, lab in enumerate(labels):
        rc, it, vm, va = _oracle_run(oracle, jg, d, lab)
        assert (rc == 0) == bool(good[sc]), (sc, lab)
        if rc != 0:
            continue
        assert it == off["it"][sc], (sc, lab)
        worst = max(worst, np.abs(off["vm"][sc] - vm).max(), np.abs(off["va"][sc] - va).max())
    its = off["it"][good]
    groups = [int(-(-np.sum(its > k) // 64)) for k in range(int(its.max()))]       # lane groups in use at every iteration (the lanes are packed between iterations)
    print(f"\n[{name} x {batch}] worst |dV|, |dtheta| against the oracle {worst:.2e}; iterations {np.bincount(its).tolist()}; lane groups per iteration {groups}")
    assert worst <= 1e-8
    if (name, batch) == ("case118", 130):
        assert groups[0] == 3 and groups[-1] == 1, "this batch is the one that compacts from three lane groups to one"


def test_getter_fails_while_off_and_returns_todays_values_when_on(jg, grids):
    d = grids["case118"]
    labels = _labels(jg, d["s"], 65)
    ref = _run_refactorising(jg, d, labels, True)
    an = jg.contingencyAnalysis(d["s"], labels)
    jg.setFirstIteration_(an, False)
    _keep(jg, an, False)
    jg.powerflow._push_voltage(an, *d["start"])
    jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
    with pytest.raises(jg._lib.JGridError, match="jg_nr_set_keep_increment"):
        an.increment
    _keep(jg, an, True)
    with pytest.raises(jg._lib.JGridError, match="jg_nr_set_keep_increment"):      # nothing of the runs before the switch comes back
        an.increment
    jg.powerflow._push_voltage(an, *d["start"])
    jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
    assert np.array_equal(np.atleast_2d(an.increment), ref["inc"])
    _same_bits(_result(an), ref)
    an.close()


def test_refinement_keeps_its_increment(jg, grids):
    """k_refine_apply writes method.increment: switching refinement on switches the increment back on, and the switch refuses to go off under it"""
    d = grids["case118"]
    labels = _labels(jg, d["s"], 65)
    out = []
    for switched in (False, True):
        an = jg.contingencyAnalysis(d["s"], labels)
        jg.setFirstIteration_(an, False)
        if switched:
            _keep(jg, an, False)
        jg.setRefinement_(an, True)
        if switched:
            assert jg._lib.lib().jg_nr_set_keep_increment(an._h, 0) == 1 and b"jg_nr_set_refine" in jg._lib.lib().jg_last_error()
        jg.powerflow._push_voltage(an, *d["start"])
        jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
        res = _result(an)
        res["inc"] = np.atleast_2d(an.increment).copy()
        out.append(res)
        an.close()
    _same_bits(out[0], out[1])
    assert np.array_equal(out[0]["inc"], out[1]["inc"])
    assert (out[0]["status"] == 0).sum() >= 63 and np.abs(out[0]["inc"]).max() > 0.0


@pytest.mark.parametrize("top_cap", [0, -1], ids=["top-default", "top-none"])
def test_shared_factor_first_step_and_its_fall_back(jg, grids, monkeypatch, top_cap):
    d = grids["case1354pegase"]
    s, batch = d["s"], 70
    labels = _labels(jg, s, batch)
    single = jg.newtonRaphson(s)
    jg.powerFlow_(single)
    base = jg.BaseCase(single, top_cap=top_cap)
    assert (base.info["top_pivots"] > 0) == (top_cap == 0)
    start0 = (single.voltage.magnitude.copy(), single.voltage.angle.copy())
    res = {}
    for keep in (False, True, "stored"):
        monkeypatch.delenv("JG_SWEEP_DEAD", raising=False)
        if keep == "stored":
            monkeypatch.setenv("JG_SWEEP_DEAD", "0")
        an = jg.contingencyAnalysis(s, labels)
        _keep(jg, an, keep is True)
        base.attach(an)
        jg.startFromBase_(an)
        jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
        assert jg.firstIterationCounts(an) == (1, 0)
        res[keep, "shared"] = _result(an)
        jg.powerflow._push_voltage(an, *start0)                     # the same state, but not through startFromBase_: the first iteration refactorises
        jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
        assert jg.firstIterationCounts(an) == (1, 1)
        res[keep, "fallback"] = _result(an)
        an.close()
    monkeypatch.delenv("JG_SWEEP_DEAD", raising=False)
    for other in (True, "stored"):
        _same_bits(res[False, "shared"], res[other, "shared"])
        _same_bits(res[False, "fallback"], res[other, "fallback"])
    a, b = res[False, "shared"], res[False, "fallback"]
    good = a["status"] == 0
    assert good.sum() >= batch - 3 and np.array_equal(a["status"], b["status"])
    assert np.abs(a["vm"][good] - b["vm"][good]).max() <= 1e-8 and np.abs(a["va"][good] - b["va"][good]).max() <= 1e-8
    base.close(); single.close()


def test_pipeline_with_a_pool_hands_lanes_over_without_increment_rows(jg, oracle, grids, monkeypatch):
    """The pipeline switches the increment off on its batch and pool handles; the same pipeline with every handle switched back on gives the same records"""
    import torch
    d = grids["case1354pegase"]
    s, batch, njobs = d["s"], 128, 3
    n = s.bus.number
    labels = [int(x) for x in jg.outageList(s, batch * njobs, seed=3)]
    jobs = [labels[i * batch:(i + 1) * batch] for i in range(njobs)]
    jobs[-1] = jobs[-1][:batch - 5]
    out = {}
    for keep in (False, True, "stored"):
        monkeypatch.delenv("JG_SWEEP_DEAD", raising=False)
        if keep == "stored":
            monkeypatch.setenv("JG_SWEEP_DEAD", "0")
        pipe = jg.ContingencyPipeline(s, batch, inflight=2, start=d["start"], pool=64)
        assert pipe.pools
        every = pipe.handles + [p.handle for p in pipe.pools]
        for an in every:
            with pytest.raises(jg._lib.JGridError, match="jg_nr_set_keep_increment"):
                an.increment
            if keep is True:
                _keep(jg, an, True)
        rec = [torch.full((batch, 2 * n + 2), -7.0, dtype=torch.float64, device="cuda") for _ in range(njobs)]
        torch.cuda.current_stream().synchronize()
        res = pipe.run(jobs, iteration=ITERATION, tolerance=TOLERANCE, on_done=lambda j, an: torch.cuda.current_stream().synchronize(),
                       record=lambda j: rec[j].data_ptr(), records=njobs)
        out[keep] = (res, [r.cpu().numpy().copy() for r in rec])
        handed = sorted(pipe._stragglers.pending)                   # the jobs that handed scenarios to a pool (jg_nr_move_lanes) in this run
        assert handed, "no job of this run finished scenarios in a pool: the hand-off is what this test is about"
        pipe.close()
    monkeypatch.delenv("JG_SWEEP_DEAD", raising=False)
    for j in range(njobs):
        for other in (True, "stored"):
            (it_a, st_a), (it_b, st_b) = out[False][0][j], out[other][0][j]
            assert np.array_equal(it_a, it_b) and np.array_equal(st_a, st_b) and not np.any(st_a == 4)
            assert np.array_equal(out[False][1][j], out[other][1][j], equal_nan=True)     # V | theta | iterations | status, bitwise
    (it0, st0), r0 = out[False][0][0], out[False][1][0]
    for sc in range(0, batch, 9):                                   # and a sample of job 0 against the oracle
        rc, it, vm, va = _oracle_run(oracle, jg, d, jobs[0][sc])
        assert (rc == 0) == (st0[sc] == 0)
        if rc == 0:
            assert it == it0[sc] and np.abs(r0[sc, :n] - vm).max() <= 1e-8 and np.abs(r0[sc, n:2 * n] - va).max() <= 1e-8

