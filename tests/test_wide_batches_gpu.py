"""Batches of 1 024 to 4 160 lanes -- what contingency.recommendedLanes hands every grid below 5 000 buses -- held against the oracle, lane by lane.

Everything here depends on the LANE count, not on the grid, so the grids are small (14, 118 and 1 354 buses) and the oracle solves a scenario in well under a
millisecond.  What these widths reach and narrower tests do not (csrc/jg_engine.hpp: map_block; csrc/jg_compact.hip: k_compact, k_lanes_permute, k_lanes_move; csrc/jg_nr.hip: k_check;
csrc/jg_gn.hip: k_gn_gain; csrc/jg_comp.hip: k_csweep, k_ctop):
  * 16, 32 and 64 pinned lane groups; 17 and 65 balanced groups with the group list read from memory; after compaction a count of the OTHER mapping class under
    a grid sized for the handle's class (9..15 groups under 16, the eight-entry scalar list under 17, ...);
  * more than 1 024 lanes: every thread of the compaction owns a run of lanes (the packed two-counter scan), every thread of the in-place lane move up to four
    lanes of a row, ragged at 1 025 and 4 097 lanes; above 4 096 lanes the two-pass move is the default path;
  * Gauss-Newton at 16 pinned and 17 balanced groups (flags, no list).

The scenario family is indexed by the lane number b and shared by every width (oracle results are cached per scenario): lane b of case118 loses the non-bridge
branch L[b % K], has its demand scaled by a factor of its own in [0.9, 1.1] and starts from the flat start perturbed by amp(b) x noise_b, where amp comes from a
hash of b -- late finishers then sit in every lane group and the compaction has to swap lanes across groups.  The last lane of every width repeats lane 3.

Bounds: |dV|, |dtheta| <= 1e-8 against the oracle (the bar of every NR and GN parity test of the project: tests/test_nr_gpu.py, tests/test_se_scale_gpu.py), status and
iteration count equal.  Iteration counts may be compared exactly because the oracle's own runs stop clear of the tolerance (preconditions below)."""
import math
import time
from functools import lru_cache
from types import SimpleNamespace as NS

import numpy as np
import pytest

from conftest import load_case
from test_nr_gpu import _non_bridge_branches

gpu = pytest.mark.gpu

WIDTHS = [1024, 1025, 2048, 4096, 4097]
NSCEN = 4096                                   # scenarios of the family: the widest handle has 4 096 lanes of their own plus the duplicate of lane 3
ITERATION, TOLERANCE = 20, 1e-8
MARGIN = 1e-3                                  # every converged oracle run: last check <= tol / (1 + MARGIN), the check before >= tol * (1 + MARGIN)
# amp(b): three tiers picked by one hash of b, the place within the tier by a second -- (share of the lanes, lowest amplitude, highest amplitude).  From the oracle's runs:
# the first tier takes 3 or 4 iterations, the second 4, the third 5 to 7, so about two thirds of every width are still active after the third verdict, a quarter after the
# fourth and a few dozen lanes after the fifth -- group counts of both mapping classes under a grid sized for the handle's (4 096 lanes: 64, 64, 64, 41, 15, 1, 1).
# Amplitudes above 1 send single lanes on walks of ten to twenty iterations, where an iteration count is no longer a stable property of the scenario: the top stays at 1.
# The seeds were chosen on the oracle alone, for the margins below (a lane in a few thousand stops within 0.1 % of the tolerance under most seeds).
FACTOR_SEED, NOISE_SEED = 20261019, 4103
AMP_TIERS = ((0.35, 0.011, 0.02), (0.35, 0.1, 0.5), (0.30, 0.55, 1.0))


def _hash01(b, salt):
    """[0, 1) from the lane number alone (a 32-bit integer mix, the same on every platform)"""
    x = (np.asarray(b, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = x * np.uint64(0x85EBCA77) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = x * np.uint64(0xC2B2AE3D) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 4294967296.0


def _amp(b):
    pick, place = _hash01(b, 1), _hash01(b, 2)
    amp, edge = np.zeros(np.shape(b)), 0.0
    for share, lo, hi in AMP_TIERS:
        amp = np.where((pick >= edge) & (pick < edge + share + 1e-12), lo + (hi - lo) * place, amp)
        edge += share
    return amp


_CTX = {}


def _family(jg, oracle):
    """The scenario family on case118, built once: per scenario the outage label, the demand, the start point."""
    if "fam" not in _CTX:
        t = load_case("case118")
        s = jg.powerSystem(t)
        jg.acModel_(s)
        osys = oracle.OracleSystem(t)
        flat = oracle.OracleNR(osys)
        vm0, va0 = flat.vm.copy(), flat.va.copy()                  # the flat start of newtonRaphson() (initialize: the same arrays on both sides, tests/test_nr_gpu.py)
        n = osys.n
        L = _non_bridge_branches(t, 10 ** 9, seed=118)             # every non-bridge branch, shuffled
        b = np.arange(NSCEN)
        factor = np.random.default_rng(FACTOR_SEED).uniform(0.9, 1.1, NSCEN)
        rng = np.random.default_rng(NOISE_SEED)
        amp = _amp(b)[:, None]
        vm = vm0[None, :] * (1.0 + 0.04 * amp * rng.uniform(-1, 1, (NSCEN, n)))
        va = va0[None, :] + 0.15 * amp * rng.uniform(-1, 1, (NSCEN, n))
        label = np.array([L[k % len(L)] for k in b])
        _CTX["fam"] = NS(t=t, s=s, osys=osys, n=n, L=L, label=label, factor=factor, pd=osys.pd[None, :] * factor[:, None], qd=osys.qd[None, :] * factor[:, None],
                         vm=vm, va=va, jg=jg, oracle=oracle)
    return _CTX["fam"]


def _patched(fam, osys, s, label):
    o = fam.oracle.OracleNR(osys)
    ptr, dy = fam.jg.outagePatch(s, int(label))
    for p, d in zip(ptr, dy):
        o.add_ybus(p - 1, d)
    return o


def _finish(o, status):
    vm, va = o.voltage()
    _, f, inc = o.vectors()
    return NS(status=status, iteration=o.iteration, vm=vm, va=va, history=o.history.max(axis=1).copy(), f=f, inc=inc)


@lru_cache(maxsize=None)
def _oracle_lane(b):
    """scenario b of the family solved by the oracle alone"""
    fam = _CTX["fam"]
    o = _patched(fam, fam.osys, fam.s, fam.label[b])
    o.set_power(fam.osys.ps, fam.osys.qs, fam.pd[b], fam.qd[b])
    o.set_voltage(fam.vm[b], fam.va[b])
    return _finish(o, o.power_flow(iteration=ITERATION, tolerance=TOLERANCE))


def _scenarios(lanes):
    """lane -> scenario of the family: its own number, and lane 3's scenario once more in the last lane"""
    sc = np.arange(lanes)
    sc[-1] = 3
    return sc


def _groups_in_use(it):
    """ceil(#{it > k} / 64) for k = 0, 1, ...: the lane groups in use after each verdict, from the iteration counts alone"""
    it = np.asarray(it)
    return [int(math.ceil(int((it > k).sum()) / 64)) for k in range(int(it.max()))]


def _margins_hold(r):
    """the run stopped clear of the tolerance on both sides (tests/gs_reference.py: margins_hold), so its iteration count does not hang on a rounding"""
    h = r.history
    return h[-1] * (1.0 + MARGIN) <= TOLERANCE and (h.size < 2 or h[-2] >= TOLERANCE * (1.0 + MARGIN))


def _preconditions(jg, oracle, lanes):
    """What must hold of the ORACLE's runs before a width says anything about the device; returns the oracle's results per lane."""
    _family(jg, oracle)
    ref = [_oracle_lane(int(b)) for b in _scenarios(lanes)]
    st = np.array([r.status for r in ref])
    it = np.array([r.iteration for r in ref])
    conv = st == 0
    assert conv.sum() >= 0.99 * lanes, f"the oracle converges on {conv.sum()} of {lanes} lanes"
    bad = [b for b, r in enumerate(ref) if r.status == 0 and not _margins_hold(r)]
    assert not bad, f"oracle runs that stop within {MARGIN:g} of the tolerance: lanes {bad[:10]}, last two checks {[ref[b].history[-2:].tolist() for b in bad[:10]]}"
    assert len(set(it[conv].tolist())) >= 3
    seq = _groups_in_use(it)
    groups = -(-lanes // 64)
    assert any(8 < g < groups and g % 8 for g in seq), (lanes, seq)      # a balanced count with the list in memory, under a grid sized for the handle's class
    assert any(1 <= g <= 8 for g in seq), (lanes, seq)                  # the eight-entry scalar list
    # ... and both from lanes that CONVERGE (a lane that runs into the iteration limit would hold one group to the end all by itself)
    seqc = _groups_in_use(it[conv])
    assert any(8 < g < groups and g % 8 for g in seqc) and any(1 <= g <= 8 for g in seqc), (lanes, seqc)
    return ref, st, it, seq


@pytest.mark.parametrize("lanes", WIDTHS)
def test_the_oracle_side_of_every_width_holds_its_preconditions(jg, oracle, lanes):
    """No GPU: share of converged lanes, margins at the tolerance, spread of the iteration counts and the group-count sequence each width must walk through."""
    ref, st, it, seq = _preconditions(jg, oracle, lanes)
    print(f"[wide {lanes}] oracle: status {np.bincount(st).tolist()}, iterations {np.bincount(it).tolist()}, groups in use {seq}")


@gpu
@pytest.mark.parametrize("lanes", WIDTHS)
def test_every_lane_of_a_wide_batch_equals_the_oracle(jg, oracle, lanes):
    """16 pinned groups, 17 balanced groups with a ragged last group, 32 groups, 64 groups, 65 groups with the two-pass lane move: status and iteration count of EVERY lane
    equal the oracle's, V and theta of every converged lane within 1e-8, the duplicate of lane 3 bitwise lane 3, mismatch and last increment of moved lanes their own."""
    t0 = time.perf_counter()
    ref, st, it, seq = _preconditions(jg, oracle, lanes)
    t_oracle = time.perf_counter() - t0
    fam = _family(jg, oracle)
    sc = _scenarios(lanes)
    t0 = time.perf_counter()
    an = jg.newtonRaphson(fam.s, batch=lanes)
    for b in range(lanes):
        jg.setOutage_(an, b, int(fam.label[sc[b]]))
    jg.setInjection_(an, fam.osys.ps[None, :] - fam.pd[sc], fam.osys.qs[None, :] - fam.qd[sc])
    jg.powerflow._push_voltage(an, fam.vm[sc], fam.va[sc])
    jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
    dit, dst = np.array(an.method.iteration), np.array(an.status)
    vm, va = np.array(an.voltage.magnitude), np.array(an.voltage.angle)
    f, inc = an.mismatch, an.increment
    t_device = time.perf_counter() - t0
    conv = st == 0
    dv = np.abs(vm - np.array([r.vm for r in ref]))[conv].max()
    da = np.abs(va - np.array([r.va for r in ref]))[conv].max()
    print(f"[wide {lanes}] {conv.sum()} converged lanes against the oracle: max |dV| {dv:.2e}, |dtheta| {da:.2e}; iterations {np.bincount(it).tolist()} (device {np.bincount(dit).tolist()}), "
          f"status {np.bincount(st).tolist()}; groups in use {seq}; oracle {t_oracle:.2f} s, device side {t_device:.2f} s")
    assert np.array_equal(dst, st), np.flatnonzero(dst != st)[:10]
    assert np.array_equal(dit, it), [(int(b), int(dit[b]), int(it[b])) for b in np.flatnonzero(dit != it)[:10]]
    assert dv <= 1e-8 and da <= 1e-8
    assert np.array_equal(vm[lanes - 1], vm[3]) and np.array_equal(va[lanes - 1], va[3]) and dit[lanes - 1] == dit[3]
    # lanes the compaction moved: early finishers of the first groups (their slots are the holes) and late finishers of the last (the stragglers that fill them)
    order = np.flatnonzero(conv)
    early, late = order[it[order] == it[order].min()], order[it[order] == it[order].max()]
    mid = order[it[order] == int(np.median(it[order]))]
    picks = sorted(set(early[:3].tolist() + early[-2:].tolist() + late[:2].tolist() + late[-3:].tolist() + mid[len(mid) // 2:len(mid) // 2 + 2].tolist() + [3, lanes - 1]))
    assert np.abs(f[conv]).max() < 1e-8
    for b in picks:
        r = ref[b]
        assert np.abs(inc[b] - r.inc).max() <= 1e-9 * max(1.0, np.abs(r.inc).max()) + 1e-12, b
        assert np.abs(f[b]).max() < 1e-8 and np.abs(r.f).max() < 1e-8
    an.close()


# ---- the lane move one array at a time (csrc/jg_compact.hip: Compaction::launch_compact) ----------------------------------------------------------------
# Above 4 096 lanes the lanes move in two passes through the factor storage, all arrays at once when they fit it together: 6 n + 2 max_patch doubles per lane (V, theta,
# P, Q, the increment, the patch values) against 4 (factor entries + Jordan rows).  Only grids of a handful of buses miss that, and move one array at a time.
#   ring of 3 buses, max_patch 8: 34 staged doubles per lane against 4 (9 + 0) = 36: all arrays at once (the smallest meshed grid; nothing meshed falls below);
#   path of 3 buses, max_patch 8: 34 against 4 (7 + 0) = 28: ONE ARRAY AT A TIME.
# Scenario b scales the demand by a factor from a hash of b and starts from the flat start perturbed by _amp(b) x noise_b.
TINY = {"ring 3": [(0, 1), (1, 2), (2, 0)], "path 3": [(0, 1), (1, 2)]}
TINY_LANES, TINY_PATCH, TINY_SEED, TINY_NOISE = 4097, 8, 3, 981      # the noise seed was chosen on the oracle alone, for the margins (as NOISE_SEED above)


def _tiny(jg, oracle, name):
    """slack, one PV bus, one PQ bus (tests/dc_grids.py: table, with a reactive demand added); the scenario family of TINY_LANES lanes, built once"""
    key = "tiny:" + name
    if key not in _CTX:
        from dc_grids import table
        t = table(3, TINY[name], 0, TINY_SEED, units=1)
        t["bus_qd"] = 0.4 * t["bus_pd"]
        s = jg.powerSystem(t)
        jg.acModel_(s)
        osys = oracle.OracleSystem(t)
        flat = oracle.OracleNR(osys)
        n = osys.n
        b = np.arange(TINY_LANES)
        b[-1] = 3                                                  # the last lane repeats lane 3
        factor = 0.5 + 1.5 * _hash01(b, 3)
        rng = np.random.default_rng(TINY_NOISE)
        noise_v, noise_a = rng.uniform(-1, 1, (TINY_LANES, n)), rng.uniform(-1, 1, (TINY_LANES, n))
        noise_v[-1], noise_a[-1] = noise_v[3], noise_a[3]
        amp = _amp(b)[:, None]
        Y = s.model.ac.nodalMatrix
        entries = len(jg._lib.Plan(n, Y.colptr - 1, Y.rowval - 1).get("e_row"))
        _CTX[key] = NS(t=t, s=s, osys=osys, n=n, pd=osys.pd[None, :] * factor[:, None], qd=osys.qd[None, :] * factor[:, None],
                       vm=flat.vm[None, :] * (1.0 + 0.04 * amp * noise_v), va=flat.va[None, :] + 0.15 * amp * noise_a, oracle=oracle,
                       staged=6 * n + 2 * TINY_PATCH, factor=4 * entries, ref=None)
    return _CTX[key]


def _tiny_preconditions(jg, oracle, name):
    """The oracle's runs alone: every lane converges clear of the tolerance, and the lane groups in use fall at least once to a count >= 1 -- a compaction that
    permutes while lanes are active, and a restore that sends lanes home."""
    g = _tiny(jg, oracle, name)
    if g.ref is None:
        g.ref = []
        for b in range(TINY_LANES):
            o = oracle.OracleNR(g.osys)
            o.set_power(g.osys.ps, g.osys.qs, g.pd[b], g.qd[b])
            o.set_voltage(g.vm[b], g.va[b])
            g.ref.append(_finish(o, o.power_flow(iteration=ITERATION, tolerance=TOLERANCE)))
    st, it = np.array([r.status for r in g.ref]), np.array([r.iteration for r in g.ref])
    assert np.all(st == 0), np.flatnonzero(st != 0)[:10]
    bad = [b for b, r in enumerate(g.ref) if not _margins_hold(r)]
    assert not bad, f"oracle runs that stop within {MARGIN:g} of the tolerance: lanes {bad[:10]}, last two checks {[g.ref[b].history[-2:].tolist() for b in bad[:10]]}"
    seq = _groups_in_use(it)
    assert any(1 <= b < a for a, b in zip(seq, seq[1:])), seq
    assert (g.staged > g.factor) == (name == "path 3"), (name, g.staged, g.factor)      # which of the two staged moves the width takes
    return g, it, seq


@pytest.mark.parametrize("name", list(TINY))
def test_the_oracle_side_of_the_tiny_grids_holds_its_preconditions(jg, oracle, name):
    g, it, seq = _tiny_preconditions(jg, oracle, name)
    print(f"[tiny {name}] oracle: iterations {np.bincount(it).tolist()}, groups in use {seq}; {g.staged} staged doubles per lane against {g.factor} of the factor")


@gpu
@pytest.mark.parametrize("name", list(TINY))
def test_lanes_of_a_tiny_grid_move_through_a_factor_too_small_for_all_arrays(jg, oracle, name):
    """4 097 lanes (65 groups: the two-pass move) of a 3-bus grid.  On the path all arrays together exceed the factor storage (34 doubles per lane against 28), so
    every compaction and the restore move ONE ARRAY AT A TIME; on the ring they just fit (34 against 36) and go at once.  Either way: status and iteration count of every
    lane equal the oracle's, V and theta within 1e-8, the duplicate of lane 3 bitwise lane 3."""
    g, it, seq = _tiny_preconditions(jg, oracle, name)
    an = jg.newtonRaphson(g.s, batch=TINY_LANES, max_patch=TINY_PATCH)
    jg.setInjection_(an, g.osys.ps[None, :] - g.pd, g.osys.qs[None, :] - g.qd)
    jg.powerflow._push_voltage(an, g.vm, g.va)
    jg.powerFlow_(an, iteration=ITERATION, tolerance=TOLERANCE)
    dit, dst = np.array(an.method.iteration), np.array(an.status)
    vm, va = np.array(an.voltage.magnitude), np.array(an.voltage.angle)
    dv = np.abs(vm - np.array([r.vm for r in g.ref])).max()
    da = np.abs(va - np.array([r.va for r in g.ref])).max()
    print(f"[tiny {name}] max |dV| {dv:.2e}, |dtheta| {da:.2e}; iterations {np.bincount(it).tolist()} (device {np.bincount(dit).tolist()}); groups in use {seq}; "
          f"{g.staged} staged doubles per lane against {g.factor} of the factor")
    assert np.array_equal(dst, np.zeros(TINY_LANES, dtype=dst.dtype)), np.flatnonzero(dst != 0)[:10]
    assert np.array_equal(dit, it), [(int(b), int(dit[b]), int(it[b])) for b in np.flatnonzero(dit != it)[:10]]
    assert dv <= 1e-8 and da <= 1e-8
    assert np.array_equal(vm[-1], vm[3]) and np.array_equal(va[-1], va[3]) and dit[-1] == dit[3]
    an.close()


@lru_cache(maxsize=None)
def _base(name):
    """(tables, system, oracle system, base-case solution by the oracle's own Newton-Raphson) of a grid"""
    jg, oracle = _CTX["jg"], _CTX["oracle"]
    t = load_case(name)
    s = jg.powerSystem(t)
    jg.acModel_(s)
    osys = oracle.OracleSystem(t)
    return NS(t=t, s=s, osys=osys, jg=jg, oracle=oracle)


@lru_cache(maxsize=None)
def _oracle_outage(name, label, start_key):
    """the outage of one branch of a grid from the pipeline's start, solved by the oracle alone (cached per label: the jobs cycle their labels)"""
    g = _base(name)
    o = _patched(g, g.osys, g.s, label)
    o.set_voltage(*_CTX[start_key])
    return _finish(o, o.power_flow(iteration=ITERATION, tolerance=TOLERANCE))


def _records(torch, count, lanes, n):
    ring = [torch.full((lanes, 2 * n + 2), -7.0, dtype=torch.float64, device="cuda") for _ in range(count)]
    torch.cuda.current_stream().synchronize()                     # the fill runs on torch's stream, the library writes on its own: finish it first
    return ring


@gpu
@pytest.mark.parametrize("name,lanes", [pytest.param("case118", None, id="case118"), pytest.param("case1354pegase", 1088, id="case1354pegase-1088")])
def test_the_default_width_through_the_pipeline(jg, oracle, name, lanes):
    """ContingencyPipeline at the width recommendedLanes gives case118 (4 096 lanes = 64 groups, two jobs on two handles) and on case1354pegase at 1 088 lanes (17 groups,
    factorisation tasks below a real multifrontal top): the shared-factor first step is on, every lane of job 0 equals the oracle started from the base solution, and every
    job is bitwise what a pipeline with ONE batch in flight gives."""
    import torch
    _CTX["jg"], _CTX["oracle"] = jg, oracle
    g = _base(name)
    s, n = g.s, g.osys.n
    if lanes is None:
        lanes = jg.recommendedLanes(n)
        assert lanes == 4096
        pool = [int(x) for x in jg.outageList(s, s.branch.number, seed=3)]
        labels = [pool[k % len(pool)] for k in range(2 * lanes)]          # the grid has fewer candidates than lanes: the labels cycle, every lane is still checked
        jobs = [labels[:lanes], labels[lanes:]]
    else:
        jobs = [[int(x) for x in jg.outageList(s, lanes, seed=3)]]
    base = jg.newtonRaphson(s)
    jg.powerFlow_(base)
    assert base.status == 0
    start = (base.voltage.magnitude.copy(), base.voltage.angle.copy())
    base.close()
    _CTX["start:" + name] = start
    out = {}
    t0 = time.perf_counter()
    for inflight in (2, 1):
        pipe = jg.ContingencyPipeline(s, lanes, inflight=inflight, start=start)
        rec = _records(torch, len(jobs), lanes, n)
        res = pipe.run(jobs, iteration=ITERATION, tolerance=TOLERANCE, on_done=lambda j, an: torch.cuda.current_stream().synchronize(),
                       record=lambda j: rec[j].data_ptr(), records=len(jobs))
        started = [jg.firstIterationCounts(h) for h in pipe.handles]
        assert sum(c[0] for c in started) == len(jobs) and sum(c[1] for c in started) == 0, "every batch started on the base case's shared factor"
        out[inflight] = (res, [r.cpu().numpy() for r in rec])
        pipe.close()
    t_device = time.perf_counter() - t0
    for j in range(len(jobs)):
        (it_a, st_a), (it_b, st_b) = out[2][0][j], out[1][0][j]
        assert np.array_equal(it_a, it_b) and np.array_equal(st_a, st_b)
        assert np.array_equal(out[2][1][j], out[1][1][j], equal_nan=True)           # V | theta | iterations | status, bitwise
        assert np.array_equal(out[2][1][j][:, 2 * n], it_a.astype(float)) and np.array_equal(out[2][1][j][:, 2 * n + 1], st_a.astype(float))
    t0 = time.perf_counter()
    ref = [_oracle_outage(name, lab, "start:" + name) for lab in jobs[0]]
    t_oracle = time.perf_counter() - t0
    st, it = np.array([r.status for r in ref]), np.array([r.iteration for r in ref])
    conv = st == 0
    assert conv.sum() >= 0.99 * lanes
    bad = [b for b, r in enumerate(ref) if r.status == 0 and not _margins_hold(r)]
    assert not bad, f"oracle runs that stop within {MARGIN:g} of the tolerance: lanes {bad[:10]}"
    r0 = out[2][1][0]
    (dit, dst) = out[2][0][0]
    dv = np.abs(r0[:, :n] - np.array([r.vm for r in ref]))[conv].max()
    da = np.abs(r0[:, n:2 * n] - np.array([r.va for r in ref]))[conv].max()
    print(f"[pipeline {name} x {lanes}] {conv.sum()} converged lanes of job 0 against the oracle: max |dV| {dv:.2e}, |dtheta| {da:.2e}; iterations {np.bincount(it).tolist()}, "
          f"status {np.bincount(st).tolist()}; groups in use {_groups_in_use(it)}; oracle {t_oracle:.2f} s, device side (both pipelines) {t_device:.2f} s")
    assert np.array_equal(dst, st), np.flatnonzero(dst != st)[:10]
    assert np.array_equal(dit, it), [(int(b), int(dit[b]), int(it[b])) for b in np.flatnonzero(dit != it)[:10]]
    assert dv <= 1e-8 and da <= 1e-8


@gpu
@pytest.mark.parametrize("batch", [1024, 1088])
def test_gauss_newton_at_sixteen_and_seventeen_groups(jg, oracle, batch):
    """Gauss-Newton at 16 pinned and at 17 balanced lane groups (flags, no list: the count a launch maps by is always the handle's) on the all-families set of the
    modified IEEE 14 system, every lane with readings of its own.  The oracle takes each lane's RAW readings (the same numpy draw setNoise_ makes) and derives that
    lane's means and weights by its own value rules; they are first held against what the device holds (measurementDevice), then the lane is solved: equal status
    and iteration count, V and theta within 1e-8 -- the direct route, per lane, not the detour over a 256-lane handle."""
    from test_lanes_gpu import _monitoring
    from test_oracle_se import se_case14
    from test_se_gpu import _all_families
    t, osys, vm, va = se_case14(oracle)
    tab = _all_families(oracle, osys, vm, va, dict(correlated=True)).arrays()
    t0 = time.perf_counter()
    an = jg.gaussNewton(_monitoring(jg, oracle, "case14"), batch=batch)
    z1, v1, s1, z2, v2, s2 = an._z
    assert np.array_equal(tab["mean1"], z1) and np.array_equal(tab["var1"], v1) and np.array_equal(tab["mean2"], z2) and np.array_equal(tab["var2"], v2)
    seed, scale = 1400 + batch, 0.1
    jg.setNoise_(an, np.random.default_rng(seed), scale=scale)
    rng = np.random.default_rng(seed)                              # the draw of setNoise_ once more: z + scale x sigma x N(0, 1), magnitudes first, then angles
    n1 = z1[None, :] + scale * np.sqrt(v1)[None, :] * rng.standard_normal((batch, z1.size))
    n2 = z2[None, :] + scale * np.sqrt(v2)[None, :] * rng.standard_normal((batch, z2.size))
    mean, wd, wo = jg.measurementDevice(an)
    assert len(np.unique(mean, axis=0)) == batch                  # every lane has readings of its own
    jg.stateEstimation_(an)
    dit, dst = np.array(an.method.iteration), np.array(an.status)
    dvm, dva = np.array(an.voltage.magnitude), np.array(an.voltage.angle)
    t_device = time.perf_counter() - t0
    corr = np.asarray(an.method._corr, dtype=np.int64)
    t0 = time.perf_counter()
    worst_v = worst_a = worst_w = 0.0
    its, sts = np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.int64)
    for b in range(batch):
        lane = dict(tab)
        lane["mean1"], lane["mean2"] = np.ascontiguousarray(n1[b]), np.ascontiguousarray(n2[b])
        gn = oracle.OracleGN(osys, lane)
        # this lane's means and weights, as the oracle derives them and as the device holds them: the same formulas in C and in numpy; the precision of a correlated
        # PMU pair holds a difference of two products, so they agree to a few hundred ulps (1e-12 relative), four orders below what the 1e-8 on the state can see
        for dev, orc in ((mean[b], gn.mean), (wd[b], gn.wdiag), (wo[b], gn.woff[corr - 1])):
            worst_w = max(worst_w, float((np.abs(dev - orc) / np.maximum(np.abs(orc), 1e-300)).max()) if orc.size else 0.0)
        sts[b] = gn.state_estimation()
        its[b] = gn.iteration
        h = gn.history                                            # the largest increment at every check: the count must not hang on a rounding here either
        assert sts[b] != 0 or (h[-1] * (1.0 + MARGIN) <= 1e-8 and (h.size < 2 or h[-2] >= 1e-8 * (1.0 + MARGIN))), (b, h[-2:])
        v = gn.vectors()
        if sts[b] == 0:
            worst_v, worst_a = max(worst_v, np.abs(dvm[b] - v["magnitude"]).max()), max(worst_a, np.abs(dva[b] - v["angle"]).max())
    t_oracle = time.perf_counter() - t0
    print(f"[gauss-newton {batch}] every lane against the oracle: max |dV| {worst_v:.2e}, |dtheta| {worst_a:.2e}; means and weights agree to {worst_w:.1e} relative; "
          f"iterations {np.bincount(its).tolist()}, status {np.bincount(sts).tolist()}; oracle {t_oracle:.2f} s, device side {t_device:.2f} s")
    assert worst_w <= 1e-12
    assert (sts == 0).sum() >= 0.99 * batch
    assert np.array_equal(dst, sts), np.flatnonzero(dst != sts)[:10]
    assert np.array_equal(dit, its), [(int(b), int(dit[b]), int(its[b])) for b in np.flatnonzero(dit != its)[:10]]
    assert worst_v <= 1e-8 and worst_a <= 1e-8
    an.close()
