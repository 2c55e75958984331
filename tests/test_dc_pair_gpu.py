"""The DC N-2 screen (dcPairScreen, csrc/jg_dc_pair.hip) and the lanes with two outages (jg_dc_set_outage_pairs) on the device, against the rebuild
route of tests/dc_pair_reference.py: the second branch out of service in a copy of the case table, then dc_reference.solve(t2, out=k) -- rebuild and
refactorise for every pair, never the compensation.  Islanding is held against the graph oracle (connected components), not against any linear algebra.

Tolerance of every comparison: |got - ref| <= 1e-9 * max(1, max |ref|), as in tests/test_dc_gpu.py.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import dc_pair_reference as P
import dc_reference as R
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9


def check_pair(t, rating, k, l, got_load, got_branch, base, monitored=None):
    """one pair (0-based branches) of a screen against the rebuild route; returns (islanding, scaled deviation)"""
    if P.islands(t, k, l, base):
        assert np.isnan(got_load), (k, l, got_load)
        return True, 0.0
    _, fr = P.pair_solve(t, k, l)
    assert fr is not None, (k, l)
    w, b, load = P.loading(fr, rating, monitored)
    scale = max(1.0, w)
    dev = abs(got_load - w) / scale
    assert dev <= TOL, (k, l, got_load, w, dev)
    # ties go to the lowest branch index; another index only where the two loadings agree within the tolerance
    assert got_branch == b or (got_branch >= 1 and abs(load[got_branch - 1] - w) <= TOL * scale), (k, l, got_branch, b)
    return False, dev


@pytest.mark.parametrize("case,pairs", [("case14test", 91), ("case30test", 703), ("case118", 15576), ("case300", 51681)])
def test_dense_screen_against_the_rebuild_route_every_pair(jg, case, pairs):
    t = load_case(case)
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    res = jg.dcPairScreen(s, rating=rating, dense=True)
    cand = res.candidates - 1
    nk = cand.size
    assert nk * (nk - 1) // 2 == pairs == res.totals["pairs"]
    base = P.base_components(t)
    oracle, worst, big_isl, small_ok = set(), 0.0, 0.0, np.inf
    for i in range(nk):
        for j in range(i + 1, nk):
            isl, dev = check_pair(t, rating, int(cand[i]), int(cand[j]), res.loading[i, j], int(res.branch[i, j]), base)
            det = abs(res.determinant[i, j])
            if isl:
                oracle.add((int(cand[i]) + 1, int(cand[j]) + 1))
                big_isl = max(big_isl, det)
            else:
                small_ok = min(small_ok, det)
                worst = max(worst, dev)
    print(case, "pairs", pairs, "islanding", len(oracle), "largest |det| islanding", big_isl, "smallest |det| others", small_ok, "worst loading deviation", worst)
    assert {tuple(int(x) for x in r) for r in res.islanding} == oracle and res.totals["islanding"] == len(oracle) and not res.islandingOverflow
    assert big_isl * 100 <= P.SINGULAR <= small_ok / 100           # two decades on either side of DC_SINGULAR, on the device's own determinants


def test_the_record_list_is_what_the_dense_matrix_implies(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    first = jg.dcPairScreen(s, rating=rating, dense=True)
    nk = first.candidates.size
    thr = float(np.nanmedian(first.loading[np.triu_indices(nk, 1)]))     # a threshold that splits the pairs: about half of them violate it
    res = jg.dcPairScreen(s, rating=rating, threshold=thr, dense=True)
    cand = res.candidates
    assert np.array_equal(res.loading, first.loading, equal_nan=True) and np.array_equal(res.branch, first.branch)
    want = [(cand[i], cand[j], res.branch[i, j], res.loading[i, j], res.count[i, j]) for i in range(nk) for j in range(i + 1, nk) if res.loading[i, j] > thr]
    assert 10 < len(want) < res.totals["pairs"] and res.totals["violating"] == len(want) and not res.overflow
    assert np.array_equal(res.records, np.array(want, dtype=np.float64))          # same pairs, same order, same counts, bit for bit
    # the count is the number of monitored branches above the threshold
    for r in res.records[:: max(1, len(want) // 20)]:
        _, fr = P.pair_solve(t, int(r[0]) - 1, int(r[1]) - 1)
        load = P.loading(fr, rating)[2]
        near = np.abs(load - thr) <= 1e-9 * max(1.0, load.max())
        assert int((load > thr).sum()) - int(near.sum()) <= int(r[4]) <= int((load > thr).sum()) + int(near.sum())
    # per candidate: the worst loading over all its pairs
    full = np.where(np.isnan(res.loading), 0.0, res.loading)
    assert np.array_equal(res.worst, full.max(axis=1))
    # a list that overflows keeps the FIRST records by (k, l), the totals stay exact
    cut = jg.dcPairScreen(s, rating=rating, threshold=thr, capacity=7, islandCapacity=5, block=13)
    assert cut.overflow and cut.islandingOverflow and cut.totals == res.totals
    assert np.array_equal(cut.records, res.records[:7]) and np.array_equal(cut.islanding, res.islanding[:5])
    assert np.array_equal(cut.worst, res.worst)


def _sample(jg, t, s, seed):
    """32 seeded candidates of a large grid that include two pairs of branches at a common bus"""
    cand = jg.pairCandidates(s)
    rng = np.random.default_rng(seed)
    pick = set(int(x) for x in rng.choice(cand, 28, replace=False))
    f, to = np.asarray(t["br_from"]), np.asarray(t["br_to"])
    at = {}
    for lab in cand:
        for bus in (int(f[lab - 1]), int(to[lab - 1])):
            at.setdefault(bus, []).append(int(lab))
    shared = [v for v in at.values() if len(v) >= 2]
    for v in (shared[len(shared) // 3], shared[2 * len(shared) // 3]):
        pick.update(v[:2])
    pool = iter(int(x) for x in cand if int(x) not in pick)
    while len(pick) < 32:
        pick.add(next(pool))
    return np.array(sorted(pick), dtype=np.int64)


@pytest.mark.parametrize("case", ["case_ACTIVSg10k", "case9241synth"])
def test_large_grid_sampled_pairs_row_blocks_and_repeatability(jg, case):
    t = load_case(case)
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    base = P.base_components(t)
    an = jg.dcPowerFlow(s)
    # (a) every pair of 32 seeded candidates, all branches monitored
    sample = _sample(jg, t, s, 11)
    res = jg.dcPairScreen(an, candidates=sample, rating=rating, dense=True)
    f, to = np.asarray(t["br_from"]), np.asarray(t["br_to"])
    share = sum(1 for i in range(32) for j in range(i + 1, 32) if {f[sample[i] - 1], to[sample[i] - 1]} & {f[sample[j] - 1], to[sample[j] - 1]})
    assert sample.size == 32 and share >= 2 and res.totals["pairs"] == 496
    worst, big_isl, small_ok, n_isl = 0.0, 0.0, np.inf, 0
    for i in range(32):
        for j in range(i + 1, 32):
            isl, dev = check_pair(t, rating, int(sample[i]) - 1, int(sample[j]) - 1, res.loading[i, j], int(res.branch[i, j]), base)
            det = abs(res.determinant[i, j])
            n_isl += isl
            big_isl, small_ok, worst = (max(big_isl, det), small_ok, worst) if isl else (big_isl, min(small_ok, det), max(worst, dev))
    print(case, "sample: islanding", n_isl, "largest |det| islanding", big_isl, "smallest |det| others", small_ok, "worst loading deviation", worst)
    assert small_ok >= 100 * P.SINGULAR and big_isl * 100 <= P.SINGULAR
    # the detail path on the same pairs: the worst loading of a two-outage lane (jg_dc_screen)
    pairs = [(int(sample[i]), int(sample[j])) for i in range(32) for j in range(i + 1, 32)][::5]
    lanes = jg.contingencyAnalysis(s, pairs, method="dc", rating=rating)
    for (a, b), rec in zip(pairs, lanes.screen):
        want = res.loading[list(sample).index(a), list(sample).index(b)]
        assert (rec[4] == 3 and np.isnan(want)) or abs(rec[0] - want) <= TOL * max(1.0, want), (a, b, rec, want)
    lanes.close()
    # (b) the whole grid: a row block of 8 candidates against ALL l, one pair per lane group of 64 l, against the rebuild route
    cand = jg.pairCandidates(s)
    nk = cand.size
    k0 = 3 * nk // 7
    blk = jg.dcPairScreen(an, rating=rating, rows=(k0, k0 + 8), dense=True)
    rng = np.random.default_rng(5)
    groups, worst_b = 0, 0.0
    for g in range((k0 + 8) // 64 + 1, (nk + 63) // 64):
        l = int(rng.integers(g * 64, min(g * 64 + 64, nk)))
        i = int(rng.integers(0, 8))
        isl, dev = check_pair(t, rating, int(cand[k0 + i]) - 1, int(cand[l]) - 1, blk.loading[i, l], int(blk.branch[i, l]), base)
        groups += 1
        worst_b = max(worst_b, dev)
    print(case, "row block: lane groups sampled", groups, "worst loading deviation", worst_b, blk.info)
    assert groups >= 64
    # the row-blocked result is bitwise the one-call result, and two runs are bitwise equal
    one = jg.dcPairScreen(an, rating=rating, rows=(k0, k0 + 8), dense=True, block=8)
    three = jg.dcPairScreen(an, rating=rating, rows=(k0, k0 + 8), dense=True, block=3)
    for name in ("loading", "branch", "count", "determinant"):
        assert np.array_equal(getattr(one, name), getattr(three, name), equal_nan=True), name
        assert np.array_equal(getattr(one, name), getattr(blk, name), equal_nan=True), name
    assert np.array_equal(one.records, three.records) and np.array_equal(one.worst, three.worst) and one.totals == three.totals
    # (c) ALL pairs of the default candidate list, twice
    a = jg.dcPairScreen(an, rating=rating, capacity=4096)
    b = jg.dcPairScreen(an, rating=rating, capacity=4096)
    print(case, "all pairs", a.totals, "records kept", len(a.records), "overflow", a.overflow)
    assert a.totals["pairs"] == nk * (nk - 1) // 2 and a.totals == b.totals
    assert np.array_equal(a.records, b.records) and np.array_equal(a.islanding, b.islanding) and np.array_equal(a.worst, b.worst)
    rows = a.records[(a.records[:, 0] >= cand[k0]) & (a.records[:, 0] < cand[k0 + 8])]
    assert np.array_equal(rows, one.records[:len(rows)])          # the full screen's records of that row block are the block's own
    an.close()


def _mixed_batch(jg, t, s, seed, lanes=96):
    """base case, single outages, pairs and lanes with injections of their own, mixed over two lane groups"""
    rng = np.random.default_rng(seed)
    cand = jg.pairCandidates(s)
    labels = []
    for i in range(lanes):
        kind = i % 4
        a, b = (int(x) for x in rng.choice(cand, 2, replace=False))
        labels.append(0 if kind == 0 else a if kind == 1 else (a, b))
    base = s.bus.supply.active - s.bus.demand.active
    own = {i: base * (1.0 + 0.1 * rng.standard_normal(base.size)) for i in (2, 3, 5, 70, 71)}
    return labels, own


@pytest.mark.parametrize("case", ["case118", "case300"])
def test_two_outage_lanes_against_the_rebuild_route(jg, case):
    t = load_case(case)
    s = jg.powerSystem(t)
    labels, own = _mixed_batch(jg, t, s, 21)
    comp = P.base_components(t)
    an = jg.dcPowerFlow(s, batch=len(labels))
    jg.setOutages_(an, labels)
    for lane, p in own.items():
        jg.setInjection_(an, np.array([p]), scenario0=lane)
    jg.solve_(an)
    jg.power_(an)
    wa = wf = 0.0
    n_pairs = n_isl = 0
    for i, lab in enumerate(labels):
        inj = own.get(i)
        if isinstance(lab, tuple):
            n_pairs += 1
            k, l = lab[0] - 1, lab[1] - 1
            if P.islands(t, k, l, comp):
                n_isl += 1
                assert an.status[i] == 3 and np.all(np.isnan(an.voltage.angle[i]))
                continue
            rth, rfr = P.pair_solve(t, k, l, injection=inj)
            assert an.power.from_.active[i, k] == 0.0 and an.power.from_.active[i, l] == 0.0
        else:
            rth, rfr = R.solve(t, out=lab - 1 if lab else None, injection=inj)
        assert an.status[i] == 0, (i, lab)
        a, f = R.worst(an.voltage.angle[i], rth), R.worst(an.power.from_.active[i], rfr)
        assert a <= TOL and f <= TOL, (i, lab, a, f)
        wa, wf = max(wa, a), max(wf, f)
    print(case, "two-outage lanes", n_pairs, "islanding", n_isl, "worst angle", wa, "worst flow", wf)
    assert n_pairs >= 40
    # slack bookkeeping of power! on a pair lane with injections of its own
    i = 70 if isinstance(labels[70], tuple) else 71
    k, l = labels[i][0] - 1, labels[i][1] - 1
    if an.status[i] == 0:
        t2 = dict(t)
        t2["br_status"] = np.array(t["br_status"]).copy()
        t2["br_status"][l] = 0
        pw = R.power(t2, P.pair_solve(t, k, l, injection=own[i])[0], out=k, injection=own[i])
        for name in ("injection", "supply", "generator"):
            assert R.worst(getattr(an.power, name).active[i], pw[name]) <= TOL, name
    an.close()


def test_an_islanding_pair_leaves_its_neighbours_bitwise_alone(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    scr = jg.dcPairScreen(s, rating=np.ones(s.branch.number))
    assert scr.totals["islanding"] == 74
    cut = tuple(int(x) for x in scr.islanding[len(scr.islanding) // 2])
    assert not jg.bridges(s)[cut[0] - 1] and not jg.bridges(s)[cut[1] - 1]     # neither branch alone is a bridge
    labels, _ = _mixed_batch(jg, t, s, 4)
    with_cut, without = list(labels), list(labels)
    with_cut[50], without[50] = cut, 0
    a = jg.contingencyAnalysis(s, with_cut, method="dc")
    b = jg.contingencyAnalysis(s, without, method="dc")
    assert a.status[50] == 3 and np.all(np.isnan(a.voltage.angle[50]))
    keep = np.arange(len(labels)) != 50
    assert np.array_equal(np.asarray(a.status)[keep], np.asarray(b.status)[keep])
    assert np.array_equal(a.voltage.angle[keep], b.voltage.angle[keep], equal_nan=True)
    jg.power_(a)
    jg.power_(b)
    assert np.array_equal(a.power.from_.active[keep], b.power.from_.active[keep], equal_nan=True)
    a.close()
    b.close()


def test_single_outages_take_the_one_outage_path_bit_for_bit(jg):
    t = load_case("case300")
    s = jg.powerSystem(t)
    labels = [int(x) for x in jg.outageList(s, 130)]
    labels[7] = 0
    plain = jg.contingencyAnalysis(s, labels, method="dc")
    jg.power_(plain)
    # (k, 0) tuples: no second outage is ever set
    tup = jg.contingencyAnalysis(s, [(k, 0) for k in labels], method="dc")
    # a handle that held pairs, then gets plain labels again
    cand = jg.pairCandidates(s)
    was = jg.dcPowerFlow(s, batch=130)
    jg.setOutages_(was, [(int(cand[3]), int(cand[40]))] * 130)
    jg.solve_(was)
    jg.setOutages_(was, labels)
    jg.solve_(was)
    # singles beside a pair in ANOTHER lane group, and in the same one
    mixed = list(labels)
    mixed[100] = (int(cand[3]), int(cand[40]))
    mix = jg.contingencyAnalysis(s, mixed, method="dc")
    for other in (tup, was, mix):
        jg.power_(other)
        keep = np.arange(130) != (100 if other is mix else -1)
        assert np.array_equal(np.asarray(other.status)[keep], np.asarray(plain.status)[keep])
        assert np.array_equal(other.voltage.angle[keep], plain.voltage.angle[keep])
        assert np.array_equal(other.power.from_.active[keep], plain.power.from_.active[keep])
        other.close()
    plain.close()


def test_screen_and_detail_path_agree(jg):
    t = load_case("case300")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    res = jg.dcPairScreen(s, rating=rating, dense=True)
    cand, nk = res.candidates, res.candidates.size
    rng = np.random.default_rng(9)
    idx = [(int(i), int(j)) for i, j in (sorted(rng.choice(nk, 2, replace=False)) for _ in range(200))]
    an = jg.contingencyAnalysis(s, [(int(cand[i]), int(cand[j])) for i, j in idx], method="dc", rating=rating)
    worst = 0.0
    for (i, j), rec in zip(idx, an.screen):
        want = res.loading[i, j]
        if np.isnan(want):
            assert rec[4] == 3
            continue
        assert rec[4] == 0
        dev = abs(rec[0] - want) / max(1.0, want)
        worst = max(worst, dev)
        assert dev <= TOL and (int(rec[1]) == int(res.branch[i, j]) or dev <= TOL), (i, j, rec, want)
    print("screen against detail path, 200 pairs of case300: worst deviation", worst)
    an.close()


def test_a_budget_too_small_for_the_sensitivities_fails_with_the_sizes(jg):
    t = load_case("case300")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    an = jg.dcPowerFlow(s, batch=3)
    with pytest.raises(jg._lib.JGridError, match=r"Phi needs \d+ bytes") as e:
        jg.dcPairScreen(an, rating=rating, budget=4096)
    assert e.value.code == 5 and "budget is 4096 bytes" in str(e.value)
    cand = [int(x) for x in jg.pairCandidates(s)]                    # (not bridges: a single outage of one of them islands nothing)
    pair = next((a, b) for a in cand[:20] for b in cand[20:40] if not P.islands(t, a - 1, b - 1))
    jg.setOutages_(an, [0, pair[0], pair])                           # the handle stays usable
    jg.solve_(an)
    assert np.all(np.asarray(an.status) == 0)
    assert R.worst(an.voltage.angle[2], P.pair_solve(t, pair[0] - 1, pair[1] - 1)[0]) <= TOL
    res = jg.dcPairScreen(an, rating=rating)
    assert res.totals["pairs"] == 51681 and res.info["phiBytes"] <= res.info["budgetBytes"] <= res.info["freeBytes"]
    an.close()


def test_the_new_exports_through_the_plain_c_abi(jg):
    """ctypes calls with raw pointers only: what a C driver does (include/jgrid.h)"""
    t = load_case("case14")
    (colptr, rowval, nzval), y, psh = R.model(t)
    n, nb = t["bus_type"].size, t["br_from"].size
    L = C.CDLL(jg._lib.LIB_PATH)
    L.jg_last_error.restype = C.c_char_p
    i64, f64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.jg_dc_create.argtypes = [i64, C.c_int64, i64, i64, f64, C.c_int64, C.c_double, C.c_int64, C.c_int]
    L.jg_dc_set_rhs.argtypes = [C.c_int64, f64]
    L.jg_dc_set_branches.argtypes = [C.c_int64, C.c_int64, i64, i64, f64, f64]
    L.jg_dc_set_rating.argtypes = [C.c_int64, f64]
    L.jg_dc_set_outage_pairs.argtypes = [C.c_int64, C.c_int64, C.c_int64, i64, i64]
    L.jg_dc_solve.argtypes = [C.c_int64]
    L.jg_dc_get_angle.argtypes = [C.c_int64, f64, i32]
    L.jg_dc_get_flows.argtypes = [C.c_int64, f64]
    L.jg_dc_pair_build.argtypes = [C.c_int64, C.c_int64, i64, C.c_int64, i64, C.c_int64, f64]
    L.jg_dc_pair_screen.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int64, f64, C.c_int64, i64, i64, f64, f64, i32, i32, f64]
    L.jg_dc_pair_time_kernel.argtypes = [C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, f64]
    L.jg_dc_pair_release.argtypes = [C.c_int64]
    L.jg_dc_destroy.argtypes = [C.c_int64]
    L.jg_dc_destroy.restype = None
    arr = lambda a, ct: (ct * len(a))(*a)
    h = C.c_int64(0)
    slack = R.slack_of(t)
    assert L.jg_dc_create(C.byref(h), n, arr(colptr.tolist(), C.c_int64), arr(rowval.tolist(), C.c_int64), arr(nzval.tolist(), C.c_double), slack + 1,
                          float(t["bus_va"][slack]), 2, 0) == 0, L.jg_last_error()
    cand = [int(x) for x in jg.pairCandidates(jg.powerSystem(t))]
    nk = len(cand)
    info = (C.c_double * 8)()
    assert L.jg_dc_pair_build(h, nk, arr(cand, C.c_int64), 0, None, 0, info) == 1                 # no branches yet: a bad argument, not a crash
    assert L.jg_dc_set_rhs(h, arr(R.rhs_of(t, psh).tolist(), C.c_double)) == 0
    assert L.jg_dc_set_branches(h, nb, arr([int(x) for x in t["br_from"]], C.c_int64), arr([int(x) for x in t["br_to"]], C.c_int64),
                                arr(y.tolist(), C.c_double), arr([float(x) for x in t["br_shift"]], C.c_double)) == 0
    rating = P.rating_of(t)
    tot, rec, isl = (C.c_int64 * 6)(), (C.c_double * (5 * 256))(), (C.c_int64 * (2 * 64))()
    assert L.jg_dc_pair_screen(h, 0, 1, 1.0, 256, rec, 64, isl, tot, None, None, None, None, None) == 4  # no build yet
    assert L.jg_dc_pair_build(h, nk, arr(cand, C.c_int64), 0, None, 0, info) == 0, L.jg_last_error()
    assert info[0] >= nk and info[1] == 64 and info[2] == info[0] * 64 * 8
    assert L.jg_dc_pair_screen(h, 0, nk - 1, 1.0, 256, rec, 64, isl, tot, None, None, None, None, None) == 1   # no rating yet
    assert L.jg_dc_set_rating(h, arr(rating.tolist(), C.c_double)) == 0
    worst, dl, db = (C.c_double * nk)(), (C.c_double * ((nk - 1) * nk))(), (C.c_int32 * ((nk - 1) * nk))()
    assert L.jg_dc_pair_screen(h, 0, nk - 1, 0.0, 256, rec, 64, isl, tot, worst, dl, db, None, None) == 0, L.jg_last_error()
    assert tot[0] == nk * (nk - 1) // 2 and tot[1] + tot[2] == tot[0] == tot[3] + tot[4] and tot[5] == 0      # threshold 0: every pair is a record or islanding
    base = P.base_components(t)
    r = np.array(rec[:5 * tot[3]]).reshape(-1, 5)
    assert np.all(np.diff(r[:, 0] * 1000 + r[:, 1]) > 0)           # sorted by (k, l)
    for row in r:
        check_pair(t, rating, int(row[0]) - 1, int(row[1]) - 1, row[3], int(row[2]), base)
    ms = (C.c_double * 3)()
    assert L.jg_dc_pair_time_kernel(h, 0, 0, nk - 1, 3, ms) == 0 and min(ms[:]) > 0
    # a lane with two outages through the raw call
    a, b = int(r[0, 0]), int(r[0, 1])
    assert L.jg_dc_set_outage_pairs(h, 0, 2, arr([a, a], C.c_int64), arr([b, 0], C.c_int64)) == 0
    assert L.jg_dc_set_outage_pairs(h, 0, 1, arr([a], C.c_int64), arr([a], C.c_int64)) == 1      # the same branch twice
    assert L.jg_dc_solve(h) == 0, L.jg_last_error()
    th, st, fr = (C.c_double * (2 * n))(), (C.c_int32 * 2)(), (C.c_double * (2 * nb))()
    assert L.jg_dc_get_angle(h, th, st) == 0 and L.jg_dc_get_flows(h, fr) == 0
    rth, rfr = P.pair_solve(t, a - 1, b - 1)
    assert st[0] == 0 and R.worst(np.array(th[:n]), rth) <= TOL and R.worst(np.array(fr[:nb]), rfr) <= TOL
    rth, rfr = R.solve(t, out=a - 1)
    assert st[1] == 0 and R.worst(np.array(th[n:]), rth) <= TOL and R.worst(np.array(fr[nb:]), rfr) <= TOL
    assert L.jg_dc_pair_release(h) == 0 and L.jg_dc_pair_release(h) == 0
    L.jg_dc_destroy(h)
    assert L.jg_dc_pair_release(C.c_int64(0)) == 1 and L.jg_dc_set_outage_pairs(C.c_int64(0), 0, 0, None, None) == 1
