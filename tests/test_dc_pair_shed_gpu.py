"""Pairs of the DC N-2 screen that hold a bridge, screened on the slack's island (dcPairScreen(..., islands="shed"), csrc/jg_dc_pair.hip) on the device,
against the rebuild route of tests/dc_pair_shed_reference.py: the model of the slack's component with both branches deleted, rebuilt and refactorised for
every pair, never the identity the kernel uses.  Which branches are bridges, and what leaves with them, comes from the search of
tests/dc_series_shed_reference.py.

Tolerance of every comparison with the rebuild: |got - ref| <= 1e-9 * max(1, |ref|); a worst-branch index may differ from the reference's only where the
two loadings agree within it.  The count is held EXACTLY: the threshold of the hand grid (2.0) and of case14test (0.4) is checked, here on the host, to
have no reference loading within 1e-9 of it.  No case is skipped.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_island_reference as I
import dc_pair_reference as P
import dc_pair_shed_reference as Q
import dc_reference as R
import dc_series_shed_reference as H
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
FIELDS = ("records", "islanding", "worst", "loading", "branch", "count", "determinant")


def same(a, b, names=FIELDS):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in names) and a.totals == b.totals and a.overflow == b.overflow and \
        a.islandingOverflow == b.islandingOverflow


def check_pair(g, rating, k, l, got_load, got_branch, got_count, thr):
    """one pair (0-based branches) against the rebuild route; returns (scaled deviation, distance of the nearest reference loading from the threshold)"""
    fr, keep = Q.rebuild(g, k, l)
    w, b, load = P.loading(fr, rating)
    scale = max(1.0, w)
    dev = abs(got_load - w) / scale
    assert dev <= TOL, (k, l, got_load, w, dev)
    assert got_branch == b or (got_branch >= 1 and abs(load[got_branch - 1] - w) <= TOL * scale), (k, l, got_branch, b)
    gap = float(np.abs(load - thr).min()) / scale
    assert gap > TOL, (k, l, gap)                                 # the pinned threshold: no reference loading within the tolerance of it
    assert got_count == int((load > thr).sum()), (k, l, got_count, int((load > thr).sum()))
    if got_branch >= 1:                                            # a masked row is never the worst: both ends of the worst branch stayed
        assert keep[g.f[got_branch - 1]] and keep[g.to[got_branch - 1]], (k, l, got_branch)
    return dev, gap


_HAND = {}


def hand(jg):
    """the 200-bus grid, every in-service branch a candidate (272: five chunks of 64 lanes, bridges in tiles and in lanes), dense: computed once"""
    if not _HAND:
        t, marks, _ = I.hand_grid()
        s = jg.powerSystem(t)
        rating = Q.hand_rating(t)
        every = jg.shedCandidates(s)
        thr = 2.0                                                 # splits the pairs: the reference's worst loadings run from 0.8 to 10.5, 798 of the sample's 1482 above it
        res = jg.dcPairScreen(s, candidates=every, rating=rating, threshold=thr, dense=True, islands="shed")
        br = H.bridges(t)
        _HAND.update(t=t, marks=marks, s=s, rating=rating, every=every, thr=thr, res=res, br=br, g=Q.Grid(t), cols=Q.sample(t, br, None, 40))
    return _HAND


def test_hand_grid_sample_against_the_rebuild_route(jg):
    h = hand(jg)
    t, res, br, g, every, cols, thr = h["t"], h["res"], h["br"], h["g"], h["every"], h["cols"], h["thr"]
    lab = np.array(sorted(br)) + 1
    print("hand grid: candidates", every.size, "bridges by the search", lab.size, "shed by the screen", res.shed.size, "pairs", res.totals["pairs"],
          "violating", res.totals["violating"], "still status 3", res.totals["islanding"])
    assert every.size > 4 * 64 and np.array_equal(res.shed, lab) and res.totals["pairs"] == every.size * (every.size - 1) // 2
    assert res.shed.dtype == np.int64 and res.shedBuses.dtype == np.int64 and res.shedFlow.shape == (lab.size,)
    pos = {int(k): int(np.flatnonzero(every == k + 1)[0]) for k in cols}
    worst, gap, kinds = 0.0, 1.0, {}
    for a in range(cols.size):
        for b in range(a + 1, cols.size):
            k, l = int(cols[a]), int(cols[b])
            kd = Q.kind(br, g, k, l)
            i, j = pos[k], pos[l]
            if kd == "plain" and Q.joint_cut(g, k, l):
                assert np.isnan(res.loading[i, j]) and res.branch[i, j] == 0 and res.count[i, j] == 0, (k, l)
                kinds["cut"] = kinds.get("cut", 0) + 1
                continue
            kinds[kd] = kinds.get(kd, 0) + 1
            assert res.loading[i, j] == res.loading[j, i]          # (the dense result is mirrored)
            d, gp = check_pair(g, h["rating"], k, l, res.loading[i, j], int(res.branch[i, j]), int(res.count[i, j]), thr)
            worst, gap = max(worst, d), min(gap, gp)
    print("hand grid sample:", cols.size, "candidates, pairs by kind", kinds, "worst scaled deviation", worst, "nearest loading to the threshold", gap)
    assert all(kinds.get(kd, 0) > 0 for kd in ("plain", "outside", "inside", "disjoint", "nested"))
    # every pair with a bridge is finite, and status 3 is left to the joint cuts of two non-bridges
    isb = np.isin(every, lab)
    either = isb[:, None] | isb[None, :]
    off = ~np.eye(every.size, dtype=bool)
    assert not np.isnan(res.loading[either & off]).any()
    assert res.totals["islanding"] == int(np.isnan(res.loading[~either & off]).sum()) // 2 == res.islanding.shape[0]
    assert not np.isin(res.islanding, lab).any()


def test_pairs_of_two_non_bridges_and_calls_without_the_keyword_are_bitwise_what_they_were(jg):
    h = hand(jg)
    s, every, rating, thr, res = h["s"], h["every"], h["rating"], h["thr"], h["res"]
    plain = jg.pairCandidates(s)
    fresh = jg.dcPairScreen(s, candidates=plain, rating=rating, threshold=thr, dense=True)       # an analysis no shed-mode screen ever ran on
    assert fresh.shed is None and fresh.shedFlow is None and fresh.recordShed is None
    at = np.searchsorted(every, plain)
    assert np.array_equal(every[at], plain) and plain.size < every.size
    for name in ("loading", "branch", "count", "determinant"):
        assert np.array_equal(getattr(res, name)[np.ix_(at, at)], getattr(fresh, name), equal_nan=True), name
    assert np.array_equal(res.islanding, fresh.islanding)
    keep = np.isin(res.records[:, 0], plain) & np.isin(res.records[:, 1], plain)
    assert np.array_equal(res.records[keep], fresh.records) and not res.recordShed[keep].any() and (res.recordShed[~keep] != 0).any(axis=1).all()
    an = jg.dcPowerFlow(s)
    before = jg.dcPairScreen(an, candidates=plain, rating=rating, threshold=thr, dense=True)
    shed = jg.dcPairScreen(an, candidates=every, rating=rating, threshold=thr, dense=True, islands="shed")
    after = jg.dcPairScreen(an, candidates=plain, rating=rating, threshold=thr, dense=True)
    every_skip = jg.dcPairScreen(an, candidates=every, rating=rating, threshold=thr, dense=True)     # the mode does not leak: a bridge pair is status 3 again
    an.close()
    assert same(before, fresh) and same(after, fresh) and same(shed, res) and np.array_equal(shed.shedFlow, res.shedFlow)
    isb = np.isin(every, res.shed)
    assert every_skip.shed is None and np.isnan(every_skip.loading[isb][:, ~isb]).all()
    assert np.array_equal(every_skip.loading[np.ix_(at, at)], fresh.loading, equal_nan=True)


_C300 = {}


def edges(jg):
    """case300, 130 candidates chosen so that bridges sit at the positions 0, 3, 63 (tile positions 0 and 3, lanes 0 and 63 of the first chunk) and 64, 67,
    127 (the same of the second), non-bridges everywhere else; a third chunk of two lanes"""
    if not _C300:
        t = load_case("case300")
        s = jg.powerSystem(t)
        br = H.bridges(t)
        every = jg.shedCandidates(s)
        want = {0, 3, 63, 64, 67, 127}
        cand, last = [], 0
        for p in range(130):
            pick = next(int(x) for x in every if x > last and ((int(x) - 1 in br) == (p in want)))
            cand.append(pick)
            last = pick
        cand = np.array(cand, dtype=np.int64)
        rating = P.rating_of(t)
        ref = jg.dcPairScreen(s, candidates=cand, rating=rating, threshold=1.0, dense=True, islands="shed", block=200)
        _C300.update(t=t, s=s, br=br, cand=cand, rating=rating, ref=ref, want=sorted(want))
    return _C300


def test_block_and_tile_edges_are_bitwise_the_single_block_call(jg):
    c = edges(jg)
    s, cand, rating, ref, br, t = c["s"], c["cand"], c["rating"], c["ref"], c["br"], c["t"]
    isb = np.array([int(x) - 1 in br for x in cand])
    print("case300: candidates", cand.size, "bridges at positions", np.flatnonzero(isb), "pairs", ref.totals["pairs"], "violating", ref.totals["violating"],
          "status 3", ref.totals["islanding"])
    assert np.array_equal(np.flatnonzero(isb), c["want"]) and np.array_equal(ref.shed, cand[isb])
    g = Q.Grid(t)
    worst = 0.0
    near = [p for p in range(cand.size) if isb[p] or p in (1, 2, 62, 65, 126, 128, 129)]      # the bridges and the non-bridges beside them
    for a in near:
        for b in near:
            if a < b:
                k, l = int(cand[a]) - 1, int(cand[b]) - 1
                if Q.kind(br, g, k, l) == "plain" and Q.joint_cut(g, k, l):
                    assert np.isnan(ref.loading[a, b])
                    continue
                fr, _ = Q.rebuild(g, k, l)
                w, bb, load = P.loading(fr, rating)
                dev = abs(ref.loading[a, b] - w) / max(1.0, w)
                assert dev <= TOL, (a, b, ref.loading[a, b], w)
                worst = max(worst, dev)
    print("case300:", len(near), "positions around the bridges, every pair of them: worst scaled deviation", worst)
    for block in (1, 3):
        r = jg.dcPairScreen(s, candidates=cand, rating=rating, threshold=1.0, dense=True, islands="shed", block=block)
        assert same(r, ref), block
        assert np.array_equal(r.shedFlow, ref.shedFlow) and np.array_equal(r.recordShed, ref.recordShed)
    for k0, k1, block in ((1, 130, None), (3, 66, 5), (62, 63, 1), (65, 129, 3)):
        r = jg.dcPairScreen(s, candidates=cand, rating=rating, threshold=1.0, dense=True, islands="shed", rows=(k0, k1), block=block)
        k1 = min(k1, cand.size - 1)
        assert k0 % 4 != 0
        for name in ("loading", "branch", "count", "determinant"):
            full = np.triu(getattr(ref, name), 1)[k0:k1]           # a block comes back as screened: 0 where l <= k
            assert np.array_equal(getattr(r, name), full, equal_nan=True), (k0, k1, name)
        rows = np.isin(ref.records[:, 0], cand[k0:k1])
        assert np.array_equal(r.records, ref.records[rows]) and np.array_equal(r.recordShed, ref.recordShed[rows])
        assert np.array_equal(r.shed, ref.shed) and np.array_equal(r.shedFlow, ref.shedFlow)          # one entry per bridge among ALL candidates


def test_case14test_every_pair(jg):
    t = load_case("case14test")
    s = jg.powerSystem(t)
    g = Q.Grid(t)
    br = H.bridges(t)
    rating = P.rating_of(t)
    every = jg.shedCandidates(s)
    thr = 0.4
    res = jg.dcPairScreen(s, candidates=every, rating=rating, threshold=thr, dense=True, islands="shed")
    cuts, worst, kinds = [], 0.0, {}
    for i in range(every.size):
        for j in range(i + 1, every.size):
            k, l = int(every[i]) - 1, int(every[j]) - 1
            kd = Q.kind(br, g, k, l)
            if kd == "plain" and Q.joint_cut(g, k, l):
                cuts.append((k + 1, l + 1))
                assert np.isnan(res.loading[i, j])
                continue
            kinds[kd] = kinds.get(kd, 0) + 1
            worst = max(worst, check_pair(g, rating, k, l, res.loading[i, j], int(res.branch[i, j]), int(res.count[i, j]), thr)[0])
    print("case14test: candidates", every.size, "bridges", len(br), "pairs by kind", kinds, "joint cuts of two non-bridges", len(cuts), "worst scaled deviation", worst)
    assert len(cuts) > 0 and np.array_equal(res.islanding, np.array(cuts, dtype=np.int64).reshape(-1, 2)) and res.totals["islanding"] == len(cuts)
    assert np.array_equal(res.shed, np.array(sorted(br)) + 1)


def test_shed_flow_against_the_base_flows(jg):
    h = hand(jg)
    t, res, br, marks = h["t"], h["res"], h["br"], h["marks"]
    _, f0, _ = I.solve(t)
    f, to = np.asarray(t["br_from"]) - 1, np.asarray(t["br_to"]) - 1
    slack = R.slack_of(t)
    worst = 0.0
    for j, k in enumerate(sorted(br)):
        S, m, sgn = br[k]
        want = sgn * f0[k]
        dev = abs(res.shedFlow[j] - want) / max(1.0, abs(want))
        assert dev <= TOL and res.shedBuses[j] == int(S.sum()) and res.shedM[j] == m + 1, (k, res.shedFlow[j], want)
        worst = max(worst, dev)
    at = {name: int(np.flatnonzero(res.shed == marks[name][0] + 1)[0]) for name in ("at_slack", "pocket")}
    k = marks["pocket"][0]
    assert res.shedM[at["at_slack"]] == slack + 1 and res.shedFlow[at["at_slack"]] != 0                 # m at the slack: a zero column, the flow is still there
    assert res.shedM[at["pocket"]] == to[k] + 1 and t["br_shift"][k] != 0 and res.shedBuses[at["pocket"]] == 85      # m the to end, a shifter on the bridge
    print("hand grid:", len(br), "bridges: worst scaled deviation of the flow that left", worst)


def test_records_totals_worst_and_record_shed_with_a_list_that_overflows(jg):
    h = hand(jg)
    s, every, rating, thr, res, marks = h["s"], h["every"], h["rating"], h["thr"], h["res"], h["marks"]
    nk = every.size
    want = [(every[i], every[j], res.branch[i, j], res.loading[i, j], res.count[i, j]) for i in range(nk) for j in range(i + 1, nk) if res.loading[i, j] > thr]
    print("hand grid: pairs", res.totals["pairs"], "violating", res.totals["violating"], "records", res.records.shape[0])
    assert 0 < len(want) < res.totals["pairs"] and res.totals["violating"] == len(want) and not res.overflow
    assert np.array_equal(res.records, np.array(want, dtype=np.float64))          # sorted by (k, l), bit for bit what the dense matrix implies
    assert np.array_equal(res.worst, np.nanmax(res.loading, axis=1))
    assert res.recordShed.shape == (len(want), 2) and res.recordShed.dtype == np.int64
    assert np.array_equal(res.recordShed, jg.pairShed(s, res.records[:, :2]))
    isb = np.isin(every, res.shed)
    rs = {(int(a), int(b)): tuple(int(x) for x in q) for (a, b), q in zip(res.records[:, :2], res.recordShed)}
    chain, far = [k + 1 for k in marks["chain"]], [k + 1 for k in marks["far"]]
    for pair, q in (((chain[0], chain[1]), (chain[0], 0)), ((far[0], far[9]), (far[0], 0))):
        assert pair not in rs or rs[pair] == q
    assert all((q[0] in (0, a)) and (q[1] in (0, b)) for (a, b), q in rs.items())
    assert all((q[0] != 0 or q[1] != 0) == bool(isb[np.searchsorted(every, a)] or isb[np.searchsorted(every, b)]) for (a, b), q in rs.items())
    small = jg.dcPairScreen(s, candidates=every, rating=rating, threshold=thr, islands="shed", capacity=7, islandCapacity=2, block=50)
    assert small.overflow and small.totals == res.totals and np.array_equal(small.records, res.records[:7]) and np.array_equal(small.recordShed, res.recordShed[:7])
    assert small.islandingOverflow == (res.totals["islanding"] > 2) and np.array_equal(small.islanding, res.islanding[:2])
    assert np.array_equal(small.worst, res.worst) and np.array_equal(small.shedFlow, res.shedFlow)


def test_bad_input_and_a_mode_that_does_not_leak(jg):
    h = hand(jg)
    s, every, rating, marks, res = h["s"], h["every"], h["rating"], h["marks"], h["res"]
    with pytest.raises(ValueError):
        jg.dcPairScreen(s, rating=rating, islands="both")
    with pytest.raises(ValueError):                               # a candidate out of service still raises
        jg.dcPairScreen(s, candidates=np.r_[every[:5], marks["open_loop"][0] + 1], rating=rating, islands="shed")
    default = jg.dcPairScreen(s, rating=rating, islands="shed", rows=(0, 4))        # the default candidates: every in-service branch, bridges included
    assert np.array_equal(default.candidates, every) and np.array_equal(default.shed, res.shed)
    # the library's flag is the mode of the NEXT build alone, also when that build is refused
    an = jg.dcPowerFlow(s)
    jg.dcPairScreen(an, candidates=every, rating=rating, rows=(0, 1))               # (sets the right-hand side and the rating)
    L, n = jg._lib.lib(), np.zeros(1, dtype=np.int64)
    q = [np.zeros(every.size, dtype=np.int64) for _ in range(4)]
    info = np.zeros(8)
    jg._lib.check(L.jg_dc_pair_set_island_mode(an._h, 1))
    assert L.jg_dc_pair_build(an._h, 1, every[:1].copy(), 0, None, 0, info) != 0    # refused: two or more candidates
    jg._lib.check(L.jg_dc_pair_build(an._h, int(every.size), every, 0, None, 0, info))
    jg._lib.check(L.jg_dc_pair_get_shed_table(an._h, 0, int(every.size), n, *q))
    assert n[0] == 0
    jg._lib.check(L.jg_dc_pair_set_island_mode(an._h, 1))
    jg._lib.check(L.jg_dc_pair_build(an._h, int(every.size), every, 0, None, 0, info))
    jg._lib.check(L.jg_dc_pair_get_shed_table(an._h, 0, int(every.size), n, *q))
    assert n[0] == res.shed.size
    jg._lib.check(L.jg_dc_pair_build(an._h, int(every.size), every, 0, None, 0, info))
    jg._lib.check(L.jg_dc_pair_get_shed_table(an._h, 0, int(every.size), n, *q))
    assert n[0] == 0
    assert L.jg_dc_pair_set_island_mode(an._h, 2) != 0
    an.close()
