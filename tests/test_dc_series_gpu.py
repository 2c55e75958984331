"""The DC N-1 screen over a series of injection profiles (dcSeriesScreen, csrc/jg_dc_series.hip) on the device, against the rebuild route of
tests/dc_series_reference.py: dc_reference.solve(t, out=k, injection=p) -- rebuild and refactorise for every case, never the compensation.  Bridges are
held against the graph oracle (connected components), not against any linear algebra.

Tolerance of every comparison: |got - ref| <= 1e-9 * max(1, |ref worst loading|), as in tests/test_dc_gpu.py; a worst-branch index may differ from the
reference's only where the two loadings agree within it, a count only by the number of branches within it of the threshold (tests/test_dc_pair_gpu.py).
No case is skipped.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_pair_reference as P
import dc_series_reference as S
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9


def check_case(t, rating, k, p, got_load, got_branch, got_count=None, thr=1.0, monitored=None):
    """one case (0-based branch k, not a bridge; profile p) of a screen against the rebuild route; returns the scaled deviation"""
    _, fr = S.rebuild(t, k, p)
    assert fr is not None, k
    w, b, load = P.loading(fr, rating, monitored)
    scale = max(1.0, w)
    dev = abs(got_load - w) / scale
    assert dev <= TOL, (k, got_load, w, dev)
    # ties go to the lowest branch index; another index only where the two loadings agree within the tolerance
    assert got_branch == b or (got_branch >= 1 and abs(load[got_branch - 1] - w) <= TOL * scale), (k, got_branch, b)
    if got_count is not None:
        near = int((np.abs(load - thr) <= TOL * scale).sum())
        assert int((load > thr).sum()) - near <= got_count <= int((load > thr).sum()) + near, (k, got_count)
    return dev


def same(a, b, dense=True):
    """two results agree bit for bit"""
    names = ["records", "islanding", "worst", "worstProfile", "violatingProfile", "base"] + (["loading", "branch", "count"] if dense else [])
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in names) and a.totals == b.totals and a.overflow == b.overflow


@pytest.mark.parametrize("case,T,with_bridges", [("case14test", 130, True), ("case30test", 65, False), ("case118", 3, False), ("case300", 2, True)])
def test_dense_screen_against_the_rebuild_route_every_case(jg, case, T, with_bridges):
    t = load_case(case)
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    prof = S.profiles(t, T)
    res = jg.dcSeriesScreen(s, prof, rating=rating, dense=True)
    cand = res.candidates - 1
    bridge = S.bridges(t)
    assert res.loading.shape == (cand.size, T) and res.profiles == T and res.totals["cases"] == cand.size * T
    assert not np.isin(cand, bridge).any() and res.islanding.size == 0 and res.totals["islanding"] == 0
    worst = 0.0
    for i, k in enumerate(cand):
        for tt in range(T):
            worst = max(worst, check_case(t, rating, int(k), prof[tt], res.loading[i, tt], int(res.branch[i, tt]), int(res.count[i, tt])))
    print(case, "profiles", T, "candidates", cand.size, "cases", cand.size * T, "worst scaled deviation of the worst loading", worst)
    for tt in range(T):                                              # the base case of every profile
        _, fr = S.rebuild(t, None, prof[tt])
        w, b, load = P.loading(fr, rating)
        assert abs(res.base[tt, 0] - w) <= TOL * max(1.0, w), (tt, res.base[tt], w)
        assert int(res.base[tt, 1]) == b or abs(load[int(res.base[tt, 1]) - 1] - w) <= TOL * max(1.0, w)
        near = int((np.abs(load - 1.0) <= TOL * max(1.0, w)).sum())
        assert abs(int(res.base[tt, 2]) - int((load > 1.0).sum())) <= near
    if with_bridges:                                                 # ALL in-service branches as candidates: the bridges among them
        every = S.in_service(t) + 1
        full = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, dense=True)
        isb = np.isin(every - 1, bridge)
        print(case, "all in-service candidates", every.size, "bridges by the graph oracle", int(isb.sum()), "by the screen", full.islanding.size)
        assert isb.sum() > 0 and np.array_equal(full.islanding, every[isb]) and full.totals["islanding"] == int(isb.sum())
        assert np.isnan(full.loading[isb]).all() and not np.isnan(full.loading[~isb]).any()
        assert not np.isin(full.records[:, 0], every[isb]).any() and np.array_equal(full.worst[isb], np.zeros(int(isb.sum())))
        assert np.array_equal(every[~isb], res.candidates)
        assert np.array_equal(full.loading[~isb], res.loading) and np.array_equal(full.branch[~isb], res.branch) and np.array_equal(full.count[~isb], res.count)
        assert np.array_equal(full.worstProfile, res.worstProfile) and np.array_equal(full.violatingProfile, res.violatingProfile)


def test_agreement_with_the_lane_path(jg):
    """column t of the dense result = the batched N-1 lanes with setInjection_ of profile t: screenSummary_'s worst loading and its branch"""
    D = jg.dcpowerflow
    t = load_case("case118")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    prof = S.profiles(t, 3)
    res = jg.dcSeriesScreen(s, prof, rating=rating, dense=True)
    labels = [0] + [int(x) for x in res.candidates]
    worst = 0.0
    for tt in (0, 2):
        an = jg.dcPowerFlow(s, batch=len(labels))
        D.setOutages_(an, labels)
        D.setInjection_(an, np.tile(prof[tt], (len(labels), 1)))
        D.solve_(an)
        rec = D.screenSummary_(an, rating)
        an.close()
        assert (rec[:, 4] == 0).all()
        got = np.r_[res.base[tt, 0], res.loading[:, tt]]
        gotb = np.r_[res.base[tt, 1], res.branch[:, tt]]
        dev = np.abs(got - rec[:, 0]) / np.maximum(1.0, rec[:, 0])
        worst = max(worst, float(dev.max()))
        assert (dev <= TOL).all(), (tt, dev.max())
        for j in np.flatnonzero(gotb != rec[:, 1]):                   # another branch only on a tie within the tolerance
            _, fr = S.rebuild(t, None if j == 0 else labels[j] - 1, prof[tt])
            load = P.loading(fr, rating)[2]
            assert abs(load[int(gotb[j]) - 1] - load[int(rec[j, 1]) - 1]) <= TOL * max(1.0, rec[j, 0]), (tt, j)
    print("case118: lanes", len(labels), "x 2 profiles, worst scaled deviation screen - lane path", worst)


def test_the_record_list_is_what_the_dense_matrix_implies(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    T = 70
    prof = S.profiles(t, T)
    every = S.in_service(t) + 1                                       # (the bridges ride along: never in the records, aside in the column summaries)
    first = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, dense=True)
    thr = float(np.median(first.loading[np.isfinite(first.loading)]))   # a threshold that splits the cases: about half of them violate it
    res = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True)
    cand, nk = res.candidates, res.candidates.size
    assert np.array_equal(res.loading, first.loading, equal_nan=True) and np.array_equal(res.branch, first.branch)
    want = [(cand[i], tt, res.branch[i, tt], res.loading[i, tt], res.count[i, tt]) for i in range(nk) for tt in range(T) if res.loading[i, tt] > thr]
    print("case118: cases", res.totals["cases"], "threshold", thr, "violating", res.totals["violating"], "records", res.records.shape[0], "bridges", res.totals["islanding"])
    assert 10 < len(want) < res.totals["cases"] and res.totals["violating"] == len(want) and not res.overflow and res.totals["cases"] == nk * T
    assert np.array_equal(res.records, np.array(want, dtype=np.float64))          # same cases, same order, same counts, bit for bit
    for r in res.records[:: max(1, len(want) // 20)]:                 # the count is the number of monitored branches above the threshold
        check_case(t, rating, int(r[0]) - 1, prof[int(r[1])], r[3], int(r[2]), int(r[4]), thr)
    full = np.where(np.isnan(res.loading), 0.0, res.loading)
    assert res.totals["islanding"] == int(np.isnan(res.loading[:, 0]).sum()) > 0
    assert np.array_equal(res.worst, full.max(axis=1))
    assert np.array_equal(res.worstProfile, full.max(axis=0))
    assert np.array_equal(res.violatingProfile, (res.loading > thr).sum(axis=0)) and res.violatingProfile.dtype == np.int64
    # a list that overflows keeps the FIRST records by (k, t), the totals and the summaries stay exact
    cut = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, capacity=7, block=13)
    assert cut.overflow and cut.totals == res.totals and np.array_equal(cut.records, res.records[:7])
    for name in ("worst", "worstProfile", "violatingProfile", "base", "islanding"):
        assert np.array_equal(getattr(cut, name), getattr(res, name)), name


def test_results_do_not_depend_on_blocks_slices_other_profiles_or_other_screens(jg):
    D = jg.dcpowerflow
    t = load_case("case14test")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    T = 130
    prof = S.profiles(t, T)
    every = S.in_service(t) + 1
    thr = 0.4
    ref = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True)
    nk = every.size
    print("case14test: cases", ref.totals["cases"], "violating", ref.totals["violating"], "bridges", ref.totals["islanding"])
    assert 0 < ref.totals["violating"] < ref.totals["cases"]
    for block in (1, 5):                                              # (the default block is `ref`)
        assert same(jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True, block=block), ref), block
    for k0, k1 in ((0, 3), (3, 11), (11, nk), (5, 6)):                # a slice of the rows: an unaligned first row, one row, the tail
        part = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True, rows=(k0, k1), block=4)
        lab = every[k0:k1]
        assert part.rows == (k0, k1) and part.totals["cases"] == (k1 - k0) * T
        assert np.array_equal(part.loading, ref.loading[k0:k1], equal_nan=True) and np.array_equal(part.branch, ref.branch[k0:k1]) and np.array_equal(part.count, ref.count[k0:k1])
        assert np.array_equal(part.records, ref.records[np.isin(ref.records[:, 0], lab)]) and np.array_equal(part.islanding, ref.islanding[np.isin(ref.islanding, lab)])
        assert np.array_equal(part.worst[k0:k1], ref.worst[k0:k1]) and not part.worst[:k0].any() and not part.worst[k1:].any()
        assert np.array_equal(part.base, ref.base)
        sub = np.where(np.isnan(ref.loading[k0:k1]), 0.0, ref.loading[k0:k1])
        assert np.array_equal(part.worstProfile, sub.max(axis=0)) and np.array_equal(part.violatingProfile, (sub > thr).sum(axis=0))
    a, b = 3, 68                                                      # a subset of the profiles: columns a:b of the full screen
    part = jg.dcSeriesScreen(s, prof[a:b], candidates=every, rating=rating, threshold=thr, dense=True)
    assert np.array_equal(part.loading, ref.loading[:, a:b], equal_nan=True) and np.array_equal(part.branch, ref.branch[:, a:b]) and np.array_equal(part.count, ref.count[:, a:b])
    assert np.array_equal(part.base, ref.base[a:b]) and np.array_equal(part.worstProfile, ref.worstProfile[a:b]) and np.array_equal(part.violatingProfile, ref.violatingProfile[a:b])
    keep = (ref.records[:, 1] >= a) & (ref.records[:, 1] < b)
    assert np.array_equal(part.records, ref.records[keep] - np.array([0.0, a, 0.0, 0.0, 0.0]))
    # on one analysis beside the pair screen, in either order, and beside solved lanes: each result is what a fresh analysis gives
    pair_ref = jg.dcPairScreen(s, rating=rating, dense=True)
    an = jg.dcPowerFlow(s, batch=3)
    D.setOutages_(an, [0, int(ref.candidates[0]), int(ref.candidates[1])])
    D.setInjection_(an, prof[5:6], scenario0=2)
    D.solve_(an)
    angle = an.voltage.angle.copy()
    flows = np.zeros((3, s.branch.number))
    jg._lib.check(jg._lib.lib().jg_dc_get_flows(an._h, flows.reshape(-1)))
    pair_after = None
    for order in ("pair first", "series first"):
        if order == "pair first":
            pair_after = jg.dcPairScreen(an, rating=rating, dense=True)
        got = jg.dcSeriesScreen(an, prof, candidates=every, rating=rating, threshold=thr, dense=True)
        assert same(got, ref), order
        if order == "series first":
            pair_after = jg.dcPairScreen(an, rating=rating, dense=True)
        for name in ("records", "islanding", "worst", "loading", "branch", "count", "determinant"):
            assert np.array_equal(getattr(pair_after, name), getattr(pair_ref, name), equal_nan=True), (order, name)
    th = np.zeros((3, s.bus.number))
    st = np.zeros(3, dtype=np.int32)
    jg._lib.check(jg._lib.lib().jg_dc_get_angle(an._h, th.reshape(-1), st))
    fl = np.zeros_like(flows)
    jg._lib.check(jg._lib.lib().jg_dc_get_flows(an._h, fl.reshape(-1)))
    assert np.array_equal(th, angle, equal_nan=True) and np.array_equal(fl, flows, equal_nan=True)      # the handle's own lanes are untouched
    D.solve_(an)
    assert np.array_equal(an.voltage.angle, angle, equal_nan=True)
    an.close()


def _sample(jg, t, s, seed):
    """32 seeded candidates of a large grid that include two pairs of branches at a common bus (the shape of the pair test's sample)"""
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
def test_large_grid_sample(jg, case):
    t = load_case(case)
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    prof = S.profiles(t, 8)
    sample = _sample(jg, t, s, 11)
    an = jg.dcPowerFlow(s)
    res = jg.dcSeriesScreen(an, prof, candidates=sample, rating=rating, dense=True)
    assert sample.size == 32 and res.totals["cases"] == 256 and res.totals["islanding"] == 0
    worst = 0.0
    for i in range(32):
        for tt in range(8):
            worst = max(worst, check_case(t, rating, int(sample[i]) - 1, prof[tt], res.loading[i, tt], int(res.branch[i, tt]), int(res.count[i, tt])))
    print(case, "32 candidates x 8 profiles, all branches monitored: worst scaled deviation", worst)
    # a strict subset of the branches monitored: every third rated branch; half of the cases against the rebuild route
    mon = (np.flatnonzero((np.asarray(t["br_status"]) == 1) & (rating > 0)) + 1)[::3]
    sub = jg.dcSeriesScreen(an, prof, candidates=sample, monitored=mon, rating=rating, dense=True)
    an.close()
    assert 0 < mon.size < s.branch.number and np.isin(sub.branch[sub.branch > 0], mon).all()
    worst_m = 0.0
    for i in range(0, 32, 2):
        for tt in range(8):
            worst_m = max(worst_m, check_case(t, rating, int(sample[i]) - 1, prof[tt], sub.loading[i, tt], int(sub.branch[i, tt]), int(sub.count[i, tt]), monitored=mon - 1))
    print(case, "monitored", mon.size, "of", s.branch.number, "branches: worst scaled deviation", worst_m)


def test_a_budget_too_small_is_refused_with_the_sizes(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    prof = S.profiles(t, 70)
    an = jg.dcPowerFlow(s)
    first = jg.dcSeriesScreen(an, prof, rating=rating)
    need = first.info["phiBytes"] + first.info["f0Bytes"]
    print("case118, 70 profiles: Phi", first.info["phiBytes"], "bytes, F0", first.info["f0Bytes"], "bytes")
    assert first.info["f0Bytes"] == first.info["rows"] * 128 * 8
    for budget in (int(first.info["phiBytes"]) + 4096, int(need) - 8):      # Phi alone would fit; Phi + F0 without their scratch would not
        with pytest.raises(jg._lib.JGridError) as e:
            jg.dcSeriesScreen(an, prof, rating=rating, budget=budget)
        print(e.value)
        assert e.value.code == 5 and "Phi needs" in str(e.value) and "F0 needs" in str(e.value) and str(int(first.info["f0Bytes"])) in str(e.value)
    again = jg.dcSeriesScreen(an, prof, rating=rating)                  # the analysis still works afterwards
    assert same(again, first, dense=False)
    an.close()
