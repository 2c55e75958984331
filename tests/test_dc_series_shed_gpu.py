"""Bridge candidates of the DC series screen on the slack's island (dcSeriesScreen(..., islands="shed"), csrc/jg_dc_series.hip) on the device, against the
rebuild route dc_island_reference.solve(t, out=k, injection=p): the model of the slack's component alone, rebuilt and refactorised for every case, never
the identity the kernel uses.  Which branches are bridges, and what leaves with them, comes from the search of tests/dc_series_shed_reference.py.

Tolerance of every comparison: |got - ref| <= 1e-9 * max(1, |ref worst loading|); a worst-branch index may differ from the reference's only where the two
loadings agree within it, a count only by the number of branches within it of the threshold (tests/test_dc_series_gpu.py).  No case is skipped.  Every
figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_island_reference as I
import dc_pair_reference as P
import dc_reference as R
import dc_series_reference as S
import dc_series_shed_reference as H
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
NAMES = ("records", "islanding", "worst", "worstProfile", "violatingProfile", "base", "loading", "branch", "count")


def check_case(t, rating, k, p, got_load, got_branch, got_count, thr=1.0):
    """one case (0-based branch k, bridge or not; profile p) against the rebuild route on the slack's component; returns the scaled deviation"""
    _, fr, _ = I.solve(t, out=k, injection=p)
    w, b, load = P.loading(fr, rating)
    scale = max(1.0, w)
    dev = abs(got_load - w) / scale
    assert dev <= TOL, (k, got_load, w, dev)
    assert got_branch == b or (got_branch >= 1 and abs(load[got_branch - 1] - w) <= TOL * scale), (k, got_branch, b)
    near = int((np.abs(load - thr) <= TOL * scale).sum())
    assert int((load > thr).sum()) - near <= got_count <= int((load > thr).sum()) + near, (k, got_count)
    return dev


def same(a, b, names=NAMES):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in names) and a.totals == b.totals and a.overflow == b.overflow


def hand_rating(t):
    """ratings at the scale of each branch's own base flow (so that the worst branch differs from case to case), every seventh branch not rated"""
    r = 0.05 + 1.2 * np.abs(R.solve(t)[1])
    r[::7] = 0.0
    return r


_HAND = {}


def hand(jg):
    """the 200-bus grid, T = 65 (one chunk of 64 profiles full, one with a single profile), every in-service branch a candidate: computed once"""
    if not _HAND:
        t, marks, _ = I.hand_grid()
        s = jg.powerSystem(t)
        rating = hand_rating(t)
        prof = S.profiles(t, 65)
        every = S.in_service(t) + 1
        thr = 2.0                                                 # splits the cases: the seeded profiles load the grid between 1 and 7 times these ratings
        res = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True, islands="shed")
        _HAND.update(t=t, marks=marks, s=s, rating=rating, prof=prof, every=every, thr=thr, res=res, br=H.bridges(t))
    return _HAND


def test_every_bridge_case_of_the_hand_grid_against_the_rebuild_route(jg):
    h = hand(jg)
    t, res, br, prof, every, marks = h["t"], h["res"], h["br"], h["prof"], h["every"], h["marks"]
    lab = np.array(sorted(br)) + 1
    print("hand grid: candidates", every.size, "bridges by the search", lab.size, "shed by the screen", res.shed.size, "still status 3", res.islanding.size)
    assert np.array_equal(res.shed, lab) and res.islanding.size == 0 and res.totals["islanding"] == 0 and not np.isnan(res.loading).any()
    assert res.shed.dtype == np.int64 and res.shedBuses.dtype == np.int64 and res.shedFlow.shape == (lab.size, 65) and res.shedDemand is None and res.unserved is None
    f, to = np.asarray(t["br_from"]) - 1, np.asarray(t["br_to"]) - 1
    slack = R.slack_of(t)
    # the shapes the grid was built for
    at = {name: [int(np.flatnonzero(res.shed == k + 1)[0]) for k in marks[name] if k in br] for name in ("at_slack", "pocket", "chain", "behind_doubled", "far")}
    assert res.shedM[at["at_slack"][0]] == slack + 1                                        # m at the slack: a zero column
    k = marks["pocket"][0]
    assert res.shedBuses[at["pocket"][0]] == 85 and res.shedM[at["pocket"][0]] == to[k] + 1 and t["br_shift"][k] != 0      # m the to end, a shifter on the bridge
    assert sorted(res.shedBuses[at["chain"]]) == [1, 2] and sorted(res.shedBuses[at["far"]]) == list(range(1, 11))
    assert len(at["behind_doubled"]) == 1 and not any(k in br for k in marks["doubled"]) and marks["open_loop"][0] + 1 not in every
    worst = wg = 0.0
    F0 = S.base_flows(t, prof)
    ykk = R.admittance(t)
    for j, k in enumerate(sorted(br)):
        i = int(np.flatnonzero(every == k + 1)[0])
        Sk, m, sgn = br[k]
        assert res.shedBuses[j] == int(Sk.sum()) and res.shedM[j] == m + 1
        for tt in range(65):
            worst = max(worst, check_case(t, h["rating"], k, prof[tt], res.loading[i, tt], int(res.branch[i, tt]), int(res.count[i, tt]), h["thr"]))
            want = I.shed(t, k, injection=prof[tt], keep=~Sk)
            assert want["buses"] == res.shedBuses[j]
            g = sgn * F0[k, tt]                                                             # what left m over the bridge on the unsplit grid, by the rebuild route
            # injection = -shedFlow: the right-hand side summed over what leaves.  The unsplit model's right-hand side also carries the bridge's OWN
            # shiftPower entry at its end in S (-/+ shiftAngle y at the from / to end), which belongs to the bridge and not to what the buses inject:
            # 0 on every bridge but the phase shifter of the pocket, where leaving it out would miss by shiftAngle y = 0.26
            own = sgn * float(t["br_shift"][k]) * ykk[k]
            dev = max(abs(res.shedFlow[j, tt] - g) / max(1.0, abs(g)), abs(-res.shedFlow[j, tt] - (want["injection"] + own)) / max(1.0, abs(want["injection"])))
            assert dev <= TOL, (k, tt, res.shedFlow[j, tt], g, want["injection"], own)
            wg = max(wg, dev)
    print("hand grid:", lab.size, "bridges x 65 profiles: worst scaled deviation of the worst loading", worst, "of the flow that left", wg)


def test_non_bridge_cases_and_calls_without_the_keyword_are_bitwise_what_they_were(jg):
    h = hand(jg)
    s, prof, every, rating, thr, res = h["s"], h["prof"], h["every"], h["rating"], h["thr"], h["res"]
    isb = np.isin(every, res.shed)
    fresh = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True)      # an analysis no shed-mode screen ever ran on
    assert np.array_equal(fresh.islanding, every[isb]) and np.isnan(fresh.loading[isb]).all() and fresh.totals["islanding"] == int(isb.sum())
    assert fresh.shed is None and fresh.shedFlow is None
    for name in ("loading", "branch", "count"):
        assert np.array_equal(getattr(res, name)[~isb], getattr(fresh, name)[~isb]), name
    assert np.array_equal(res.base, fresh.base)
    for order in ("default first", "shed first"):
        an = jg.dcPowerFlow(s)
        got = []
        for islands in (("skip", "shed", "skip") if order == "default first" else ("shed", "skip")):
            kw = dict(islands="shed") if islands == "shed" else {}
            got.append((islands, jg.dcSeriesScreen(an, prof, candidates=every, rating=rating, threshold=thr, dense=True, **kw)))
        an.close()
        for islands, r in got:
            assert same(r, res if islands == "shed" else fresh), (order, islands)
            if islands == "shed":
                assert np.array_equal(r.shedFlow, res.shedFlow) and np.array_equal(r.shed, res.shed)


def test_results_do_not_depend_on_blocks_or_other_profiles_and_the_summaries_include_the_bridges(jg):
    h = hand(jg)
    s, prof, every, rating, thr, res = h["s"], h["prof"], h["every"], h["rating"], h["thr"], h["res"]
    isb = np.isin(every, res.shed)
    for block in (1, 3):                                              # (the default block is `res`)
        r = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=thr, dense=True, islands="shed", block=block)
        assert same(r, res), block
        for name in ("shed", "shedBuses", "shedM", "shedFlow"):
            assert np.array_equal(getattr(r, name), getattr(res, name)), (block, name)
    a, b = 3, 65                                                      # a subset of the profiles: columns a:b of the full screen
    part = jg.dcSeriesScreen(s, prof[a:b], candidates=every, rating=rating, threshold=thr, dense=True, islands="shed")
    for name in ("loading", "branch", "count"):
        assert np.array_equal(getattr(part, name), getattr(res, name)[:, a:b]), name
    assert np.array_equal(part.shedFlow, res.shedFlow[:, a:b]) and np.array_equal(part.worstProfile, res.worstProfile[a:b])
    T, nk = 65, every.size
    want = [(every[i], tt, res.branch[i, tt], res.loading[i, tt], res.count[i, tt]) for i in range(nk) for tt in range(T) if res.loading[i, tt] > thr]
    onb = int(np.isin(res.records[:, 0], every[isb]).sum())
    print("hand grid: cases", res.totals["cases"], "threshold", thr, "violating", res.totals["violating"], "of them on bridge candidates", onb)
    assert 0 < len(want) < nk * T and res.totals["violating"] == len(want) and not res.overflow and onb > 0
    assert np.array_equal(res.records, np.array(want, dtype=np.float64))          # sorted by (k, t), bit for bit what the dense matrix implies
    assert np.array_equal(res.worst, res.loading.max(axis=1)) and (res.worst[isb] > 0).all()
    assert np.array_equal(res.worstProfile, res.loading.max(axis=0))
    assert np.array_equal(res.violatingProfile, (res.loading > thr).sum(axis=0))
    tb = int(np.argmax(res.loading[isb].max(axis=0)))                  # a profile whose worst case over everything is a bridge case, if there is one
    print("hand grid: worst bridge case", res.loading[isb].max(), "worst other case", res.loading[~isb].max(), "profile", tb)


def test_a_tile_that_straddles_the_block_edge_and_mixes_bridges_with_others(jg):
    t = load_case("case14test")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    T = 130
    prof = S.profiles(t, T)
    br = H.bridges(t)
    every = S.in_service(t) + 1
    cand = every[every != int(every[~np.isin(every - 1, list(br))][0])]       # one non-bridge less: a count that is no multiple of the tile of 4
    if cand.size % 4 == 0:
        cand = cand[cand != int(cand[~np.isin(cand - 1, list(br))][0])]
    ref = jg.dcSeriesScreen(s, prof, candidates=cand, rating=rating, threshold=0.4, dense=True, islands="shed")
    isb = np.isin(cand - 1, list(br))
    pos = np.flatnonzero(isb)
    print("case14test: candidates", cand.size, "bridges at positions", pos, "cases", ref.totals["cases"], "violating", ref.totals["violating"])
    assert cand.size % 4 != 0 and np.array_equal(ref.shed, cand[isb]) and isb.sum() == len(br) and ref.islanding.size == 0
    worst = 0.0
    for i in pos:
        for tt in range(T):
            worst = max(worst, check_case(t, rating, int(cand[i]) - 1, prof[tt], ref.loading[i, tt], int(ref.branch[i, tt]), int(ref.count[i, tt]), 0.4))
    print("case14test:", pos.size, "bridges x 130 profiles: worst scaled deviation", worst)
    k0 = next(int(p) for p in range(1, cand.size) if p % 4 and isb[p // 4 * 4:p // 4 * 4 + 4].any() and not isb[p // 4 * 4:p // 4 * 4 + 4].all())
    for k0, k1 in ((k0, cand.size), (k0, k0 + 1), (1, cand.size - 1)):
        part = jg.dcSeriesScreen(s, prof, candidates=cand, rating=rating, threshold=0.4, dense=True, islands="shed", rows=(k0, k1), block=5)
        lab = cand[k0:k1]
        assert k0 % 4 != 0 and part.totals["cases"] == (k1 - k0) * T
        for name in ("loading", "branch", "count"):
            assert np.array_equal(getattr(part, name), getattr(ref, name)[k0:k1]), (k0, k1, name)
        keep = np.isin(ref.shed, lab)
        assert np.array_equal(part.shed, ref.shed[keep]) and np.array_equal(part.shedFlow, ref.shedFlow[keep]) and np.array_equal(part.shedM, ref.shedM[keep])
        assert np.array_equal(part.records, ref.records[np.isin(ref.records[:, 0], lab)])
        assert np.array_equal(part.worstProfile, ref.loading[k0:k1].max(axis=0))


def test_agreement_with_the_lane_path(jg):
    """column t of the bridge rows = the batched lanes with setInjection_ of profile t and setOutages_(..., islands="shed")"""
    D = jg.dcpowerflow
    h = hand(jg)
    s, prof, every, rating, res = h["s"], h["prof"], h["every"], h["rating"], h["res"]
    labels = [int(x) for x in res.shed]
    rows = np.flatnonzero(np.isin(every, res.shed))
    worst = 0.0
    for tt in (0, 64):
        an = jg.dcPowerFlow(s, batch=len(labels))
        D.setOutages_(an, labels, islands="shed")
        D.setInjection_(an, np.tile(prof[tt], (len(labels), 1)))
        D.solve_(an)
        rec = D.screenSummary_(an, rating)
        flow = np.atleast_1d(an.island.flow).copy()
        an.close()
        assert (rec[:, 4] == 4).all()
        dev = np.abs(res.loading[rows, tt] - rec[:, 0]) / np.maximum(1.0, rec[:, 0])
        gdev = np.abs(res.shedFlow[:, tt] - flow) / np.maximum(1.0, np.abs(flow))
        worst = max(worst, float(dev.max()), float(gdev.max()))
        assert (dev <= TOL).all() and (gdev <= TOL).all(), (tt, dev.max(), gdev.max())
        for j in np.flatnonzero(res.branch[rows, tt] != rec[:, 1]):   # another branch only on a tie within the tolerance
            _, fr, _ = I.solve(h["t"], out=labels[j] - 1, injection=prof[tt])
            load = P.loading(fr, rating)[2]
            assert abs(load[int(res.branch[rows[j], tt]) - 1] - load[int(rec[j, 1]) - 1]) <= TOL * max(1.0, rec[j, 0]), (tt, j)
    print("hand grid:", len(labels), "bridge lanes x 2 profiles, worst scaled deviation screen - lane path", worst)


def test_demand_shed_against_direct_sums(jg):
    h = hand(jg)
    t, s, prof, every, rating, res, br = h["t"], h["s"], h["prof"], h["every"], h["rating"], h["res"], h["br"]
    demand = np.abs(np.random.default_rng(4).standard_normal(prof.shape)) + np.asarray(t["bus_pd"])[None, :]
    got = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, threshold=h["thr"], dense=True, islands="shed", demand=demand)
    assert same(got, res) and got.shedDemand.shape == res.shedFlow.shape
    want = np.stack([demand[:, br[int(k) - 1][0]].sum(axis=1) for k in got.shed])
    # a difference of two prefix sums over all n buses: each carries at most n eps sum |v| of rounding (tests/test_dc_island_gpu.py)
    bound = 4 * demand.shape[1] * np.finfo(np.float64).eps * max(1.0, float(np.abs(demand).sum(axis=1).max()))
    dev = float(np.abs(got.shedDemand - want).max())
    print("hand grid: shedDemand worst deviation from the direct sums", dev, "bound", bound)
    assert dev <= bound and np.array_equal(got.unserved, got.shedDemand.sum(axis=1))


def test_large_grid_sample(jg):
    """32 seeded bridges of the 10k-bus grid x 8 profiles (tests/test_dc_series_shed_host.py holds the restatement against the same sample)"""
    t = load_case("case_ACTIVSg10k")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    prof = S.profiles(t, 8)
    pick, _ = H.sample(t)
    lab = np.array(sorted(pick), dtype=np.int64) + 1
    res = jg.dcSeriesScreen(s, prof, candidates=lab, rating=rating, dense=True, islands="shed")
    assert lab.size == 32 and res.totals["cases"] == 256 and res.totals["islanding"] == 0 and np.array_equal(res.shed, lab)
    worst = 0.0
    for i, k in enumerate(sorted(pick)):
        assert res.shedBuses[i] == int(pick[k][0].sum()) and res.shedM[i] == pick[k][1] + 1
        for tt in range(8):
            worst = max(worst, check_case(t, rating, k, prof[tt], res.loading[i, tt], int(res.branch[i, tt]), int(res.count[i, tt])))
    print("case_ACTIVSg10k: 32 bridges x 8 profiles, worst scaled deviation", worst)


def test_bad_input(jg):
    h = hand(jg)
    with pytest.raises(ValueError):
        jg.dcSeriesScreen(h["s"], h["prof"], rating=h["rating"], islands="nonsense")
    default = jg.dcSeriesScreen(h["s"], h["prof"][:2], rating=h["rating"], islands="shed")      # the default candidates: every in-service branch, bridges included
    assert np.array_equal(default.candidates, jg.shedCandidates(h["s"])) and np.array_equal(default.shed, h["res"].shed)
