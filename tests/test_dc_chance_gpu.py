"""The DC probabilistic N-1 screen (dcChanceScreen, csrc/jg_dc_chance.hip) on the device, against the rebuild-and-refactorise route of
tests/dc_chance_reference.py: per candidate the matrix rebuilt without it and refactorised, one solve per factor, never the compensation.  Bridges are held
against the graph (dc_series_reference.bridges), not against any linear algebra.

Tolerances.  Mean and standard deviation: |got - ref| <= 1e-9 * max(1, max |ref|), TOL and the measure of tests/test_dc_pair_gpu.py.  Probability: the
device's P against scipy's erfc applied to the device's OWN mean and standard deviation, absolute; P_BOUND is ten times the largest deviation measured on
an MI355X over every case of the parity test (DESIGN.md 3.18 has the figure) and may not exceed 1e-9.  Record sets: the cases whose reference P lies
within NEAR = 1e-6 of the threshold are left out, at most 1 % of the reference records (tests/test_dc_chance_host.py checks that share on the CPU for the
seeds used here); the worst probability per candidate is held against the reference within the same NEAR.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import dc_chance_reference as Q
import dc_reference as R
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
P_MEASURED = 8.9e-15                # largest |P device - P scipy| over the 24 parity cases on an MI355X (where mu is close to the rating and sigma small)
P_BOUND = 10 * P_MEASURED


def labels(cand):
    return [int(k) + 1 for k in cand]


def screen(jg, g, r, cand=None, **kw):
    kw.setdefault("probability", Q.PROBABILITY)
    kw.setdefault("dense", True)
    kw.setdefault("rating", g["rating"])
    return jg.dcChanceScreen(jg.powerSystem(g["t"]), g["L"][:r], candidates=labels(g["cand"] if cand is None else cand), **kw)


def check_dense(g, res, mom, cand, thr=Q.PROBABILITY):
    """a dense screen against the moments `mom` of the rebuild route, candidate by candidate; returns (worst scaled deviation of mean and std, largest
    |P - scipy(P of the device's own mean and std)|, reference records, cases near the threshold)"""
    rating = g["rating"]
    mon = res.monitored - 1
    assert res.mean.shape == res.std.shape == res.probability.shape == (len(cand), mon.size) and np.array_equal(res.candidates, labels(cand))
    dev, pdev, want, near_all = 0.0, 0.0, [], 0
    for i, k in enumerate(cand):
        if mom[i] is None:
            assert res.status[i] == 3 and np.isnan(res.worst[i]) and res.worstBranch[i] == 0 and res.count[i] == 0, k
            assert np.isnan(res.mean[i]).all() and np.isnan(res.std[i]).all() and np.isnan(res.probability[i]).all(), k
            continue
        mu, S = mom[i]
        sigma = np.sqrt((S ** 2).sum(axis=1))
        d = max(R.worst(res.mean[i], mu[mon]), R.worst(res.std[i], sigma[mon]))
        assert res.status[i] == 0 and d <= TOL, (k, d)
        dev = max(dev, d)
        own = Q.probability(res.mean[i], res.std[i], rating[mon])
        pdev = max(pdev, float(np.abs(res.probability[i] - own).max()))
        at = np.flatnonzero(mon == k)
        assert all(res.mean[i, j] == 0.0 and res.std[i, j] == 0.0 and res.probability[i, j] == 0.0 for j in at), k
        assert np.all(res.probability[i][rating[mon] == 0] == 0.0)
        # the summaries are what the device's own dense probabilities imply, bit for bit: ties go to the lowest branch
        p = res.probability[i]
        assert res.worst[i] == p.max() and res.count[i] == int((p >= thr).sum()), k
        assert res.worstBranch[i] == (int(mon[int(np.argmax(p))]) + 1 if p.max() > 0 else 0), k
        # and against the reference
        ref = Q.probability(mu[mon], sigma[mon], rating[mon])
        ref[mon == k] = 0.0
        near = np.abs(ref - thr) <= Q.NEAR
        near_all += int(near.sum())
        assert abs(res.worst[i] - ref.max()) <= Q.NEAR, (k, res.worst[i], ref.max())
        assert np.array_equal((p >= thr)[~near], (ref >= thr)[~near]), k
        want += [(k + 1, int(mon[j]) + 1) for j in np.flatnonzero(p >= thr)]
    assert res.bridges.tolist() == [k + 1 for k, m in zip(cand, mom) if m is None]
    assert res.total == len(want) == res.totals["records"] and res.totals["cases"] == len(cand) and res.totals["bridges"] == res.bridges.size
    if not res.overflow:
        assert [(int(a), int(b)) for a, b in res.records[:, :2]] == want               # sorted by (k, m)
        for row in res.records:
            i, j = cand.index(int(row[0]) - 1), int(np.searchsorted(mon, int(row[1]) - 1))
            assert row[2] == res.mean[i, j] and row[3] == res.std[i, j] and row[4] == res.probability[i, j]
    return dev, pdev, want, near_all


@pytest.mark.parametrize("r", [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("name", Q.GRIDS)
def test_dense_parity_with_the_rebuild_route_and_the_probabilities(jg, name, r):
    """every kernel instance (lds 8, 16, 24, 32) and every padding edge of S; mean and std at TOL, P at P_BOUND, records as a set"""
    g = Q.grid(name)
    mom = Q.cut(g["mom"], r)
    res = screen(jg, g, r)
    dev, pdev, want, near = check_dense(g, res, mom, g["cand"])
    print(name, "r", r, "candidates", len(g["cand"]), "monitored", res.monitored.size, "bridges", res.bridges.size, "records", len(want), "near the threshold", near,
          "worst scaled deviation of mean and std", dev, "largest |P - scipy|", pdev)
    assert P_BOUND <= 1e-9 and pdev <= P_BOUND
    assert near <= 0.01 * max(1, len(want)) and len(want) > 0 and 0 < res.bridges.size < len(g["cand"])
    bm, bS = g["base"]
    mon = res.monitored - 1
    bs = np.sqrt((bS[:, :r] ** 2).sum(axis=1))
    assert R.worst(res.base.mean, bm[mon]) <= TOL and R.worst(res.base.std, bs[mon]) <= TOL
    assert np.abs(res.base.probability - Q.probability(res.base.mean, res.base.std, g["rating"][mon])).max() <= P_BOUND
    assert res.info["buildMs"] > 0 and res.info["sBytes"] == res.info["rows"] * ((r + 7) // 8 * 8) * 8


def test_records_keep_the_first_by_candidate_and_branch_and_exact_totals(jg):
    g = Q.grid("case118")
    one = screen(jg, g, 8)
    check_dense(g, one, Q.cut(g["mom"], 8), g["cand"])
    assert one.total > 100 and not one.overflow
    key = one.records[:, 0] * 100000 + one.records[:, 1]
    assert np.all(np.diff(key) > 0)
    cut = screen(jg, g, 8, capacity=37, dense=False)
    assert cut.overflow and cut.total == one.total and np.array_equal(cut.records, one.records[:37])
    assert np.array_equal(cut.worst, one.worst, equal_nan=True) and np.array_equal(cut.count, one.count) and np.array_equal(cut.worstBranch, one.worstBranch)
    none = screen(jg, g, 8, capacity=0, dense=False)
    assert none.overflow and none.total == one.total and none.records.shape == (0, 5)
    print("case118: records", one.total, "kept with capacity 37:", cut.records.shape[0])


_EDGE = {}


def edge_reference():
    """case118, its first 130 in-service branches, 3 factors: computed once"""
    if not _EDGE:
        g = dict(Q.grid("case118"))
        on = [int(k) for k in np.flatnonzero(np.asarray(g["t"]["br_status"]) == 1)][:130]
        _EDGE.update(g=g, cand=on, mom=Q.moments(g["t"], on, g["p0"], g["L"][:3]))
    return _EDGE["g"], _EDGE["cand"], _EDGE["mom"]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_candidate_counts_around_the_lane_width(jg, count):
    g, cand, mom = edge_reference()
    res = screen(jg, g, 3, cand=cand[:count])
    dev, pdev, want, near = check_dense(g, res, mom[:count], cand[:count])
    print("candidates", count, "records", len(want), "bridges", res.bridges.size, "worst scaled deviation", dev, "largest |P - scipy|", pdev)
    assert pdev <= P_BOUND


def test_blocks_that_split_a_lane_chunk_give_bit_identical_results(jg):
    g, cand, mom = edge_reference()
    one = screen(jg, g, 3, cand=cand)
    fields = ("mean", "std", "probability", "worst", "worstBranch", "count", "status", "records", "bridges")
    for block in (40, 64, 65, 1000):
        res = screen(jg, g, 3, cand=cand, block=block)
        for f in fields:
            assert np.array_equal(getattr(res, f), getattr(one, f), equal_nan=True), (block, f)
        assert res.total == one.total and res.totals == one.totals
    part = screen(jg, g, 3, cand=cand, rows=(10, 75), block=23)
    assert part.rows == (10, 75) and part.mean.shape[0] == 65
    for f in ("mean", "std", "probability"):
        assert np.array_equal(getattr(part, f), getattr(one, f)[10:75], equal_nan=True), f
    for f in ("worst", "worstBranch", "count", "status"):
        assert np.array_equal(getattr(part, f)[10:75], getattr(one, f)[10:75], equal_nan=True), f
    lab = np.array(labels(cand))
    keep = (one.records[:, 0] >= lab[10]) & (one.records[:, 0] <= lab[74])
    assert np.array_equal(part.records, one.records[keep]) and part.total == int(keep.sum())


def test_monitored_lists_disjoint_from_equal_to_and_inside_the_candidates(jg):
    g = Q.grid("case30test")
    cand = g["cand"][::2]
    mom = Q.cut(g["mom"], 9)[::2]
    on = [int(k) for k in np.flatnonzero(np.asarray(g["t"]["br_status"]) == 1)]
    rated = [k for k in on if g["rating"][k] > 0]
    unrated = [k for k in on if g["rating"][k] == 0]
    for what, mon in (("disjoint", [k for k in on if k not in cand]), ("equal", list(cand)), ("a subset", list(cand[::3])), ("an unrated branch among them", rated[:6] + unrated[:2])):
        res = screen(jg, g, 9, cand=cand, monitored=labels(mon))
        assert np.array_equal(res.monitored, np.unique(labels(mon)))
        dev, pdev, want, near = check_dense(g, res, mom, cand)
        print("monitored", what, len(mon), "records", len(want), "worst scaled deviation", dev, "largest |P - scipy|", pdev)
        assert pdev <= P_BOUND
        assert set(int(x) for x in res.records[:, 1]) <= set(labels(k for k in mon if g["rating"][k] > 0))
    assert unrated and np.all(res.probability[res.status == 0][:, np.isin(res.monitored - 1, unrated)] == 0.0) and np.all(res.base.probability[np.isin(res.monitored - 1, unrated)] == 0.0)


def test_an_all_zero_factor_gives_certainty(jg):
    g = Q.grid("case14test")
    n = g["t"]["bus_type"].size
    res = jg.dcChanceScreen(jg.powerSystem(g["t"]), np.zeros((1, n)), candidates=labels(g["cand"]), rating=g["rating"] * 0.5, probability=0.5, dense=True)
    ok = res.status == 0
    assert np.all(res.std[ok] == 0.0) and np.all(res.base.std == 0.0)
    assert set(np.unique(res.probability[ok]).tolist()) == {0.0, 1.0} and set(np.unique(res.base.probability).tolist()) <= {0.0, 1.0}
    mon = res.monitored - 1
    assert np.array_equal(res.probability[ok] == 1.0, np.abs(res.mean[ok]) > (g["rating"] * 0.5)[mon][None, :])
    for i, k in enumerate(g["cand"]):
        if ok[i]:
            assert R.worst(res.mean[i], R.solve(g["t"], out=k)[1][mon]) <= TOL
    assert res.total == int((res.probability[ok] == 1.0).sum()) and np.all(res.records[:, 4] == 1.0)


def test_an_injection_of_the_call_replaces_the_systems_own(jg):
    g = Q.grid("case30test")
    t, cand = g["t"], g["cand"]
    p1 = g["p0"] * 1.15 + 0.02 * np.random.default_rng(3).standard_normal(g["p0"].size)
    res = screen(jg, g, 8, injection=p1)
    mom = Q.moments(t, cand, p1, g["L"][:8])
    dev, pdev, want, _ = check_dense(g, res, mom, cand)
    own = screen(jg, g, 8)
    same = screen(jg, g, 8, injection=g["p0"])
    ok = own.status == 0
    print("injection of the call: worst scaled deviation", dev, "records", len(want), "against", own.total, "of the system's own")
    assert R.worst(res.base.mean, R.solve(t, injection=p1)[1][res.monitored - 1]) <= TOL
    assert np.abs(res.mean[ok] - own.mean[ok]).max() > 1e-3 and np.array_equal(res.std, own.std, equal_nan=True)
    assert R.worst(same.mean[ok], own.mean[ok]) <= TOL and np.array_equal(same.std, own.std, equal_nan=True)


def test_refusals_a_second_build_after_release_and_a_pair_screen_left_alone(jg):
    g = Q.grid("case30test")
    t, rating = g["t"], g["rating"]
    n = t["bus_type"].size
    s = jg.powerSystem(t)
    with pytest.raises(ValueError, match="33 factors"):
        jg.dcChanceScreen(s, np.zeros((33, n)), rating=rating)
    with pytest.raises(ValueError, match="no shed mode"):
        jg.dcChanceScreen(s, g["L"][:2], rating=rating, islands="shed")
    an = jg.dcPowerFlow(s)
    pair = jg.dcPairScreen(an, rating=rating)
    L = jg._lib.lib()
    cand = np.array(labels(g["cand"]), dtype=np.int64)
    info, dims = np.zeros(12), np.zeros(6, dtype=np.int64)
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_chance_build(an._h, 33, np.zeros(33 * n), cand.size, cand, 0, None, None, 0, info))
    assert e.value.code == 1 and "33 factors" in str(e.value)
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_chance_get_dims(an._h, dims))
    assert e.value.code == 4
    jg._lib.check(L.jg_dc_chance_build(an._h, 17, np.ascontiguousarray(g["L"][:17]).reshape(-1), cand.size, cand, 0, None, None, 0, info))
    jg._lib.check(L.jg_dc_chance_get_dims(an._h, dims))
    assert dims.tolist()[:2] == [cand.size, 64] and dims[4] == 17 and dims[5] == 24
    ms = np.zeros(3)
    with pytest.raises(jg._lib.JGridError) as e:                  # no block has been screened yet
        jg._lib.check(L.jg_dc_chance_time_kernel(an._h, 0, 0, cand.size, 3, ms))
    assert e.value.code == 4
    jg._lib.check(L.jg_dc_chance_release(an._h))
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_chance_get_dims(an._h, dims))
    assert e.value.code == 4
    res = jg.dcChanceScreen(an, g["L"][:8], candidates=cand, rating=rating, probability=Q.PROBABILITY, dense=True)      # builds again, screens, releases
    check_dense(g, res, Q.cut(g["mom"], 8), g["cand"])
    again = jg.dcPairScreen(an, rating=rating)
    assert np.array_equal(again.records, pair.records) and again.totals == pair.totals and np.array_equal(again.worst, pair.worst)
    jg._lib.check(L.jg_dc_chance_release(an._h))                  # nothing held: still fine
    an.close()


def test_the_new_exports_through_the_plain_c_abi(jg):
    """ctypes calls with raw pointers only, null optional outputs: what a C driver does (include/jgrid.h)"""
    g = Q.grid("case14test")
    t = g["t"]
    (colptr, rowval, nzval), y, psh = R.model(t)
    n, nb = t["bus_type"].size, t["br_from"].size
    L = C.CDLL(jg._lib.LIB_PATH)
    L.jg_last_error.restype = C.c_char_p
    i64, f64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.jg_dc_create.argtypes = [i64, C.c_int64, i64, i64, f64, C.c_int64, C.c_double, C.c_int64, C.c_int]
    L.jg_dc_set_rhs.argtypes = [C.c_int64, f64]
    L.jg_dc_set_branches.argtypes = [C.c_int64, C.c_int64, i64, i64, f64, f64]
    L.jg_dc_set_rating.argtypes = [C.c_int64, f64]
    L.jg_dc_chance_build.argtypes = [C.c_int64, C.c_int64, f64, C.c_int64, i64, C.c_int64, i64, f64, C.c_int64, f64]
    L.jg_dc_chance_screen.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int64, f64, i64, f64, i32, i32, i32, f64, f64, f64]
    L.jg_dc_chance_get_dims.argtypes = [C.c_int64, i64]
    L.jg_dc_chance_get_base.argtypes = [C.c_int64, f64, f64, f64]
    L.jg_dc_chance_time_kernel.argtypes = [C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, f64]
    L.jg_dc_chance_release.argtypes = [C.c_int64]
    L.jg_dc_destroy.argtypes = [C.c_int64]
    L.jg_dc_destroy.restype = None
    arr = lambda a, ct: (ct * len(a))(*a)
    h = C.c_int64(0)
    slack = R.slack_of(t)
    assert L.jg_dc_create(C.byref(h), n, arr(colptr.tolist(), C.c_int64), arr(rowval.tolist(), C.c_int64), arr(nzval.tolist(), C.c_double), slack + 1,
                          float(t["bus_va"][slack]), 2, 0) == 0, L.jg_last_error()
    cand, r = labels(g["cand"]), 5
    nk = len(cand)
    fac = arr(g["L"][:r].reshape(-1).tolist(), C.c_double)
    info = (C.c_double * 12)()
    assert L.jg_dc_chance_build(h, r, fac, nk, arr(cand, C.c_int64), 0, None, None, 0, info) == 1           # no branches yet: a bad argument, not a crash
    assert L.jg_dc_set_rhs(h, arr(R.rhs_of(t, psh).tolist(), C.c_double)) == 0
    assert L.jg_dc_set_branches(h, nb, arr([int(x) for x in t["br_from"]], C.c_int64), arr([int(x) for x in t["br_to"]], C.c_int64),
                                arr(y.tolist(), C.c_double), arr([float(x) for x in t["br_shift"]], C.c_double)) == 0
    tot, rec = (C.c_int64 * 5)(), (C.c_double * (5 * 512))()
    assert L.jg_dc_chance_screen(h, 0, 1, 0.05, 512, rec, tot, None, None, None, None, None, None, None) == 4   # no build yet
    assert L.jg_dc_chance_build(h, 0, fac, nk, arr(cand, C.c_int64), 0, None, None, 0, info) == 1 and b"factors" in L.jg_last_error()
    assert L.jg_dc_chance_build(h, r, fac, nk, arr(cand, C.c_int64), 0, None, None, 0, info) == 0, L.jg_last_error()
    dims = (C.c_int64 * 6)()
    assert L.jg_dc_chance_get_dims(h, dims) == 0 and dims[0] == nk and dims[1] == 64 and dims[4] == r and dims[5] == 8
    assert dims[3] == int((np.asarray(t["br_status"]) == 1).sum())                                        # monitored null: every branch in service
    assert info[8] == dims[2] * 8 * 8
    assert L.jg_dc_chance_screen(h, 0, nk, 0.05, 512, rec, tot, None, None, None, None, None, None, None) == 1   # no rating yet
    assert L.jg_dc_set_rating(h, arr(g["rating"].tolist(), C.c_double)) == 0
    assert L.jg_dc_chance_screen(h, 0, nk, 0.0, 512, rec, tot, None, None, None, None, None, None, None) == 1    # probability 0
    assert L.jg_dc_chance_screen(h, 0, nk, 0.05, 512, rec, tot, None, None, None, None, None, None, None) == 0, L.jg_last_error()
    nbr = sum(m is None for m in g["mom"])
    assert tot[0] == nk and tot[2] == nbr and tot[3] == tot[1] > 0 and tot[4] == 0
    rows = np.array(rec[:5 * tot[3]]).reshape(-1, 5)
    assert np.all(np.diff(rows[:, 0] * 1000 + rows[:, 1]) > 0)    # sorted by (k, m)
    mom = Q.cut(g["mom"], r)
    for k, m, mu, sigma, p in rows:
        rm, rS = mom[g["cand"].index(int(k) - 1)]
        assert abs(mu - rm[int(m) - 1]) <= TOL * max(1.0, np.abs(rm).max()) and abs(sigma - np.sqrt((rS[int(m) - 1] ** 2).sum())) <= TOL
        assert abs(p - float(Q.probability(mu, sigma, g["rating"][int(m) - 1]))) <= P_BOUND and p >= 0.05
    worst, st = (C.c_double * nk)(), (C.c_int32 * nk)()
    assert L.jg_dc_chance_screen(h, 0, nk, 0.05, 0, None, tot, worst, None, None, st, None, None, None) == 0 and tot[3] == 0 and tot[4] == 1
    assert [int(x) for x in st] == [3 if m is None else 0 for m in g["mom"]]
    mean = (C.c_double * dims[3])()
    assert L.jg_dc_chance_get_base(h, mean, None, None) == 0
    assert R.worst(np.array(mean[:]), g["base"][0][np.asarray(t["br_status"]) == 1]) <= TOL
    ms = (C.c_double * 3)()
    assert L.jg_dc_chance_time_kernel(h, 0, 0, nk, 3, ms) == 0 and min(ms[:]) > 0
    assert L.jg_dc_chance_time_kernel(h, 1, 0, nk, 3, ms) == 0 and min(ms[:]) > 0
    assert L.jg_dc_chance_release(h) == 0 and L.jg_dc_chance_release(h) == 0
    L.jg_dc_destroy(h)
    assert L.jg_dc_chance_release(C.c_int64(0)) == 1
