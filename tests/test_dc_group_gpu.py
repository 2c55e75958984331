"""The DC common-mode screen (dcGroupScreen, csrc/jg_dc_group.hip) on the device, against the rebuild route of tests/dc_group_reference.py: the members
out of service in a copy of the case table, the matrix rebuilt and refactorised for every group, never the compensation.  Islanding is held against the
graph oracle (connected components), not against any linear algebra.

Tolerance of every comparison: |got - ref| <= 1e-9 * max(1, max |ref|), the measure and the bound of tests/test_dc_pair_gpu.py.  Every group a test
screens has, by the k x k formula on the host (route (b)), a smallest pivot below 1e-12 or above 1e-6: no case sits near DC_SINGULAR = 1e-9, and the
test asserts it.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_grids as G
import dc_group_reference as Q
import dc_reference as R
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
_CACHE = {}


def table_of(name):
    return G.family(name) if name in G.FAMILIES else load_case(name)


def reference(name):
    """per grid, computed once and left unchanged: the table, the dense sensitivities of route (b), the components of the whole graph, the ratings"""
    if name not in _CACHE:
        t = table_of(name)
        Phi, f0 = Q.dense_sensitivities(t)
        _CACHE[name] = (t, Phi, f0, Q.base_components(t), Q.rating_of(t))
    return _CACHE[name]


def labels_of(groups):
    return [tuple(int(s) + 1 for s in S) for S in groups]


def check_pivots(name, groups):
    """the pivot condition of the module's docstring, on the host; returns the smallest pivots"""
    _, Phi, f0, _, _ = reference(name)
    small = np.array([Q.group_flows(Phi, f0, S)[1] for S in groups])
    print(name, "smallest pivots: largest below the gap", small[small < 1e-9].max(initial=0.0), "smallest above", small[small >= 1e-9].min(initial=np.inf))
    assert np.all((small < 1e-12) | (small > 1e-6)), small[(small >= 1e-12) & (small <= 1e-6)]
    return small


def check_screen(name, groups, res, monitored=None, threshold=1.0):
    """every group (0-based branches) of a dense screen against the rebuild route; returns (islanding groups, worst scaled deviation)"""
    t, _, _, base, rating = reference(name)
    mon = res.monitored - 1
    assert res.flows.shape == (len(groups), mon.size) and res.groups == labels_of(groups)
    isl, worst_dev, want_rec = [], 0.0, []
    for g, S in enumerate(groups):
        ref = Q.group_solve(t, S, base)
        if ref is None:
            isl.append(g)
            assert res.status[g] == 3 and np.isnan(res.worst[g]) and res.worstBranch[g] == 0 and res.count[g] == 0, (g, S)
            assert np.all(np.isnan(res.flows[g])), (g, S)
            continue
        assert res.status[g] == 0, (g, S)
        got = res.flows[g]
        dev = R.worst(got, ref[mon])
        assert dev <= TOL, (g, S, dev)
        assert all(got[np.searchsorted(mon, s)] == 0.0 for s in S if s in set(mon.tolist())), (g, S)
        w, b, load = Q.loading(ref, rating, mon)
        scale = max(1.0, w)
        assert abs(res.worst[g] - w) <= TOL * scale, (g, S, res.worst[g], w)
        assert res.worstBranch[g] == b or (res.worstBranch[g] >= 1 and abs(load[res.worstBranch[g] - 1] - w) <= TOL * scale), (g, S, res.worstBranch[g], b)
        near = int((np.abs(load - threshold) <= TOL * scale).sum())
        over = int((load > threshold).sum())
        assert over - near <= res.count[g] <= over + near, (g, S, res.count[g], over, near)
        worst_dev = max(worst_dev, dev, abs(res.worst[g] - w) / scale)
        # what the device's own flows imply: the records of this group, bit for bit
        dl = np.abs(got) * np.where(rating[mon] > 0, 1.0 / np.where(rating[mon] > 0, rating[mon], 1.0), 0.0)
        assert res.worst[g] == dl.max() and int((dl > threshold).sum()) == res.count[g]
        want_rec += [(g, int(mon[j]) + 1, got[j], dl[j]) for j in np.flatnonzero(dl > threshold)]
    assert res.islanding.tolist() == isl and res.totals == dict(groups=len(groups), violating=len(want_rec), islanding=len(isl))
    if not res.overflow:
        assert np.array_equal(res.violating, np.array(want_rec, dtype=np.float64).reshape(-1, 4))
    return isl, worst_dev, want_rec


def split_threshold(name, groups):
    """a threshold that some of the post-outage loadings exceed and most do not, from the rebuild route"""
    t, _, _, base, rating = reference(name)
    loads = [Q.loading(fr, rating)[2] for fr in (Q.group_solve(t, S, base) for S in groups[:12]) if fr is not None]
    return float(np.quantile(np.concatenate(loads), 0.97))


@pytest.mark.parametrize("name", ["case14test", "case30test", "case118", "pegaseShaped 160"])
def test_parity_with_the_rebuild_route_for_groups_of_one_to_eight(jg, name):
    t = reference(name)[0]
    groups = Q.seeded_groups(t, 23, [1, 2, 3, 4, 5, 6, 7, 8, 8] * 4, whole=True)
    check_pivots(name, groups)
    thr = split_threshold(name, groups)
    res = jg.dcGroupScreen(jg.powerSystem(t), labels_of(groups), rating=reference(name)[4], threshold=thr, dense=True)
    isl, dev, rec = check_screen(name, groups, res, threshold=thr)
    print(name, "groups", len(groups), "candidates", res.candidates.size, "islanding", len(isl), "records", len(rec), "worst scaled deviation", dev,
          "buildMs", res.buildMs, "screenMs", res.screenMs)
    assert np.array_equal(res.candidates, np.unique([s + 1 for S in groups for s in S])) and res.candidates.size % 64 != 0
    assert len(isl) < len(groups) and len(rec) > 0 and res.buildMs > 0 and res.screenMs > 0
    assert R.worst(res.base, R.solve(t)[1][res.monitored - 1]) <= TOL
    if name != "case14test":                                      # (14 buses on 20 branches: no 8 of them leave the grid whole)
        assert any(len(S) == 8 and g not in isl for g, S in enumerate(groups))


def test_groups_of_one_agree_with_the_single_outage_screen(jg):
    name = "case118"
    t, _, _, _, rating = reference(name)
    s = jg.powerSystem(t)
    on = [int(k) for k in np.flatnonzero(np.asarray(t["br_status"]) == 1)][::3]
    check_pivots(name, [(k,) for k in on])
    res = jg.dcGroupScreen(s, [(k + 1,) for k in on], rating=rating)
    lanes = jg.dcpowerflow.dcContingencyAnalysis(s, [k + 1 for k in on], rating=rating)
    n3 = 0
    for g, rec in enumerate(lanes.screen):
        if rec[4] == 3:
            n3 += 1
            assert res.status[g] == 3 and np.isnan(res.worst[g])
        else:
            assert res.status[g] == 0 and abs(res.worst[g] - rec[0]) <= TOL * max(1.0, rec[0]), (g, res.worst[g], rec)
    lanes.close()
    print("single outages", len(on), "bridges", n3)
    assert 0 < n3 < len(on) and res.islanding.size == n3


def test_groups_of_two_agree_with_the_pair_screen(jg):
    name = "case30test"
    t, _, _, _, rating = reference(name)
    s = jg.powerSystem(t)
    pair = jg.dcPairScreen(s, rating=rating, dense=True)
    cand = pair.candidates
    pairs = [(i, j) for i in range(cand.size) for j in range(i + 1, cand.size)][::7]
    check_pivots(name, [(int(cand[i]) - 1, int(cand[j]) - 1) for i, j in pairs])
    res = jg.dcGroupScreen(s, [(int(cand[i]), int(cand[j])) for i, j in pairs], rating=rating)
    worst, n3 = 0.0, 0
    for g, (i, j) in enumerate(pairs):
        want = pair.loading[i, j]
        if np.isnan(want):
            n3 += 1
            assert res.status[g] == 3 and np.isnan(res.worst[g]), (g, i, j)
            continue
        dev = abs(res.worst[g] - want) / max(1.0, want)
        assert res.status[g] == 0 and dev <= TOL and res.count[g] == pair.count[i, j], (g, i, j, res.worst[g], want)
        worst = max(worst, dev)
    print("pairs", len(pairs), "islanding", n3, "worst scaled deviation from the pair screen", worst)
    assert 0 < n3 < len(pairs)


def test_a_bridge_and_a_joint_cut_of_three_give_status_three_and_leave_the_others_alone(jg):
    name = "mesh 8x8"
    t, _, _, base, rating = reference(name)
    s = jg.powerSystem(t)
    f, to, on = np.asarray(t["br_from"]) - 1, np.asarray(t["br_to"]) - 1, np.asarray(t["br_status"]) == 1
    slack = R.slack_of(t)
    cut = next(tuple(int(k) for k in np.flatnonzero(on & ((f == b) | (to == b)))) for b in range(t["bus_type"].size)
               if b != slack and int((on & ((f == b) | (to == b))).sum()) == 3)
    assert not any(Q.islands(t, (cut[i], cut[j]), base) for i in range(3) for j in range(i + 1, 3)) and Q.islands(t, cut, base)
    plain = Q.seeded_groups(t, 31, [1, 2, 3, 4, 5, 6, 7, 8, 2, 3])
    groups = plain[:4] + [cut] + plain[4:]
    check_pivots(name, groups)
    res = jg.dcGroupScreen(s, labels_of(groups), rating=rating, threshold=0.2, dense=True)
    isl, dev, _ = check_screen(name, groups, res, threshold=0.2)
    assert 4 in isl and res.status[4] == 3 and np.isnan(res.worst[4]) and np.all(np.isnan(res.flows[4])) and 4 in res.islanding.tolist()
    alone = jg.dcGroupScreen(s, labels_of(plain), rating=rating, threshold=0.2, dense=True)
    keep = [g for g in range(len(groups)) if g != 4]
    assert np.array_equal(res.flows[keep], alone.flows, equal_nan=True) and np.array_equal(res.worst[keep], alone.worst, equal_nan=True)
    assert np.array_equal(res.count[keep], alone.count) and np.array_equal(res.worstBranch[keep], alone.worstBranch)
    # a group that holds a bridge: case14test's radial branch with two others
    name = "case14test"
    t = reference(name)[0]
    s = jg.powerSystem(t)
    bridge = int(np.flatnonzero(jg.bridges(s))[0])
    others = [k for k in range(t["br_from"].size) if k != bridge and t["br_status"][k] == 1]
    groups = [(others[0],), tuple(sorted((bridge, others[1], others[2]))), (others[3], others[4])]
    check_pivots(name, groups)
    res = jg.dcGroupScreen(s, labels_of(groups), rating=reference(name)[4], dense=True)
    isl, _, _ = check_screen(name, groups, res)
    print("joint cut", cut, "bridge group", groups[1], "islanding", isl, "worst scaled deviation on the mesh", dev)
    assert 1 in isl and res.status.tolist()[1] == 3


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_group_counts_around_the_lane_width(jg, count):
    name = "case30test"
    t, _, _, _, rating = reference(name)
    groups = Q.seeded_groups(t, 41, ([1, 2, 3, 1, 2] * 26)[:count])
    check_pivots(name, groups)
    res = jg.dcGroupScreen(jg.powerSystem(t), labels_of(groups), rating=rating, threshold=0.3, dense=True)
    isl, dev, rec = check_screen(name, groups, res, threshold=0.3)
    print("groups", count, "islanding", len(isl), "records", len(rec), "worst scaled deviation", dev)


def test_blocks_give_the_same_whatever_their_size_and_every_instance_runs(jg):
    name = "case118"
    t, _, _, _, rating = reference(name)
    s = jg.powerSystem(t)
    # blocks of four groups whose largest has 2, 4, 5 and 8 members: K = 2, 4 (full), 8 (padded), 8 (full), then 114 more groups of every size
    sizes = [1, 2, 2, 1, 3, 4, 1, 4, 5, 1, 2, 3, 8, 7, 6, 8] + [1, 2, 3, 4, 5, 6, 7, 8] * 14 + [2, 2]
    groups = Q.seeded_groups(t, 53, sizes, whole=True)
    assert len(groups) == 130
    check_pivots(name, groups)
    thr = split_threshold(name, groups)
    one = jg.dcGroupScreen(s, labels_of(groups), rating=rating, threshold=thr, dense=True)
    isl, dev, rec = check_screen(name, groups, one, threshold=thr)
    print("130 groups: islanding", len(isl), "records", len(rec), "worst scaled deviation", dev)
    assert len(rec) > 20
    for rows in (4, 64, 65):
        res = jg.dcGroupScreen(s, labels_of(groups), rating=rating, threshold=thr, dense=True, rows=rows)
        for field in ("flows", "worst", "worstBranch", "count", "status", "violating", "islanding", "base"):
            assert np.array_equal(getattr(res, field), getattr(one, field), equal_nan=True), (rows, field)
        assert res.totals == one.totals
    # fewer records than violators: the FIRST by (group, branch), the totals exact
    cut = jg.dcGroupScreen(s, labels_of(groups), rating=rating, threshold=thr, capacity=7, rows=64)
    assert cut.overflow and cut.totals == one.totals and np.array_equal(cut.violating, one.violating[:7])
    assert np.array_equal(cut.worst, one.worst, equal_nan=True) and np.array_equal(cut.count, one.count)
    none = jg.dcGroupScreen(s, labels_of(groups), rating=rating, threshold=thr, capacity=0)
    assert none.overflow and none.totals == one.totals and none.violating.shape == (0, 4)


def test_monitored_as_a_strict_subset_that_excludes_members(jg):
    name = "case30test"
    t, _, _, _, rating = reference(name)
    groups = Q.seeded_groups(t, 61, [1, 2, 3, 4, 5, 6, 2, 3])
    check_pivots(name, groups)
    members = sorted({s for S in groups for s in S})
    on = [int(k) for k in np.flatnonzero(np.asarray(t["br_status"]) == 1)]
    mon = np.array([k for k in on if k not in members[::2]][::2], dtype=np.int64)
    assert set(members) - set(mon.tolist()) and set(members) & set(mon.tolist())
    res = jg.dcGroupScreen(jg.powerSystem(t), labels_of(groups), monitored=mon + 1, rating=rating, threshold=0.3, dense=True)
    assert np.array_equal(res.monitored, mon + 1)
    isl, dev, rec = check_screen(name, groups, res, threshold=0.3)
    print("monitored", mon.size, "of", len(on), "islanding", len(isl), "records", len(rec), "worst scaled deviation", dev)
    assert set(res.violating[:, 1].astype(int).tolist()) <= set((mon + 1).tolist())


def test_a_second_build_on_a_handle_that_holds_a_pair_screen_then_release_and_destroy(jg):
    name = "case30test"
    t, _, _, _, rating = reference(name)
    s = jg.powerSystem(t)
    an = jg.dcPowerFlow(s)
    pair = jg.dcPairScreen(an, rating=rating)
    first = Q.seeded_groups(t, 71, [2, 3, 4])
    second = Q.seeded_groups(t, 73, [1, 5, 8, 2, 3])
    check_pivots(name, first + second)
    L = jg._lib.lib()
    info = np.zeros(8)
    # two builds in a row on the handle: the second replaces the first
    for groups in (first, second):
        lab = labels_of(groups)
        off = np.zeros(len(lab) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in lab])
        jg._lib.check(L.jg_dc_group_build(an._h, len(lab), off, np.array([x for g in lab for x in g], dtype=np.int64), 0, None, 0, info))
    dims = np.zeros(6, dtype=np.int64)
    jg._lib.check(L.jg_dc_group_get_dims(an._h, dims))
    assert dims[0] == 5 and dims[1] == 64 and dims[5] == 8 and dims[2] == len({s for S in second for s in S})
    ms = np.zeros(3)
    with pytest.raises(jg._lib.JGridError) as e:                  # no block has been screened yet
        jg._lib.check(L.jg_dc_group_time_kernel(an._h, 0, 0, 5, 3, ms))
    assert e.value.code == 4
    res = jg.dcGroupScreen(an, labels_of(second), rating=rating, threshold=0.3, dense=True)       # builds again, screens, releases
    check_screen(name, second, res, threshold=0.3)
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_group_get_dims(an._h, dims))
    assert e.value.code == 4
    again = jg.dcPairScreen(an, rating=rating)
    assert np.array_equal(again.records, pair.records) and again.totals == pair.totals
    # a refused build names the group and leaves the handle usable
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_group_build(an._h, 2, np.array([0, 1, 3], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64), 0, None, 0, info))
    assert e.value.code == 1 and "group 1" in str(e.value)
    jg._lib.check(L.jg_dc_group_release(an._h))                   # nothing held: still fine
    an.close()
