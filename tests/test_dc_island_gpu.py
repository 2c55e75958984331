"""Bridge outages of the DC N-1 screen solved on the slack's island (islands="shed") against the restatement, which deletes the branch, SEARCHES for the
slack's component and rebuilds + refactorises the DC model on it (tests/dc_island_reference.py) -- the library keeps its ONE factor of the whole grid.

Angles on the slack's side: the scaling and bound of tests/test_dc_gpu.py (max |got - ref| <= 1e-9 * max(1, max |ref|)); on the side that leaves they
are NaN exactly.  No lane is skipped."""
import numpy as np
import pytest

import dc_island_reference as I
import dc_reference as R
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9


def check_lanes(jg, t, an, labels, injection=None, rating=None, lanes=None):
    """lanes of a solved shed-mode batch against the restatement: status, angles, flows, what was shed, and (with a rating) the screen record"""
    jg.power_(an)
    th, fr, st = np.atleast_2d(an.voltage.angle), np.atleast_2d(an.power.from_.active), np.atleast_1d(an.status)
    isl = an.island
    f, to = np.asarray(t["br_from"]).astype(np.int64) - 1, np.asarray(t["br_to"]).astype(np.int64) - 1
    wa = wf = 0.0
    for s in (range(len(labels)) if lanes is None else lanes):
        lab = int(labels[s])
        inj = None if injection is None else injection[s]
        rth, rfr, keep = I.solve(t, out=lab - 1 if lab else None, injection=inj)
        split = not keep.all()
        assert st[s] == (4 if split else 0), (s, lab, st[s])
        assert np.array_equal(np.isnan(th[s]), ~keep), (s, lab)
        a, b = I.worst(th[s], rth, keep), R.worst(fr[s], rfr)
        print("lane", s, "branch", lab, "shed", int((~keep).sum()), "angle", a, "flow", b)
        assert a <= TOL and b <= TOL, (s, lab, a, b)
        wa, wf = max(wa, a), max(wf, b)
        dead = ~keep[f] | ~keep[to]
        if lab:
            dead[lab - 1] = True
        assert np.all(fr[s][dead] == 0.0), (s, lab)
        want = I.shed(t, lab - 1, injection=inj, keep=keep) if split else dict(buses=0, injection=0.0, demand=0.0, supply=0.0)
        assert isl.buses[s] == want["buses"] and abs(isl.injection[s] - want["injection"]) <= TOL * max(1.0, abs(want["injection"])), (s, lab)
        if split:
            m = f[lab - 1] if keep[f[lab - 1]] else to[lab - 1]
            g = rfr_before(t, lab - 1, inj) * (1.0 if m == f[lab - 1] else -1.0)
            assert isl.m[s] == m + 1 and abs(isl.flow[s] - g) <= TOL * max(1.0, abs(g)), (s, lab)
        else:
            assert isl.m[s] == 0 and isl.flow[s] == 0.0
        if inj is None or not split:
            # a difference of two prefix sums over all n buses: each carries at most n eps sum |v| of rounding (eps = 2.2e-16), the restatement's own sum less
            for name, v in (("demand", np.asarray(t["bus_pd"])), ("supply", R.supply(t))):
                bound = 4 * v.size * np.finfo(np.float64).eps * max(1.0, float(np.abs(v).sum()))
                assert abs(getattr(isl, name)[s] - want[name]) <= bound, (s, lab, name, getattr(isl, name)[s], want[name], bound)
        else:
            assert np.isnan(isl.demand[s]) and np.isnan(isl.supply[s])
        pw = I.power(t, rth, rfr, keep, injection=inj)
        for name in ("injection", "supply", "generator"):
            got = np.atleast_2d(getattr(an.power, name).active)[s]
            assert np.array_equal(np.isnan(got), np.isnan(pw[name])), (s, lab, name)
            ok = ~np.isnan(pw[name])
            assert R.worst(got[ok], pw[name][ok]) <= TOL, (s, lab, name)
        if rating is not None:
            m = np.abs(rfr)
            load = np.where(rating > 0, m / np.where(rating > 0, rating, 1.0), 0.0)
            rec = an.screen[s]
            assert abs(rec[0] - load.max()) <= TOL * max(1.0, load.max()) and abs(rec[2] - m.max()) <= TOL * max(1.0, m.max()), (s, lab)
            # the branch named: two branches in series carry the same flow up to rounding (8-9 and 9-10 of case118, 4.5 each), and which of them is
            # larger by an ulp differs between two correct routes.  So the branch is held EXACTLY against the lane's own flows as power_ returns them
            # (the first of equals: ties go to the lowest branch), and against the restatement through its value there
            gm = np.abs(fr[s])
            gload = np.where(rating > 0, gm / np.where(rating > 0, rating, 1.0), 0.0)
            assert int(rec[1]) == (int(np.argmax(gload)) + 1 if gload.max() > 0 else 0) and rec[0] == gload.max(), (s, lab)      # 0: nothing loaded
            assert int(rec[3]) == (int(np.argmax(gm)) + 1 if gm.max() > 0 else 0) and rec[2] == gm.max(), (s, lab)
            assert load.max() - load[max(int(rec[1]) - 1, 0)] <= TOL * max(1.0, load.max()) and m.max() - m[max(int(rec[3]) - 1, 0)] <= TOL * max(1.0, m.max()), (s, lab)
            assert rec[4] == st[s]
    print("worst angle", wa, "worst flow", wf)


_BASE = {}


def rfr_before(t, k, inj):
    """flow on branch k of the unsplit grid (its own injections where the lane has them)"""
    if inj is not None:
        return R.solve(t, injection=inj)[1][k]
    key = id(t)
    if key not in _BASE:
        _BASE.clear()
        _BASE[key] = R.solve(t)[1]
    return _BASE[key][k]


def against_the_default(jg, s, labels, an, is_bridge, rating=None):
    """the same batch without the keyword: status 3 on the bridge lanes, every other lane bitwise what shed mode gives"""
    ref = jg.contingencyAnalysis(s, labels, method="dc", rating=rating)
    lab = np.asarray([int(x) if x else 0 for x in labels])
    br = np.where(lab > 0, is_bridge[np.maximum(lab, 1) - 1], False)
    assert br.any() and not br.all()
    assert np.all(np.asarray(ref.status)[br] == 3) and np.all(np.asarray(ref.status)[~br] == 0) and np.all(np.isnan(ref.voltage.angle[br]))
    assert np.all(np.asarray(an.status)[br] == 4) and np.all(np.asarray(an.status)[~br] == 0)
    assert np.array_equal(an.voltage.angle[~br], ref.voltage.angle[~br])
    jg.power_(ref)
    jg.power_(an)
    assert np.array_equal(an.power.from_.active[~br], ref.power.from_.active[~br])
    for name in ("injection", "supply", "generator"):
        assert np.array_equal(getattr(an.power, name).active[~br], getattr(ref.power, name).active[~br])
    if rating is not None:
        assert np.array_equal(an.screen[~br], ref.screen[~br])
    assert ref.island is None
    ref.close()


@pytest.mark.parametrize("case", ["case14", "case118"])
def test_every_in_service_branch_in_one_batch(jg, case):
    t = load_case(case)
    s = jg.powerSystem(t)
    labels = np.flatnonzero(s.branch.layout.status == 1) + 1
    rating = 0.5 + np.random.default_rng(5).random(s.branch.number)
    rating[::7] = 0.0
    an = jg.contingencyAnalysis(s, labels, method="dc", rating=rating, islands="shed")
    is_bridge = jg.bridges(s)
    assert set(np.flatnonzero(np.asarray(an.status) == 4)) == set(np.flatnonzero(is_bridge[labels - 1])) and set(np.unique(an.status)) == {0, 4}
    check_lanes(jg, t, an, labels, rating=rating)
    against_the_default(jg, s, labels, an, is_bridge, rating=rating)
    an.close()


@pytest.fixture(scope="module")
def hand():
    t, marks, perm = I.hand_grid()
    return t, marks


def test_hand_built_grid_lane_by_lane(jg, hand):
    """S of one bus; S of 85 buses with loops and a phase shifter inside, behind a bridge that is a phase shifter and whose to-end stays; m the slack; nested
    bridges; the base lane; non-bridge lanes in between -- 157 lanes: three lane groups, the last partly filled"""
    t, marks = hand
    s = jg.powerSystem(t)
    is_bridge = jg.bridges(s)
    special = [marks[k][0] for k in ("at_slack", "pocket", "behind_doubled", "open_loop", "core_shifter", "pocket_shifter")] + marks["chain"] + marks["far"] + marks["doubled"]
    rest = [k for k in range(s.branch.number) if k not in special]
    labels = np.array([0] + [k + 1 for k in special] + [k + 1 for k in rest[:136]])
    assert labels.size == 157 and is_bridge[labels[1:] - 1].sum() == 15
    rating = np.full(s.branch.number, 2.0)
    an = jg.contingencyAnalysis(s, labels, method="dc", rating=rating, islands="shed")
    assert an.status[0] == 0 and an.island.buses[0] == 0                    # the base lane
    assert an.island.buses[1] == 1 and an.island.m[1] == s.bus.layout.slack and an.island.buses[2] == 85
    check_lanes(jg, t, an, labels, rating=rating)
    against_the_default(jg, s, labels, an, is_bridge, rating=rating)
    an.close()


def test_a_planted_tie_among_the_surviving_branches_goes_to_the_lowest(jg, hand):
    """the two parallel branches of the hand-built grid made identical carry bitwise the same flow; with only them rated, the record of a lane that sheds
    the pocket names the first of them, and a rated branch inside what left (flow 0) never shows"""
    t, marks = hand
    t = {k: np.array(v) for k, v in t.items()}
    a, b = marks["doubled"]
    for key in ("br_x", "br_tap", "br_shift"):
        t[key][b] = t[key][a]
    s = jg.powerSystem(t)
    rating = np.zeros(s.branch.number)
    rating[[a, b, marks["pocket_shifter"][0]]] = 1.0, 1.0, 1e-6               # the pocket's branch would win by far if it counted
    labels = [marks["pocket"][0] + 1, marks["pocket"][0] + 1]
    an = jg.contingencyAnalysis(s, labels, method="dc", rating=rating, islands="shed")
    jg.power_(an)
    fr = an.power.from_.active
    assert fr[0, a] == fr[0, b] and fr[0, a] != 0.0 and fr[0, marks["pocket_shifter"][0]] == 0.0
    assert np.all(an.screen[:, 1] == a + 1) and np.all(an.screen[:, 0] == abs(fr[0, a])) and np.all(an.screen[:, 4] == 4)
    check_lanes(jg, t, an, labels, rating=rating)
    an.close()


def test_seventy_lanes_with_injections_of_their_own(jg, hand):
    """every lane its own injections, every other lane a bridge: two lane groups, the second holds 6 lanes"""
    t, marks = hand
    s = jg.powerSystem(t)
    is_bridge = jg.bridges(s)
    br = [marks[k][0] for k in ("at_slack", "pocket", "behind_doubled")] + marks["chain"] + marks["far"]
    non = [int(k) for k in np.flatnonzero(~is_bridge & (s.branch.layout.status == 1))]
    labels = np.array([(br[(i // 2) % len(br)] if i % 2 == 0 else non[3 * i]) + 1 for i in range(70)])
    assert is_bridge[labels - 1].sum() == 35
    rng = np.random.default_rng(70)
    base = s.bus.supply.active - s.bus.demand.active
    own = base[None, :] * (1.0 + 0.2 * rng.standard_normal((70, base.size)))
    an = jg.dcPowerFlow(s, batch=70)
    jg.setOutages_(an, labels, islands="shed")
    jg.setInjection_(an, own)
    jg.solve_(an)
    assert np.array_equal(np.asarray(an.status), np.where(is_bridge[labels - 1], 4, 0))
    check_lanes(jg, t, an, labels, injection=list(own))
    an.close()


def test_mode_applies_to_the_lanes_set_after_it_and_pairs_keep_status_3(jg, hand):
    t, marks = hand
    s = jg.powerSystem(t)
    k, l = marks["pocket"][0] + 1, marks["at_slack"][0] + 1
    an = jg.dcPowerFlow(s, batch=4)
    jg.setOutages_(an, [k, (k, l)], islands="shed")
    jg.setOutages_(an, [k, 0], scenario0=2)                                  # the default again: this lane is skipped
    jg.solve_(an)
    assert list(an.status) == [4, 3, 3, 0] and list(an.island.buses) == [85, 0, 0, 0]
    assert np.all(np.isnan(an.voltage.angle[1])) and np.all(np.isnan(an.voltage.angle[2]))
    with pytest.raises(ValueError):
        jg.setOutages_(an, [k], islands="island")
    jg.setOutages_(an, [0, 0, 0, 0])                                         # no island lane left: the plain kernels run, nothing is shed
    jg.solve_(an)
    assert list(an.status) == [0, 0, 0, 0] and not np.any(an.island.buses) and not np.isnan(an.voltage.angle).any()
    an.close()


def test_every_bridge_of_the_10k_bus_grid(jg):
    """3 977 bridges in 512-lane batches, the last one short (393 lanes: its last lane group holds 9).  One lane per lane group and every lane that sheds
    more than 10 buses go to the restatement; every lane is held to status 4 and to the NaN pattern of its interval"""
    t = load_case("case_ACTIVSg10k")
    s = jg.powerSystem(t)
    tb = jg.islandTable(s)
    bridges = np.flatnonzero(tb.side != 0) + 1
    assert bridges.size == 3977
    size = (tb.hi - tb.lo + 1)[bridges - 1]
    rng = np.random.default_rng(10)
    full = jg.dcPowerFlow(s, batch=512)
    checked = big = 0
    for b0 in range(0, bridges.size, 512):
        labels = bridges[b0:b0 + 512]
        an = full if labels.size == 512 else jg.dcPowerFlow(s, batch=labels.size)
        jg.setOutages_(an, labels, islands="shed")
        jg.solve_(an)
        assert np.all(np.asarray(an.status) == 4)                            # no lane is skipped
        assert np.array_equal(an.island.buses, size[b0:b0 + 512]) and np.array_equal(np.isnan(an.voltage.angle).sum(axis=1), size[b0:b0 + 512])
        gone = (tb.preorder[None, :] >= tb.lo[labels - 1][:, None]) & (tb.preorder[None, :] <= tb.hi[labels - 1][:, None])
        assert np.array_equal(np.isnan(an.voltage.angle), gone)
        lanes = {int(g * 64 + rng.integers(0, min(64, labels.size - g * 64))) for g in range((labels.size + 63) // 64)}
        large = set(int(i) for i in np.flatnonzero(size[b0:b0 + 512] > 10))
        big += len(large)
        check_lanes(jg, t, an, labels, lanes=sorted(lanes | large))
        checked += len(lanes | large)
        if an is not full:
            an.close()
    full.close()
    print("lanes against the restatement", checked, "of them shedding more than 10 buses", big)
    assert checked >= 63 and big >= 1
