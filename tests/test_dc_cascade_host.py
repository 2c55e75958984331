"""The DC cascading-outage screen, host side (no device): the argument checks of dcCascadeScreen that run before the device is touched, and the two routes
of tests/dc_cascade_reference.py against each other -- the cascade on the k x k formula from a dense inverse (b) against the cascade on rebuild and
refactorise with the graph oracle (a): equal sequences and statuses, final flows within 1e-9 * max(1, max |ref|) (tests/test_dc_group_host.py).

Every in-service branch as a single initiating event, trip = 1, most = 8, both rules, by route (a): no cascade is ambiguous (margin below 1e-6), the
smallest margin is 2.9e-5, and stable / islanding / truncated are
    case14test        3 / 15 / 0   (worst)     3 / 15 / 0   (all)
    case30test       16 / 26 / 0              15 / 26 / 1
    mesh 8x8         58 / 33 / 23             58 / 13 / 43
    pegaseShaped 160 117 / 127 / 26          115 / 102 / 53
with cascades of 7 trips in every grid but case14test under "worst".  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_cascade_reference as K
import dc_grids as G
import dc_group_reference as Q
import dc_reference as R
from conftest import load_case

TOL = 1e-9


def hand_made():
    """test_dc_group_host's ring of 6 buses: a double circuit (1-2), a triple circuit (2-3), an out-of-service twin (label 7) and a set of 9 (5-6)"""
    edges = ([(0, 1), (0, 1), (1, 2), (2, 1), (1, 2), (2, 3), (2, 3), (3, 4)] + [(4, 5)] * 9 + [(5, 0)])
    t = G.table(6, edges, 0, 21)
    t["br_status"][6] = 0
    return t


@pytest.mark.parametrize("kw,text", [
    (dict(events=[(1, 2), ()]), "event 1 () is empty"),
    (dict(events=[tuple(range(9, 18))]), "has 9 members, 8 at the most"),
    (dict(events=[(1, 2, 3)], most=2), "event 0 (1, 2, 3) has 3 members, 2 at the most"),
    (dict(events=[(1,), (3, 4, 3)]), "event 1 (3, 4, 3) names a branch twice"),
    (dict(events=[(1, 99)]), "event 0 (1, 99): 99 is no branch label"),
    (dict(events=[(2,), (5,), (6, 7)]), "event 2 (6, 7): branch 7 is out of service"),
    (dict(events=[]), "one or more events are needed"),
    (dict(events=[(1,)], trip=-0.5), "trip >= 0"),
    (dict(events=[(1,)], rule="first"), "rule is \"all\" or \"worst\""),
    (dict(events=[(1,)], most=1), "most is 2 to 8"),
    (dict(events=[(1,)], most=9), "most is 2 to 8"),
    (dict(events=[(1,)], rows=0), "rows >= 1"),
    (dict(events=[(1,)], islands="shed"), "no shed mode"),
    (dict(events=[(1,)], rating=None), "rating (per branch"),
    (dict(events=[(1,)], rating=np.ones(3)), "one value per branch"),
])
def test_a_bad_argument_is_refused_on_the_host_and_named(kw, text):
    import juliagrid.jl_amd as jg
    t = hand_made()
    s = jg.powerSystem(t)
    kw = dict(dict(rating=np.ones(t["br_from"].size)), **kw)
    with pytest.raises(ValueError) as e:
        jg.dcCascadeScreen(s, kw.pop("events"), **kw)
    print(e.value)
    assert text in str(e.value)


def test_the_screen_is_exported_and_takes_an_outage_list_as_it_is():
    import juliagrid.jl_amd as jg
    from juliagrid.jl_amd.dccascade import _event_lists
    assert "dcCascadeScreen" in jg.__all__ and jg.DC_CASCADE_MAX == jg.DC_GROUP_MAX == 8 and jg.DC_CASCADE_TRUNCATED == 5
    s = jg.powerSystem(hand_made())
    labels, offsets, members = _event_lists(s, list(jg.outageList(s, 5)), 8)
    assert all(len(x) == 1 for x in labels) and offsets.tolist() == [0, 1, 2, 3, 4, 5] and members.size == 5
    groups, _ = jg.parallelGroups(s)
    labels, offsets, members = _event_lists(s, groups, 8)
    assert labels == groups and offsets.tolist() == [0, 2, 5, 13]


def _table(name):
    return G.family(name) if name in G.FAMILIES else load_case(name)


SHARES = {"case14test": ((3, 15, 0), (3, 15, 0)), "case30test": ((16, 26, 0), (15, 26, 1)), "mesh 8x8": ((58, 33, 23), (58, 13, 43)),
          "pegaseShaped 160": ((117, 127, 26), (115, 102, 53))}


@pytest.mark.parametrize("name", ["case14test", "case30test", "mesh 8x8", "pegaseShaped 160"])
def test_the_two_routes_agree_and_the_shares_and_margins_are_what_the_tests_rest_on(name):
    t = _table(name)
    rating = K.ratings(t)
    mon = K.default_monitored(t, rating)
    Phi, f0 = Q.dense_sensitivities(t)
    base = Q.base_components(t)
    for rule, want in zip(("worst", "all"), SHARES[name]):
        ra = [K.cascade_rebuild(t, (k,), rating, mon, 1.0, rule, 8, base) for k in K.in_service(t)]
        rb = [K.cascade_formula(Phi, f0, (k,), rating, mon, 1.0, rule, 8) for k in K.in_service(t)]
        ambiguous = sum(a.margin < K.AMBIGUOUS for a in ra)
        dev = 0.0
        for a, b in zip(ra, rb):
            if a.margin < K.AMBIGUOUS:
                continue
            assert K.same_sequence(a, b), (a.tripped, b.tripped, a.status, b.status)
            assert (a.flows is None) == (b.flows is None) == (a.status == 3)
            if a.flows is not None:
                dev = max(dev, R.worst(b.flows, a.flows), float(np.abs(np.array(a.loading[1:]) - np.array(b.loading[1:])).max(initial=0.0)))
            assert Q.islands(t, a.tripped, base) == (a.status == 3)
        pivots = np.array([p for b in rb for p in b.pivots])
        print(name, rule, "cascades", len(ra), "stable / islanding / truncated", K.shares(ra), "ambiguous", ambiguous, "smallest margin",
              min(a.margin for a in ra), "deepest", max(a.stages for a in ra), "most out", max(len(a.tripped) for a in ra),
              "worst deviation of (b) from (a)", dev, "pivots: largest below the gap", pivots[pivots < 1e-9].max(initial=0.0), "smallest above",
              pivots[pivots >= 1e-9].min(initial=np.inf))
        assert dev <= TOL and ambiguous == 0 and ambiguous <= 0.05 * len(ra)
        assert min(a.margin for a in ra) >= 2.9e-5 and K.shares(ra) == want
        assert np.all((pivots < 1e-12) | (pivots > 1e-6))
        if name != "case14test" and rule == "worst":
            assert max(a.stages for a in ra) == 7


def test_a_ring_where_the_outage_of_one_path_trips_the_other_and_splits_the_grid():
    """Two parallel paths between buses 0 and 3 (0-1-2-3 and 0-5-4-3).  With one branch of the first path out the ring is a path and all exchange runs over
    the second; one of its branches is rated below what it then carries, the others far above: it trips, and a path without a branch is split.  Status 3
    after exactly one trip, under either rule."""
    ring = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)]
    t = G.table(6, ring, 0, 5)
    base = Q.base_components(t)
    out, weak = 1, 4                                              # (1-2) leaves; (4-5) is the weak branch of the other path
    after = Q.group_solve(t, (out,), base)
    assert after is not None and abs(after[weak]) > 1e-3 and all(Q.islands(t, (out, k), base) for k in range(6) if k != out)
    rating = np.full(6, 1e3)
    rating[weak] = 0.5 * abs(after[weak])
    assert abs(R.solve(t)[1][weak]) / rating[weak] != 1.0
    Phi, f0 = Q.dense_sensitivities(t)
    for rule in ("all", "worst"):
        for r in (K.cascade_rebuild(t, (out,), rating, np.arange(6), 1.0, rule, 8, base), K.cascade_formula(Phi, f0, (out,), rating, np.arange(6), 1.0, rule, 8)):
            print(rule, "tripped", r.tripped, "stage", r.stage, "loading", r.loading, "status", r.status)
            assert r.status == 3 and r.stages == 1 and r.tripped == [out, weak] and r.stage == [0, 1] and r.flows is None and r.pending == 0
            assert np.isnan(r.loading[0]) and abs(r.loading[1] - 2.0) <= 1e-9


def test_a_grid_that_truncates_at_two_outages():
    name = "mesh 8x8"
    t = _table(name)
    rating = K.ratings(t)
    mon = K.default_monitored(t, rating)
    base = Q.base_components(t)
    ra = [K.cascade_rebuild(t, (k,), rating, mon, 1.0, "all", 2, base) for k in K.in_service(t)]
    cut = [r for r in ra if r.status == K.TRUNCATED]
    print("most = 2: stable / islanding / truncated", K.shares(ra), "pending", sorted({r.pending for r in cut}))
    assert cut and all(len(r.tripped) + r.pending > 2 and r.flows is not None and r.worst > 1.0 for r in cut)
    assert any(len(r.tripped) == 1 and r.stages == 0 and r.pending >= 2 for r in cut)          # two or more overloaded at once: nothing is appended
    assert any(len(r.tripped) == 2 and r.stages == 1 and r.pending >= 1 for r in cut)          # one trip fits, the next stage does not
    assert all(len(r.tripped) <= 2 for r in ra)
