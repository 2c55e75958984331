"""The DC common-mode screen, host side (no device): parallelGroups on a hand-made grid, the argument checks of dcGroupScreen that run before the device
is touched, and the two routes of tests/dc_group_reference.py against each other -- the k x k formula from a dense inverse (b) against rebuild and
refactorise (a), the singular groups against the graph oracle.

Tolerance: max |got - ref| <= 1e-9 * max(1, max |ref|), as in tests/test_dc_pair_host.py.  Every figure is printed before it is asserted; the worst
deviation of route (b) from route (a) is the figure of DESIGN.md 3.17."""
import numpy as np
import pytest

import dc_grids as G
import dc_group_reference as Q
import dc_reference as R
from conftest import load_case

TOL = 1e-9


def hand_made():
    """a ring of 6 buses with a double circuit (1-2), a triple circuit (2-3, one copy reversed), an out-of-service twin (3-4) and a set of 9 (5-6)"""
    edges = ([(0, 1), (0, 1), (1, 2), (2, 1), (1, 2), (2, 3), (2, 3), (3, 4)] + [(4, 5)] * 9 + [(5, 0)])
    t = G.table(6, edges, 0, 21)
    t["br_status"][6] = 0                                         # the twin of 2-3 (label 7) is out of service: 2-3 is a single circuit
    return t


def test_parallel_groups_of_a_hand_made_grid():
    import juliagrid.jl_amd as jg
    s = jg.powerSystem(hand_made())
    groups, rest = jg.parallelGroups(s)
    assert groups == [(1, 2), (3, 4, 5), (9, 10, 11, 12, 13, 14, 15, 16)] and rest == [(17,)]
    assert all(len(g) <= jg.DC_GROUP_MAX for g in groups)
    assert "dcGroupScreen" in jg.__all__ and "parallelGroups" in jg.__all__


@pytest.mark.parametrize("groups,text", [
    ([(1, 2), ()], "group 1 () is empty"),
    ([tuple(range(9, 18))], "has 9 members, 8 at the most"),
    ([(1,), (3, 4, 3)], "group 1 (3, 4, 3) names a branch twice"),
    ([(1, 99)], "group 0 (1, 99): 99 is no branch label"),
    ([(2,), (5,), (6, 7)], "group 2 (6, 7): branch 7 is out of service"),
    ([], "one or more groups are needed"),
])
def test_a_bad_group_is_refused_on_the_host_and_named(groups, text):
    import juliagrid.jl_amd as jg
    t = hand_made()
    s = jg.powerSystem(t)
    with pytest.raises(ValueError) as e:
        jg.dcGroupScreen(s, groups, rating=np.ones(t["br_from"].size))
    print(e.value)
    assert text in str(e.value)


def test_rating_and_threshold_are_checked_first():
    import juliagrid.jl_amd as jg
    t = hand_made()
    s = jg.powerSystem(t)
    with pytest.raises(ValueError):
        jg.dcGroupScreen(s, [(1, 2)])
    with pytest.raises(ValueError):
        jg.dcGroupScreen(s, [(1, 2)], rating=np.ones(3))
    with pytest.raises(ValueError):
        jg.dcGroupScreen(s, [(1, 2)], rating=np.ones(t["br_from"].size), threshold=-1.0)


def _tables():
    return {"case14test": lambda: load_case("case14test"), "case30test": lambda: load_case("case30test"),
            "mesh 8x8": lambda: G.family("mesh 8x8"), "pegaseShaped 160": lambda: G.family("pegaseShaped 160")}


@pytest.mark.parametrize("name", ["case14test", "case30test", "mesh 8x8", "pegaseShaped 160"])
def test_the_k_by_k_formula_agrees_with_the_rebuild_route(name):
    t = _tables()[name]()
    Phi, f0 = Q.dense_sensitivities(t)
    _, base_flow = R.solve(t)
    assert R.worst(f0, base_flow) <= TOL
    base = Q.base_components(t)
    sizes = [1, 2, 3, 4, 5, 6, 7, 8] * 12
    groups = Q.seeded_groups(t, 17, sizes)
    worst, small_ok, big_isl, n_isl = 0.0, np.inf, 0.0, 0
    for S in groups:
        fr, small = Q.group_flows(Phi, f0, S)
        ref = Q.group_solve(t, S, base)
        if ref is None:                                           # the graph falls apart: the k x k system is singular, and only then
            n_isl += 1
            big_isl = max(big_isl, small)
            assert fr is None, (S, small)
            continue
        small_ok = min(small_ok, small)
        assert fr is not None, (S, small)
        assert all(ref[s] == 0.0 and fr[s] == 0.0 for s in S)
        dev = R.worst(fr, ref)
        assert dev <= TOL, (S, small, dev)
        worst = max(worst, dev)
    print(name, "groups", len(groups), "islanding", n_isl, "largest smallest-pivot islanding", big_isl, "smallest pivot others", small_ok,
          "worst flow deviation of (b) from (a)", worst)
    assert n_isl < len(groups)
    assert big_isl * 100 <= Q.SINGULAR <= small_ok / 100          # DC_SINGULAR separates the two sets by two decades or more on either side


def test_a_joint_cut_of_three_non_bridges_is_singular():
    """mesh 8x8: the three branches at a bus that has exactly three -- no member is a bridge, every pair of them leaves the grid whole, the group cuts
    the bus off"""
    t = G.family("mesh 8x8")
    f, to, on = np.asarray(t["br_from"]) - 1, np.asarray(t["br_to"]) - 1, np.asarray(t["br_status"]) == 1
    slack = R.slack_of(t)
    base = Q.base_components(t)
    found = None
    for bus in range(t["bus_type"].size):
        at = [int(k) for k in np.flatnonzero(on & ((f == bus) | (to == bus)))]
        if bus != slack and len(at) == 3:
            found = tuple(at)
            break
    assert found is not None
    assert not any(Q.islands(t, (k,), base) for k in found)
    assert not any(Q.islands(t, (found[i], found[j]), base) for i in range(3) for j in range(i + 1, 3))
    assert Q.islands(t, found, base)
    Phi, f0 = Q.dense_sensitivities(t)
    fr, small = Q.group_flows(Phi, f0, found)
    print("joint cut", found, "smallest pivot", small)
    assert fr is None and small < 1e-12
