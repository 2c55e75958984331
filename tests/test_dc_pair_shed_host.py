"""Pairs of the DC N-2 screen that hold a bridge, on the slack's island (dcPairScreen(..., islands="shed")), host side (no device): the numpy restatement of
the table of csrc/jg_dc_pair.hpp (tests/dc_pair_shed_reference.py: Restatement) against the rebuild route (rebuild: the DC model of the slack's component
with both branches deleted, refactorised per pair, never the identity).  Which branches are bridges and what leaves with them comes from a search of the
graph, not from the library's table; the table (jg.islandTable, jg.pairShed) is held against that search.

Tolerance: |got - ref| <= 1e-9 * max(1, |ref|) per branch flow, the project's DC one.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_island_reference as I
import dc_pair_shed_reference as Q
import dc_series_shed_reference as H
from conftest import load_case

TOL = 1e-9


def grid(name):
    return I.hand_grid()[0] if name == "hand_grid" else load_case(name)


def every_pair(t, cols, br):
    """every pair of `cols`: the restatement against the rebuild; returns ({kind: pairs}, worst scaled deviation)"""
    g = Q.Grid(t)
    rs = Q.Restatement(t, cols, br, g)
    kinds, worst = {}, 0.0
    for i in range(len(cols)):
        for j in range(i + 1, len(cols)):
            k, l = int(cols[i]), int(cols[j])
            got, kd = rs.flows(i, j)
            kinds[kd] = kinds.get(kd, 0) + 1
            if kd == "plain":
                assert (got is None) == Q.joint_cut(g, k, l), (k, l)      # a joint cut of two non-bridges stays status 3
                if got is None:
                    continue
            assert got is not None, (k, l, kd)                     # no pair with a bridge is singular on these grids
            ref, keep = Q.rebuild(g, k, l)
            if kd != "plain":                                      # what leaves is S_k u S_l: a mixed pair is never a joint cut beyond that
                assert np.array_equal(~keep & g.base, rs.gone(k, l)[1]), (k, l, kd)
            dev = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
            assert dev <= TOL, (k, l, kd, dev)
            assert np.all(got[rs.gone(k, l)[0]] == 0.0) and np.all(ref[rs.gone(k, l)[0]] == 0.0)
            worst = max(worst, dev)
    return kinds, worst


CASES = {"hand_grid": (None, 40), "case14test": (None, 1000), "case300": (40, 40)}


@pytest.mark.parametrize("case", list(CASES))
def test_the_restatement_agrees_with_the_rebuild_route_on_every_pair_of_the_sample(case):
    t = grid(case)
    br = H.bridges(t)
    cols = Q.sample(t, br, *CASES[case])
    nb = int(sum(int(c) in br for c in cols))
    kinds, worst = every_pair(t, cols, br)
    print(case, "candidates", cols.size, "bridges", nb, "pairs by kind", kinds, "worst scaled deviation", worst)
    assert nb == (len(br) if CASES[case][0] is None else CASES[case][0])
    if case == "hand_grid":
        assert nb == 15 and cols.size == 55
    if case != "case14test":                                       # all four kinds with a bridge occur
        assert all(kinds.get(kd, 0) > 0 for kd in ("outside", "disjoint", "inside", "nested")), kinds
    assert kinds.get("outside", 0) > 0 and kinds.get("plain", 0) > 0


@pytest.mark.parametrize("case", ["hand_grid", "case14test", "case300"])
def test_nestedness_from_the_table_agrees_with_the_search(case):
    import juliagrid.jl_amd as jg
    t = grid(case)
    g = Q.Grid(t)
    br = H.bridges(t)
    tb = jg.islandTable(jg.powerSystem(t))
    assert sorted(br) == [int(k) for k in np.flatnonzero(tb.side != 0)]
    ks = sorted(br)
    nested = 0
    for a in ks:
        for b in ks:
            if a == b:
                continue
            inside = not (br[b][0] & ~br[a][0]).any()              # S_b inside S_a, by the searched sides
            assert inside == bool(tb.lo[a] <= tb.lo[b] and tb.hi[b] <= tb.hi[a]), (a, b)
            disjoint = not (br[a][0] & br[b][0]).any()
            assert inside or disjoint or not (br[a][0] & ~br[b][0]).any(), (a, b)      # nested or disjoint, nothing else
            nested += inside
        for l in np.flatnonzero(g.y != 0):                         # "behind" is one test for every kind of branch: preorder[from] in the interval
            if int(l) != a:
                behind = bool(br[a][0][g.f[l]] and br[a][0][g.to[l]])
                assert behind == bool(tb.lo[a] <= tb.preorder[g.f[l]] <= tb.hi[a]), (a, int(l))
    print(case, "bridges", len(ks), "ordered nested pairs", nested)


def test_record_shed_on_hand_picked_pairs():
    import juliagrid.jl_amd as jg
    t, marks, _ = I.hand_grid()
    s = jg.powerSystem(t)
    lab = {name: [k + 1 for k in ks] for name, ks in marks.items()}
    core = 1                                                       # a ring branch of the core
    far = lab["far"]
    pairs = [(lab["chain"][0], lab["chain"][1]),                   # nested: only the outer one
             (far[0], far[9]), (far[3], far[4]), (far[9], far[0]),  # a path of ten nested bridges, in either order
             (core, lab["pocket"][0]),                             # a bridge with a core branch
             (lab["at_slack"][0], lab["pocket"][0]), (lab["at_slack"][0], core), (lab["at_slack"][0], far[5]),      # the bridge at the slack with any other
             (lab["doubled"][0], lab["behind_doubled"][0]), (lab["doubled"][0], lab["doubled"][1]),                 # a doubled branch is no bridge
             (lab["behind_doubled"][0], far[2]), (core, 2)]
    want = [(lab["chain"][0], 0), (far[0], 0), (far[3], 0), (0, far[0]), (0, lab["pocket"][0]),
            (lab["at_slack"][0], lab["pocket"][0]), (lab["at_slack"][0], 0), (lab["at_slack"][0], far[5]),
            (0, lab["behind_doubled"][0]), (0, 0), (lab["behind_doubled"][0], far[2]), (0, 0)]
    got = jg.pairShed(s, pairs)
    print(np.c_[np.array(pairs), got])
    assert got.dtype == np.int64 and np.array_equal(got, np.array(want, dtype=np.int64))
    assert jg.pairShed(s, np.zeros((0, 2))).shape == (0, 2)


def test_arguments_are_refused_before_the_device_is_touched():
    import juliagrid.jl_amd as jg
    t = load_case("case14test")
    s = jg.powerSystem(t)
    with pytest.raises(ValueError):
        jg.dcPairScreen(s, rating=np.ones(t["br_from"].size), islands="both")
