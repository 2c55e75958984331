"""The DC N-2 screen, host side (no device): the numpy restatement of the Phi / 2 x 2 formulas (tests/dc_pair_reference.py) against the rebuild route on
ALL pairs of the candidate branches, the set of singular pairs against the graph oracle, and the argument checks that run before the device is touched.

Tolerance: max |got - ref| <= 1e-9 * max(1, max |ref|), as in tests/test_dc_gpu.py.  The determinants measured here (largest |det| of an islanding pair,
smallest of the others) are the table of DESIGN.md 3.9."""
import numpy as np
import pytest

import dc_pair_reference as P
import dc_reference as R
from conftest import load_case

TOL = 1e-9


def candidates_of(t):
    import juliagrid.jl_amd as jg
    return jg.pairCandidates(jg.powerSystem(t)) - 1


@pytest.mark.parametrize("case,pairs,islanding", [("case14test", 91, 6), ("case30test", 703, 28), ("case118", 15576, 74)])
def test_the_restatement_agrees_with_the_rebuild_route_on_all_pairs(case, pairs, islanding):
    t = load_case(case)
    cand = candidates_of(t)
    Phi, f0, _ = P.sensitivities(t, cand)
    base = P.base_components(t)
    singular, oracle, worst, big_isl, small_ok, count = set(), set(), 0.0, 0.0, np.inf, 0
    for i in range(cand.size):
        for j in range(i + 1, cand.size):
            count += 1
            k, l = int(cand[i]), int(cand[j])
            fr, det = P.pair_flows(Phi, f0, cand, i, j)
            if fr is None:
                singular.add((k, l))
            if P.islands(t, k, l, base):
                oracle.add((k, l))
                big_isl = max(big_isl, abs(det))
                continue
            small_ok = min(small_ok, abs(det))
            assert fr is not None, (k, l, det)
            _, ref = P.pair_solve(t, k, l)
            assert ref is not None and ref[k] == 0.0 and ref[l] == 0.0
            dev = R.worst(fr, ref)
            assert dev <= TOL, (k, l, det, dev)
            worst = max(worst, dev)
    print(case, "pairs", count, "islanding", len(oracle), "largest |det| islanding", big_isl, "smallest |det| others", small_ok, "worst flow deviation", worst)
    assert count == pairs and len(oracle) == islanding
    assert singular == oracle                                     # the 2 x 2 system is singular exactly where the graph falls apart
    assert big_isl * 100 <= P.SINGULAR <= small_ok / 100          # DC_SINGULAR separates the two sets by two decades or more on either side


def test_a_pair_islands_although_neither_branch_is_a_bridge():
    """the two lines of a radial loop: each alone leaves the grid whole (no candidate is a bridge), both together cut it -- and the 2 x 2 system is singular"""
    t = load_case("case30test")
    cand = candidates_of(t)
    base = P.base_components(t)
    assert not any(P.islands(t, int(k), int(k), base) for k in cand)
    Phi, f0, _ = P.sensitivities(t, cand)
    cut = [(i, j) for i in range(cand.size) for j in range(i + 1, cand.size) if P.islands(t, int(cand[i]), int(cand[j]), base)]
    assert len(cut) == 28
    for i, j in cut:
        fr, det = P.pair_flows(Phi, f0, cand, i, j)
        assert fr is None and abs(det) < 1e-12


def test_arguments_are_refused_before_anything_touches_the_device():
    import juliagrid.jl_amd as jg
    t = load_case("case14test")
    s = jg.powerSystem(t)
    rating = np.ones(s.branch.number)
    off = int(np.flatnonzero(np.asarray(t["br_status"]) != 1)[0]) + 1
    for method in ("nr", "bx", "xb"):
        with pytest.raises(ValueError, match="tuple"):
            jg.contingencyAnalysis(s, [1, (2, 3)], method=method)
    with pytest.raises(IndexError):
        jg.contingencyAnalysis(s, [(1, s.branch.number + 1)], method="dc")          # an unknown branch
    with pytest.raises(ValueError, match="differ"):
        jg.contingencyAnalysis(s, [(4, 4)], method="dc")                            # k == l
    with pytest.raises(IndexError):
        jg.dcPairScreen(s, candidates=[1, 2, s.branch.number + 1], rating=rating)
    with pytest.raises(ValueError, match="twice"):
        jg.dcPairScreen(s, candidates=[1, 2, 2], rating=rating)                     # k == l
    with pytest.raises(ValueError, match="out of service"):
        jg.dcPairScreen(s, candidates=[1, 2, off], rating=rating)
    with pytest.raises(ValueError):
        jg.dcPairScreen(s, candidates=[1, 2, 3])                                    # no rating: nothing to screen against
    with pytest.raises(ValueError):
        jg.dcPairScreen(s, candidates=[1, 2, 3], rating=rating[:-1])
    a, b = jg.dcpowerflow.outagePairs([0, None, 3, (4, 5), (6, 0)], s.branch.number)
    assert a.tolist() == [0, 0, 3, 4, 6] and b.tolist() == [0, 0, 0, 5, 0]
