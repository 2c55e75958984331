"""The DC transfer-capability screen, host side (no device): the numpy restatement of tests/dc_transfer_reference.py (flows and sensitivities by the
rebuild route, limits by the formula) against the flow-space check -- at lambda = TC the reported branch sits at its rating and no eligible branch is beyond
it -- and the argument checks that run before the device is touched.

Tolerance: the project's DC one, 1e-9 x max(1, largest monitored loading at lambda = TC).  Every figure is printed before it is asserted.  The rating
multiplier of a case is the one tests/test_dc_transfer_gpu.py uses: chosen so that the restatement finds capabilities of both signs."""
import numpy as np
import pytest

import dc_pair_reference as P
import dc_series_reference as S
import dc_transfer_reference as X
from conftest import load_case

CASES = [("case14test", 5, 2.0), ("case30test", 1, 0.75), ("case118", 5, 2.0), ("case300", 3, 8.0)]      # case, transfers, rating multiplier


@pytest.mark.parametrize("case,T,mult", CASES)
def test_the_restatement_holds_in_flow_space(case, T, mult):
    t = load_case(case)
    rating = mult * P.rating_of(t)
    cand = np.setdiff1d(S.in_service(t), S.bridges(t))
    f, to = np.asarray(t["br_from"]), np.asarray(t["br_to"])
    cand = cand[f[cand] != to[cand]]
    P0, D = X.own_injection(t), X.directions(t, T)
    ref = X.screen(t, cand, D, rating)
    near = X.near_cutoff(ref, rating)
    tc = ref["tc"]
    print(case, "candidates", cand.size, "transfers", T, "cases", tc.size, "positive", int((tc > 0).sum()), "negative", int((tc < 0).sum()),
          "monitored |g| within 1e-9 of the cutoff", near)
    assert near == 0
    assert (tc > 0).sum() * 4 >= tc.size and (tc < 0).sum() >= 1 and not np.isnan(tc).any()
    worst, small = 0.0, np.inf
    for i, k in enumerate(cand):
        for tt in range(T):
            dev, _ = X.check_flow_space(t, rating, int(k), P0, D[tt], tc[i, tt], int(ref["branch"][i, tt]), ref["f"][int(k)], ref["gs"][int(k)][:, tt])
            worst, small = max(worst, dev), min(small, abs(ref["g"][i, tt]))
    for tt in range(T):
        dev, _ = X.check_flow_space(t, rating, None, P0, D[tt], ref["base"][tt, 0], int(ref["base"][tt, 1]), ref["f"][None], ref["gs"][None][:, tt])
        worst = max(worst, dev)
    print(case, "largest |loading - 1| of a reported branch at lambda = TC", worst, "smallest limiting |g|", small)


def test_a_direction_that_does_not_balance_is_taken_by_the_slack():
    """the sensitivity of a direction equals that of the direction with the slack's entry set to whatever balances it"""
    import dc_reference as R
    t = load_case("case14test")
    P0 = X.own_injection(t)
    d = X.directions(t, 1)[0]
    d[3] += 0.25                                                   # no longer sums to zero
    e = d.copy()
    e[R.slack_of(t)] -= e.sum()
    _, ga = X.flows_and_sensitivity(t, None, P0, d[None, :])
    _, gb = X.flows_and_sensitivity(t, None, P0, e[None, :])
    print("case14test: sum of the direction", d.sum(), "largest difference of the sensitivities", float(np.abs(ga - gb).max()))
    assert abs(d.sum()) > 0.2 and np.abs(ga - gb).max() <= 1e-12


def test_transfer_direction():
    import juliagrid.jl_amd as jg
    t = load_case("case14test")
    s = jg.powerSystem(t)
    lab = sorted(s.bus.label)
    d = jg.transferDirection(s, lab[:2], [lab[4]])
    assert d.shape == (s.bus.number,) and d[s.bus.label[lab[0]] - 1] == 0.5 and d[s.bus.label[lab[1]] - 1] == 0.5 and d[s.bus.label[lab[4]] - 1] == -1.0
    assert np.count_nonzero(d) == 3 and abs(d.sum()) < 1e-15
    d = jg.transferDirection(s, lab[:2], lab[5:8], sourceShare=[3, 1], sinkShare=[2, 2, 4])
    assert np.allclose(d[[s.bus.label[x] - 1 for x in lab[:2]]], [0.75, 0.25]) and np.allclose(d[[s.bus.label[x] - 1 for x in lab[5:8]]], [-0.25, -0.25, -0.5])
    with pytest.raises(KeyError):
        jg.transferDirection(s, [max(lab) + 1], [lab[0]])
    with pytest.raises(ValueError):
        jg.transferDirection(s, [], [lab[0]])
    with pytest.raises(ValueError, match="Share"):
        jg.transferDirection(s, lab[:2], [lab[4]], sourceShare=[1.0])
    with pytest.raises(ValueError, match="Share"):
        jg.transferDirection(s, lab[:2], [lab[4]], sourceShare=[0.0, 0.0])


def test_arguments_are_refused_before_anything_touches_the_device(monkeypatch):
    import juliagrid.jl_amd as jg
    t = load_case("case14test")
    s = jg.powerSystem(t)
    n, nb = s.bus.number, s.branch.number
    rating = np.ones(nb)
    D = X.directions(t, 3)
    off = int(np.flatnonzero(np.asarray(t["br_status"]) != 1)[0]) + 1

    def touched():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(jg._lib, "lib", touched)
    with pytest.raises(ValueError, match="rating"):
        jg.dcTransferScreen(s, D)                                                   # no rating: nothing limits
    with pytest.raises(ValueError):
        jg.dcTransferScreen(s, D, rating=rating[:-1])
    for c in (0.0, -1e-6, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            jg.dcTransferScreen(s, D, rating=rating, cutoff=c)
    for bad in (D[0], D[:, :-1], D[:0], np.zeros((2, 3, n))):                       # one direction as a vector, another bus count, empty, 3-D
        with pytest.raises(ValueError, match="transfers"):
            jg.dcTransferScreen(s, bad, rating=rating)
    for v in (np.nan, np.inf):
        q = D.copy()
        q[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            jg.dcTransferScreen(s, q, rating=rating)
    q = D.copy()
    q[2] = 0.0
    with pytest.raises(ValueError, match="transfer 2 is all zero"):
        jg.dcTransferScreen(s, q, rating=rating)
    with pytest.raises(ValueError, match="amount"):
        jg.dcTransferScreen(s, D, rating=rating, amount=[1.0, 2.0])
    with pytest.raises(ValueError, match="amount"):
        jg.dcTransferScreen(s, D, rating=rating, amount=float("nan"))
    with pytest.raises(ValueError, match="injection"):
        jg.dcTransferScreen(s, D, rating=rating, injection=np.zeros(n - 1))
    with pytest.raises(IndexError):
        jg.dcTransferScreen(s, D, candidates=[1, 2, nb + 1], rating=rating)
    with pytest.raises(ValueError, match="twice"):
        jg.dcTransferScreen(s, D, candidates=[1, 2, 2], rating=rating)
    with pytest.raises(ValueError, match="out of service"):
        jg.dcTransferScreen(s, D, candidates=[1, off], rating=rating)
    with pytest.raises(ValueError, match="one or more"):
        jg.dcTransferScreen(s, D, candidates=[], rating=rating)
    with pytest.raises(IndexError):
        jg.dcTransferScreen(s, D, candidates=[1], monitored=[1, nb + 1], rating=rating)
    with pytest.raises(ValueError, match="rows"):
        jg.dcTransferScreen(s, D, candidates=[1, 2], rating=rating, rows=(2, 1))
    with pytest.raises(ValueError, match="block"):
        jg.dcTransferScreen(s, D, candidates=[1, 2], rating=rating, block=0)
