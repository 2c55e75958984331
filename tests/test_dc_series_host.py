"""The DC N-1 screen over a series of injection profiles, host side (no device): the numpy restatement of the formulas (tests/dc_series_reference.py)
against the rebuild route, the bridges (|1 - Phi[k,k]| < DC_SINGULAR) against the graph oracle, and the argument checks that run before the device is
touched.

Tolerance: |got - ref| <= 1e-9 * max(1, worst |ref| loading), the project's DC one (tests/test_dc_gpu.py).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_pair_reference as P
import dc_series_reference as S
from conftest import load_case

TOL = 1e-9


@pytest.mark.parametrize("case", ["case14test", "case30test"])
def test_the_restatement_agrees_with_the_rebuild_route(case):
    t = load_case(case)
    rating = P.rating_of(t)
    cand = S.in_service(t)
    prof = S.profiles(t, 5)
    Phi, _, _ = P.sensitivities(t, cand)
    F0 = S.base_flows(t, prof)
    bridge = set(int(k) for k in S.bridges(t))
    worst, cases = 0.0, 0
    for i, k in enumerate(cand):
        for tt in range(5):
            fr = S.series_flows(Phi, F0, cand, i, tt)
            if int(k) in bridge:
                assert fr is None, (k, tt)
                continue
            assert fr is not None, (k, tt)
            _, ref = S.rebuild(t, int(k), prof[tt])
            assert ref is not None and ref[k] == 0.0
            w, b, load = P.loading(ref, rating)
            gw, gb, gload = P.loading(fr, rating)
            scale = max(1.0, w)
            dev = max(abs(gw - w), float(np.abs(gload - load).max())) / scale
            assert dev <= TOL, (k, tt, gw, w, dev)
            assert gb == b or abs(load[gb - 1] - w) <= TOL * scale, (k, tt, gb, b)
            worst = max(worst, dev)
            cases += 1
    print(case, "cases", cases, "bridges", len(bridge), "worst scaled deviation of the loadings", worst)
    assert cases == (cand.size - len(bridge)) * 5 and cases > 0


def test_bridges_are_the_candidates_with_a_vanishing_denominator():
    big, small = 0.0, np.inf
    for case in ("case14test", "case30test", "case118", "case300"):
        t = load_case(case)
        cand = S.in_service(t)
        d = np.abs(S.diag(P.sensitivities(t, cand)[0], cand))
        oracle = np.isin(cand, S.bridges(t))
        print(case, "in service", cand.size, "bridges", int(oracle.sum()), "largest |d_k| on a bridge", d[oracle].max(initial=0.0), "smallest |d_k| elsewhere", d[~oracle].min())
        assert np.array_equal(d < S.SINGULAR, oracle)
        big, small = max(big, d[oracle].max(initial=0.0)), min(small, d[~oracle].min())
    print("all four: largest |d_k| on a bridge", big, "smallest elsewhere", small)
    assert big * 100 <= S.SINGULAR <= small / 100                  # two decades on either side of DC_SINGULAR


def test_arguments_are_refused_before_anything_touches_the_device(monkeypatch):
    import juliagrid.jl_amd as jg
    t = load_case("case14test")
    s = jg.powerSystem(t)
    n, nb = s.bus.number, s.branch.number
    rating = np.ones(nb)
    prof = S.profiles(t, 3)
    off = int(np.flatnonzero(np.asarray(t["br_status"]) != 1)[0]) + 1

    def touched():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(jg._lib, "lib", touched)
    with pytest.raises(ValueError, match="rating"):
        jg.dcSeriesScreen(s, prof)                                                  # no rating: nothing to screen against
    with pytest.raises(ValueError):
        jg.dcSeriesScreen(s, prof, rating=rating[:-1])
    for thr in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            jg.dcSeriesScreen(s, prof, rating=rating, threshold=thr)
    for bad in (prof[0], prof[:, :-1], prof[:0], np.zeros((2, 3, n))):              # one profile as a vector, another bus count, empty, 3-D
        with pytest.raises(ValueError, match="injections"):
            jg.dcSeriesScreen(s, bad, rating=rating)
    for v in (np.nan, np.inf):
        q = prof.copy()
        q[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            jg.dcSeriesScreen(s, q, rating=rating)
    with pytest.raises(IndexError):
        jg.dcSeriesScreen(s, prof, candidates=[1, 2, nb + 1], rating=rating)
    with pytest.raises(IndexError):
        jg.dcSeriesScreen(s, prof, candidates=[0, 2], rating=rating)
    with pytest.raises(ValueError, match="twice"):
        jg.dcSeriesScreen(s, prof, candidates=[1, 2, 2], rating=rating)
    with pytest.raises(ValueError, match="out of service"):
        jg.dcSeriesScreen(s, prof, candidates=[1, off], rating=rating)
    with pytest.raises(ValueError, match="one or more"):
        jg.dcSeriesScreen(s, prof, candidates=[], rating=rating)
    with pytest.raises(IndexError):
        jg.dcSeriesScreen(s, prof, candidates=[1], monitored=[1, nb + 1], rating=rating)
    with pytest.raises(ValueError, match="rows"):
        jg.dcSeriesScreen(s, prof, candidates=[1, 2], rating=rating, rows=(2, 1))
    with pytest.raises(ValueError, match="block"):
        jg.dcSeriesScreen(s, prof, candidates=[1, 2], rating=rating, block=0)
