"""The DC transfer-capability screen (dcTransferScreen, csrc/jg_dc_transfer.hip) on the device, against the rebuild route of
tests/dc_transfer_reference.py: dc_reference.solve(t, out=k, injection=P0 + lambda d) -- rebuild and refactorise for every case, never the compensation.
Bridges are held against the graph oracle (connected components), not against any linear algebra.

Every capability is judged in FLOW space, never on lambda (X.check_flow_space): at lambda = TC_got, flows by the rebuild route with k out, S = max(1,
largest monitored loading there) -- the reported branch sits at loading 1 within 1e-9 S, no eligible branch is beyond its rating by more than 1e-9 S on
the side its sensitivity pushes it, and the reported branch differs from the restatement's only where both sit at loading 1 within that tolerance.  The
directions of a test have no monitored |g| within 1e-9 of the cutoff (asserted on the restatement's g).  The rating multiplier of a case was chosen on the
CPU so that the restatement alone finds capabilities of both signs (at least a quarter positive, at least one negative; with dc_pair_reference.rating_of
unscaled every case of case118 is negative).  No case is skipped.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_pair_reference as P
import dc_series_reference as S
import dc_transfer_reference as X
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
MULT = {"case14test": 2.0, "case30test": 0.75, "case118": 2.0, "case300": 8.0, "case_ACTIVSg10k": 4.0, "case9241synth": 4.0}


def same(a, b, dense=True):
    """two results agree bit for bit"""
    names = ["records", "islanding", "worst", "capability", "limitingOutage", "limitingBranch", "base"] + (["capabilityCases", "branch"] if dense else [])
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in names) and a.totals == b.totals and a.overflow == b.overflow


def minima(res):
    """capability, limitingOutage, limitingBranch as the dense result and the base case imply them: base first, then candidates ascending, strict"""
    T = res.transfers
    cap, out, br = res.base[:, 0].copy(), np.zeros(T, dtype=np.int64), res.base[:, 1].astype(np.int64)
    for i, k in enumerate(res.candidates[res.rows[0]:res.rows[1]]):
        for tt in range(T):
            if res.capabilityCases[i, tt] < cap[tt]:
                cap[tt], out[tt], br[tt] = res.capabilityCases[i, tt], k, res.branch[i, tt]
    return cap, out, br


@pytest.mark.parametrize("case,T,with_bridges", [("case14test", 5, True), ("case30test", 1, False), ("case118", 5, False), ("case300", 3, True)])
def test_dense_screen_against_the_rebuild_route_every_case(jg, case, T, with_bridges):
    t = load_case(case)
    s = jg.powerSystem(t)
    rating = MULT[case] * P.rating_of(t)
    P0, D = X.own_injection(t), X.directions(t, T)
    res = jg.dcTransferScreen(s, D, rating=rating, dense=True)
    cand = res.candidates - 1
    bridge = S.bridges(t)
    ref = X.screen(t, cand, D, rating)
    near = X.near_cutoff(ref, rating)
    tc = ref["tc"]
    print(case, "transfers", T, "candidates", cand.size, "cases", tc.size, "restatement: positive", int((tc > 0).sum()), "negative", int((tc < 0).sum()),
          "monitored |g| within 1e-9 of the cutoff", near)
    assert near == 0 and (tc > 0).sum() * 4 >= tc.size and (tc < 0).sum() >= 1
    assert res.capabilityCases.shape == (cand.size, T) and res.transfers == T and res.totals["cases"] == cand.size * T
    assert not np.isin(cand, bridge).any() and res.islanding.size == 0 and res.totals["islanding"] == 0 and res.records.shape == (0, 5)
    worst = 0.0
    for i, k in enumerate(cand):
        for tt in range(T):
            dev, _ = X.check_flow_space(t, rating, int(k), P0, D[tt], res.capabilityCases[i, tt], int(res.branch[i, tt]), ref["f"][int(k)], ref["gs"][int(k)][:, tt],
                                        ref_branch=int(ref["branch"][i, tt]))
            worst = max(worst, dev)
    print(case, "cases", tc.size, "largest |loading - 1| of a reported branch at lambda = TC_got", worst)
    for tt in range(T):                                              # the base case of every transfer
        dev, _ = X.check_flow_space(t, rating, None, P0, D[tt], res.base[tt, 0], int(res.base[tt, 1]), ref["f"][None], ref["gs"][None][:, tt],
                                    ref_branch=int(ref["base"][tt, 1]))
        load0 = P.loading(ref["f"][None], rating)[2]
        nearr = int((np.abs(load0 - 1.0) <= TOL * max(1.0, load0.max())).sum())
        print(case, "transfer", tt, "base capability", res.base[tt, 0], "branch", int(res.base[tt, 1]), "above their rating", int(res.base[tt, 2]), "deviation", dev)
        assert abs(int(res.base[tt, 2]) - int(ref["base"][tt, 2])) <= nearr
    cap, out, br = minima(res)                                       # the per-transfer minima are what the dense result implies
    print(case, "capability", res.capability, "limiting outage", res.limitingOutage, "limiting branch", res.limitingBranch)
    assert np.array_equal(res.capability, cap) and np.array_equal(res.limitingOutage, out) and np.array_equal(res.limitingBranch, br)
    assert np.array_equal(res.worst, res.capabilityCases.min(axis=1))
    if with_bridges:                                                 # ALL in-service branches as candidates: the bridges among them
        every = S.in_service(t) + 1
        full = jg.dcTransferScreen(s, D, candidates=every, rating=rating, dense=True, amount=np.inf)
        isb = np.isin(every - 1, bridge)
        print(case, "all in-service candidates", every.size, "bridges by the graph oracle", int(isb.sum()), "by the screen", full.islanding.size)
        assert isb.sum() > 0 and np.array_equal(full.islanding, every[isb]) and full.totals["islanding"] == int(isb.sum())
        assert np.isnan(full.capabilityCases[isb]).all() and not np.isnan(full.capabilityCases[~isb]).any() and np.isnan(full.worst[isb]).all()
        assert not np.isin(full.records[:, 0], every[isb]).any() and not np.isin(full.limitingOutage, every[isb]).any()
        assert full.totals["limited"] == int(np.isfinite(full.capabilityCases).sum()) == full.records.shape[0]      # amount = +inf: every finite case
        assert np.array_equal(every[~isb], res.candidates)
        assert np.array_equal(full.capabilityCases[~isb], res.capabilityCases) and np.array_equal(full.branch[~isb], res.branch)
        assert np.array_equal(full.capability, res.capability) and np.array_equal(full.limitingOutage, res.limitingOutage) and np.array_equal(full.limitingBranch, res.limitingBranch)


def test_agreement_with_the_series_screen_on_the_device(jg):
    """ratings 1.2 x the largest base / N-1 flow per branch (CPU, rebuild route): nothing violates at zero transfer, so every capability is positive;
    dcSeriesScreen at P0 + capability[t] d_t then has its worst loading (base case and outages) at 1, and at 0.999 capability[t] nothing violates"""
    t = load_case("case118")
    s = jg.powerSystem(t)
    P0, D = X.own_injection(t), X.directions(t, 5)
    cand = jg.pairCandidates(s)
    worst = np.abs(X.R.solve(t, injection=P0)[1])
    for k in cand - 1:
        worst = np.maximum(worst, np.abs(X.R.solve(t, out=int(k), injection=P0)[1]))
    rating = 1.2 * worst
    rating[::7] = 0.0                                                # (some branches not rated)
    an = jg.dcPowerFlow(s)
    res = jg.dcTransferScreen(an, D, rating=rating)
    print("case118: capability", res.capability, "limiting outage", res.limitingOutage, "limiting branch", res.limitingBranch)
    assert (res.capability > 0).all() and np.isfinite(res.capability).all() and (res.base[:, 2] == 0).all()
    at = jg.dcSeriesScreen(an, P0[None, :] + res.capability[:, None] * D, rating=rating)
    below = jg.dcSeriesScreen(an, P0[None, :] + 0.999 * res.capability[:, None] * D, rating=rating)
    an.close()
    w = np.maximum(at.worstProfile, at.base[:, 0])
    print("case118: worst loading of the series screen at the capability", w, "violating at 0.999 of it", below.violatingProfile, below.base[:, 2])
    assert (np.abs(w - 1.0) <= TOL).all()
    assert (np.abs(np.where(res.limitingOutage == 0, at.base[:, 0], at.worstProfile) - 1.0) <= TOL).all()
    assert (below.violatingProfile == 0).all() and (below.base[:, 2] == 0).all()


def test_the_record_list_is_what_the_dense_matrix_implies(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    rating = MULT["case118"] * P.rating_of(t)
    T = 5
    D = X.directions(t, T)
    every = S.in_service(t) + 1                                       # (the bridges ride along: never in the records)
    first = jg.dcTransferScreen(s, D, candidates=every, rating=rating, dense=True)
    assert first.records.shape == (0, 5) and first.totals["limited"] == 0 and not first.overflow          # amount=None gives none
    amount = np.nanmedian(first.capabilityCases, axis=0)             # an amount per transfer that splits its cases
    res = jg.dcTransferScreen(s, D, candidates=every, rating=rating, dense=True, amount=amount)
    cand, nk = res.candidates, res.candidates.size
    assert np.array_equal(res.capabilityCases, first.capabilityCases, equal_nan=True) and np.array_equal(res.branch, first.branch)
    want = [(cand[i], tt, res.branch[i, tt], res.capabilityCases[i, tt]) for i in range(nk) for tt in range(T) if res.capabilityCases[i, tt] < amount[tt]]
    print("case118: cases", res.totals["cases"], "amounts", amount, "limited", res.totals["limited"], "records", res.records.shape[0], "bridges", res.totals["islanding"])
    assert 10 < len(want) < res.totals["cases"] and res.totals["limited"] == len(want) and not res.overflow and res.totals["cases"] == nk * T
    assert np.array_equal(res.records[:, :4], np.array(want, dtype=np.float64))      # same cases, same order (k, t), bit for bit
    P0 = X.own_injection(t)
    for r in res.records[:: max(1, len(want) // 20)]:                 # the fifth entry is g of the limiting branch
        k, tt, b = int(r[0]) - 1, int(r[1]), int(r[2])
        _, g = X.flows_and_sensitivity(t, k, P0, D[tt:tt + 1])
        print("record", r, "restatement's g", g[b - 1, 0])
        assert abs(r[4] - g[b - 1, 0]) <= TOL * max(1.0, np.abs(g).max())
    assert res.totals["islanding"] == int(np.isnan(res.capabilityCases[:, 0]).sum()) > 0
    # a list that overflows keeps the FIRST records by (k, t), the totals and the summaries stay exact
    cut = jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, capacity=7, block=13)
    assert cut.overflow and cut.totals == res.totals and np.array_equal(cut.records, res.records[:7])
    assert same(cut, jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, capacity=7), dense=False)
    for name in ("worst", "capability", "limitingOutage", "limitingBranch", "base", "islanding"):
        assert np.array_equal(getattr(cut, name), getattr(res, name), equal_nan=True), name
    one = jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=float(amount[0]))       # one value for every transfer
    assert one.totals["limited"] == int((res.capabilityCases < amount[0]).sum())


@pytest.mark.parametrize("T", [1, 5, 65])
def test_results_do_not_depend_on_blocks_slices_other_transfers_or_other_screens(jg, T):
    D_ = jg.dcpowerflow
    t = load_case("case14test")
    s = jg.powerSystem(t)
    rating = MULT["case14test"] * P.rating_of(t)
    D = X.directions(t, T)
    every = S.in_service(t) + 1
    amount = 3.0
    ref = jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, dense=True)
    nk = every.size
    print("case14test: transfers", T, "cases", ref.totals["cases"], "limited", ref.totals["limited"], "bridges", ref.totals["islanding"])
    assert 0 < ref.totals["limited"] < ref.totals["cases"]
    cap, out, br = minima(ref)
    assert np.array_equal(ref.capability, cap) and np.array_equal(ref.limitingOutage, out) and np.array_equal(ref.limitingBranch, br)
    for block in (1, 5):                                              # (the default block is `ref`)
        assert same(jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, dense=True, block=block), ref), block
    parts = []
    for k0, k1 in ((0, 3), (3, 11), (11, nk)):                        # slices of the rows, an unaligned first row among them: concatenated, the full screen
        part = jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, dense=True, rows=(k0, k1), block=4)
        parts.append(part)
        lab = every[k0:k1]
        assert part.rows == (k0, k1) and part.totals["cases"] == (k1 - k0) * T
        assert np.array_equal(part.records, ref.records[np.isin(ref.records[:, 0], lab)]) and np.array_equal(part.islanding, ref.islanding[np.isin(ref.islanding, lab)])
        assert np.array_equal(part.worst[k0:k1], ref.worst[k0:k1], equal_nan=True) and np.isinf(part.worst[:k0]).all() and np.isinf(part.worst[k1:]).all()
        assert np.array_equal(part.base, ref.base)
        cap, out, br = minima(part)
        assert np.array_equal(part.capability, cap) and np.array_equal(part.limitingOutage, out) and np.array_equal(part.limitingBranch, br)
    assert np.array_equal(np.vstack([p.capabilityCases for p in parts]), ref.capabilityCases, equal_nan=True)
    assert np.array_equal(np.vstack([p.branch for p in parts]), ref.branch) and np.array_equal(np.vstack([p.records for p in parts]), ref.records)
    if T > 1:                                                         # a subset of the transfers: its columns of the full screen
        a, b = (1, 4) if T == 5 else (3, 62)
        part = jg.dcTransferScreen(s, D[a:b], candidates=every, rating=rating, amount=amount, dense=True)
        assert np.array_equal(part.capabilityCases, ref.capabilityCases[:, a:b], equal_nan=True) and np.array_equal(part.branch, ref.branch[:, a:b])
        assert np.array_equal(part.base, ref.base[a:b]) and np.array_equal(part.capability, ref.capability[a:b]) and np.array_equal(part.limitingOutage, ref.limitingOutage[a:b])
        keep = (ref.records[:, 1] >= a) & (ref.records[:, 1] < b)
        assert np.array_equal(part.records, ref.records[keep] - np.array([0.0, a, 0.0, 0.0, 0.0]))
    if T != 5:
        return
    # on one analysis beside the pair and the series screen, before and after: each result is what a fresh analysis gives
    prof = S.profiles(t, 3)
    pair_ref = jg.dcPairScreen(s, rating=rating, dense=True)
    series_ref = jg.dcSeriesScreen(s, prof, candidates=every, rating=rating, dense=True)
    an = jg.dcPowerFlow(s)
    pair_names = ("records", "islanding", "worst", "loading", "branch", "count", "determinant")
    series_names = ("records", "islanding", "worst", "worstProfile", "violatingProfile", "base", "loading", "branch", "count")
    for order in ("others first", "transfer first"):
        if order == "others first":
            pair_got, series_got = jg.dcPairScreen(an, rating=rating, dense=True), jg.dcSeriesScreen(an, prof, candidates=every, rating=rating, dense=True)
        got = jg.dcTransferScreen(an, D, candidates=every, rating=rating, amount=amount, dense=True)
        assert same(got, ref), order
        if order == "transfer first":
            pair_got, series_got = jg.dcPairScreen(an, rating=rating, dense=True), jg.dcSeriesScreen(an, prof, candidates=every, rating=rating, dense=True)
        for name in pair_names:
            assert np.array_equal(getattr(pair_got, name), getattr(pair_ref, name), equal_nan=True), (order, name)
        for name in series_names:
            assert np.array_equal(getattr(series_got, name), getattr(series_ref, name), equal_nan=True), (order, name)
    # a base profile of the call's own: the system's injections given explicitly are the default
    explicit = jg.dcTransferScreen(an, D, candidates=every, rating=rating, amount=amount, dense=True, injection=X.own_injection(t))
    an.close()
    dev = np.nanmax(np.abs(explicit.capabilityCases - ref.capabilityCases) / np.maximum(1.0, np.abs(ref.capabilityCases)))
    print("case14test: injection given explicitly, largest scaled difference of the capabilities", dev)
    assert dev <= TOL


def _sample(jg, s, seed):
    cand = jg.pairCandidates(s)
    return np.sort(np.random.default_rng(seed).choice(cand, 32, replace=False)).astype(np.int64)


@pytest.mark.parametrize("case", ["case_ACTIVSg10k", "case9241synth"])
def test_large_grid_sample(jg, case):
    t = load_case(case)
    s = jg.powerSystem(t)
    rating = MULT[case] * P.rating_of(t)
    P0, D = X.own_injection(t), X.directions(t, 4)
    sample = _sample(jg, s, 11)
    # cutoff 1e-3 here: of the 2 million monitored sensitivities of such a sample some always lie within 1e-9 of 1e-6 (1 on the 10k-bus grid, 39 on
    # case9241synth, counted on the CPU with the rebuild route), none within 1e-9 of 1e-3 -- the condition every comparison of this file rests on
    cutoff = 1e-3
    res = jg.dcTransferScreen(s, D, candidates=sample, rating=rating, dense=True, cutoff=cutoff)
    assert sample.size == 32 and res.totals["cases"] == 128 and res.totals["islanding"] == 0
    worst, near = 0.0, 0
    rated = rating > 0
    for i, k in enumerate(sample - 1):
        f, g = X.flows_and_sensitivity(t, int(k), P0, D)
        near += int((np.abs(np.abs(g[rated]) - cutoff) <= 1e-9).sum())
        for tt in range(4):
            want = X.limits(f, g[:, tt], rating, int(k), cutoff)
            dev, _ = X.check_flow_space(t, rating, int(k), P0, D[tt], res.capabilityCases[i, tt], int(res.branch[i, tt]), f, g[:, tt], ref_branch=want[1], cutoff=cutoff)
            worst = max(worst, dev)
    print(case, "32 candidates x 4 directions: positive", int((res.capabilityCases > 0).sum()), "negative", int((res.capabilityCases < 0).sum()),
          "monitored |g| within 1e-9 of the cutoff", near, "largest |loading - 1| of a reported branch at lambda = TC_got", worst)
    assert near == 0


def test_a_budget_too_small_is_refused_with_the_sizes(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    rating = MULT["case118"] * P.rating_of(t)
    D = X.directions(t, 70)
    an = jg.dcPowerFlow(s)
    first = jg.dcTransferScreen(an, D, rating=rating)
    need = first.info["phiBytes"] + first.info["gBytes"]
    print("case118, 70 transfers: Phi", first.info["phiBytes"], "bytes, G", first.info["gBytes"], "bytes")
    assert first.info["gBytes"] == first.info["rows"] * 128 * 8
    for budget in (int(first.info["phiBytes"]) + 4096, int(need) - 8):      # Phi alone would fit; Phi + G without their scratch would not
        with pytest.raises(jg._lib.JGridError) as e:
            jg.dcTransferScreen(an, D, rating=rating, budget=budget)
        print(e.value)
        assert e.value.code == 5 and "Phi needs" in str(e.value) and "G needs" in str(e.value) and str(int(first.info["gBytes"])) in str(e.value)
    again = jg.dcTransferScreen(an, D, rating=rating)                   # the analysis still works afterwards
    assert same(again, first, dense=False)
    an.close()


def test_the_host_checks_raise_before_any_device_call(jg, monkeypatch):
    t = load_case("case14test")
    s = jg.powerSystem(t)
    an = jg.dcPowerFlow(s)
    rating = np.ones(s.branch.number)
    D = X.directions(t, 2)

    def touched():
        raise AssertionError("a device call was made")
    monkeypatch.setattr(jg._lib, "lib", touched)
    for kw, err in ((dict(cutoff=0.0), "cutoff"), (dict(transfers=D[0]), "transfers"), (dict(transfers=np.where(D == 0, np.nan, D)), "finite"),
                    (dict(transfers=D * np.array([[1.0], [0.0]])), "transfer 1 is all zero"), (dict(candidates=[]), "one or more")):
        args = dict(dict(transfers=D, rating=rating), **kw)
        with pytest.raises(ValueError, match=err):
            jg.dcTransferScreen(an, **args)
    monkeypatch.undo()
    an.close()
