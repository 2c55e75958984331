"""Bridge candidates of the DC transfer-capability screen on the slack's island (dcTransferScreen(..., islands="shed"), csrc/jg_dc_transfer.hip) on the
device.  Every bridge case is judged in FLOW space as tests/dc_transfer_reference.py: check_flow_space does, with the flows of the rebuild route
dc_island_reference.solve(t, out=k, injection=P0 + TC d): the model of the slack's component alone, rebuilt and refactorised, never the identity the
kernel uses.  Which branches are bridges, and what leaves with them, comes from the search of tests/dc_series_shed_reference.py.

Tolerance: the project's DC one, 1e-9 * max(1, largest monitored loading).  No case is skipped.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_island_reference as I
import dc_pair_reference as P
import dc_series_reference as S
import dc_series_shed_reference as H
import dc_transfer_reference as X
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = X.TOL
NAMES = ("capability", "limitingOutage", "limitingBranch", "base", "worst", "records", "islanding", "capabilityCases", "branch")


def flows(t, k, inj):
    return I.solve(t, out=k, injection=inj)[1]


def check_flow_space(t, rating, k, P0, d, tc, branch, monitored=None):
    """X.check_flow_space for a bridge case: f, g and the flows at P0 + tc d by the rebuild route on the slack's component (a branch that left carries 0
    there whatever the injection, so its g is 0 and it is not eligible)"""
    f = flows(t, k, P0)
    g = flows(t, k, P0 + d) - f
    ok = X.eligible(g, rating, k, X.CUTOFF, monitored)
    mon = rating > 0 if monitored is None else np.isin(np.arange(rating.size), monitored) & (rating > 0)
    assert not (np.abs(np.abs(g[mon]) - X.CUTOFF) <= 1e-9).any(), k        # (no sensitivity of the seeded directions sits on the cutoff)
    if not np.isfinite(tc):
        assert tc == np.inf and branch == 0 and not ok.any(), (k, tc, branch, int(ok.sum()))
        return 0.0
    assert branch >= 1 and ok[branch - 1], (k, tc, branch)
    fr = flows(t, k, P0 + tc * d)
    load = P.loading(fr, rating, monitored)[2]
    scale = max(1.0, float(load.max()))
    pushed = np.where(ok, np.sign(g) * fr / np.where(rating > 0, rating, 1.0), 0.0)
    dev = abs(pushed[branch - 1] - 1.0)
    assert dev <= TOL * scale, (k, tc, branch, pushed[branch - 1], scale)
    over = float(pushed.max()) - 1.0
    assert over <= TOL * scale, (k, tc, int(np.argmax(pushed)) + 1, over, scale)
    return dev / scale


def directions(t, br):
    """3 seeded directions: two of tests/dc_transfer_reference.py, and one whose sources lie behind the bridge with the largest side that leaves"""
    D = X.directions(t, 3)
    Sk = max((sp[0] for sp in br.values()), key=lambda m: int(m.sum()))
    rng = np.random.default_rng(9)
    src = rng.choice(np.flatnonzero(Sk), min(3, int(Sk.sum())), replace=False)
    snk = rng.choice(np.flatnonzero(~Sk), 3, replace=False)
    D[2] = 0.0
    D[2, src] = 1.0 / src.size
    D[2, snk] = -1.0 / 3
    return D


def same(a, b, names=NAMES):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in names) and a.totals == b.totals and a.overflow == b.overflow


def grid(case):
    if case == "hand_grid":
        t = I.hand_grid()[0]
        r = 0.05 + 1.2 * np.abs(S.rebuild(t, None, X.own_injection(t))[1])     # ratings at the scale of each branch's own base flow
        r[::7] = 0.0
        return t, r
    t = load_case(case)
    return t, P.rating_of(t)


@pytest.mark.parametrize("case", ["hand_grid", "case14test"])
def test_every_bridge_case_in_flow_space_and_everything_else_bitwise(jg, case):
    t, rating = grid(case)
    s = jg.powerSystem(t)
    br = H.bridges(t)
    D = directions(t, br)
    P0 = X.own_injection(t)
    every = S.in_service(t) + 1
    if case == "case14test":                                         # a candidate count that is no multiple of 4
        every = every[every != int(every[~np.isin(every - 1, list(br))][0])]
        assert every.size % 4 != 0
    amount = np.array([0.5, 2.0, 1.0])
    an = jg.dcPowerFlow(s)
    before = jg.dcTransferScreen(an, D, candidates=every, rating=rating, amount=amount, dense=True)
    res = jg.dcTransferScreen(an, D, candidates=every, rating=rating, amount=amount, dense=True, islands="shed")
    after = jg.dcTransferScreen(an, D, candidates=every, rating=rating, amount=amount, dense=True)
    an.close()
    isb = np.isin(every - 1, list(br))
    print(case, "candidates", every.size, "bridges by the search", int(isb.sum()), "shed by the screen", res.shed.size, "still status 3", res.islanding.size)
    assert np.array_equal(res.shed, every[isb]) and res.islanding.size == 0 and res.totals["islanding"] == 0 and not np.isnan(res.capabilityCases).any()
    # without the keyword: what it was, before and after a shed-mode screen on the same analysis, and on a fresh one after none
    assert same(before, after) and same(before, jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, dense=True))
    assert np.array_equal(before.islanding, every[isb]) and np.isnan(before.capabilityCases[isb]).all() and before.shed is None and before.shedTransfer is None
    # the non-bridge cases: bit for bit those of the call without the keyword
    assert np.array_equal(res.capabilityCases[~isb], before.capabilityCases[~isb]) and np.array_equal(res.branch[~isb], before.branch[~isb])
    assert np.array_equal(res.base, before.base)
    worst = 0.0
    f0 = flows(t, None, P0)
    G = np.stack([flows(t, None, P0 + d) - f0 for d in D], axis=1)
    for j, k in enumerate(sorted(br)):
        i = int(np.flatnonzero(every == k + 1)[0])
        Sk, m, sgn = br[k]
        assert res.shedBuses[j] == int(Sk.sum()) and res.shedM[j] == m + 1
        assert abs(res.shedFlow[j] - sgn * f0[k]) <= TOL * max(1.0, abs(f0[k])) and np.all(np.abs(res.shedTransfer[j] - sgn * G[k]) <= TOL * np.maximum(1.0, np.abs(G[k])))
        for tt in range(3):
            worst = max(worst, check_flow_space(t, rating, k, P0, D[tt], float(res.capabilityCases[i, tt]), int(res.branch[i, tt])))
    behind = np.abs(res.shedTransfer[:, 2]) > 1e-3
    print(case, int(isb.sum()), "bridges x 3 directions: worst scaled deviation of the limiting branch from its rating", worst,
          "; bridges with a part of direction 2 behind them", int(behind.sum()), "largest", float(np.abs(res.shedTransfer).max()))
    assert behind.any()                                              # a source of direction 2 lies in a pocket: part of the direction is shed
    # the summaries take the bridge cases like any other
    assert np.array_equal(res.worst, res.capabilityCases.min(axis=1))
    cases = np.minimum(res.capabilityCases.min(axis=0), res.base[:, 0])
    assert np.array_equal(res.capability, cases)
    want = [(every[i], tt, res.branch[i, tt], res.capabilityCases[i, tt]) for i in range(every.size) for tt in range(3) if res.capabilityCases[i, tt] < amount[tt]]
    onb = int(np.isin(res.records[:, 0], every[isb]).sum())
    print(case, "cases", res.totals["cases"], "limited", res.totals["limited"], "of them on bridge candidates", onb)
    assert res.totals["limited"] == len(want) and np.array_equal(res.records[:, :4], np.array(want, dtype=np.float64).reshape(-1, 4))
    for r in res.records[np.isin(res.records[:, 0], every[isb])]:    # g of the limiting branch of a bridge record, against the rebuild route
        k = int(r[0]) - 1
        g = flows(t, k, P0 + D[int(r[1])]) - flows(t, k, P0)
        assert abs(r[4] - g[int(r[2]) - 1]) <= TOL * max(1.0, float(np.abs(g).max())), r
    # blocks, and a slice of the rows whose first row is no multiple of the kernel's chunk
    for block in (1, 3):
        r = jg.dcTransferScreen(s, D, candidates=every, rating=rating, amount=amount, dense=True, islands="shed", block=block)
        assert same(r, res), block
        for name in ("shed", "shedBuses", "shedM", "shedFlow", "shedTransfer"):
            assert np.array_equal(getattr(r, name), getattr(res, name)), (block, name)
    k0, k1 = 3, every.size - 1
    part = jg.dcTransferScreen(s, D, candidates=every, rating=rating, dense=True, islands="shed", rows=(k0, k1), block=5)
    keep = np.isin(res.shed, every[k0:k1])
    assert np.array_equal(part.capabilityCases, res.capabilityCases[k0:k1]) and np.array_equal(part.branch, res.branch[k0:k1])
    assert np.array_equal(part.shed, res.shed[keep]) and np.array_equal(part.shedTransfer, res.shedTransfer[keep]) and np.array_equal(part.shedFlow, res.shedFlow[keep])
    part = jg.dcTransferScreen(s, D[1:], candidates=every, rating=rating, dense=True, islands="shed")       # a subset of the transfers: its columns
    assert np.array_equal(part.capabilityCases, res.capabilityCases[:, 1:]) and np.array_equal(part.shedTransfer, res.shedTransfer[:, 1:])


def test_a_bridge_whose_outage_leaves_nothing_eligible(jg):
    t, rating = grid("hand_grid")
    s = jg.powerSystem(t)
    br = H.bridges(t)
    k = max(br, key=lambda q: int(br[q][0].sum()))                   # the bridge of the 85-bus pocket
    Sk = br[k][0]
    f, to = np.asarray(t["br_from"]) - 1, np.asarray(t["br_to"]) - 1
    inside = np.flatnonzero(Sk[f] & Sk[to] & (np.asarray(t["br_status"]) == 1) & (rating > 0))
    D = directions(t, br)
    P0 = X.own_injection(t)
    other = min(q for q in S.in_service(t) if q not in br)
    cand = np.array(sorted((k + 1, other + 1)), dtype=np.int64)
    res = jg.dcTransferScreen(s, D, candidates=cand, monitored=inside + 1, rating=rating, dense=True, islands="shed")
    i = int(np.flatnonzero(cand == k + 1)[0])
    print("hand grid: only the", inside.size, "rated branches inside the pocket monitored; bridge", k + 1, "capability", res.capabilityCases[i], "branch", res.branch[i])
    assert inside.size > 10 and np.all(res.capabilityCases[i] == np.inf) and np.all(res.branch[i] == 0) and np.array_equal(res.shed, [k + 1])
    assert np.isfinite(res.capabilityCases[1 - i, 2]) and res.branch[1 - i, 2] > 0                           # with the pocket attached, direction 2 loads it
    for tt in range(3):
        check_flow_space(t, rating, k, P0, D[tt], float(res.capabilityCases[i, tt]), int(res.branch[i, tt]), monitored=inside)


def test_bad_input(jg):
    t, rating = grid("case14test")
    s = jg.powerSystem(t)
    with pytest.raises(ValueError):
        jg.dcTransferScreen(s, X.directions(t, 1), rating=rating, islands="nonsense")
    res = jg.dcTransferScreen(s, X.directions(t, 1), rating=rating, islands="shed")      # the default candidates: every in-service branch, bridges included
    assert np.array_equal(res.candidates, jg.shedCandidates(s)) and res.shed.size == len(H.bridges(t))
