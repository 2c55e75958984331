"""What the DC transfer-capability screen is held against (tests/test_dc_transfer_host.py, tests/test_dc_transfer_gpu.py): the reference's user loop, restated
in numpy on the REBUILD route -- every flow comes from dc_reference.solve(t, out=k, injection=...), which rebuilds and refactorises for the outage, never
from the compensation the library uses.

  own_injection(t)          P0: the case's own net injections, supply - demand per bus
  directions(t, T)          seeded transfer directions [T, buses]: +1 over 3 source buses, -1 over 3 sink buses, seeded shares
  flows_and_sensitivity(t, k, P0, D)   f [branches] = from-flows at P0 with branch k (0-based, or None) out; g [branches, T] = flows at P0 + d_t minus f
                            (the flows are affine in the injection, so the difference is the sensitivity; the slack takes what d_t does not balance)
  limits(f, g, rating, k, cutoff, monitored)   TC and its branch by the formula: limit_m = (sign(g) r_m - f) / g over the eligible rows (monitored,
                            rated, m != k, |g| > cutoff), the least of them, ties to the lowest branch; (+inf, 0) when no row is eligible
  screen(t, cand, D, ...)   the whole restatement: TC [K, T], branch [K, T], g of the limiting branch, base [T, 3]; bridges from the graph oracle (NaN rows)
  check_flow_space(...)     the comparison every test uses: a capability is judged by the FLOWS at lambda = TC on the rebuild route, never by lambda itself
                            (a limiting branch may move by as little as 3e-6 per unit of transfer, with TC in the hundreds)
"""
import numpy as np

import dc_pair_reference as P
import dc_reference as R
import dc_series_reference as S

TOL = 1e-9                          # the project's DC tolerance
CUTOFF = 1e-6                       # default cutoff of dcTransferScreen


def own_injection(t):
    return R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64)


def directions(t, T, seed=5):
    n = t["bus_type"].size
    rng = np.random.default_rng(seed)
    D = np.zeros((T, n))
    for i in range(T):
        pick = rng.choice(n, 6, replace=False)
        for buses, sign in ((pick[:3], 1.0), (pick[3:], -1.0)):
            w = 0.2 + rng.random(3)
            D[i, buses] = sign * w / w.sum()
    return D


def flows_and_sensitivity(t, k, P0, D):
    """(f, g) with branch k out of service by the rebuild route; (None, None) when the rebuilt matrix is singular"""
    _, f = R.solve(t, out=k, injection=P0)
    if f is None:
        return None, None
    g = np.stack([R.solve(t, out=k, injection=P0 + d)[1] - f for d in D], axis=1)
    return f, g


def eligible(g, rating, k, cutoff=CUTOFF, monitored=None):
    ok = (rating > 0) & (np.abs(g) > cutoff)
    if monitored is not None:
        m = np.zeros(rating.size, dtype=bool)
        m[monitored] = True
        ok &= m
    if k is not None:
        ok[k] = False
    return ok


def limits(f, g, rating, k, cutoff=CUTOFF, monitored=None):
    """(TC, branch 1-based or 0, g of that branch or 0) of one case: f, g [branches] of the case"""
    ok = eligible(g, rating, k, cutoff, monitored)
    if not ok.any():
        return np.inf, 0, 0.0
    lim = np.full(rating.size, np.inf)
    lim[ok] = (np.sign(g[ok]) * rating[ok] - f[ok]) / g[ok]
    b = int(np.argmin(lim))                                       # (the first of equal values: the lowest branch)
    return float(lim[b]), b + 1, float(g[b])


def screen(t, cand, D, rating, P0=None, cutoff=CUTOFF, monitored=None):
    """dict(tc [K, T], branch [K, T], g [K, T], base [T, 3], f {k: f}, gs {k: g}) for the candidates `cand` (0-based; None inside f / gs is the base case)"""
    P0 = own_injection(t) if P0 is None else P0
    bridge = set(int(x) for x in S.bridges(t))
    K, T = len(cand), D.shape[0]
    out = dict(tc=np.full((K, T), np.nan), branch=np.zeros((K, T), dtype=np.int64), g=np.zeros((K, T)), base=np.zeros((T, 3)), f={}, gs={})
    f, g = flows_and_sensitivity(t, None, P0, D)
    out["f"][None], out["gs"][None] = f, g
    rated = rating > 0
    if monitored is not None:
        m = np.zeros(rating.size, dtype=bool)
        m[monitored] = True
        rated &= m
    above = int((np.abs(f[rated]) / rating[rated] > 1.0).sum())
    for tt in range(T):
        tc, b, _ = limits(f, g[:, tt], rating, None, cutoff, monitored)
        out["base"][tt] = (tc, b, above)
    for i, k in enumerate(cand):
        if int(k) in bridge:
            continue
        f, g = flows_and_sensitivity(t, int(k), P0, D)
        assert f is not None, k
        out["f"][int(k)], out["gs"][int(k)] = f, g
        for tt in range(T):
            out["tc"][i, tt], out["branch"][i, tt], out["g"][i, tt] = limits(f, g[:, tt], rating, int(k), cutoff, monitored)
    return out


def near_cutoff(ref, rating, cutoff=CUTOFF, monitored=None):
    """number of (case, monitored rated branch) whose |g| lies within 1e-9 of the cutoff: a test's directions must have none"""
    ok = rating > 0
    if monitored is not None:
        m = np.zeros(rating.size, dtype=bool)
        m[monitored] = True
        ok &= m
    return int(sum((np.abs(np.abs(g[ok]) - cutoff) <= 1e-9).sum() for g in ref["gs"].values()))


def check_flow_space(t, rating, k, P0, d, tc, branch, f, g, ref_branch=None, cutoff=CUTOFF, monitored=None):
    """One case (outage k 0-based or None, direction d) in flow space: `tc`, `branch` are what is judged, f / g [branches] the restatement's flows and
    sensitivity of the case (they decide who is eligible and which side a branch is pushed to).  At lambda = tc, flows by the rebuild route at
    P0 + tc d with k out, S = max(1, largest monitored loading): the reported branch sits at loading 1 within TOL S on the side its g pushes it, no
    eligible branch is beyond its rating on that side by more than TOL S, and the reported branch may differ from `ref_branch` only where both sit at
    loading 1 within that tolerance.  tc = +inf: no row is eligible and no branch is reported.  Returns (deviation of the reported branch from 1, S)."""
    ok = eligible(g, rating, k, cutoff, monitored)
    if not np.isfinite(tc):
        assert tc == np.inf and branch == 0 and not ok.any(), (k, tc, branch, int(ok.sum()))
        return 0.0, 1.0
    assert branch >= 1 and ok[branch - 1], (k, tc, branch)
    _, fr = R.solve(t, out=k, injection=P0 + tc * d)
    assert fr is not None, k
    load = P.loading(fr, rating, monitored)[2]
    scale = max(1.0, float(load.max()))
    pushed = np.where(ok, np.sign(g) * fr / np.where(rating > 0, rating, 1.0), 0.0)
    dev = abs(pushed[branch - 1] - 1.0)
    assert dev <= TOL * scale, (k, tc, branch, pushed[branch - 1], scale)
    over = float(pushed.max()) - 1.0
    assert over <= TOL * scale, (k, tc, int(np.argmax(pushed)) + 1, over, scale)
    if ref_branch is not None and ref_branch != branch:
        assert ref_branch >= 1 and abs(pushed[ref_branch - 1] - 1.0) <= TOL * scale, (k, branch, ref_branch, pushed[ref_branch - 1])
    return dev, scale
