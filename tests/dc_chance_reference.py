"""What the DC probabilistic N-1 screen (dcChanceScreen, csrc/jg_dc_chance.hip) is held against: the rebuild-and-refactorise route, never the
compensation (tests/test_dc_chance_host.py, tests/test_dc_chance_gpu.py).

  factors(t, r, seed)            seeded factors L [r, buses]: every row N(0, 1) x 0.1 x |own injection| on a seeded subset of the buses that inject;
                                 row 0 always has a non-zero entry at the slack (which every route must ignore).  The first r rows of factors(t, 32, seed)
                                 ARE factors(t, r, seed): a grid's references for several r share their solves
  rebuild(t, k, p0, L)           (mu, S) with branch k (0-based, or None: the base case) out of service: mu = dc_reference.solve(t, out=k, injection=p0),
                                 column j of S = solve(t, out=k, injection=L_j) - solve(t, out=k, injection=0), which removes the shift-angle part.  The
                                 matrix is rebuilt without k and refactorised by every solve.  None when the rebuilt matrix is singular or k is a bridge
  moments(t, cand, p0, L)        per candidate of `cand`: (mu [branches], S [branches, r]) or None; computed by rebuild
  probability(mu, sigma, rating) P(|f| > rating) of f ~ N(mu, sigma^2) with scipy's erfc; sigma == 0: 1 if |mu| > rating, else 0; unrated: 0
  sample_flows(t, k, P)          flows [T, branches] of the injections P [T, buses] with branch k out of service: the rebuilt matrix, refactorised once,
                                 solved for every sample (the Monte-Carlo route)
  formula(Phi, f0, S0, cols, i)  the screen's formula in numpy on a dense Phi (dc_pair_reference.sensitivities): (mu, sigma) [branches] for the candidate
                                 at position i of `cols`; None below SINGULAR.  expanded(...) is the same with the variance expanded over a Gram matrix,
                                 the form csrc/jg_dc_chance.hpp rules out

  candidates_of(t)               the candidates the tests screen (0-based, ascending): every in-service branch that is no self-loop, bridges included; of
                                 more than 70, a seeded choice of 70 (two lane chunks, the second partly filled)
  records_of(mom, cand, rating, mon, thr)   the reference records [(k label, m label, P)] sorted by (k, m), and the number of cases whose P lies within
                                 NEAR of thr (left out of a comparison of record SETS; the tests cap their share at 1 % of the records)

Bridges: dc_series_reference.bridges (the graph).  Ratings: dc_pair_reference.rating_of.  SEED and PROBABILITY are what the host and the device tests share:
the host test checks on the CPU that no grid of GRIDS has more than 1 % of its reference records within NEAR of PROBABILITY."""
import numpy as np
import scipy.sparse.linalg as sla
from scipy.special import erfc

import dc_pair_reference as P
import dc_reference as R
import dc_series_reference as SR

GRIDS = ("case14test", "case30test", "case118", "pegaseShaped 160")
SEED, PROBABILITY, NEAR = 5, 0.05, 1e-6
SINGULAR = P.SINGULAR               # DC_SINGULAR of csrc/jg_dc.hpp
rating_of = P.rating_of
bridges = SR.bridges


def own_injection(t):
    return R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64)


def factors(t, r, seed=5, most=32):
    rng = np.random.default_rng(seed)
    own = own_injection(t)
    n = own.size
    live = np.flatnonzero(own != 0.0)
    L = np.zeros((most, n))
    for j in range(most):
        at = rng.choice(live, size=max(1, min(live.size, 2 + live.size // 3)), replace=False)
        L[j, at] = rng.standard_normal(at.size) * 0.1 * np.abs(own[at])
    L[0, R.slack_of(t)] = 0.1 * float(np.abs(own).max())                # the slack takes what a factor does not balance: this entry moves nothing
    assert r <= most
    return L[:r].copy()


def rebuild(t, k, p0, L):
    mu = R.solve(t, out=k, injection=p0)[1]
    if mu is None or not np.isfinite(mu).all():
        return None
    zero = R.solve(t, out=k, injection=np.zeros(p0.size))[1]
    S = np.stack([R.solve(t, out=k, injection=Lj)[1] - zero for Lj in L], axis=1)
    return mu, S


def moments(t, cand, p0, L):
    br = set(int(b) for b in bridges(t))
    return [None if int(k) in br else rebuild(t, int(k), p0, L) for k in cand]


def probability(mu, sigma, rating):
    mu, sigma, rating = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64), np.asarray(rating, dtype=np.float64))
    rated, rand = rating > 0, sigma > 0
    s = np.where(rand, sigma, 1.0) * np.sqrt(2.0)
    p = 0.5 * erfc((rating - mu) / s) + 0.5 * erfc((rating + mu) / s)
    p = np.where(rand, p, (np.abs(mu) > rating).astype(np.float64))
    return np.where(rated, p, 0.0)


def sample_flows(t, k, Pn):
    B, y, psh = R.assemble(t, k)
    n = t["bus_type"].size
    slack = R.slack_of(t)
    keep = np.r_[0:slack, slack + 1:n]
    lu = sla.splu(B[keep][:, keep].tocsc())
    rhs = (np.asarray(Pn, dtype=np.float64) - np.asarray(t["bus_gs"], dtype=np.float64)[None, :] - psh[None, :]).T
    th = np.zeros((n, rhs.shape[1]))
    th[keep] = lu.solve(np.ascontiguousarray(rhs[keep]))
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    return (y[:, None] * (th[f] - th[to] - np.asarray(t["br_shift"], dtype=np.float64)[:, None])).T


def formula(Phi, f0, S0, cols, i):
    k = cols[i]
    d = 1.0 - Phi[k, i]
    if abs(d) < SINGULAR:
        return None
    g = Phi[:, i] / d
    mu = f0 + g * f0[k]
    sigma = np.sqrt(((S0 + g[:, None] * S0[k][None, :]) ** 2).sum(axis=1))       # the squares of the COMBINED sensitivities
    mu[k] = sigma[k] = 0.0
    return mu, sigma


def expanded(Phi, S0, cols, i):
    """the variance as v_m + 2 g <S_m, S_k> + g^2 v_k: what the screen does NOT compute"""
    k = cols[i]
    g = Phi[:, i] / (1.0 - Phi[k, i])
    v = (S0 ** 2).sum(axis=1)
    return v + 2.0 * g * (S0 @ S0[k]) + g * g * v[k]


def candidates_of(t, most=70, seed=17):
    on = np.flatnonzero((np.asarray(t["br_status"]).astype(np.int64) == 1) & (np.asarray(t["br_from"]) != np.asarray(t["br_to"])))
    if on.size > most:
        on = np.sort(np.random.default_rng(seed).choice(on, size=most, replace=False))
    return [int(k) for k in on]


def records_of(mom, cand, rating, mon, thr):
    rec, near = [], 0
    for k, m in zip(cand, mom):
        if m is None:
            continue
        mu, S = m
        p = probability(mu[mon], np.sqrt((S[mon] ** 2).sum(axis=1)), rating[mon])
        p[np.asarray(mon) == k] = 0.0
        near += int((np.abs(p - thr) <= NEAR).sum())
        rec += [(k + 1, int(mon[j]) + 1, float(p[j])) for j in np.flatnonzero(p >= thr)]
    return rec, near


_CACHE = {}


def grid(name):
    """per grid of GRIDS, computed once and left unchanged: dict(t, cand, p0, L [32, buses], mom (moments of every candidate for the 32 factors), base (the
    base case's (mu, S)), rating).  The reference of r < 32 factors is the first r columns of every S"""
    if name not in _CACHE:
        import dc_grids as G
        from conftest import load_case
        t = G.family(name) if name in G.FAMILIES else load_case(name)
        cand, p0, L = candidates_of(t), own_injection(t), factors(t, 32, SEED)
        _CACHE[name] = dict(t=t, cand=cand, p0=p0, L=L, mom=moments(t, cand, p0, L), base=rebuild(t, None, p0, L), rating=rating_of(t))
    return _CACHE[name]


def cut(mom, r):
    """the moments of the first r factors"""
    return [None if m is None else (m[0], m[1][:, :r]) for m in mom]
