"""Dense numpy restatement of the critical-measurement and critical-pair screen (dcCriticalScreen, csrc/jg_dcse_critical.hip), the check of
tests/test_dcse_critical_host.py and tests/test_dcse_critical_gpu.py, built on tests/dcse_reference.py (matrices, gain).

  screen(t, ms, correlation)   Omega = W^-1 - H G^-1 H' from a DENSE INVERSE of the gain, all m x m entries at once -- never the library's blocks of 512
                               columns on a sparse factor.  Singles: w_i Omega_ii <= SINGULAR among rows in service.  Pairs i < j of the other rows in
                               service: w_j (Omega_jj - Omega_ij^2 / Omega_ii) <= SINGULAR, gamma = sign(Omega_ij); every other pair
                               gamma = Omega_ij / sqrt(Omega_ii Omega_jj).  Partner of row j: the largest |gamma| over the other live rows, the lowest row
                               on ties; -1 where there is none
  thinned_case14 / ordered_case118 / seeded_grid   the three measurement sets of the tests, each with planned or random critical structure

Rows are 0-based here.
"""
from types import SimpleNamespace as NS

import numpy as np

import dc_reference as R
import dcse_reference as S

SINGULAR = 1e-6                  # DCSE_SINGULAR, csrc/jg_dcse.hpp


def screen(t, ms, correlation=None):
    H, w, _, slack = S.matrices(t, ms)
    status = np.asarray(S.rows(t, ms)[1]).astype(bool)
    Hd = H.toarray()
    Gi = np.linalg.inv(S.gain(t, ms).toarray())
    Om = np.diag(1.0 / w) - Hd @ Gi @ Hd.T
    m = w.size
    d = np.diag(Om).copy()
    single = status & (w * d <= SINGULAR)
    live = status & ~single
    both = live[:, None] & live[None, :] & ~np.eye(m, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        pivot = w[None, :] * (d[None, :] - Om ** 2 / d[:, None])               # [i, j]: row i removed first, then row j
        gamma = Om / np.sqrt(np.outer(d, d))
    upper = np.triu(np.ones((m, m), dtype=bool), 1)
    crit_u = both & upper & (pivot <= SINGULAR)
    crit = crit_u | crit_u.T                                                     # the rule is stated for i < j; the partner sees it from both rows
    gamma = np.where(crit, np.sign(Om), gamma)
    gamma[~both] = 0.0
    ag = np.abs(gamma)
    partner = np.full(m, -1, dtype=np.int64)
    pgamma = np.full(m, np.nan)
    gap = np.full(m, np.inf)                                                     # best minus second best |gamma| of a row
    for j in range(m):
        if not live[j] or not ag[:, j].max() > 0.0:
            continue
        i = int(np.argmax(ag[:, j]))                                             # the first of equal maxima
        partner[j], pgamma[j] = i, gamma[i, j]
        rest = np.delete(ag[:, j], i)
        gap[j] = ag[i, j] - (rest.max() if rest.size else 0.0)
    c = -1.0 if correlation is None else float(correlation)
    corr_u = both & upper & ~crit_u & (ag >= c) if c >= 0.0 else np.zeros((m, m), dtype=bool)
    ii, jj = np.nonzero(crit_u | corr_u)                                         # row-major: sorted by (i, j)
    records = np.stack([ii, jj, gamma[ii, jj]], axis=1) if ii.size else np.zeros((0, 3))
    pv = np.where(both & upper, pivot, np.nan)
    return NS(omega=Om, variance=d, status=status, single=single, live=live, gamma=gamma, pivot=pv, critical=np.flatnonzero(single),
              critical_pairs=list(zip(*np.nonzero(crit_u))), records=records, totals=(int(single.sum()), int(crit_u.sum()), int(corr_u.sum())),
              partner=partner, partner_gamma=pgamma, gap=gap, w=w, is_pair=crit_u, is_candidate=both & upper)


def margins(ref):
    """(largest w Omega of a critical row, smallest of another row in service, largest pivot of a critical pair, smallest of another pair)"""
    wo = ref.w * ref.variance
    p = ref.pivot
    return (float(wo[ref.single].max()), float(wo[ref.live].min()), float(p[ref.is_pair].max()), float(p[ref.is_candidate & ~ref.is_pair].min()))


def _leaves(t):
    """(leaf bus, neighbour, branch), all 0-based, of buses with exactly one branch (in service); the slack is left out"""
    f, to = np.asarray(t["br_from"]).astype(int) - 1, np.asarray(t["br_to"]).astype(int) - 1
    n = t["bus_type"].size
    deg = np.bincount(np.r_[f, to], minlength=n)
    out = []
    for b in np.flatnonzero(deg == 1):
        if b == R.slack_of(t):
            continue
        k = int(np.flatnonzero((f == b) | (to == b))[0])
        out.append((int(b), int(to[k] if f[k] == b else f[k]), k))
    return out


def _subset(full, keep_w, keep_p, w_order=None, p_order=None):
    """the rows of a full_set that stay, in the given order"""
    wi = np.flatnonzero(keep_w) if w_order is None else np.asarray([k for k in w_order if keep_w[k]])
    pi = np.flatnonzero(keep_p) if p_order is None else np.asarray([k for k in p_order if keep_p[k]])
    return S.meters(full.w_kind[wi], full.w_index[wi], full.w_mean[wi], full.w_variance[wi], full.w_status[wi], full.p_index[pi], full.p_bus[pi],
                    full.p_angle[pi], full.p_variance[pi], full.p_status[pi])


def _plan(t, full, pair_leaf=None, mixed_leaf=None, single_leaf=None):
    """which rows of the full set leave so that
         pair_leaf     is seen by the from- and the to-wattmeter of its only branch alone (a critical pair)
         mixed_leaf    by the from-wattmeter of its branch and its own PMU alone (a critical pair of a wattmeter and a PMU)
         single_leaf   by its own PMU alone (a critical measurement)"""
    n = t["bus_type"].size
    keep_w, keep_p = np.ones(full.w_index.size, dtype=bool), np.ones(full.p_index.size, dtype=bool)
    inj = lambda b: b                                              # full_set: injections first, then (from, to) per branch
    frm = lambda k: n + 2 * k
    if pair_leaf is not None:
        b, nb, k = pair_leaf
        keep_w[[inj(b), inj(nb)]] = False
        keep_p[b] = False
    if mixed_leaf is not None:
        b, nb, k = mixed_leaf
        keep_w[[inj(b), inj(nb), frm(k) + 1]] = False
    if single_leaf is not None:
        b, nb, k = single_leaf
        keep_w[[inj(b), inj(nb), frm(k), frm(k) + 1]] = False
    return keep_w, keep_p


def thinned_case14(load_case):
    """m < 64: one partial wave.  The only leaf of the 14-bus grid (bus 8) keeps the from- and the to-wattmeter of its branch alone: a critical pair.  Bus
    `lonely` loses every wattmeter that sees it and keeps its PMU: a critical measurement.  One row is out of service.  The slack's angle is 0."""
    t = load_case("case14")
    t = dict(t)
    t["bus_va"] = np.asarray(t["bus_va"], dtype=np.float64).copy()
    t["bus_va"][R.slack_of(t)] = 0.0
    th, _ = R.solve(t)
    full = S.full_set(t, th)
    n = t["bus_type"].size
    f, to = np.asarray(t["br_from"]).astype(int) - 1, np.asarray(t["br_to"]).astype(int) - 1
    leaf, = _leaves(t)
    keep_w, keep_p = _plan(t, full, pair_leaf=leaf)
    deg = np.bincount(np.r_[f, to], minlength=n)
    lonely = next(int(b) for b in np.argsort(deg, kind="stable") if b not in leaf[:2] and b != R.slack_of(t) and deg[b] == 2)
    for k in np.flatnonzero((f == lonely) | (to == lonely)):
        keep_w[[n + 2 * k, n + 2 * k + 1, int(f[k] if to[k] == lonely else to[k])]] = False
    keep_w[lonely] = False
    ms = _subset(full, keep_w, keep_p)
    ms.w_status[3] = 0
    return t, ms, NS(pair=leaf, single=lonely)


def ordered_case118(load_case):
    """m > 512 and no multiple of 512, 64 or 32.  Leaf A: the from- and the to-wattmeter of its branch, neighbours in the stored order, inside one group
    of 64 columns.  Leaf B: the from-wattmeter of its branch (a row of the first block of 512) and its PMU (a row of the second block).  Leaf C: its PMU
    alone.  One row is out of service."""
    t = dict(load_case("case118"))
    t["bus_va"] = np.asarray(t["bus_va"], dtype=np.float64).copy()
    t["bus_va"][R.slack_of(t)] = 0.0
    th, _ = R.solve(t)
    full = S.full_set(t, th)
    lv = sorted(_leaves(t))
    a, c, b = lv[0], lv[1], lv[-1]                                 # B is the leaf with the highest number: its PMU is among the last rows
    keep_w, keep_p = _plan(t, full, pair_leaf=a, mixed_leaf=b, single_leaf=c)
    ms = _subset(full, keep_w, keep_p)
    ms.w_status[40] = 0
    return t, ms, NS(pair=a, mixed=b, single=c)


def seeded_grid(jg=None, seed=49, name="pegaseShaped 160", share_w=0.7, share_p=0.15):
    """a seeded grid of tests/dc_grids.py with a randomly thinned full set: every wattmeter stays with probability share_w, every PMU with share_p, two of
    the wattmeters that stay are out of service.  Nothing is planned; the draw is what the seed gives (tests/test_dcse_critical_host.py pins that the
    gain has full rank and what the set holds)."""
    import dc_grids
    t = dc_grids.family(name, jg)
    th, _ = R.solve(t)
    full = S.full_set(t, th)
    rng = np.random.default_rng(seed)
    keep_w = rng.random(full.w_index.size) < share_w
    keep_p = rng.random(full.p_index.size) < share_p
    ms = _subset(full, keep_w, keep_p)
    off = rng.choice(ms.w_index.size, size=2, replace=False)
    ms.w_status[off] = 0
    return t, ms
