"""numpy / scipy restatement of the reference's DC state estimation (behaviour only), the check of tests/test_dcse_host.py and tests/test_dcse_gpu.py.

  meters(...)            a measurement set as plain arrays: wattmeters in stored order (kind 0 bus / 1 from / 2 to, 1-based index, mean, variance,
                         status), then PMUs (1-based index, at-a-bus flag, angle, variance, status)
  model(t, ms)           dcStateEstimationWls: coefficient (1-based CSC as sparse(row, col, val) stores it: columns ascending, rows ascending inside a
                         column, out-of-service rows as stored zeros), mean, precision, index (PMU -> row; branch PMUs have no row)
  solve(t, ms, z, removed)   solve!: slack column out of H, G = H' W H, G[slack, slack] = 1, theta = G^-1 H' W z, + the slack's angle.  A lane with
                         removed rows REBUILDS H with those rows zeroed (and their means) and refactorises (scipy splu) -- never the low-rank
                         compensation the library uses, and no Omega, no U
  residuals(...)         residualTest!: r = z - H theta (H without the slack column, theta = voltage.angle) and |r_i| / sqrt(|1 / w_i - h_i G^-1 h_i'|) from an splu-solved H G^-1 H' of the REDUCED set
  objective(...)         chiTest: sum w r^2

`t` is a table dict of tests/conftest.py: load_case; the DC model comes from tests/dc_reference.py, which is pinned to the reference's own vectors.
It is pinned to the reference's recorded results by tests/test_dcse_host.py.
"""
from types import SimpleNamespace as NS

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

import dc_reference as R


def meters(w_kind=(), w_index=(), w_mean=(), w_variance=(), w_status=None, p_index=(), p_bus=None, p_angle=(), p_variance=(), p_status=None):
    f = lambda a: np.asarray(a, dtype=np.float64).copy()
    i = lambda a: np.asarray(a, dtype=np.int64).copy()
    nw, npm = len(w_index), len(p_index)
    return NS(w_kind=i(w_kind), w_index=i(w_index), w_mean=f(w_mean), w_variance=f(w_variance), w_status=i(np.ones(nw) if w_status is None else w_status),
              p_index=i(p_index), p_bus=np.ones(npm, dtype=bool) if p_bus is None else np.asarray(p_bus, dtype=bool).copy(), p_angle=f(p_angle),
              p_variance=f(p_variance), p_status=i(np.ones(npm) if p_status is None else p_status))


def full_set(t, th, var_w=1e-2, var_p=1e-5):
    """injection + from + to wattmeters on every bus and every branch, then a PMU on every bus, with exact readings of the DC power flow `th`"""
    n, nb = t["bus_type"].size, np.asarray(t["br_from"]).size
    pw = R.power(t, th)
    fr = pw["from_"]
    kind = np.r_[np.zeros(n), np.tile([1, 2], nb)]
    index = np.r_[np.arange(1, n + 1), np.repeat(np.arange(1, nb + 1), 2)]
    mean = np.r_[pw["injection"], np.stack([fr, -fr], axis=1).reshape(-1)]
    return meters(kind, index, mean, np.full(mean.size, var_w), None, np.arange(1, n + 1), None, th, np.full(n, var_p))


def rows(t, ms):
    """per row of se.coefficient: (columns 0-based, values with status 1), status, variance, the reading z and the constant taken out of it"""
    (colptr, rowval, nzval), y, psh = R.model(t)
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    shift = np.asarray(t["br_shift"], dtype=np.float64)
    slack = R.slack_of(t)
    va_slack = float(np.asarray(t["bus_va"], dtype=np.float64)[slack])
    ent, status, var, z, off = [], [], [], [], []
    for k in range(ms.w_index.size):
        j = int(ms.w_index[k]) - 1
        if ms.w_kind[k] == 0:                                        # column j of the nodal matrix; meanPi
            p = slice(colptr[j] - 1, colptr[j + 1] - 1)
            ent.append((rowval[p] - 1, nzval[p].copy()))
            off.append(-psh[j] - t["bus_gs"][j])
        else:                                                        # +-admittance on the two ends; meanPij
            a = y[j] if ms.w_kind[k] == 1 else -y[j]
            ent.append((np.array([f[j], to[j]]), np.array([a, -a])))
            off.append(shift[j] * a)
        status.append(ms.w_status[k]); var.append(ms.w_variance[k]); z.append(ms.w_mean[k])
    index = {}
    for k in range(ms.p_index.size):
        if not ms.p_bus[k]:
            continue
        index[k] = len(ent)                                          # 0-based PMU -> 0-based row
        ent.append((np.array([int(ms.p_index[k]) - 1]), np.array([1.0])))
        off.append(-va_slack)                                        # meanθi
        status.append(ms.p_status[k]); var.append(ms.p_variance[k]); z.append(ms.p_angle[k])
    return ent, np.array(status, dtype=np.int64), np.array(var), np.array(z), np.array(off), index


def model(t, ms):
    ent, status, var, z, off, index = rows(t, ms)
    n, m = t["bus_type"].size, len(ent)
    r = np.concatenate([np.full(c.size, i) for i, (c, _) in enumerate(ent)])
    c = np.concatenate([c for c, _ in ent])
    v = np.concatenate([v * status[i] for i, (_, v) in enumerate(ent)])
    order = np.lexsort((r, c))                                       # sparse(row, col, val): column-major, rows ascending (no duplicates in a row)
    colptr = np.r_[1, 1 + np.cumsum(np.bincount(c, minlength=n))]
    mean = status * (z + status * off)                               # status * meanPij has status inside the admittance as well: 0 or 1, the same
    return NS(colptr=colptr.astype(np.int64), rowval=(r[order] + 1).astype(np.int64), nzval=v[order], mean=mean, precision=1.0 / var,
              index={k + 1: i + 1 for k, i in index.items()}, number=m, inservice=int(status.sum()))


def matrices(t, ms, z=None, removed=(), drop_slack=True):
    """H (csr, slack column zeroed unless drop_slack is False, out-of-service and removed rows zeroed), w, mean with the same rows zeroed"""
    mo = model(t, ms)
    n, m = t["bus_type"].size, mo.number
    H = sp.csc_matrix((mo.nzval, mo.rowval - 1, mo.colptr - 1), shape=(m, n)).tocsr()
    mean = mo.mean.copy() if z is None else np.asarray(z, dtype=np.float64).copy()
    keep = np.ones(m)
    keep[list(removed)] = 0.0
    mean *= keep
    slack = R.slack_of(t)
    col = np.ones(n)
    if drop_slack:
        col[slack] = 0.0
    H = sp.diags(keep) @ H @ sp.diags(col)
    return H.tocsr(), mo.precision, mean, slack


def gain(t, ms, removed=()):
    H, w, _, slack = matrices(t, ms, None, removed)
    G = (H.T @ sp.diags(w) @ H).tolil()
    G[slack, slack] = 1.0
    return G.tocsc()


def solve(t, ms, z=None, removed=()):
    """theta [n] (slack angle added), or None where the rebuilt gain is singular (the removed rows made the grid unobservable)"""
    H, w, mean, slack = matrices(t, ms, z, removed)
    G = gain(t, ms, removed)
    try:
        lu = sla.splu(G)
    except RuntimeError:
        return None
    d = np.abs(lu.U.diagonal())
    if d.min() <= 1e-10 * d.max():
        return None
    th = lu.solve(H.T @ (w * mean))
    th[slack] = 0.0
    return th + float(np.asarray(t["bus_va"], dtype=np.float64)[slack])


def residuals(t, ms, th, z=None, removed=(), rows=None):
    """(r, normalised residuals) of residualTest! (badData.jl:66-82): rows with r == 0 carry 0.  th is analysis.voltage.angle, the slack's angle
    included: the reference multiplies the coefficient WITHOUT its slack column by that vector, and its recorded 5186.3 for "PMU 10" on the 14-bus grid
    with the slack at -0.17 comes out only this way (5080.4 with the angles relative to the slack).
    rows: normalise only these rows (the others carry NaN): a solve per row is minutes for the 45 412 rows of the 10k-bus grid."""
    H, w, mean, slack = matrices(t, ms, z, removed)
    lu = sla.splu(gain(t, ms, removed))
    r = mean - H @ th
    sel = np.arange(H.shape[0]) if rows is None else np.asarray(sorted(set(int(i) for i in rows)), dtype=np.int64)
    nr = np.full(H.shape[0], np.nan)
    for c0 in range(0, sel.size, 256):
        q = sel[c0:c0 + 256]
        Hq = H[q]
        X = lu.solve(Hq.T.toarray())                                 # G^-1 h_i'  [n, rows of the chunk]
        c = np.asarray(Hq.multiply(sp.csr_matrix(X.T)).sum(axis=1)).ravel()
        nr[q] = np.where(r[q] != 0.0, np.abs(r[q]) / np.sqrt(np.abs(1.0 / w[q] - c)), 0.0)
    return r, nr


def objective(t, ms, th, z=None, removed=()):
    """chiTest (badData.jl:963-977): the FULL coefficient (slack column included) times analysis.voltage.angle"""
    H, w, mean, _ = matrices(t, ms, z, removed, drop_slack=False)
    r = mean - H @ th
    return float(r @ (w * r))


class Rebuilt:
    """one measurement set with the rows `removed` taken out: H rebuilt, the gain assembled and factorised anew (splu), kept for several readings"""

    def __init__(self, t, ms, removed=()):
        self.removed = [int(i) for i in removed]
        self.H, self.w, _, self.slack = matrices(t, ms, None, self.removed)
        self.Hfull = matrices(t, ms, None, self.removed, drop_slack=False)[0]
        self.G = gain(t, ms, self.removed)
        self.va = float(np.asarray(t["bus_va"], dtype=np.float64)[self.slack])
        self.keep = np.ones(self.H.shape[0])
        self.keep[self.removed] = 0.0
        self.status = np.asarray(rows(t, ms)[1], dtype=np.float64) * self.keep
        try:
            self.lu = sla.splu(self.G)
            d = np.abs(self.lu.U.diagonal())
            self.singular = bool(d.min() <= 1e-10 * d.max())
        except RuntimeError:
            self.lu, self.singular = None, True

    def solve(self, z):
        """theta [n] with the slack's angle added; z = se.mean of the lane"""
        z = np.asarray(z, dtype=np.float64) * self.status
        th = self.lu.solve(self.H.T @ (self.w * z))
        th[self.slack] = 0.0
        return th + self.va

    def objective(self, z, th):
        r = np.asarray(z, dtype=np.float64) * self.status - self.Hfull @ th
        return float(r @ (self.w * r))

    def variances(self, rows_=None, dense=False):
        """1 / w_i - h_i G^-1 h_i' of the rows (all by default): from splu solves, or from a dense inverse of the gain (large grids, all rows)"""
        m = self.H.shape[0]
        sel = np.arange(m) if rows_ is None else np.asarray(sorted(set(int(i) for i in rows_)), dtype=np.int64)
        out = np.full(m, np.nan)
        if dense:
            Gi = np.linalg.inv(self.G.toarray())
            Hs = self.H[sel]
            out[sel] = 1.0 / self.w[sel] - np.asarray(Hs.multiply(sp.csr_matrix(Hs @ Gi)).sum(axis=1)).ravel()
            return out
        for c0 in range(0, sel.size, 256):
            q = sel[c0:c0 + 256]
            Hq = self.H[q]
            X = self.lu.solve(Hq.T.toarray())
            out[q] = 1.0 / self.w[q] - np.asarray(Hq.multiply(sp.csr_matrix(X.T)).sum(axis=1)).ravel()
        return out

    def normalized(self, z, th, variances):
        """normalised residuals of residualTest! for one lane (NaN where `variances` is NaN); th = voltage.angle"""
        r = np.asarray(z, dtype=np.float64) * self.status - self.H @ th
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(r != 0.0, np.abs(r) / np.sqrt(np.abs(variances)), 0.0)
