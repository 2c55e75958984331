"""The reference's user loop for a PAIR of outages, and what the DC N-2 screen is held against (tests/test_dc_pair_host.py, tests/test_dc_pair_gpu.py).

  pair_solve(t, k, l)      updateBranch!(k, status = 0), updateBranch!(l, status = 0), solve!, power!: the second branch goes out of service in a COPY of
                           the case table, then dc_reference.solve(t2, out=k) -- rebuild and refactorise, never the compensation
  islands(t, k, l)         the islanding oracle, independent of any linear algebra: both branches leave the bus graph; True when the number of connected
                           components among the buses grows (scipy.sparse.csgraph.connected_components)
  sensitivities(t, cols)   numpy restatement of the issue's formulas: Phi[:, cols] = y_m a_m' B^-1 a_k and the base flows f0
  pair_flows(...)          f_m(S) = f0_m + Phi[m,k] c_k + Phi[m,l] c_l with the 2 x 2 system (I - Phi_SS) c = f0_S; returns (flows, det)
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla
from scipy.sparse.csgraph import connected_components

import dc_reference as R

SINGULAR = 1e-9                     # DC_SINGULAR of csrc/jg_dc.hpp


def pair_solve(t, k, l, injection=None):
    """(theta, from) with branches k and l (0-based) out of service, by the rebuild route"""
    t2 = dict(t)
    t2["br_status"] = np.array(t["br_status"]).copy()
    t2["br_status"][l] = 0
    th, fr = R.solve(t2, out=k, injection=injection)
    return th, fr


def _components(t, out=()):
    n = t["bus_type"].size
    on = np.asarray(t["br_status"]).astype(np.int64) == 1
    on[list(out)] = False
    f = np.asarray(t["br_from"]).astype(np.int64)[on] - 1
    to = np.asarray(t["br_to"]).astype(np.int64)[on] - 1
    g = sp.coo_matrix((np.ones(f.size), (f, to)), shape=(n, n))
    return connected_components(g, directed=False)[0]


def islands(t, k, l, base=None):
    return _components(t, (k, l)) > (_components(t) if base is None else base)


def base_components(t):
    return _components(t)


def sensitivities(t, cols):
    """Phi [branches, len(cols)] for the candidate branches `cols` (0-based), f0 [branches], admittance"""
    B, y, psh = R.assemble(t)
    n, nb = t["bus_type"].size, y.size
    slack = R.slack_of(t)
    keep = np.r_[0:slack, slack + 1:n]
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    A = sp.coo_matrix((np.r_[np.ones(nb), -np.ones(nb)], (np.r_[f, to], np.r_[np.arange(nb), np.arange(nb)])), shape=(n, nb)).tocsc()
    lu = sla.splu(B[keep][:, keep].tocsc())
    Z = np.zeros((n, len(cols)))
    Z[keep] = lu.solve(A[keep][:, list(cols)].toarray())
    Phi = y[:, None] * (Z[f] - Z[to])
    _, f0 = R.solve(t)
    return Phi, f0, y


def pair_flows(Phi, f0, cols, i, j):
    """flows with the candidates at positions i, j of `cols` out of service; (None, det) when the 2 x 2 system is singular"""
    k, l = cols[i], cols[j]
    M = np.array([[1.0 - Phi[k, i], -Phi[k, j]], [-Phi[l, i], 1.0 - Phi[l, j]]])
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    if abs(det) < SINGULAR:
        return None, det
    c = np.array([M[1, 1] * f0[k] - M[0, 1] * f0[l], M[0, 0] * f0[l] - M[1, 0] * f0[k]]) / det
    fr = f0 + Phi[:, i] * c[0] + Phi[:, j] * c[1]
    fr[k] = fr[l] = 0.0
    return fr, det


def loading(fr, rating, monitored=None):
    """(worst |from| / rating, its branch 1-based with ties to the lowest index (0: none), loadings) over the rated (and monitored) branches"""
    ok = rating > 0
    if monitored is not None:
        m = np.zeros(rating.size, dtype=bool)
        m[monitored] = True
        ok &= m
    load = np.where(ok, np.abs(fr) / np.where(ok, rating, 1.0), 0.0)
    w = float(load.max())
    return w, (int(np.argmax(load)) + 1 if w > 0 else 0), load


def rating_of(t, seed=3):
    """seeded ratings around the base flows' scale, every seventh branch not rated"""
    r = 0.5 + np.random.default_rng(seed).random(t["br_from"].size)
    r[::7] = 0.0
    return r
