"""What the DC common-mode screen (dcGroupScreen, csrc/jg_dc_group.hip) is held against: two routes to the flows with a GROUP of branches out of service,
independent of each other and of the library (tests/test_dc_group_host.py, tests/test_dc_group_gpu.py).

  (a) the rebuild route
  islands(t, S)            the islanding oracle, independent of any linear algebra: the members leave the bus graph; True when the number of connected
                           components among the buses grows
  group_solve(t, S)        updateBranch!(s, status = 0) for every member, solve!, power!: the members go out of service in a COPY of the case table, then
                           dc_reference.solve -- the matrix rebuilt without them and refactorised (scipy splu), never the compensation.  None when
                           islands(t, S)
  (b) the k x k formula, in numpy from a DENSE inverse of the nodal matrix
  dense_sensitivities(t)   Phi [branches, branches] = y_m a_m' B^-1 a_k and the base flows f0
  group_flows(Phi, f0, S)  (I - Phi_SS) c = f0_S by LU with partial pivoting, f_m = f0_m + sum_s Phi[m,s] c_s, 0 on the members; returns
                           (flows, smallest |pivot|) -- the flows are None when that pivot is below SINGULAR

S holds 0-based branch indices."""
import numpy as np

import dc_pair_reference as P
import dc_reference as R

SINGULAR = 1e-9                     # DC_SINGULAR of csrc/jg_dc.hpp
loading = P.loading
rating_of = P.rating_of
base_components = P.base_components


def islands(t, S, base=None):
    return P._components(t, tuple(int(s) for s in S)) > (P._components(t) if base is None else base)


def group_solve(t, S, base=None):
    """flows [branches] with the branches S out of service by the rebuild route; None when the grid without them is disconnected"""
    if islands(t, S, base):
        return None
    t2 = dict(t)
    t2["br_status"] = np.array(t["br_status"]).copy()
    t2["br_status"][list(S)] = 0
    _, fr = R.solve(t2)
    return fr


def dense_sensitivities(t):
    B, y, psh = R.assemble(t)
    n, nb = t["bus_type"].size, y.size
    slack = R.slack_of(t)
    keep = np.r_[0:slack, slack + 1:n]
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    Binv = np.zeros((n, n))
    Binv[np.ix_(keep, keep)] = np.linalg.inv(B[keep][:, keep].toarray())
    Z = Binv[:, f] - Binv[:, to]                                  # B^-1 a_k, the slack's component dropped
    Phi = y[:, None] * (Z[f] - Z[to])
    th = Binv @ R.rhs_of(t, psh)
    f0 = y * (th[f] - th[to] - np.asarray(t["br_shift"], dtype=np.float64))
    return Phi, f0


def lu_solve(M, b):
    """x and the smallest |pivot| of LU with partial pivoting (row j takes the largest entry of column j among the rows i >= j)"""
    M, b = np.array(M, dtype=np.float64), np.array(b, dtype=np.float64)
    k = b.size
    small = np.inf
    for j in range(k):
        i = j + int(np.argmax(np.abs(M[j:, j])))
        M[[j, i]] = M[[i, j]]
        b[[j, i]] = b[[i, j]]
        small = min(small, abs(M[j, j]))
        if abs(M[j, j]) < SINGULAR:
            return None, small
        l = M[j + 1:, j] / M[j, j]
        M[j + 1:] -= l[:, None] * M[j]
        b[j + 1:] -= l * b[j]
    x = np.zeros(k)
    for j in range(k - 1, -1, -1):
        x[j] = (b[j] - M[j, j + 1:] @ x[j + 1:]) / M[j, j]
    return x, small


def group_flows(Phi, f0, S):
    S = [int(s) for s in S]
    c, small = lu_solve(np.eye(len(S)) - Phi[np.ix_(S, S)], f0[S])
    if c is None:
        return None, small
    fr = f0 + Phi[:, S] @ c
    fr[S] = 0.0
    return fr, small


def seeded_groups(t, seed, sizes, whole=False):
    """one group per entry of `sizes`: that many in-service branches (0-based, ascending) drawn by `seed`.  `whole`: every second group is drawn again,
    up to 400 times, until the grid without it stays connected (random large groups of a small grid nearly always island)"""
    rng = np.random.default_rng(seed)
    on = np.flatnonzero((np.asarray(t["br_status"]) == 1) & (np.asarray(t["br_from"]) != np.asarray(t["br_to"])))
    base = base_components(t) if whole else None
    out = []
    for g, k in enumerate(sizes):
        for _ in range(400 if whole and g % 2 == 0 else 1):
            S = tuple(sorted(int(x) for x in rng.choice(on, size=k, replace=False)))
            if not whole or not islands(t, S, base):
                break
        out.append(S)
    return out
