"""What the DC N-1 screen over a series of injection profiles is held against (tests/test_dc_series_host.py, tests/test_dc_series_gpu.py).

  profiles(t, T)            seeded profiles [T, buses]: the case's own net injections x (1 + 0.3 N(0,1)) per bus, profile 0 the case's own
  rebuild(t, k, p)          the reference's user loop for ONE case: updateBus! / updateGenerator! to profile p, updateBranch!(k, status = 0), solve!, power!
                            = dc_reference.solve(t, out=k, injection=p): rebuild and refactorise, never the compensation
  bridges(t)                the islanding oracle, independent of any linear algebra: in-service branches whose removal splits the bus graph
  base_flows(t, P)          F0 [branches, T]: the flows of every profile with no outage (the rebuild route without an outage)
  series_flows(...)         numpy restatement of the screen's formulas: d_k = 1 - Phi[k,k], c = F0[k,t] / d_k, f_m = F0[m,t] + Phi[m,k] c, f_k = 0
"""
import numpy as np

import dc_pair_reference as P
import dc_reference as R

SINGULAR = P.SINGULAR               # DC_SINGULAR of csrc/jg_dc.hpp


def profiles(t, T, seed=7):
    own = R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64)
    p = own[None, :] * (1.0 + 0.3 * np.random.default_rng(seed).standard_normal((T, own.size)))
    p[0] = own
    return p


def rebuild(t, k, p):
    """(theta, from) of profile p with branch k (0-based, or None) out of service"""
    return R.solve(t, out=k, injection=p)


def in_service(t):
    return np.flatnonzero(np.asarray(t["br_status"]).astype(np.int64) == 1)


def bridges(t):
    """0-based in-service branches whose outage raises the number of connected components"""
    base = P._components(t)
    return np.array([k for k in in_service(t) if P._components(t, (int(k),)) > base], dtype=np.int64)


def base_flows(t, prof):
    return np.stack([rebuild(t, None, p)[1] for p in prof], axis=1)


def diag(Phi, cols):
    """d_k = 1 - Phi[k,k] per candidate"""
    return 1.0 - Phi[np.asarray(cols), np.arange(len(cols))]


def series_flows(Phi, F0, cols, i, tt):
    """flows of profile tt with the candidate at position i of `cols` out of service; None when it is a bridge"""
    k = cols[i]
    d = 1.0 - Phi[k, i]
    if abs(d) < SINGULAR:
        return None
    fr = F0[:, tt] + Phi[:, i] * (F0[k, tt] / d)
    fr[k] = 0.0
    return fr
