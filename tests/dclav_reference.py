"""numpy restatement of the batched DC least-absolute-value estimator (csrc/jg_dclav.hip), dense, f64, one lane, and the same LP through scipy's HiGHS.

The model is the reference's dcLavStateEstimation (src/stateEstimation/dcStateEstimation.jl:201-313, src/backend/expressions.jl:381-421), unweighted:

    minimise  sum_i (u_i + v_i)   subject to   h_i theta + u_i - v_i = z_i,  u, v >= 0,  theta_slack = 0        (= min |z - H theta|_1)
    dual:     maximise z'y        subject to   H'y = 0,  -1 <= y <= 1

  lav_ipm(H, z, ...)     Mehrotra predictor-corrector on that pair, the statements of the device in the device's order: one step length for the primal
                         and the dual side, the start from the unit-weight least-squares estimate, the three stopping tests, the status codes
  lav_linprog(H, z)      scipy.optimize.linprog(method="highs") on the primal LP
  lav_rows(t, ms)        H (dense, slack column zeroed, out-of-service rows zeroed), z (se.mean) and the in-service mask of a measurement set of
                         tests/dcse_reference.py

H is [m, n] with the slack's column zero; rows with status 0 are all-zero and carry z = 0: they leave the model.
"""
from types import SimpleNamespace as NS

import numpy as np

import dcse_reference as S

START_FLOOR = 1e-8
STEP_BACK = 0.995


def lav_rows(t, ms, z=None):
    H, _, mean, slack = S.matrices(t, ms, z)
    status = np.asarray(S.rows(t, ms)[1], dtype=np.float64)
    return H.toarray(), mean * status, status > 0, slack


def _gain(H, q, slack):
    G = H.T @ (q[:, None] * H)
    G[slack, slack] = 1.0                                            # the slack's row and column hold nothing else: its column of H is zero
    return G


def _boundary(x, dx):
    """largest step that keeps x + a dx >= 0 (inf where nothing shrinks)"""
    neg = dx < 0.0
    return float(np.min(-x[neg] / dx[neg])) if neg.any() else np.inf


def lav_ipm(H, z, on=None, slack=0, iteration=50, tolerance=1e-8, theta0=None):
    """-> NS(theta, u, v, y, status, iterations, objective, gap, residual, margins).  status 0 solved, 5 iteration limit, 1 unobservable, 3 a non-finite
    pivot.  margins: per verdict, the largest of the three deciding quantities over its bound (a zero quantity on a zero bound counts 0)."""
    m, n = H.shape
    on = np.ones(m, dtype=bool) if on is None else np.asarray(on, dtype=bool)
    H = H * on[:, None]
    z = np.where(on, z, 0.0)
    m_in = int(on.sum())
    hnorm = float(np.abs(H).sum(axis=0).max())
    nan = NS(theta=np.full(n, np.nan), u=None, v=None, y=np.full(m, np.nan), status=1, iterations=0, objective=np.nan, gap=np.nan, residual=np.full(m, np.nan),
             margins=[])
    G = _gain(H, on.astype(np.float64), slack)
    d = np.linalg.eigvalsh(G)
    if not (d.min() > 1e-12 * d.max()):
        return nan
    theta = np.linalg.solve(G, H.T @ z) if theta0 is None else np.asarray(theta0, dtype=np.float64).copy()
    theta[slack] = 0.0
    r0 = z - H @ theta
    s = max(np.abs(r0[on]).sum() / m_in, START_FLOOR)
    u = np.where(on, np.maximum(r0, 0.0) + s, 0.0)
    v = np.where(on, np.maximum(-r0, 0.0) + s, 0.0)
    y = np.zeros(m)
    status, it, margins = 5, 0, []
    while True:
        r = z - H @ theta
        rp = np.where(on, r - u + v, 0.0)
        rd = -(H.T @ y)
        gap = float((u * (1.0 - y) + v * (1.0 + y))[on].sum())
        obj = float(np.abs(r[on]).sum())
        tests = ((np.abs(rp).max(), tolerance * (1.0 + np.abs(z).max())), (np.abs(rd).max(), tolerance * hnorm), (gap, tolerance * (1.0 + obj)))
        margins.append(max(0.0 if a == 0.0 else (a / b if b > 0.0 else np.inf) for a, b in tests))
        if (np.abs(rp).max() <= tolerance * (1.0 + np.abs(z).max()) and np.abs(rd).max() <= tolerance * hnorm and gap <= tolerance * (1.0 + obj)):
            status = 0
            break
        if it >= iteration:
            break
        dd = u[on] / (1.0 - y[on]) + v[on] / (1.0 + y[on])
        q = np.zeros(m)
        q[on] = 1.0 / dd
        G = _gain(H, q, slack)
        if not np.isfinite(G).all():
            status = 3
            break
        # predictor: target 0, so c = -u + v and rp - c = r
        dth = np.linalg.solve(G, H.T @ (q * r) - rd)
        dth[slack] = 0.0
        dya = q * (r - H @ dth)
        with np.errstate(divide="ignore", invalid="ignore"):
            dua = np.where(on, -u + u * dya / (1.0 - y), 0.0)
            dva = np.where(on, -v - v * dya / (1.0 + y), 0.0)
        aa = min(1.0, _boundary(u[on], dua[on]), _boundary(v[on], dva[on]), _boundary(1.0 - y[on], -dya[on]), _boundary(1.0 + y[on], dya[on]))
        gap_aff = float(((u + aa * dua) * (1.0 - y - aa * dya) + (v + aa * dva) * (1.0 + y + aa * dya))[on].sum())
        smu = (gap_aff / gap) ** 3 * gap / (2.0 * m_in)
        # corrector: target sigma mu plus the second-order terms
        cu = smu - u * (1.0 - y) + dua * dya
        cv = smu - v * (1.0 + y) - dva * dya
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(on, cu / (1.0 - y) - cv / (1.0 + y), 0.0)
        dth = np.linalg.solve(G, H.T @ (q * (rp - c)) - rd)
        dth[slack] = 0.0
        dy = q * (rp - c - H @ dth)
        with np.errstate(divide="ignore", invalid="ignore"):
            du = np.where(on, (cu + u * dy) / (1.0 - y), 0.0)
            dv = np.where(on, (cv - v * dy) / (1.0 + y), 0.0)
        a = min(1.0, STEP_BACK * min(_boundary(u[on], du[on]), _boundary(v[on], dv[on]), _boundary(1.0 - y[on], -dy[on]), _boundary(1.0 + y[on], dy[on])))
        theta, u, v, y = theta + a * dth, u + a * du, v + a * dv, y + a * dy
        it += 1
    return NS(theta=theta, u=u, v=v, y=y, status=status, iterations=it, objective=obj, gap=gap, residual=np.where(on, r, 0.0), margins=margins)


def lav_linprog(H, z, on=None, slack=0):
    """-> NS(theta, objective): variables (theta, u, v) of the in-service rows, the slack's angle fixed at 0"""
    from scipy.optimize import linprog
    m, n = H.shape
    on = np.ones(m, dtype=bool) if on is None else np.asarray(on, dtype=bool)
    Hs, zs = H[on], z[on]
    k = Hs.shape[0]
    A = np.hstack([Hs, np.eye(k), -np.eye(k)])
    cost = np.r_[np.zeros(n), np.ones(2 * k)]
    bounds = [(0.0, 0.0) if j == slack else (None, None) for j in range(n)] + [(0.0, None)] * (2 * k)
    out = linprog(cost, A_eq=A, b_eq=zs, bounds=bounds, method="highs")
    assert out.status == 0, out.message
    return NS(theta=out.x[:n], objective=float(out.fun))
