"""numpy restatement of the batched DC Huber / Schweppe-Huber estimator (csrc/jg_dchuber.hip), dense, f64, one lane, and an independent certificate.

The rows are those of the DC WLS model, row i scaled by 1 / sigma_i (H~, z~), with a bound kappa_i = c omega_i > 0 per row (omega = 1: Huber;
omega in (0, 1]: Schweppe's leverage weights):

    minimise  1/2 sum s_i^2 + sum kappa_i (u_i + v_i)   subject to   h~_i theta + s_i + u_i - v_i = z~_i,  u, v >= 0,  theta_slack = 0
              (= min sum rho_kappa_i(z~_i - h~_i theta), rho Huber's function)
    dual:     maximise z~'y - 1/2 y'y   subject to   H~'y = 0,  -kappa <= y <= kappa,  with s = y

  huber_ipm(H, z, kappa, ...)            Mehrotra predictor-corrector on that pair, the statements of the device in the device's order: one step length for
                                         both sides, the start from the least-squares estimate, the three stopping tests, the status codes
  huber_certificate(H, z, theta, kappa)  max |H' clip(z - H theta, +-kappa)| / (max_j sum_i |H_ij| max kappa): the gradient of the convex objective, scaled
                                         as the dual stopping test scales it; zero at the optimum, so no second solver is needed
  huber_loss(r, kappa)                   sum rho_kappa(r)
  huber_rows(t, ms)                      H~, z~ (dense, slack column zeroed, out-of-service rows zeroed), the in-service mask, the slack, sigma
  schweppe_omega(H, on, slack, floor)    omega_i = sqrt(Omega_ii / sigma_i^2) = sqrt(1 - h~_i G^-1 h~_i'), clipped to [floor, 1]

H is [m, n] with the slack's column zero; rows with status 0 are all-zero and carry z = 0: they leave the model.
"""
from types import SimpleNamespace as NS

import numpy as np

import dcse_reference as S

START_FLOOR = 1e-8
STEP_BACK = 0.995


def huber_rows(t, ms, z=None):
    H, w, mean, slack = S.matrices(t, ms, z)
    status = np.asarray(S.rows(t, ms)[1], dtype=np.float64)
    scale = np.sqrt(w)
    return H.toarray() * scale[:, None], mean * status * scale, status > 0, slack, 1.0 / scale


def huber_loss(r, kappa):
    a = np.abs(r)
    return float(np.where(a <= kappa, 0.5 * a * a, kappa * a - 0.5 * kappa * kappa).sum())


def huber_weight(r, kappa):
    a = np.abs(r)
    return np.where(a <= kappa, 1.0, kappa / np.where(a > 0.0, a, 1.0))


def huber_certificate(H, z, theta, kappa):
    return float(np.abs(H.T @ np.clip(z - H @ theta, -kappa, kappa)).max() / (np.abs(H).sum(axis=0).max() * np.max(kappa)))


def _gain(H, q, slack):
    G = H.T @ (q[:, None] * H)
    G[slack, slack] = 1.0                                            # the slack's row and column hold nothing else: its column of H is zero
    return G


def schweppe_omega(H, on, slack, floor=1e-3):
    Hs = H * np.asarray(on, dtype=np.float64)[:, None]
    X = np.linalg.solve(_gain(Hs, np.asarray(on, dtype=np.float64), slack), Hs.T)
    lev = np.einsum("ij,ji->i", Hs, X)
    return np.clip(np.sqrt(np.maximum(1.0 - lev, 0.0)), floor, 1.0)


def _boundary(x, dx):
    """largest step that keeps x + a dx >= 0 (inf where nothing shrinks)"""
    neg = dx < 0.0
    return float(np.min(-x[neg] / dx[neg])) if neg.any() else np.inf


def huber_ipm(H, z, kappa, on=None, slack=0, iteration=50, tolerance=1e-8):
    """-> NS(theta, u, v, y, status, iterations, objective, gap, residual, weight, margin, margins).  status 0 solved, 5 iteration limit, 1 unobservable, 3 a
    non-finite pivot.  objective: the Huber loss at theta; margins: per verdict, the largest of the three deciding quantities over its bound (margin: the last)."""
    m, n = H.shape
    on = np.ones(m, dtype=bool) if on is None else np.asarray(on, dtype=bool)
    k = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (m,)).copy()
    H = H * on[:, None]
    z = np.where(on, z, 0.0)
    m_in = int(on.sum())
    hnorm = float(np.abs(H).sum(axis=0).max())
    kmax = float(k[on].max()) if m_in else 0.0
    nan = NS(theta=np.full(n, np.nan), u=None, v=None, y=np.full(m, np.nan), status=1, iterations=0, objective=np.nan, gap=np.nan, residual=np.full(m, np.nan),
             weight=np.full(m, np.nan), margin=np.nan, margins=[])
    G = _gain(H, on.astype(np.float64), slack)
    d = np.linalg.eigvalsh(G)
    if not (d.min() > 1e-12 * d.max()):
        return nan
    theta = np.linalg.solve(G, H.T @ z)
    theta[slack] = 0.0
    r0 = z - H @ theta
    y = np.where(on, np.clip(r0, -0.5 * k, 0.5 * k), 0.0)
    r1 = r0 - y
    s = max(np.abs(r1[on]).sum() / m_in, START_FLOOR)
    u = np.where(on, np.maximum(r1, 0.0) + s, 0.0)
    v = np.where(on, np.maximum(-r1, 0.0) + s, 0.0)
    status, it, margins = 5, 0, []
    while True:
        r = z - H @ theta
        rp = np.where(on, r - y - u + v, 0.0)
        rd = -(H.T @ y)
        gap = float((u * (k - y) + v * (k + y))[on].sum())
        obj = float((0.5 * y * y + k * (u + v))[on].sum())
        dual, dual_bound = np.abs(rd).max(), tolerance * hnorm * kmax                # (no column but the slack's: both are 0, and the device's test 0 <= 0 holds)
        tests = (np.abs(rp).max() / (tolerance * (1.0 + np.abs(z).max())), 0.0 if dual == 0.0 else (dual / dual_bound if dual_bound > 0.0 else np.inf),
                 gap / (tolerance * (1.0 + obj)))
        margins.append(max(tests))
        if max(tests) <= 1.0:
            status = 0
            break
        if it >= iteration:
            break
        dd = 1.0 + u[on] / (k[on] - y[on]) + v[on] / (k[on] + y[on])
        q = np.zeros(m)
        q[on] = 1.0 / dd
        G = _gain(H, q, slack)
        if not np.isfinite(G).all():
            status = 3
            break
        # predictor: target 0, so c = -u + v and rp - c = r - y
        dth = np.linalg.solve(G, H.T @ (q * (r - y)) - rd)
        dth[slack] = 0.0
        dya = q * (r - y - H @ dth)
        with np.errstate(divide="ignore", invalid="ignore"):
            dua = np.where(on, -u + u * dya / (k - y), 0.0)
            dva = np.where(on, -v - v * dya / (k + y), 0.0)
        aa = min(1.0, _boundary(u[on], dua[on]), _boundary(v[on], dva[on]), _boundary((k - y)[on], -dya[on]), _boundary((k + y)[on], dya[on]))
        gap_aff = float(((u + aa * dua) * (k - y - aa * dya) + (v + aa * dva) * (k + y + aa * dya))[on].sum())
        smu = (gap_aff / gap) ** 3 * gap / (2.0 * m_in)
        # corrector: target sigma mu plus the second-order terms
        cu = smu - u * (k - y) + dua * dya
        cv = smu - v * (k + y) - dva * dya
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(on, cu / (k - y) - cv / (k + y), 0.0)
        dth = np.linalg.solve(G, H.T @ (q * (rp - c)) - rd)
        dth[slack] = 0.0
        dy = q * (rp - c - H @ dth)
        with np.errstate(divide="ignore", invalid="ignore"):
            du = np.where(on, (cu + u * dy) / (k - y), 0.0)
            dv = np.where(on, (cv - v * dy) / (k + y), 0.0)
        a = min(1.0, STEP_BACK * min(_boundary(u[on], du[on]), _boundary(v[on], dv[on]), _boundary((k - y)[on], -dy[on]), _boundary((k + y)[on], dy[on])))
        theta, u, v, y = theta + a * dth, u + a * du, v + a * dv, y + a * dy
        it += 1
    r = np.where(on, r, 0.0)
    return NS(theta=theta, u=u, v=v, y=y, status=status, iterations=it, objective=huber_loss(r[on], k[on]), gap=gap, residual=r,
              weight=np.where(on, huber_weight(r, k), 1.0), margin=margins[-1], margins=margins)
