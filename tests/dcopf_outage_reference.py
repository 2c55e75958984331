"""Dense numpy restatement of ONE lane of the DC optimal power flow with a branch out (csrc/jg_dcopf.hip, jg_dcopf_set_branch_outages), and the route
it is held against: the model of the system rebuilt without the branch.

The lane keeps the base problem's rows, variables and scaling (tests/dcopf_reference.py: `model`, the iteration of `admm`).  With branch k (admittance y,
buses f and t, balance rows r_f and r_t) out its matrix is A_s = A + p d', p = -y (e_rf - e_rt), d = e_f - e_t, formed here explicitly; the branch's own
flow and angle rows stay and are free rows; the two balance rows lose the branch's shift power.  K_s = P + sigma I + A_s' rho A_s is factorised densely:
no Woodbury, nothing of the package beyond the PowerSystem container.
"""
import importlib
from types import SimpleNamespace as NS

import numpy as np

import dcopf_reference as R

INF = R.INF


def lane(md, system, k):
    """The lane's unscaled A_s, l, u for the base model `md` (of R.model, with the lane's demand and generator outage in its l, u) and branch label k,
    the rows it frees and p, d."""
    br = system.branch
    y = 1.0 / (br.parameter.turnsRatio[k - 1] * br.parameter.reactance[k - 1])
    f, t = int(br.layout.from_[k - 1]) - 1, int(br.layout.to[k - 1]) - 1
    kind, ref = md.kind, md.ref
    rf = next(i for i in range(md.m) if kind[i] == "balance" and ref[i] == f + 1)
    rt = next(i for i in range(md.m) if kind[i] == "balance" and ref[i] == t + 1)
    free = [i for i in range(md.m) if kind[i] in ("flow", "angle") and ref[i] == k]
    p, d = np.zeros(md.m), np.zeros(md.n)
    p[rf], p[rt] = -y, y
    d[f], d[t] = 1.0, -1.0
    l, u = md.l.copy(), md.u.copy()
    l[free], u[free] = -np.inf, np.inf
    share = y * br.parameter.shiftAngle[k - 1]                          # the base rows hold -(.. - share) at f and -(.. + share) at t
    l[rf] -= share; u[rf] -= share
    l[rt] += share; u[rt] += share
    return NS(A=md.A + np.outer(p, d), l=l, u=u, free=free, p=p, d=d, rf=rf, rt=rt, f=f, t=t, y=y)


def admm(md, A_s, l, u, rho=0.1, sigma=1e-6, alpha=1.6, tolerance=1e-9, iteration=100000, check=25, adapt_every=200, x0=None, y0=None, z0=None,
         woodbury=None):
    """R.admm's iteration with the lane's own matrix A_s and the BASE problem's scaling (c and E come from md.A, not from A_s).  `woodbury`: the lane
    (of `lane`); the solves then go the device's way, on the factor of the base K with the rank-2 correction, for measuring what that costs."""
    c = 1.0 / max(np.abs(md.P).max(), np.abs(md.q).max())
    E = 1.0 / np.sqrt((md.A ** 2).sum(axis=1))
    P, q, A = c * md.P, c * md.q, A_s * E[:, None]
    lo = np.where(l <= -INF, -1e30, E * np.maximum(l, -1e300))
    up = np.where(u >= INF, 1e30, E * np.minimum(u, 1e300))
    free_u, free_l = up >= INF, lo <= -INF

    def factor(r):
        rv = np.where(md.eq, 1e3 * r, r)
        if woodbury is None:
            return rv, np.linalg.cholesky(np.diag(P + sigma) + A.T @ (rv[:, None] * A))
        A0, p = md.A * E[:, None], E * woodbury.p
        Lc = np.linalg.cholesky(np.diag(P + sigma) + A0.T @ (rv[:, None] * A0))
        U = np.stack((A0.T @ (rv * p), woodbury.d), axis=1)
        W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, U))
        return rv, (Lc, U, W, np.linalg.inv(np.array([[-(p @ (rv * p)), 1.0], [1.0, 0.0]]) + U.T @ W))

    def solve(Lc, b):
        if woodbury is None:
            return np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
        Lc, U, W, M = Lc
        x0 = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
        return x0 - W @ (M @ (U.T @ x0))

    x = np.zeros(md.n) if x0 is None else np.array(x0, dtype=np.float64)
    y = np.zeros(md.m) if y0 is None else np.asarray(y0) * c / E
    z = A @ x if z0 is None else np.asarray(z0) * E
    rv, Lc = factor(rho)
    refac, status, it = 0, 5, iteration
    for k in range(1, iteration + 1):
        xt = solve(Lc, sigma * x - q + A.T @ (rv * z - y))
        zt = A @ xt
        x = alpha * xt + (1 - alpha) * x
        zr = alpha * zt + (1 - alpha) * z
        zn = np.clip(zr + y / rv, lo, up)
        yn = y + rv * (zr - zn)
        dy, y, z = yn - y, yn, zn
        if k % check and k != iteration:
            continue
        ax, aty, px = A @ x, A.T @ y, P * x
        prim, dual = np.abs(ax - z).max(), np.abs(px + q + aty).max()
        pn, dn = max(np.abs(ax).max(), np.abs(z).max()), max(np.abs(px).max(), np.abs(aty).max(), np.abs(q).max())
        if prim <= tolerance + tolerance * pn and dual <= tolerance + tolerance * dn:
            status, it = 0, k
            break
        d = np.where(free_u, np.minimum(dy, 0), dy)
        d = np.where(free_l, np.maximum(d, 0), d)
        nd = np.abs(d).max()
        if nd > 1e-4 and (up * np.maximum(d, 0) + lo * np.minimum(d, 0)).sum() <= -1e-4 * nd and np.abs(A.T @ d).max() <= 1e-4 * nd:
            status, it = 2, k
            break
        if adapt_every and k % adapt_every == 0 and dual > 0:
            r = np.sqrt((prim / (pn + 1e-10)) / (dual / (dn + 1e-10)))
            new = min(max(rho * r, 1e-6), 1e6)
            if (r < 0.2 or r > 5.0) and new != rho:
                rho = new
                rv, Lc = factor(rho)
                refac += 1
    obj = 0.5 * x @ (md.P * x) + md.q @ x + md.constant
    return NS(x=x, y=y * E / c, z=z / E, objective=obj, iterations=it, status=status, refactorisations=refac, rho=rho)


def solve(system, k, demand=None, out_generator=0, **kw):
    """The restatement for one lane: branch label k out (0: none) of `system`; returns the base model, the lane and the result."""
    md = R.model(system, demand=demand, out_generator=out_generator)
    if not k:
        return md, None, admm(md, md.A, md.l, md.u, **kw)
    ln = lane(md, system, k)
    return md, ln, admm(md, ln.A, ln.l, ln.u, **kw)


def rebuilt(case_tables, k, demand=None, out_generator=0, edit=None):
    """The rebuilt route: the system from a copy of the tables with branch k's status 0 (after `edit(tables)`), and dcopf_reference.model of it."""
    jg = importlib.import_module("juliagrid.jl_amd")
    t = {name: np.array(v) for name, v in case_tables.items()}
    if edit is not None:
        edit(t)
    t["br_status"][k - 1] = 0
    s = jg.powerSystem(t)
    jg.dcModel_(s)
    return s, R.model(s, demand=demand, out_generator=out_generator)


def bridges(system):
    """The in-service branches whose removal disconnects the bus graph, by a search of the graph without each (independent of the library's table)."""
    br, n = system.branch, system.bus.number
    live = [k for k in range(br.number) if br.layout.status[k] == 1]
    found = []
    for k in live:
        adj = {i: [] for i in range(n)}
        for j in live:
            if j != k:
                a, b = int(br.layout.from_[j]) - 1, int(br.layout.to[j]) - 1
                adj[a].append(b); adj[b].append(a)
        seen, stack = {int(br.layout.from_[k]) - 1}, [int(br.layout.from_[k]) - 1]
        while stack:
            for w in adj[stack.pop()]:
                if w not in seen:
                    seen.add(w); stack.append(w)
        if int(br.layout.to[k]) - 1 not in seen:
            found.append(k + 1)
    return found
