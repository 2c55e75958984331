"""Dense numpy restatement of the DC optimal power flow (juliagrid.jl_amd/dcoptimalpowerflow.py, csrc/jg_dcopf.hip): the model rows of the
reference's dcOptimalPowerFlow (src/optimalPowerFlow/dcOptimalPowerFlow.jl:44-277), the same ADMM iteration on the same scaling, and a KKT
certificate that depends on no solver.  Shares no code with the package beyond the PowerSystem container.
"""
import os
from types import SimpleNamespace as NS

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = 1e20


def tables(case):
    """The case fixture joined with its optimal-power-flow fields."""
    t = {}
    for name in (case + ".npz", case + "_opf.npz"):
        with np.load(os.path.join(GOLDEN, "cases", name)) as z:
            t.update({k: z[k] for k in z.files})
    return t


def golden(case):
    with np.load(os.path.join(GOLDEN, f"results_dcopf_{case}.npz")) as z:
        return {k: z[k] for k in z.files}


def model(system, demand=None, out_generator=0):
    """Dense P (its diagonal), q, constant, A, l, u, equality mask and the row / variable maps; `demand` [buses] and `out_generator` (label, 0:
    none: its capability row is 0 = pg = 0) state one lane."""
    bus, br, gen = system.bus, system.branch, system.generator
    n = bus.number
    pd = bus.demand.active if demand is None else np.asarray(demand, dtype=np.float64)
    on_g = [k for k in range(gen.number) if gen.layout.status[k] == 1]
    pg = {k: n + j for j, k in enumerate(on_g)}
    cost = gen.cost.active
    hv, nv = {}, n + len(on_g)
    for k in on_g:
        if cost.model[k] == 1 and len(cost.piecewise[k + 1]) > 2:
            hv[k] = nv
            nv += 1
    P, q, c0 = np.zeros(nv), np.zeros(nv), 0.0
    A, l, u, kind, ref = [], [], [], [], []

    def add(name, r, entries, lo, hi):
        a = np.zeros(nv)
        for j, v in entries:
            a[j] += v
        A.append(a); l.append(lo); u.append(hi); kind.append(name); ref.append(r)

    for k in on_g:
        if cost.model[k] == 2:
            c = cost.polynomial[k + 1]
            if len(c) > 3:
                raise ValueError("degree")
            if len(c) == 3:
                P[pg[k]] = 2 * c[0]; q[pg[k]] = c[1]; c0 += c[2]
            elif len(c) == 2:
                q[pg[k]] = c[0]; c0 += c[1]
            elif len(c) == 1:
                c0 += c[0]
        elif cost.model[k] == 1:
            pts = cost.piecewise[k + 1]
            if len(pts) == 2:
                s = (pts[1, 1] - pts[0, 1]) / (pts[1, 0] - pts[0, 0])
                q[pg[k]] = s; c0 += pts[0, 1] - pts[0, 0] * s
            else:
                q[hv[k]] = 1.0
                for j in range(1, len(pts)):
                    s = (pts[j, 1] - pts[j - 1, 1]) / (pts[j, 0] - pts[j - 1, 0])
                    add("piecewise", (k + 1, j - 1), [(pg[k], s), (hv[k], -1.0)], -np.inf, s * pts[j - 1, 0] - pts[j - 1, 1])
    live = [k for k in range(br.number) if br.layout.status[k] == 1]
    y = {k: 1.0 / (br.parameter.turnsRatio[k] * br.parameter.reactance[k]) for k in live}
    f = {k: int(br.layout.from_[k]) - 1 for k in live}
    t = {k: int(br.layout.to[k]) - 1 for k in live}
    for i in range(n):
        e, shift = [], 0.0
        for k in live:                                                  # B theta and the shift power of bus i, branch by branch
            if f[k] == i:
                e += [(i, y[k]), (t[k], -y[k])]; shift -= y[k] * br.parameter.shiftAngle[k]
            if t[k] == i:
                e += [(i, y[k]), (f[k], -y[k])]; shift += y[k] * br.parameter.shiftAngle[k]
        e += [(pg[k], -1.0) for k in on_g if gen.layout.bus[k] - 1 == i]
        rhs = -(pd[i] + bus.shunt.conductance[i] + shift)
        add("balance", i + 1, e, rhs, rhs)
    s = bus.layout.slack - 1
    add("slack", s + 1, [(s, 1.0)], bus.voltage.angle[s], bus.voltage.angle[s])
    for k in on_g:
        out = out_generator == k + 1
        add("capability", k + 1, [(pg[k], 1.0)], 0.0 if out else gen.capability.minActive[k], 0.0 if out else gen.capability.maxActive[k])
    for k in live:
        lo, hi = br.flow.minFromBus[k], br.flow.maxFromBus[k]
        if (lo != 0 and np.isfinite(lo)) or (hi != 0 and np.isfinite(hi)):
            off = y[k] * br.parameter.shiftAngle[k]
            add("flow", k + 1, [(f[k], y[k]), (t[k], -y[k])], lo + off, hi + off)
    for k in live:
        lo, hi = br.voltage.minDiffAngle[k], br.voltage.maxDiffAngle[k]
        if (np.isfinite(lo) and lo not in (0.0, -2 * np.pi)) or (np.isfinite(hi) and hi not in (0.0, 2 * np.pi)):
            add("angle", k + 1, [(f[k], 1.0), (t[k], -1.0)], lo, hi)
    kind = np.array(kind)
    return NS(n=nv, m=len(A), buses=n, pg=pg, hv=hv, P=P, q=q, constant=c0, A=np.array(A), l=np.array(l, dtype=np.float64), u=np.array(u, dtype=np.float64),
              eq=np.isin(kind, ("balance", "slack")), kind=kind, ref=ref)


def admm(md, l=None, u=None, rho=0.1, sigma=1e-6, alpha=1.6, tolerance=1e-9, iteration=100000, check=25, adapt_every=200, x0=None, y0=None):
    """The iteration of csrc/jg_dcopf.hip for one lane, dense: returns x, y, z of the unscaled problem, the objective (with its constant), iterations,
    status (0 solved, 2 primal infeasible, 5 iteration limit) and the count of refactorisations."""
    l = md.l if l is None else l
    u = md.u if u is None else u
    c = 1.0 / max(np.abs(md.P).max(), np.abs(md.q).max())
    E = 1.0 / np.sqrt((md.A ** 2).sum(axis=1))
    P, q, A = c * md.P, c * md.q, md.A * E[:, None]
    lo = np.where(l <= -INF, -1e30, E * np.maximum(l, -1e300))
    up = np.where(u >= INF, 1e30, E * np.minimum(u, 1e300))
    free_u, free_l = up >= INF, lo <= -INF

    def factor(r):
        rv = np.where(md.eq, 1e3 * r, r)
        return rv, np.linalg.cholesky(np.diag(P + sigma) + A.T @ (rv[:, None] * A))

    def solve(Lc, b):
        return np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))

    x = np.zeros(md.n) if x0 is None else np.array(x0, dtype=np.float64)
    y = np.zeros(md.m) if y0 is None else np.asarray(y0) * c / E
    z = A @ x
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


def parts(md, system, x):
    """theta, pg over ALL generators (0 where out of service), the helpers."""
    gp = np.zeros(system.generator.number)
    for k, j in md.pg.items():
        gp[k] = x[j]
    return x[:md.buses], gp, np.array([x[j] for j in md.hv.values()])


def duals(md, system, y):
    """The multipliers in the reference's (JuMP's) signs, in the shapes DcOptimalPowerFlow.dual has: the balance rows are stated with the opposite
    sign of the reference's, so their y stands; every other row gets -y."""
    cap = np.zeros(system.generator.number)
    out = NS(balance=None, slack=None, capability=cap, flow={}, angle={}, piecewise={})
    out.balance = y[md.kind == "balance"].copy()
    out.slack = -y[md.kind == "slack"]
    for i in range(md.m):
        if md.kind[i] == "capability":
            cap[md.ref[i] - 1] = -y[i]
        elif md.kind[i] in ("flow", "angle", "piecewise"):
            getattr(out, md.kind[i])[md.ref[i]] = -y[i]
    return out


def kkt(md, l, u, theta, pg, h, dual):
    """Solver-independent certificate on the UNSCALED problem of one lane: (largest bound violation, largest stationarity residual, largest
    complementarity product, most negative multiplier on the wrong side -- as a positive number).  theta [buses], pg over all generators, h the
    helpers in variable order, dual as `duals` gives it."""
    x = np.zeros(md.n)
    x[:md.buses] = theta
    for k, j in md.pg.items():
        x[j] = pg[k]
    for s, j in enumerate(md.hv.values()):
        x[j] = h[s]
    y = np.zeros(md.m)
    y[md.kind == "balance"] = dual.balance
    y[md.kind == "slack"] = -np.asarray(dual.slack)
    for i in range(md.m):
        if md.kind[i] == "capability":
            y[i] = -dual.capability[md.ref[i] - 1]
        elif md.kind[i] in ("flow", "angle", "piecewise"):
            y[i] = -float(getattr(dual, md.kind[i])[md.ref[i]])
    ax = md.A @ x
    bound = max(0.0, (l - ax).max(), (ax - u).max())
    stat = np.abs(md.P * x + md.q + md.A.T @ y).max()
    yp, ym = np.maximum(y, 0), np.maximum(-y, 0)
    fu, fl = u < INF, l > -INF
    comp = max(0.0, (yp[fu] * np.abs(u[fu] - ax[fu])).max(initial=0.0), (ym[fl] * np.abs(ax[fl] - l[fl])).max(initial=0.0))
    wrong = max(0.0, yp[~fu].max(initial=0.0), ym[~fl].max(initial=0.0))
    return bound, stat, comp, wrong
