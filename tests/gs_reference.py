"""numpy restatement of the reference's Gauss-Seidel power flow, vectorised over LANES (scenarios), for the tests of csrc/jg_gs.hip.

  mismatch   mismatch!(analysis::AcPowerFlow{GaussSeidel})   src/powerFlow/acPowerFlow.jl:732-764
  sweep      solve!(analysis::AcPowerFlow{GaussSeidel})      src/powerFlow/acPowerFlow.jl:985-1041
  run        powerFlow!(analysis; iteration, tolerance)      src/powerFlow/acPowerFlow.jl:1389-1433

A sweep stays sequential over the buses, as in the reference: every bus update is ONE numpy expression over the lane axis, and a row's current is
summed in index order (np.cumsum is a strict left fold; np.sum is not).  Every lane has its OWN copy of the transposed Ybus values [L, nnz] -- an
outage is the matrix of a system REBUILT with updateBranch_(status = 0), not the library's 4-entry patch -- and its own injections [L, n].
Pinned to the reference's MATPOWER vectors and iteration counts in tests/test_gs_host.py.
"""
from types import SimpleNamespace as NS

import numpy as np


def isapprox(x, y):
    """the reference's `≈` on vectors (isapprox default): ‖x − y‖ ≤ √eps · max(‖x‖, ‖y‖)"""
    return np.linalg.norm(x - y) <= np.sqrt(np.finfo(float).eps) * max(np.linalg.norm(x), np.linalg.norm(y))


def problem(system):
    """gaussSeidel(system) (acPowerFlow.jl:563-619): pattern, bus lists, set-points, start voltage, injections of ONE scenario.  `system` is the
    library's host-side PowerSystem with its AC model built; bus types are normalised as the reference does."""
    import juliagrid.jl_amd as jg
    vm, va = jg.initializeACPowerFlow(system)
    Y, bus = system.model.ac.nodalMatrix, system.bus
    n = bus.number
    colptr, rowval = np.asarray(Y.colptr) - 1, np.asarray(Y.rowval) - 1
    deg = np.diff(colptr)
    # rows padded to the longest one: the padding repeats entry 0 and is never part of a sum (the fold is read off at the row's own end)
    pad = np.zeros((n, deg.max()), dtype=np.int64)
    for i in range(n):
        pad[i, :deg[i]] = np.arange(colptr[i], colptr[i + 1])
    diag = np.array([colptr[i] + int(np.flatnonzero(rowval[colptr[i]:colptr[i + 1]] == i)[0]) for i in range(n)])
    pv = np.flatnonzero(bus.layout.type == 2)
    return NS(n=n, colptr=colptr, rowval=rowval, deg=deg, pad=pad, diag=diag, pq=np.flatnonzero(bus.layout.type == 1), pv=pv,
              vg=np.array([system.generator.voltage.magnitude[bus.supply.generator[i + 1][0] - 1] for i in pv]),
              yt=np.array(system.model.ac.nodalMatrixTranspose.nzval, dtype=np.complex128),
              v0=vm * (np.cos(va) + 1j * np.sin(va)),
              P=bus.supply.active - bus.demand.active, Q=bus.supply.reactive - bus.demand.reactive)


def lane_values(system, labels):
    """[L, nnz] transposed Ybus values: lane s is the system with branch labels[s] out of service (0: as it is), rebuilt through updateBranch_"""
    import juliagrid.jl_amd as jg
    made = {}
    for k in set(int(x) for x in labels):
        s = system.copy()
        if k:
            jg.updateBranchSystem_(s, k, status=0)
        made[k] = np.array(s.model.ac.nodalMatrixTranspose.nzval, dtype=np.complex128)
    return np.stack([made[int(x)] for x in labels])


def lanes(g, L, yt=None, P=None, Q=None):
    """state of L lanes: (yt [L, nnz], v [L, n], P [L, n], Q [L, n]), each from the problem's own where not given"""
    b = lambda a, w: np.array(np.broadcast_to(getattr(g, w) if a is None else a, (L, getattr(g, w).size)))
    return b(yt, "yt"), b(None, "v0"), b(P, "P"), b(Q, "Q")


def _fold(terms, deg):
    """per row, the sum of its first deg terms in index order: terms [L, rows, longest row]"""
    return np.take_along_axis(np.cumsum(terms, axis=2), (deg - 1)[None, :, None], axis=2)[:, :, 0]


def mismatch(g, yt, v, P, Q):
    """(stopP [L], stopQ [L]); a NaN stays (the reference's max)"""
    with np.errstate(all="ignore"):
        I = _fold(yt[:, g.pad] * v[:, g.rowval[g.pad]], g.deg)
        S = v * np.conj(I)
        mp, mq = np.abs(S.real - P), np.abs(S.imag - Q)
        both = np.concatenate([g.pq, g.pv])
        zero = np.zeros((v.shape[0], 1))
        return (np.maximum.reduce(np.concatenate([zero, mp[:, both]], axis=1), axis=1),
                np.maximum.reduce(np.concatenate([zero, mq[:, g.pq]], axis=1), axis=1))


def sweep(g, yt, v, P, Q):
    """one solve!: v [L, n] is updated in place, bus by bus"""
    L = v.shape[0]
    with np.errstate(all="ignore"):
        for i in g.pq:
            a, b = g.colptr[i], g.colptr[i + 1]
            buf = np.empty((L, b - a + 1), dtype=np.complex128)
            buf[:, 0] = (P[:, i] - 1j * Q[:, i]) / np.conj(v[:, i])
            np.multiply(yt[:, a:b], v[:, g.rowval[a:b]], out=buf[:, 1:])
            np.negative(buf[:, 1:], out=buf[:, 1:])
            v[:, i] += np.cumsum(buf, axis=1)[:, -1] / yt[:, g.diag[i]]
        for i in g.pv:
            a, b = g.colptr[i], g.colptr[i + 1]
            I = np.cumsum(yt[:, a:b] * v[:, g.rowval[a:b]], axis=1)[:, -1]
            c = np.conj(v[:, i])
            v[:, i] += ((P[:, i] + 1j * (c * I).imag) / c - I) / yt[:, g.diag[i]]
        for k, i in enumerate(g.pv):
            v[:, i] = g.vg[k] * v[:, i] / np.abs(v[:, i])


def run(g, yt, v, P, Q, iteration, tolerance):
    """powerFlow! per lane -> NS(iteration, status, stop = (P, Q) of the last check, before = max(P, Q) of the check before it (NaN: none)); v in place.
    status 0 converged, 1 the limit, 3 a maximum that is not finite (where the reference would go on to its limit on NaN)."""
    L = v.shape[0]
    out = NS(iteration=np.zeros(L, dtype=np.int64), status=np.full(L, -1), stop=(np.zeros(L), np.zeros(L)), before=np.full(L, np.nan))
    act = np.arange(L)
    ya, va, Pa, Qa = yt, v.copy(), P, Q
    last = np.full(L, np.nan)
    it = 0
    while act.size:
        sp, sq = mismatch(g, ya, va, Pa, Qa)
        conv = (sp < tolerance) & (sq < tolerance)
        bad = ~conv & ~(np.isfinite(sp) & np.isfinite(sq))
        lim = ~conv & ~bad & (it == iteration)
        done = conv | bad | lim
        if done.any():
            d = act[done]
            out.iteration[d], out.status[d] = it, np.where(conv, 0, np.where(bad, 3, 1))[done]
            out.stop[0][d], out.stop[1][d], out.before[d] = sp[done], sq[done], last[done]
            v[d] = va[done]
            keep = ~done
            act, ya, va, Pa, Qa, last, sp, sq = act[keep], ya[keep], va[keep], Pa[keep], Qa[keep], last[keep], sp[keep], sq[keep]
            if not act.size:
                break
        last = np.maximum(sp, sq)
        sweep(g, ya, va, Pa, Qa)
        it += 1
    return out


def margins_hold(out, tolerance, rel=1e-6):
    """every converged lane stopped clear of the tolerance on both sides: its last check at least `rel` below it, the check before at least `rel` above"""
    c = out.status == 0
    iterated = c & (out.iteration > 0)                            # a lane that converged at its first check has no check before it
    return bool(np.all(np.maximum(out.stop[0], out.stop[1])[c] <= tolerance * (1 - rel)) and np.all(out.before[iterated] >= tolerance * (1 + rel)))
