"""Pivot-order stores nobody reads back (jg_symbolic.hpp: bwd_dead, CompTables::dead), checked on the plan without a GPU.

The backward sweeps store x_k into the pivot-order vector W so that later rows can read it as x_c.  A row that nothing the sweep walks names as an
operand may keep that store back.  The marks come from jg_symbolic.cpp (mark_bwd_dead, build_comp_tables); here an independent walk over the exported
tables must give the same set -- for the refactorising plan (Jordan sweep: level records, both chain-task forms) and for the shared-factor plan (backward
records; the rows the dense top hands down) -- and a replay of each sweep with W[k] of every marked row overwritten with NaN as soon as the row is solved
must give the same bits for every bus.  Plans whose solution has other readers (plain rows: what a refined step sweeps over; symmetric plans: the selected
inverse and the Gauss-Newton handle) mark nothing."""
import numpy as np
import pytest

from plan_emulator import Replay, dsolve
from test_comp_cpu import _compact, _system

NR = 1 | 4 | 1 << 49                                             # what jg_nr_create asks for: in place, level 0 by the producer, Jordan rows
# a small class (the library's own top, a forced small top) and the class of a batch of 256 lanes and more (factorisation tasks, bit 50)
POLICIES = [NR, NR | 1 << 8 | 4 << 16, NR | 1 << 50, NR | 2 << 8 | 24 << 16 | 8 | 1 << 50]
CASES = ["case14test", "case118", "case1354pegase"]
TOPS = {"case14test": (0, -1), "case118": (8, -1), "case1354pegase": (0, 64)}


@pytest.fixture(scope="module")
def systems(oracle):
    return {name: _system(oracle, name) for name in CASES}


def _named_by_the_jordan_sweep(plan):
    """every row of W the Jordan sweep names as an x_c operand"""
    seg, rec = plan.replay_tables("bwdj")
    chain = plan.get("bwd_chain")
    named = set()
    for base, nchunks, wpi, rpw, *_ in seg:
        if wpi <= 0:
            for t in range(nchunks):
                nb, nE, off, _ = (int(v) for v in rec[base + t][:4])
                rows = chain[off:off + 3 * nb:3]
                named.update(int(v) for v in chain[off + 3 * nb: off + 3 * nb + nE])
                uin = chain[off + 3 * nb + nE + nb * nE: off + 3 * nb + nE + nb * nE + nb * nb].reshape(nb, nb)
                named.update(int(rows[c]) for c in range(nb) if (uin[:, c] >= 0).any())
            continue
        for r in rec[base: base + nchunks * 16 * rpw]:
            if r[0] >= 0:
                named.update(int(r[5 + 2 * t]) for t in range(min(int(r[3]), 6)))
    return named


def _jordan_sweep(plan, X, Y, poison):
    """the Jordan sweep as the kernels run it (in-chain x_c goes from row to row directly, not through W); W[k] of a poisoned row turns NaN once it is solved"""
    seg, rec = plan.replay_tables("bwdj")
    chain = plan.get("bwd_chain")
    W = Y.copy()
    out = np.full((plan.n, 2), np.nan)
    for base, nchunks, wpi, rpw, *_ in seg:
        if wpi <= 0:
            for t in range(nchunks):
                nb, nE, off, _ = (int(v) for v in rec[base + t][:4])
                rows = chain[off:off + 3 * nb].reshape(nb, 3)
                ecol = chain[off + 3 * nb: off + 3 * nb + nE]
                uext = chain[off + 3 * nb + nE: off + 3 * nb + nE + nb * nE].reshape(nb, nE)
                uin = chain[off + 3 * nb + nE + nb * nE: off + 3 * nb + nE + nb * nE + nb * nb].reshape(nb, nb)
                acc = np.array([Y[int(rows[p, 0])] for p in range(nb)])
                for p in range(nb):
                    for q in range(nE):
                        acc[p] -= X[uext[p, q]] @ W[ecol[q]]
                for c in range(nb - 1, -1, -1):
                    k = int(rows[c, 0])
                    x = dsolve(X[int(rows[c, 2])], acc[c])
                    out[int(rows[c, 1])] = x
                    W[k] = np.nan if poison[k] else x
                    for p in range(c):
                        acc[p] -= X[int(uin[p, c])] @ x
            continue
        acc, meta = {}, {}
        for c in range(nchunks):
            for w in range(16):
                r0 = base + (c * 16 + w) * rpw
                recs, key, sub = rec[r0:r0 + rpw], (c, w // wpi), w % wpi
                k = int(recs[0][0])
                if k < 0:
                    continue
                part = np.zeros(2)
                for r in recs:
                    for t in range(int(r[3])):
                        part -= X[int(r[4 + 2 * t])] @ W[int(r[5 + 2 * t])]
                if sub == 0:
                    meta[key] = (k, int(recs[0][1]), int(recs[0][2]))
                    acc[key] = Y[k] + part
                else:
                    acc[key] = acc[key] + part
        for key, (k, bus, dg) in meta.items():
            x = dsolve(X[dg], acc[key])
            out[bus] = x
            W[k] = np.nan if poison[k] else x
    return out


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", CASES)
def test_refactorising_plan_marks_exactly_the_rows_nothing_names(jg, systems, name, policy):
    n, rowptr, col, A, rhs = systems[name]
    plan = jg._lib.Plan(n, rowptr, col, policy=policy)
    dead = plan.get(103).astype(bool)
    ok, count = (int(v) for v in plan.get(104))
    info = plan.top_tables()[4]
    assert dead.size == n
    if not int(info[6]):                                         # no Jordan top: the flag is not granted, nothing is marked
        assert ok == 0 and count == 0 and not dead.any()
        assert name != "case1354pegase", "the 1354-bus grid must have a Jordan top under every policy of this test"
        return
    named = _named_by_the_jordan_sweep(plan)
    assert ok == 1 and count == int(dead.sum())
    assert set(np.flatnonzero(dead).tolist()) == set(range(n)) - named
    assert 0 < count < n
    u_ptr = plan.get("u_ptr")
    leaves_of_u = int(np.sum(~np.isin(np.arange(n), plan.get("u_col"))))
    print(f"\n[{name}, policy {policy:#x}] rows never read back {count} of {n}; rows no U column names {leaves_of_u}; rows with an empty U row {int(np.sum(np.diff(u_ptr) == 0))}")
    rp = Replay(plan, inplace=True, prefactor=True, producer=True, jordan=True)
    X, Y = rp.factor(A, rhs)
    ref = rp.backsolve(X.copy(), Y.copy())
    plain = _jordan_sweep(plan, X, Y, np.zeros(n, dtype=bool))
    poisoned = _jordan_sweep(plan, X, Y, dead)
    assert np.isfinite(ref).all() and np.array_equal(plain, ref) and np.array_equal(poisoned, ref)
    if named:                                                    # and the replay does notice a row that IS read back
        wrong = dead.copy()
        wrong[sorted(named)[0]] = True
        assert not np.array_equal(_jordan_sweep(plan, X, Y, wrong), ref, equal_nan=True)


def _comp_backward(tables, M, W0, poison, n):
    """backward rows of the shared-factor step by levels (test_comp_cpu._sweep without its checks); W of a poisoned row turns NaN once the row is stored"""
    _, top, _, (seg, rec) = tables
    W = W0.copy()
    x = np.full((n, 2), np.nan)
    for k in top:                                                # what the dense top hands down: x of the top pivots, in pivot order
        x[k] = W[k]
        if poison[k]:
            W[k] = np.nan
    for lv in sorted(set(seg[:, 4])):
        new = {}
        for base, nchunks, wpi, rpw, *_ in seg[seg[:, 4] == lv]:
            for c in range(nchunks):
                for item in range(16 // wpi):
                    tot, target = None, -1
                    for sub in range(wpi):
                        r0 = base + (c * 16 + item * wpi + sub) * rpw
                        rr = rec[r0:r0 + rpw]
                        if rr[0, 0] < 0:
                            continue
                        acc = np.zeros(2)
                        if sub == 0:
                            target = int(rr[0, 0])
                            acc = dsolve(M[rr[0, 2]], W[target])
                        for q in rr:
                            for t in range(q[3]):
                                acc -= M[q[4 + 2 * t]] @ W[q[5 + 2 * t]]
                        tot = acc if tot is None else tot + acc
                    if target >= 0:
                        new[target] = tot
        for k, v in new.items():
            x[k] = v
            W[k] = np.nan if poison[k] else v
    return x


@pytest.mark.parametrize("name", CASES)
def test_shared_factor_plan_marks_exactly_the_rows_no_backward_record_names(jg, systems, name):
    n, rowptr, col, A, rhs = systems[name]
    plan = jg._lib.Plan(n, rowptr, col, policy=1)
    rp = Replay(plan, inplace=True)
    X, Y = rp.factor(A, rhs)
    xb = rp.backsolve(X.copy(), Y.copy())                        # bus order
    perm = plan.get("perm")
    M = _compact(plan, X)
    for top_cap in TOPS[name]:
        tab = plan.comp_tables(top_cap)
        (bseg, brec), top = tab[3], tab[1]
        lib = plan_lib_get(jg, plan, top_cap, 6).astype(bool)
        n_dead, n_dead_top = (int(v) for v in plan_lib_get(jg, plan, top_cap, 7))
        named = set()
        for r in brec:
            if r[0] >= 0:
                named.update(int(r[5 + 2 * t]) for t in range(min(int(r[3]), 6)))
        assert set(np.flatnonzero(lib).tolist()) == set(range(n)) - named
        assert n_dead == int(lib.sum()) and n_dead_top == int(lib[top].sum()) and 0 < n_dead < n
        print(f"\n[{name}, top_cap {top_cap}] top pivots {top.size}; rows never read back {n_dead}, of them in the top {n_dead_top}")
        W0 = Y.copy()
        W0[top] = xb[perm[top]]
        plain = _comp_backward(tab, M, W0, np.zeros(n, dtype=bool), n)
        poisoned = _comp_backward(tab, M, W0, lib, n)
        assert np.isfinite(plain).all() and np.array_equal(plain, poisoned)
        assert np.abs(plain - xb[perm]).max() <= 1e-9 * max(1.0, np.abs(xb).max())


def plan_lib_get(jg, plan, top_cap, which):
    L = jg._lib.plan_lib()
    m = L.jg_plan_comp_export(plan.h, int(top_cap), which, None, 0)
    assert m >= 0
    out = np.zeros(max(m, 1), dtype=np.int32)
    L.jg_plan_comp_export(plan.h, int(top_cap), which, out.ctypes.data, m)
    return out[:m]


def test_plans_whose_solution_has_other_readers_mark_nothing(jg, systems):
    """plain rows (no bit 49: what the forward() + backsolve() of a refined step sweeps over) and symmetric plans (the selected inverse, the Gauss-Newton handle)"""
    n, rowptr, col, _, _ = systems["case1354pegase"]
    for policy in (1 | 4, 1, 3 | 1 << 49):
        plan = jg._lib.Plan(n, rowptr, col, policy=policy)
        assert [int(v) for v in plan.get(104)] == [0, 0] and not plan.get(103).any()
