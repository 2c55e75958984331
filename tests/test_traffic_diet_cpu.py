"""Sweep-only factorisation (jg_symbolic.hpp: top_dead, Engine::sweep_only), checked on the plan without a GPU.

With the flag a Jordan top task keeps the off-diagonal entries of its pivot columns and of its in-task triangle to itself.  That is only right if
nothing the factorisation still runs and nothing the Jordan sweep walks reads those entries, and if everything the sweep does read is still stored.
The marks come from jg_symbolic.cpp (mark_sweep_dead); here they are held against the tables by an independent walk and against the numpy replay
(tests/plan_emulator.py) with the marked entries poisoned."""
import numpy as np
import pytest

from conftest import load_case
from plan_emulator import Replay, block_jacobian_from_csc

NR = 1 | 4 | 1 << 49                                             # what jg_nr_create asks for: in place, level 0 by the producer, Jordan rows
# the library's own choice of the top, then tops forced onto small grids: (top level, soft cap of a front) -> fronts of class 2, 3 and 4, one launch per class (bit 3)
# and the factorisation below the top as TASKS (bit 50: what a batch of 256 lanes and more runs)
POLICIES = [NR, NR | 1 << 8 | 4 << 16, NR | 2 << 8 | 8 << 16 | 8, NR | 3 << 8 | 16 << 16, NR | 1 << 8 | 40 << 16, NR | 1 << 8 | 63 << 16 | 8,
            NR | 1 << 50, NR | 2 << 8 | 24 << 16 | 8 | 1 << 50]
CASES = ["case14test", "case30test", "case1354pegase"]


def _system(oracle, name):
    s = oracle.OracleSystem(load_case(name))
    a = oracle.OracleNR(s)
    a.mismatch()
    _, f0, _ = a.vectors()
    a.solve()
    J, _, _ = a.vectors()
    rowptr, col, A = block_jacobian_from_csc(s.n, s.colptr, s.rowval, a.type, a.pq, a.pvpq, a.jcolptr, a.jrowval, J)
    rhs = np.zeros((s.n, 2))
    for i in range(s.n):
        if a.pvpq[i]:
            rhs[i, 0] = f0[a.pvpq[i] - 1]
        if a.pq[i]:
            rhs[i, 1] = f0[a.pq[i] - 1]
    return s.n, rowptr, col, A, rhs


@pytest.fixture(scope="module")
def systems(oracle):
    return {name: _system(oracle, name) for name in CASES}


def _stored_by_tasks(plan):
    """entry -> number of task slots that store it into the factor entries under Jordan rows (k_fact_top's store loop), and the diagonal entries of the tasks"""
    hdr, data, _, _, _ = plan.top_tables()
    stored, diags, classes = {}, set(), set()
    for h in hdr:
        m, e, base, fprime = int(h[0]), int(h[1]), int(h[3]), int(h[11])
        f = m + e
        classes.add(int(h[9]))
        emap = data[base: base + f * fprime].reshape(f, fprime)
        diags.update(int(v) for v in data[base + int(h[8]): base + int(h[8]) + m])
        for r in range(f):
            for c in range(f):
                cd = int(emap[r, c])
                if (r < m and c >= m) or cd < 0 or (cd >> 28) & 4:    # Jordan row slot; nothing / rhs; not stored by the slot's thread
                    continue
                stored[cd & 0x0FFFFFFF] = stored.get(cd & 0x0FFFFFFF, 0) + 1
    return stored, diags, classes


def _fact_operands(seg, rec, tasks=False):
    ops = set()
    for r in rec if tasks else ():                               # factorisation TASKS (jg_symbolic.hpp): staged operands, then one memory operand per term
        for u in range((int(r[3]) >> 8) & 0xFF):
            ops.add(int(r[10 + 3 * u]) & 0xFFFFFF)
            ops.add(int(r[11 + 3 * u]))
        kind, nt = int(r[0]) & 7, int(r[3]) & 0xFF
        if kind == 7:
            continue
        for t in range(nt):
            if int(r[0]) & 128:
                ops.add(int(r[4 + 3 * t]) & 0x3FFFFFFF)
                ops.add(int(r[5 + 3 * t]))
                if kind != 3:
                    ops.add(int(r[6 + 3 * t]))
            elif kind != 3:
                ops.add(int(r[4 + t]) & 0xFFFFFF)
    for r in () if tasks else rec:
        if r[0] < 0:
            continue
        for t in range(min(int(r[3]), 4)):
            ops.add(int(r[4 + 3 * t]) & 0x3FFFFFFF)
            ops.add(int(r[5 + 3 * t]))
            if r[0] != 3:
                ops.add(int(r[6 + 3 * t]))
    return ops


def _sweep_reads(plan):
    """every block the Jordan sweep names: diagonal blocks, row terms, the blocks of its chain tasks"""
    seg, rec = plan.replay_tables("bwdj")
    chain = plan.get("bwd_chain")
    reads = set()
    for base, nchunks, wpi, rpw, *_ in seg:
        if wpi <= 0:
            for t in range(nchunks):
                nb, nE, off, _ = (int(v) for v in rec[base + t][:4])
                reads.update(int(v) for v in chain[off + 2: off + 3 * nb: 3])
                u = chain[off + 3 * nb + nE: off + 3 * nb + nE + nb * nE + nb * nb]
                reads.update(int(v) for v in u if v >= 0)
            continue
        for r in rec[base: base + nchunks * 16 * rpw]:
            if r[0] < 0:
                continue
            reads.add(int(r[2]))
            reads.update(int(r[4 + 2 * t]) for t in range(min(int(r[3]), 6)))
    return reads


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", CASES)
def test_dead_entries_have_no_reader_and_the_sweep_keeps_what_it_reads(jg, systems, name, policy):
    n, rowptr, col, A, rhs = systems[name]
    plan = jg._lib.Plan(n, rowptr, col, policy=policy)
    hdr, _, _, task_of, info = plan.top_tables()
    dead = plan.get(101).astype(bool)
    ok, dead_units, store_units = (int(v) for v in plan.get(102))
    nE = plan.get("e_row").size
    assert dead.size == nE
    if not int(info[6]):                                         # no top tasks: nothing to keep back
        assert hdr.shape[0] == 0 and not dead.any() and ok == 0 and dead_units == 0
        if name == "case1354pegase":
            pytest.fail("the 1354-bus grid must have a Jordan top under every policy of this test")
        return
    stored, diags, _ = _stored_by_tasks(plan)
    e_row, e_col = plan.get("e_row"), plan.get("e_col")
    # the marks are exactly what ONE flag of the kernel skips: every off-diagonal entry a task slot stores, each owned by one slot of one task
    assert ok == 1
    assert set(np.flatnonzero(dead).tolist()) == set(stored)
    assert all(v == 1 for v in stored.values())
    assert not (set(stored) & diags)
    assert all(task_of[min(int(e_row[en]), int(e_col[en]))] >= 0 and e_row[en] != e_col[en] for en in stored)
    assert dead_units == 2 * len(stored) and 0 < dead_units < store_units
    # no item of the factorisation reads one of them (level items, the producer's level 0); the tasks exchange update matrices through the stack
    for kind in ("fact", "pre"):
        ops = _fact_operands(*plan.replay_tables(kind), tasks=kind == "fact" and bool(int(info[8])))
        assert not (ops & set(stored)), kind
    # the sweep reads none of them, and what it reads of the top is still stored: diagonal blocks of the tasks, Jordan rows behind the entries
    reads = _sweep_reads(plan)
    assert not (reads & set(stored))
    for en in reads:
        if en >= nE:
            assert en < nE + int(info[7])
        elif task_of[min(int(e_row[en]), int(e_col[en]))] >= 0:
            assert en in diags
    # numerically: the sweep over a factor whose dead entries were never stored gives the same bits
    rp = Replay(plan, inplace=True, prefactor=True, producer=True, jordan=True)
    X, Y = rp.factor(A, rhs)
    x = rp.backsolve(X.copy(), Y.copy())
    Xp = X.copy()
    Xp[np.flatnonzero(dead)] = np.nan
    xp = rp.backsolve(Xp, Y.copy())
    assert np.isfinite(x).all() and np.array_equal(x, xp)


def test_every_front_class_is_covered(jg, systems):
    n, rowptr, col, _, _ = systems["case1354pegase"]
    classes = set()
    for policy in POLICIES:
        classes |= _stored_by_tasks(jg._lib.Plan(n, rowptr, col, policy=policy))[2]
    assert classes == {2, 3, 4}


def test_plans_without_jordan_rows_or_with_the_symmetric_kernel_refuse_the_flag(jg, systems):
    n, rowptr, col, _, _ = systems["case1354pegase"]
    for policy in (1 | 4, 3 | 1 << 49):                          # plain rows; symmetric (k_fact_top_sym)
        plan = jg._lib.Plan(n, rowptr, col, policy=policy)
        assert int(plan.get(102)[0]) == 0 and not plan.get(101).any()
