"""The shared-factor first Newton step (csrc/jg_comp.hip: k_comp_fix, k_csweep, k_ctop; jg_nr.hip: build_comp_graphs, comp_ready) at the edges that
tests/test_comp_gpu.py does not reach: every kind of Ybus edit a scenario can carry (built by hand, entry by entry), every class of lane remainder with
the exact state update, small / odd dense tops, lane groups that drop out at the first verdict, and the start-is-base flag across lane hand-offs.
The reference of every comparison is the oracle with the same edits (add_ybus); the bounds are those of test_comp_gpu.py for the same comparisons:
1e-9 x max(1e-3, |increment|max) on first increments, 1e-8 on converged V / theta against the oracle, 1e-10 against the refactorising path, equal
iteration counts.  No golden grid has a phase shifter: the test gives transformer 8 of case118 a shift angle in the tables both sides are built from.

Grids: case118 alone -- it has every category (slack-PQ, slack-PV, PV-PV, PV-PQ, PQ-PQ lines, off-nominal taps, parallel lines, bridges)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

from conftest import load_case
from plan_emulator import block_jacobian_from_csc

pytestmark = pytest.mark.gpu

CASE = "case118"
SHIFTER = (8, 0.1)                    # (branch label, shift angle in radians) of the grid variant with a phase shifter


# ---- the oracle's answers, computed once per (grid, start state, edit) and shared by every test of this file ---------------------------------
_REFS = {}


class _Reference:
    def __init__(self, oracle, tables, start):
        self.oracle, self.osys, self.start = oracle, oracle.OracleSystem(tables), (start[0].copy(), start[1].copy())
        self._first, self._flow = {}, {}

    def _nr(self, edit):
        o = self.oracle.OracleNR(self.osys)
        for p, d in zip(edit.ptr, edit.dy):
            o.add_ybus(int(p) - 1, complex(d))
        if edit.power is not None:
            o.set_power(self.osys.ps, self.osys.qs, *edit.power)
        o.set_voltage(*self.start)
        return o

    def first(self, edit):
        """the oracle's first increment at the start state"""
        if edit.key not in self._first:
            o = self._nr(edit)
            o.mismatch()
            o.solve()
            self._first[edit.key] = o.vectors()[2].copy()
        return self._first[edit.key]

    def flow(self, edit):
        """(status, iterations, V, theta) of the oracle's power_flow()"""
        if edit.key not in self._flow:
            o = self._nr(edit)
            rc = o.power_flow()
            self._flow[edit.key] = (rc, o.iteration) + tuple(x.copy() for x in o.voltage())
        return self._flow[edit.key]


def _edit(tag, ptr=(), dy=(), kind="step", power=None):
    """kind: step (a Newton step is taken: everything is compared), idle (converged at the start: no step), bridge (islanding, status 3)"""
    ptr, dy = [int(p) for p in ptr], [complex(d) for d in dy]
    key = (tuple(sorted(zip(ptr, dy), key=lambda x: x[0])), None if power is None else (power[0].tobytes(), power[1].tobytes()))
    return NS(tag=tag, ptr=ptr, dy=dy, kind=kind, power=power, key=key)


def _grid(jg, oracle, top_cap, shifter=None):
    """case118 (with branch shifter[0] turned into a phase shifter), its converged base case, a BaseCase on it and the shared oracle reference"""
    t = load_case(CASE)
    if shifter:
        t["br_shift"] = np.array(t["br_shift"], dtype=np.float64)
        t["br_shift"][shifter[0] - 1] = shifter[1]
    s = jg.powerSystem(t)
    single = jg.newtonRaphson(s)
    jg.powerFlow_(single)
    assert single.status == 0
    start = (single.voltage.magnitude.copy(), single.voltage.angle.copy())
    base = jg.BaseCase(single, top_cap=top_cap)
    key = (CASE, shifter)
    ref = _REFS.get(key)
    if ref is None or not (np.array_equal(ref.start[0], start[0]) and np.array_equal(ref.start[1], start[1])):
        ref = _REFS[key] = _Reference(oracle, t, start)
    return NS(t=t, s=s, single=single, base=base, start=start, ref=ref, n=s.bus.number)


def _close(g, *handles):
    for h in handles:
        h.close()
    g.base.close()
    g.single.close()


def _live(jg, s):
    lay = s.branch.layout
    return (lay.status == 1) & ~jg.bridges(s) & (lay.from_ != lay.to)


def _categories(jg, s):
    """first non-bridge in-service branch of every kind (labels, 1-based); bus types as the analysis normalised them"""
    lay, par, ty = s.branch.layout, s.branch.parameter, s.bus.layout.type
    live = _live(jg, s)
    ends = np.sort(np.stack([ty[lay.from_ - 1], ty[lay.to - 1]], axis=1), axis=1)

    def first(mask):
        idx = np.flatnonzero(live & mask)
        assert idx.size, "the grid has no such branch"
        return int(idx[0]) + 1

    pair = {}
    for k in np.flatnonzero(lay.status == 1):
        pair.setdefault((min(lay.from_[k], lay.to[k]), max(lay.from_[k], lay.to[k])), []).append(int(k))
    twin = np.zeros(s.branch.number, dtype=bool)
    for v in pair.values():
        if len(v) > 1:
            twin[v] = True
    plain = (par.shiftAngle == 0)
    return dict(slack_pq=first((ends[:, 0] == 1) & (ends[:, 1] == 3)), slack_pv=first((ends[:, 0] == 2) & (ends[:, 1] == 3)),
                pv_pv=first((ends[:, 0] == 2) & (ends[:, 1] == 2)), pv_pq=first((ends[:, 0] == 1) & (ends[:, 1] == 2)),
                pq_pq=first((ends[:, 0] == 1) & (ends[:, 1] == 1)), tap=first((par.turnsRatio != 0) & (par.turnsRatio != 1) & plain),
                parallel=first(twin), bridge=int(np.flatnonzero(jg.bridges(s) & (lay.status == 1))[0]) + 1)


def _outage(jg, s, label, tag, factor=1.0, order=(0, 1, 2, 3), kind="step"):
    """outagePatch order: (i,i), (j,j), (i,j), (j,i) with i the from bus"""
    ptr, dy = jg.outagePatch(s, label)
    return _edit(tag, [ptr[q] for q in order], [factor * dy[q] for q in order], kind)


def _diag(s, bus, tag, dy, kind="step"):
    return _edit(tag, [s.model.ac.nodalMatrix.position(bus, bus) + 1], [dy], kind)


def _handle(jg, s, edits, mp, one_by_one=()):
    """a batch with one hand-made edit per lane: jg_nr_patch_ybus_batch for all of them, then jg_nr_patch_ybus again for the lanes of `one_by_one`"""
    L, B = jg._lib.lib(), len(edits)
    an = jg.newtonRaphson(s, batch=B, max_patch=mp)
    width = 4 if max(len(e.ptr) for e in edits) <= 4 else 8
    ptr, dy = np.zeros((B, width), dtype=np.int64), np.zeros((B, width), dtype=np.complex128)
    for b, e in enumerate(edits):
        ptr[b, :len(e.ptr)], dy[b, :len(e.ptr)] = e.ptr, e.dy
    jg._lib.check(L.jg_nr_patch_ybus_batch(an._h, 0, B, width, np.ascontiguousarray(ptr.reshape(-1)), jg.powerflow._reim(np.ascontiguousarray(dy.reshape(-1)))))
    for b in one_by_one:
        e = edits[b]
        jg._lib.check(L.jg_nr_patch_ybus(an._h, b, len(e.ptr), np.array(e.ptr, dtype=np.int64), jg.powerflow._reim(np.array(e.dy, dtype=np.complex128))))
    return an


def _rows(an, a):
    return np.asarray(a).reshape(an.batch, -1)


def _check_first_increments(an, edits, ref, tag):
    """every lane that takes a step against the oracle's first increment; returns the worst relative error"""
    inc = _rows(an, an.increment)
    worst = 0.0
    for b, e in enumerate(edits):
        if e.kind != "step":
            continue
        want = ref.first(e)
        err = np.abs(inc[b] - want).max() / max(1e-3, np.abs(want).max())
        worst = max(worst, err)
        assert err <= 1e-9, (tag, b, e.tag, err)
    print(f"[{tag}] first increment against the oracle's over {sum(e.kind == 'step' for e in edits)} lanes: worst relative error {worst:.2e} (bound 1e-9)")
    return worst


def _check_flows(an, other, edits, ref, tag):
    """status, iteration count, V / theta of every lane against the oracle's power_flow() and against the refactorising handle"""
    st, it = np.atleast_1d(an.status), np.atleast_1d(an.method.iteration)
    st2, it2 = np.atleast_1d(other.status), np.atleast_1d(other.method.iteration)
    vm, va, vm2, va2 = (_rows(an, x) for x in (an.voltage.magnitude, an.voltage.angle, other.voltage.magnitude, other.voltage.angle))
    for b, e in enumerate(edits):
        if e.kind == "bridge":
            assert st[b] == 3 and st2[b] != 0, (tag, b, e.tag)
            continue
        rc, iters, ovm, ova = ref.flow(e)
        assert rc == 0 and st[b] == 0 and it[b] == iters, (tag, b, e.tag, rc, st[b], it[b], iters)
        assert np.abs(vm[b] - ovm).max() <= 1e-8 and np.abs(va[b] - ova).max() <= 1e-8, (tag, b, e.tag)
        assert st2[b] == 0 and it2[b] == it[b], (tag, b, e.tag)
        assert np.abs(vm[b] - vm2[b]).max() <= 1e-10 and np.abs(va[b] - va2[b]).max() <= 1e-10, (tag, b, e.tag)


def _both_paths(jg, g, edits, mp, tag, one_by_one=()):
    """One iteration, then whole power flows, of a batch on the shared factor and of its refactorising twin; returns the handles (open), the
    increments of the first iteration and the worst relative error against the oracle"""
    an = _handle(jg, g.s, edits, mp, one_by_one)
    g.base.attach(an)
    twin = _handle(jg, g.s, edits, mp, one_by_one)
    jg.powerflow._push_voltage(twin, *g.start)
    jg.startFromBase_(an)
    jg.powerFlow_(an, iteration=1)
    jg.powerFlow_(twin, iteration=1)
    assert jg.firstIterationCounts(an) == (1, 0) and jg.firstIterationCounts(twin) == (0, 1)
    inc, inc2 = _rows(an, an.increment).copy(), _rows(twin, twin.increment).copy()
    worst = _check_first_increments(an, edits, g.ref, tag)
    _check_first_increments(twin, edits, g.ref, tag + ", refactorising")
    jg.startFromBase_(an)
    jg.powerFlow_(an)
    jg.powerflow._push_voltage(twin, *g.start)
    jg.powerFlow_(twin)
    assert jg.firstIterationCounts(an) == (2, 0) and jg.firstIterationCounts(twin) == (0, 2)
    _check_flows(an, twin, edits, g.ref, tag)
    vm, va = _rows(an, an.voltage.magnitude), _rows(an, an.voltage.angle)
    for b, e in enumerate(edits):
        if e.kind == "idle":                                            # no step: the start state, and whatever increment the refactorising path reports
            assert np.array_equal(vm[b], g.start[0]) and np.array_equal(va[b], g.start[1]) and np.array_equal(inc[b], inc2[b]), (tag, b, e.tag)
    return an, twin, inc, worst


# ---- 1. edit kinds -----------------------------------------------------------------------------------------------------------------------------
def _edit_kinds(jg, s):
    cat = _categories(jg, s)
    assert cat == dict(slack_pq=105, slack_pv=106, pv_pv=24, pv_pq=1, pq_pq=4, tap=8, parallel=66, bridge=7), cat
    ty = s.bus.layout.type
    pq_bus, pv_bus, slack = int(np.flatnonzero(ty == 1)[0]) + 1, int(np.flatnonzero(ty == 2)[0]) + 1, int(s.bus.layout.slack)
    assert ty[slack - 1] == 3
    shunt = 0.03 + 0.15j
    two = _outage(jg, s, cat["pq_pq"], "two entries (i,j), (j,i) of half the PQ-PQ line", factor=0.5)
    edits = [_outage(jg, s, cat[k], f"outage {k} {cat[k]}") for k in ("slack_pq", "slack_pv", "pv_pv", "pv_pq", "pq_pq", "tap", "parallel")]
    edits += [_outage(jg, s, cat["pq_pq"], "x 0.5 of the PQ-PQ line", factor=0.5), _outage(jg, s, cat["pq_pq"], "x -0.3 of the PQ-PQ line", factor=-0.3),
              _outage(jg, s, cat["tap"], "x 0.5 of the transformer", factor=0.5), _outage(jg, s, cat["slack_pv"], "x -0.3 of the slack-PV line", factor=-0.3),
              _diag(s, pq_bus, "shunt on a PQ bus", shunt), _diag(s, pv_bus, "shunt on a PV bus", shunt),
              _diag(s, slack, "shunt on the slack bus", shunt, kind="idle"),      # enters no equation: the scenario is converged at the start like the base case
              _edit(two.tag, two.ptr[2:], two.dy[2:])]
    perm = len(edits)
    edits += [_outage(jg, s, cat["tap"], "transformer outage, diagonal first", order=(0, 1, 2, 3)),
              _outage(jg, s, cat["tap"], "transformer outage, off-diagonal first", order=(2, 3, 0, 1)),
              _outage(jg, s, cat["tap"], "transformer outage, to-bus diagonal first", order=(1, 0, 3, 2))]
    edits += [_edit("base case", kind="idle"), _outage(jg, s, cat["bridge"], "bridge outage", kind="bridge")]
    single_calls = [b for b, e in enumerate(edits) if len(e.ptr) in (1, 2)] + [perm + 2]
    return edits, [perm, perm + 1, perm + 2], single_calls


@pytest.mark.parametrize("mp", [4, 8])
def test_every_kind_of_edit_takes_the_oracles_first_step(jg, oracle, mp):
    """One lane per kind of edit, none of them drawn at random: outages by the types of their end buses, an off-nominal transformer, one of two parallel
    lines, partial parameter changes of both signs, one-entry (shunt) edits on a PQ, a PV and the slack bus, a two-entry edit, one outage with its entries in
    three orders, the base case, a bridge.  mp = 8: the same 4-entry patches in a handle with 8 slots (the unused ones are skipped).  Exempt from the
    comparison of first increments: the base case and the shunt on the slack bus (neither takes a step; the oracle agrees: 0 iterations) and the bridge.
    The grid variant with a phase shifter runs the shifter's outage, a partial change of it and the permuted order."""
    g = _grid(jg, oracle, 8)
    assert g.base.info["top_pivots"] == 8
    edits, perm, single_calls = _edit_kinds(jg, g.s)
    an, twin, inc, worst = _both_paths(jg, g, edits, mp, f"edit kinds, mp {mp}", single_calls)
    assert np.array_equal(inc[perm[0]], inc[perm[1]]) and np.array_equal(inc[perm[0]], inc[perm[2]]), "the order of a patch's entries changes the increment"
    assert all(np.array_equal(_rows(an, x)[perm[0]], _rows(an, x)[p]) for x in (an.voltage.magnitude, an.voltage.angle) for p in perm[1:])
    _close(g, an, twin)
    g = _grid(jg, oracle, 8, SHIFTER)
    lab = SHIFTER[0]
    assert g.s.branch.parameter.shiftAngle[lab - 1] == SHIFTER[1] and _live(jg, g.s)[lab - 1]
    edits = [_outage(jg, g.s, lab, "phase shifter outage"), _outage(jg, g.s, lab, "x 0.5 of the phase shifter", factor=0.5),
             _outage(jg, g.s, lab, "phase shifter outage, to-bus diagonal first", order=(1, 0, 3, 2)), _edit("base case", kind="idle")]
    assert edits[0].dy[2] != edits[0].dy[3], "an asymmetric edit"
    an, twin, inc, worst = _both_paths(jg, g, edits, mp, f"phase shifter, mp {mp}")
    assert np.array_equal(inc[0], inc[2])
    _close(g, an, twin)


def test_edits_on_three_buses_make_the_run_refactorise(jg, oracle):
    """Two outages that share a bus (7 entries on three buses, classify_patch = 2) in one lane of an mp = 8 handle: the shared factor cannot serve, the run
    must refactorise by itself -- and end where the oracle ends."""
    g = _grid(jg, oracle, 8)
    lay = g.s.branch.layout
    k1, k2 = 2, 4                                                         # buses 1 - 3 and 3 - 5: bus 3 keeps its line to bus 12
    assert lay.to[k1 - 1] == lay.from_[k2 - 1] and lay.from_[k1 - 1] != lay.to[k2 - 1] and _live(jg, g.s)[[k1 - 1, k2 - 1]].all()
    merged = {}
    for lab in (k1, k2):
        for p, d in zip(*jg.outagePatch(g.s, lab)):
            merged[int(p)] = merged.get(int(p), 0.0) + d
    assert len(merged) == 7
    edits = [_outage(jg, g.s, 1, "outage 1"), _edit("outages 2 and 4", list(merged), list(merged.values())), _outage(jg, g.s, 8, "outage 8"), _edit("base case", kind="idle")]
    an = _handle(jg, g.s, edits, 8)
    g.base.attach(an)
    twin = _handle(jg, g.s, edits, 8)
    jg.powerflow._push_voltage(twin, *g.start)
    jg.startFromBase_(an)
    jg.powerFlow_(an, iteration=1)
    assert jg.firstIterationCounts(an) == (0, 1)
    _check_first_increments(an, edits, g.ref, "three buses")
    jg.startFromBase_(an)
    jg.powerFlow_(an)
    jg.powerFlow_(twin)
    assert jg.firstIterationCounts(an) == (0, 2)
    _check_flows(an, twin, edits, g.ref, "three buses")
    _close(g, an, twin)


# ---- 2. lane remainders and the exact state update ------------------------------------------------------------------------------------------------
def _state_increments(an, inc):
    """[batch][n] increments of theta and of V in bus order, zero where the quantity is no state"""
    pvpq, pq = np.asarray(an.method.pvpq), np.asarray(an.method.pq)
    dth, dv = np.zeros((inc.shape[0], pvpq.size)), np.zeros((inc.shape[0], pvpq.size))
    dth[:, pvpq > 0] = inc[:, pvpq[pvpq > 0] - 1]
    dv[:, pq > 0] = inc[:, pq[pq > 0] - 1]
    return dth, dv


def _remainder_labels(jg, s, batch):
    """non-bridge outages in label order; the last lane active, lane 0 its duplicate (batch >= 2), lane 1 the base case (batch >= 3)"""
    ok = [int(k) + 1 for k in np.flatnonzero(_live(jg, s))]
    labels = [ok[(7 * b) % len(ok)] for b in range(batch)]
    if batch >= 2:
        labels[0] = labels[-1]
    if batch >= 3:
        labels[1] = 0
    return labels


@pytest.mark.parametrize("batch", [1, 2, 16, 17, 48, 49, 63, 64, 65, 112, 113])
def test_state_after_the_first_step_is_start_minus_increment_at_every_lane_remainder(jg, oracle, batch):
    """Both sweep kernels compute old + (-1) * x from the very x they store as the increment, so theta = theta0 - inc and V = V0 - inc hold BITWISE where
    the quantity is a state, and the start is kept bitwise elsewhere (V of PV buses, the slack).  A top increment applied twice -- what the padded lanes of
    k_ctop did to the last scenario of a batch whose size leaves 1 .. 48 lanes in its last group -- breaks exactly this relation; whether it did in a given
    run was a matter of timing, so this test pins the invariant without having been certain to fail before the lanes were guarded."""
    g = _grid(jg, oracle, 8)
    assert g.base.info["top_pivots"] == 8
    labels = _remainder_labels(jg, g.s, batch)
    edits = [_outage(jg, g.s, lab, f"outage {lab}") if lab else _edit("base case", kind="idle") for lab in labels]
    an = jg.contingencyAnalysis(g.s, labels)
    assert an.batch == batch
    g.base.attach(an)
    jg.startFromBase_(an)
    jg.powerFlow_(an, iteration=1)
    assert jg.firstIterationCounts(an) == (1, 0)
    inc = _rows(an, an.increment)
    vm, va = _rows(an, an.voltage.magnitude), _rows(an, an.voltage.angle)
    dth, dv = _state_increments(an, inc)
    it = np.atleast_1d(an.method.iteration)
    for b, lab in enumerate(labels):
        if not lab:
            assert it[b] == 0 and np.array_equal(vm[b], g.start[0]) and np.array_equal(va[b], g.start[1])
            continue
        assert it[b] == 1, (b, lab)
        assert np.array_equal(va[b], g.start[1] - dth[b]), (b, lab, np.abs(va[b] - (g.start[1] - dth[b])).max())
        assert np.array_equal(vm[b], g.start[0] - dv[b]), (b, lab, np.abs(vm[b] - (g.start[0] - dv[b])).max())
    if batch >= 2:
        assert np.array_equal(inc[0], inc[-1]) and np.array_equal(vm[0], vm[-1]) and np.array_equal(va[0], va[-1])
    _check_first_increments(an, edits, g.ref, f"remainders, batch {batch}")
    _close(g, an)


# ---- 3. top sizes -------------------------------------------------------------------------------------------------------------------------------------
# top_cap -> pivots of the dense top on case118 (plan.comp_tables(cap)[0][0] on the CPU): one below 8, three odd, none a multiple of 8, and
# k steps per wave ceil(n_top / 8) = 1, 2, 3, 4, 9: every remainder of k_ctop's unroll by 4, and two trips with a tail
TOPS = {3: 3, 11: 11, 17: 17, 30: 30, 66: 66}


def _oracle_state(oracle, osys, vm, va):
    o = oracle.OracleNR(osys)
    o.set_voltage(vm, va)
    o.mismatch()
    f0 = o.vectors()[1].copy()
    o.solve()
    J, _, inc = o.vectors()
    return o, f0, J.copy(), inc.copy()


def _bus_pairs(o, n, vec):
    out = np.zeros((n, 2))
    for i in range(n):
        if o.pvpq[i]:
            out[i, 0] = vec[o.pvpq[i] - 1]
        if o.pq[i]:
            out[i, 1] = vec[o.pq[i] - 1]
    return out


@pytest.mark.parametrize("top_cap", sorted(TOPS))
def test_small_and_odd_tops(jg, oracle, top_cap):
    """The base quantities against a dense inverse of the oracle's Jacobian (as tests/test_comp_gpu.py, from the flat start so that f_0 is not zero), a
    batch-70 first step against the oracle, and a second run on the same scratch that repeats the first bitwise (the padded partial rows stay zero)."""
    t = load_case(CASE)
    s = jg.powerSystem(t)
    flat = jg.newtonRaphson(s)
    flat._pull_voltage()
    vm, va = flat.voltage.magnitude.copy(), flat.voltage.angle.copy()
    fb = jg.BaseCase(flat, top_cap=top_cap)
    n = s.bus.number
    assert fb.info["top_pivots"] == TOPS[top_cap], fb.info
    osys = oracle.OracleSystem(t)
    o, f0, J, inc0 = _oracle_state(oracle, osys, vm, va)
    rowptr, col, A = block_jacobian_from_csc(n, osys.colptr, osys.rowval, o.type, o.pq, o.pvpq, o.jcolptr, o.jrowval, J)
    D = np.zeros((2 * n, 2 * n))
    for i in range(n):
        for p in range(rowptr[i], rowptr[i + 1]):
            D[2 * i:2 * i + 2, 2 * col[p]:2 * col[p] + 2] = A[p]
    Z = np.linalg.inv(D)
    scale = np.abs(Z).max()
    zc = fb.get(0, col.size * 4).reshape(-1, 2, 2)
    worst = max(np.abs(zc[p] - Z[2 * i:2 * i + 2, 2 * col[p]:2 * col[p] + 2]).max() for i in range(n) for p in range(rowptr[i], rowptr[i + 1]))
    assert worst <= 1e-9 * scale, (worst, scale)
    assert np.abs(fb.get(2, 2 * n).reshape(n, 2) - _bus_pairs(o, n, f0)).max() <= 1e-11 * max(1.0, np.abs(s.bus.demand.active).max())
    want = _bus_pairs(o, n, inc0)
    assert np.abs(fb.get(1, 2 * n).reshape(n, 2) - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    print(f"[top {TOPS[top_cap]}] J0^-1 on the pattern: max error {worst:.2e} (scale {scale:.2e})")
    fb.close()
    flat.close()
    g = _grid(jg, oracle, top_cap)
    assert g.base.info["top_pivots"] == TOPS[top_cap]
    labels = _remainder_labels(jg, g.s, 70)
    edits = [_outage(jg, g.s, lab, f"outage {lab}") if lab else _edit("base case", kind="idle") for lab in labels]
    an = jg.contingencyAnalysis(g.s, labels)
    g.base.attach(an)
    runs = []
    for _ in range(2):
        jg.startFromBase_(an)
        jg.powerFlow_(an, iteration=1)
        runs.append((an.increment.copy(), an.voltage.magnitude.copy(), an.voltage.angle.copy()))
    assert jg.firstIterationCounts(an) == (2, 0)
    _check_first_increments(an, edits, g.ref, f"top {TOPS[top_cap]}, batch 70")
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "a second run on the same scratch differs from the first"
    dth, dv = _state_increments(an, runs[0][0])
    act = np.array([lab != 0 for lab in labels])
    assert np.array_equal(runs[0][2][act], (g.start[1] - dth)[act]) and np.array_equal(runs[0][1][act], (g.start[0] - dv)[act])
    _close(g, an)


# ---- 4. active-mask layouts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["group 1 idle, lane 63 of group 2 active", "lane 0 of group 1 active, group 2 idle"])
def test_lane_groups_that_drop_out_at_the_first_verdict(jg, oracle, layout):
    """192 lanes; the idle ones are base-case lanes, converged at the first verdict, so their groups leave the list the sweeps walk."""
    g = _grid(jg, oracle, 8)
    ok = [int(k) + 1 for k in np.flatnonzero(_live(jg, g.s))]
    labels = [ok[(5 * b) % len(ok)] for b in range(64)] + [0] * 128
    labels[191 if layout.startswith("group 1 idle") else 64] = ok[3]
    edits = [_outage(jg, g.s, lab, f"outage {lab}") if lab else _edit("base case", kind="idle") for lab in labels]
    an, twin, inc, worst = _both_paths(jg, g, edits, 4, layout)
    assert np.array_equal(np.atleast_1d(an.method.iteration) > 0, np.array(labels) != 0)
    _close(g, an, twin)


def test_monte_carlo_injections_on_the_base_grid(jg, oracle):
    """No outages, injections per lane (J_s = J_0: the sweeps alone, k_comp_fix returns at once), batch 70, top of 8: every lane against the oracle."""
    g = _grid(jg, oracle, 8)
    B, s = 70, g.s
    rng = np.random.default_rng(7)
    f = 1.0 + 0.01 * rng.standard_normal((B, 1))
    pd, qd = s.bus.demand.active[None, :] * f, s.bus.demand.reactive[None, :] * f
    edits = [_edit(f"injections {b}", power=(pd[b].copy(), qd[b].copy())) for b in range(B)]
    an = jg.newtonRaphson(s, batch=B, max_patch=4)
    jg.setInjection_(an, s.bus.supply.active[None, :] - pd, s.bus.supply.reactive[None, :] - qd)
    g.base.attach(an)
    twin = jg.newtonRaphson(s, batch=B, max_patch=4)
    jg.setInjection_(twin, s.bus.supply.active[None, :] - pd, s.bus.supply.reactive[None, :] - qd)
    jg.startFromBase_(an)
    jg.powerFlow_(an, iteration=1)
    assert jg.firstIterationCounts(an) == (1, 0)
    _check_first_increments(an, edits, g.ref, "Monte-Carlo injections")
    jg.startFromBase_(an)
    jg.powerFlow_(an)
    jg.powerflow._push_voltage(twin, *g.start)
    jg.powerFlow_(twin)
    assert jg.firstIterationCounts(an) == (2, 0) and jg.firstIterationCounts(twin) == (0, 1)
    _check_flows(an, twin, edits, g.ref, "Monte-Carlo injections")
    _close(g, an, twin)


# ---- 5. start_is_base across hand-offs ----------------------------------------------------------------------------------------------------------
def test_a_hand_off_or_a_resume_ends_the_start_from_base(jg, oracle):
    """startFromBase_(dst), then lanes of a paused run move into dst and iterate there: dst no longer holds the base's state, so its next run must
    refactorise -- a compensated step from another state is a chord step on the wrong Jacobian.  Likewise after resume() alone."""
    g = _grid(jg, oracle, 8)
    ok = [int(k) + 1 for k in np.flatnonzero(_live(jg, g.s))]
    labels = [0] * 64 + ok[:6]                                                # 6 scenarios still active after the first verdict: the run pauses at once
    src = jg.contingencyAnalysis(g.s, labels)
    dst = jg.contingencyAnalysis(g.s, [0] * len(labels))
    g.base.attach(src)
    g.base.attach(dst)
    jg.startFromBase_(dst)
    jg.startFromBase_(src)
    left = src.run_defer(defer_at=64)
    assert left == 6
    home = dst.take_lanes(src, 0)
    assert sorted(home) == list(range(64, 70))
    it, st = dst.resume(home.size)
    src.finish()
    assert (st == 0).all()
    dst._pull_voltage()
    for lane, sc in enumerate(home):                                           # the stragglers ended where the oracle ends
        rc, iters, vm, va = g.ref.flow(_outage(jg, g.s, labels[sc], "moved"))
        assert rc == 0 and it[lane] == iters
        assert np.abs(dst.voltage.magnitude[lane] - vm).max() <= 1e-8 and np.abs(dst.voltage.angle[lane] - va).max() <= 1e-8
    assert jg.firstIterationCounts(dst) == (0, 0)
    jg.powerFlow_(dst)
    assert jg.firstIterationCounts(dst) == (0, 1), "a run after a hand-off started on the shared factor from a state that is not the base's"
    # resume() alone
    jg.startFromBase_(dst)
    dst.resume(2)
    jg.powerFlow_(dst)
    assert jg.firstIterationCounts(dst) == (0, 2), "a run after resume() started on the shared factor"
    jg.startFromBase_(dst)                                                     # ... and a fresh start from the base still takes the shared factor
    jg.powerFlow_(dst)
    assert jg.firstIterationCounts(dst) == (1, 2)
    _close(g, src, dst)
