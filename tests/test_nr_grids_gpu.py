"""Batched Newton-Raphson (csrc/jg_nr.hip: k_assemble, k_assemble1, k_check, the fast-decoupled passes; csrc/jg_engine.hip; csrc/jg_compact.hip) on the
degenerate AC grids of tests/nr_grids.py, against the oracle lane by lane.  tests/test_nr_grids_host.py holds what makes these comparisons mean
something: the coverage table (rows of 71, 40, 33, 24 and 17 entries, every row length mod 8, n = 1, 2, 16, 63, 64, 71, no PQ bus, no PV bus, the slack
as first bus, last bus, hub and leaf), the ONE tolerance (nr_grids.TOLERANCE = 1e-9, at which every oracle run that is no bridge stops clear of the
tolerance), and the oracle's own error on the increment (<= 1.9e-14 against an extended-precision dense solve).

Bounds, the project's own (tests/test_nr_gpu.py): index maps bit-exact; mismatch and Jacobian entries 1e-12 relative to the largest entry; increment 1e-9
relative to max(1, max|ref|); V and theta 1e-8 absolute; status and iteration counts equal.  Every worst deviation is printed before it is asserted.

Which assembly runs where (launch_assemble): batch 1 -> k_assemble1 (a quad of lanes per row, 64 rows per workgroup); batch 3 -> k_assemble<WAVES = 16>
(ld == 64, batch <= 32: one row per wave); batch 64 -> k_assemble<WAVES = 4> (ld == 64 but more than 32 scenarios: the throughput form); batches 65 and
130 -> the same form over 2 and 3 lane groups.  "star 71, hub last" runs at every one of them.

Worst values measured on one MI355X (`pytest -s` prints the figures of every family and batch; DESIGN.md 3.6.1 has the table per family):
    batch 1 (k_assemble1) ................ mismatch 2.10e-13, chunk maxima 3.50e-14, maxima with the last row shifted 4.60e-15, Jacobian 5.84e-16
                                           (all four on "star 71, hub last", the row of 71); increment 3.95e-14, V / theta 4.49e-14 ("comb 16 x 2 AC")
    batches 3, 64, 65, 130 ............... mismatch 2.65e-14, Jacobian 2.02e-16 ("complete 24 AC"), maxima 5.79e-15, shifted 2.69e-16, increment and
                                           V / theta 2.66e-14 ("path 40 AC"); 30 of the 76 batches hold a lane solve_ reports as singular
    full runs, batches 1, 65, 130 ........ V / theta 2.75e-14 ("comb 16 x 2 AC"); status and iteration counts equal on every lane that is no bridge; the
                                           bridge lanes end with status 3 after 0 or 1 iterations (the oracle: status 3, or status 1 at the limit)
    lane-valued types .................... V / theta 1.20e-14 ("star 71, hub last")
    fast decoupled ....................... B', B'' 0 (exact), mismatch 2.65e-14, one step 2.32e-14, full runs 1.55e-14 with equal iteration counts

What these tests can and cannot see (reasoned from the kernels, not by running a broken one).
  * A tail entry of a long row dropped or counted twice (the clamped tail of k_assemble's chunk of 4, k_assemble1's `pc + 4 * k < p1`): the row sums s1,
    s2 of that bus lose or double a term of the size of the branch admittance times V, so the mismatch row moves by ~1 against a 1e-12 bound, and the
    off-diagonal block of that entry is missing or stale in the Jacobian.  Rows of every length mod 8 are there, 71 = 8 x 8 + 7 and 40 = 8 x 5 among them.
  * A wrong diagonal position from the quad shuffle (`pd += __shfl_xor(pd, d)`): the diagonal block lands in another factor entry; the Jacobian
    comparison sees the hole and the stray block, the increment follows.  The diagonal is the first entry of the 40-row (lane 0 of the quad, first trip)
    and the last of the 71-row (lane 2, last trip, second slot).
  * A dead quad of k_assemble1 storing (n = 1, 2, 9 ... 63, 71: the last workgroup has dead quads that alias row n - 1): the store would rewrite row
    n - 1's mismatch with sums over an EMPTY entry range (p1 = p0), i.e. minus the injection alone -- seen unless the race happens to end well; on "star
    71, hub last" row n - 1 is the hub.
  * A chunk maximum that misses the last partial chunk: every step test shifts the injection of the last bus that is no slack by ten times the largest mismatch of the start point (at least 10 pu) first, so the
    largest mismatch sits in the last chunk of 16 rows (the last partial wave of k_assemble1); max|f_P| then misses by that much.
  * A bridge lane's NaN reaching a neighbour: the full runs are repeated with the bridge lanes turned into base lanes; every OTHER lane must come out bit
    for bit the same, whether its neighbour turned NaN at once (status 3), after some iterations, or ran to the limit.
  * Not seen: an error below the bounds (a wrong last bit of a sum), the order in which the quad's sums meet, and anything in launches these sizes do
    not reach (the multifrontal top of 10 000-bus plans, more than 3 lane groups: tests/test_wide_batches_gpu.py, tests/test_big_grids_gpu.py).
"""
import numpy as np
import pytest

import nr_grids as N

pytestmark = pytest.mark.gpu

ORDER = [n for n in N.NAMES if n != "one bus"] + ["one bus"]          # the grid without a single unknown runs last


def _mx(a):
    a = np.asarray(a)
    return float(np.abs(a).max()) if a.size else 0.0


def _lanes(name, B):
    lab = N.labels(name)
    return [lab[b % len(lab)] for b in range(B)]


def _analysis(jg, name, B, lanes=None):
    s = N.system(name, jg)
    an = jg.newtonRaphson(s, batch=B)
    for b, k in enumerate(lanes or ()):
        if k:
            jg.setOutage_(an, b, k)
    return s, an


def _last_free_bus(t):
    typ = t["bus_type"]
    return int(np.flatnonzero(typ != 3)[-1]) if np.any(typ != 3) else None


def _shift(name):
    """pu, far above the mismatch of the start point (0.7 at the hub of "star 71, hub last", 40 on "pegaseShaped 60")"""
    return 10.0 * max(1.0, N.first(name, 0).dp)


def _shifted_maxima(jg, s, an, name, lanes):
    """max|f_P|, max|f_Q| with _shift(name) added to the active injection of the last bus that is no slack: the largest mismatch sits in the last chunk of rows.
    Returns the worst deviation from the oracle over the lanes that are no bridge (relative to the largest mismatch), and restores the injections."""
    k = _last_free_bus(N.family(name))
    if k is None:
        return 0.0
    bus = s.bus
    P, Q = bus.supply.active - bus.demand.active, bus.supply.reactive - bus.demand.reactive
    P2 = P.copy()
    P2[k] += _shift(name)
    jg.setInjection_(an, P2, Q)
    dp, dq = (np.atleast_1d(x) for x in jg.mismatch_(an))
    sy = N.osys(name)
    ps = sy.ps.copy()
    ps[k] += _shift(name)
    worst = 0.0
    refs = {}
    for b, lab in enumerate(lanes):
        if lab in N.bridge(name):
            continue
        if lab not in refs:
            o = N.patched(name, lab)
            o.set_power(ps, sy.qs, sy.pd, sy.qd)
            refs[lab] = o.mismatch()
            assert abs(o.vectors()[1][o.pvpq[k] - 1]) == refs[lab][0] > 0.5 * _shift(name)      # the shifted row IS the largest
        op, oq = refs[lab]
        worst = max(worst, abs(dp[b] - op) / max(1.0, op, oq), abs(dq[b] - oq) / max(1.0, op, oq))
    jg.setInjection_(an)
    return worst


@pytest.mark.parametrize("name", ORDER)
def test_maps_and_one_newton_step_of_a_single_instance(jg, name):
    """batch 1: k_assemble1 and the single-instance factorisation and sweeps.  Maps bit-exact, dimJ what the types say, mismatch and Jacobian element by
    element, the increment and V, theta after solve_"""
    t = N.family(name)
    n, npq = t["bus_type"].size, int(np.sum(t["bus_type"] == 1))
    ref = N.first(name, 0)
    s, an = _analysis(jg, name, 1)
    assert np.array_equal(an.method.pq, ref.pq) and np.array_equal(an.method.pvpq, ref.pvpq) and np.array_equal(an.method.pcount, ref.pcount)
    J = an.jacobian
    assert np.array_equal(J.colptr, ref.jcolptr) and np.array_equal(J.rowval, ref.jrowval)
    assert an.dims["dimJ"] == ref.dim == n - 1 + npq and an.dims["nnzJ"] == ref.nnzJ
    assert an.dims["dimJ"] == {"one bus": 0, "two buses, PV": 1, "all PV ring 9": 8, "star 17 all PV": 16}.get(name, an.dims["dimJ"])
    assert np.array_equal(an.voltage.magnitude, ref.vm0) and np.array_equal(an.voltage.angle, ref.va0)      # both sides start from the same point
    shifted = _shifted_maxima(jg, s, an, name, [0])
    dp, dq = jg.mismatch_(an)
    f = an.mismatch
    scale = max(1.0, _mx(ref.f))
    df, dmax = _mx(f - ref.f) / scale, max(abs(dp - ref.dp), abs(dq - ref.dq)) / scale
    jv = an.jacobian.nzval
    dj = _mx(jv - ref.J) / max(_mx(ref.J), 1e-300)
    jg.solve_(an)
    inc = an.increment
    di = _mx(inc - ref.inc) / max(1.0, _mx(ref.inc))
    dv = max(_mx(an.voltage.magnitude - ref.vm), _mx(an.voltage.angle - ref.va))
    print(f"\n[{name}, batch 1] dimJ {ref.dim}: mismatch {df:.2e}, maxima {dmax:.2e}, maxima with the last row shifted {shifted:.2e}, Jacobian {dj:.2e}, "
          f"increment {di:.2e}, V / theta {dv:.2e}")
    assert df <= 1e-12 and dmax <= 1e-12 and shifted <= 1e-12
    assert dj <= 1e-12
    assert di <= 1e-9
    assert dv <= 1e-8
    assert an.method.iteration == 1
    an.close()


@pytest.mark.parametrize("B", [3, 64, 65, 130])
@pytest.mark.parametrize("name", ORDER)
def test_one_newton_step_through_the_batched_kernels(jg, name, B):
    """lane b carries label labels[b % len(labels)].  Batch 3: k_assemble<WAVES = 16>; 64: k_assemble<WAVES = 4>, one lane group; 65, 130: two and three
    groups.  Every lane that is no bridge against the oracle patched with that lane's outagePatch; lanes with the same label equal bit for bit.  A lane
    whose outage leaves a bus without any admittance has no Jacobian to factorise: solve_ then reports the singular pivot AFTER the step of the batch is
    done, and the other lanes are compared as usual."""
    lanes = _lanes(name, B)
    lab = N.labels(name)
    s, an = _analysis(jg, name, B, lanes)
    shifted = _shifted_maxima(jg, s, an, name, lanes)
    dp, dq = (np.atleast_1d(x) for x in jg.mismatch_(an))
    f = np.atleast_2d(an.mismatch).copy()
    jv = np.atleast_2d(an.jacobian.nzval).copy()
    singular = False
    try:
        jg.solve_(an)
    except RuntimeError as e:
        assert "singular" in str(e) and any(k in N.bridge(name) for k in lanes), e
        singular = True
        an._pull_voltage()
    inc = np.atleast_2d(an.increment).copy()
    vm, va = np.atleast_2d(an.voltage.magnitude), np.atleast_2d(an.voltage.angle)
    df = dmax = dj = di = dv = 0.0
    for b, k in enumerate(lanes):
        if k in N.bridge(name):
            continue
        ref = N.first(name, k)
        scale = max(1.0, _mx(ref.f))
        df = max(df, _mx(f[b] - ref.f) / scale)
        dmax = max(dmax, abs(dp[b] - ref.dp) / scale, abs(dq[b] - ref.dq) / scale)
        dj = max(dj, _mx(jv[b] - ref.J) / max(_mx(ref.J), 1e-300))
        di = max(di, _mx(inc[b] - ref.inc) / max(1.0, _mx(ref.inc)))
        dv = max(dv, _mx(vm[b] - ref.vm), _mx(va[b] - ref.va))
    print(f"\n[{name}, batch {B}] {sum(k not in N.bridge(name) for k in lanes)} lanes that are no bridge: mismatch {df:.2e}, maxima {dmax:.2e}, maxima with the "
          f"last row shifted {shifted:.2e}, Jacobian {dj:.2e}, increment {di:.2e}, V / theta {dv:.2e}" + ("; solve_ reported a singular lane" if singular else ""))
    assert df <= 1e-12 and dmax <= 1e-12 and shifted <= 1e-12
    assert dj <= 1e-12
    assert di <= 1e-9
    assert dv <= 1e-8
    for b in range(len(lab), B):                                      # the same label in another lane, another wave half, another lane group
        a = b % len(lab)
        assert np.array_equal(f[b], f[a], equal_nan=True) and np.array_equal(jv[b], jv[a], equal_nan=True), (b, a)
        assert dp[b] == dp[a] or (np.isnan(dp[b]) and np.isnan(dp[a])), (b, a)
        if lanes[b] not in N.bridge(name):
            assert np.array_equal(inc[b], inc[a]) and np.array_equal(vm[b], vm[a]) and np.array_equal(va[b], va[a]), (b, a)
    an.close()


def _run(jg, name, B, lanes):
    s, an = _analysis(jg, name, B, lanes if B > 1 else None)
    jg.powerFlow_(an, iteration=N.ITERATION, tolerance=N.TOLERANCE)
    out = (np.atleast_1d(an.status).copy(), np.atleast_1d(an.method.iteration).copy(), np.atleast_2d(an.voltage.magnitude).copy(),
           np.atleast_2d(an.voltage.angle).copy())
    an.close()
    return out


@pytest.mark.parametrize("B", [1, 65, 130])
@pytest.mark.parametrize("name", ORDER)
def test_full_runs_with_bridge_lanes_beside_healthy_ones(jg, name, B):
    """powerFlow_ at nr_grids.TOLERANCE: status and iteration count of every lane that is no bridge equal the oracle's, V and theta within 1e-8; a bridge
    lane ends with a status != 0.  Then the same batch with the bridge lanes turned into base lanes: every OTHER lane is bit for bit the same, so a
    lane that turned NaN, or ran to the limit through compactions and lane moves, has not reached its neighbours."""
    lanes = _lanes(name, B) if B > 1 else [0]
    st, it, vm, va = _run(jg, name, B, lanes)
    healthy = [b for b, k in enumerate(lanes) if k not in N.bridge(name)]
    sick = [b for b, k in enumerate(lanes) if k in N.bridge(name)]
    dv = 0.0
    for b in healthy:
        ref = N.run(name, lanes[b])
        assert st[b] == 0 == ref.status, (b, lanes[b], st[b])
        assert it[b] == ref.iteration, (b, lanes[b], it[b], ref.iteration)
        dv = max(dv, _mx(vm[b] - ref.vm), _mx(va[b] - ref.va))
    print(f"\n[{name}, batch {B}] {len(healthy)} lanes against the oracle: V / theta {dv:.2e}; iterations {np.bincount(it[healthy]).tolist()}; bridge lanes: "
          f"status {sorted(set(int(x) for x in st[sick]))}, iterations {sorted(set(int(x) for x in it[sick]))}")
    assert dv <= 1e-8
    assert all(st[b] != 0 for b in sick)
    if sick:
        st2, it2, vm2, va2 = _run(jg, name, B, [0 if k in N.bridge(name) else k for k in lanes])
        assert np.array_equal(st2[healthy], st[healthy]) and np.array_equal(it2[healthy], it[healthy])
        assert np.array_equal(vm2[healthy], vm[healthy]) and np.array_equal(va2[healthy], va[healthy])
        assert np.all(st2[sick] == 0) and np.array_equal(vm2[sick[0]], vm2[0])


# the PV bus that turns PQ in two lanes, and the reactive injection it is given
LANE_TYPES = {"star 40, hub first PV": 0, "star 71, hub last": 12, "all PV ring 9": 1}
LANE_Q = 0.05


def _typed_reference(name):
    """the oracle with bus LANE_TYPES[name] as a PQ bus that injects LANE_Q, from the start point of the device (newtonRaphson()'s, with that bus still PV)"""
    t = N.family(name)
    k = LANE_TYPES[name]
    assert t["bus_type"][k] == 2
    tp = t["bus_type"].copy()
    tp[k] = 1
    sy = N.osys(name)
    qs = sy.qs.copy()
    qs[k] = LANE_Q + sy.qd[k]
    o = N.patched(name, 0, types=tp, qs=qs)
    base = N.first(name, 0)
    o.set_voltage(base.vm0, base.va0)
    return tp, N.finish(o, o.power_flow(iteration=N.ITERATION, tolerance=N.TOLERANCE))


@pytest.mark.parametrize("name", list(LANE_TYPES))
def test_lane_valued_bus_types_across_the_wave_boundary(jg, name):
    """k_assemble<.., LT = true>: batch 65, lanes 63 and 64 (the last of the first lane group, the first of the second) have a PV bus turned PQ -- on "star
    40" the hub itself, the row of 40 entries.  Those lanes against an oracle built with that type vector; the untouched lanes bit for bit what a batch
    without any edit computes."""
    B, edited = 65, [63, 64]
    tp, ref = _typed_reference(name)
    assert ref.status == 0 and N.margins_hold(ref), ref.history[-2:]
    k = LANE_TYPES[name]
    s, an = _analysis(jg, name, B)
    _, plain = _analysis(jg, name, B)
    jg.setBusType_(an, tp, edited)
    bus = s.bus
    P = np.broadcast_to(bus.supply.active - bus.demand.active, (B, bus.number)).copy()
    Q = np.broadcast_to(bus.supply.reactive - bus.demand.reactive, (B, bus.number)).copy()
    Q[edited, k] = LANE_Q
    jg.setInjection_(an, P, Q)
    jg.powerFlow_(an, iteration=N.ITERATION, tolerance=N.TOLERANCE)
    jg.powerFlow_(plain, iteration=N.ITERATION, tolerance=N.TOLERANCE)
    typ, _ = jg.busType(an)
    dv = max(max(_mx(an.voltage.magnitude[b] - ref.vm), _mx(an.voltage.angle[b] - ref.va)) for b in edited)
    print(f"\n[{name}] bus {k + 1} PV -> PQ in lanes {edited}: V / theta {dv:.2e}, iterations {[int(an.method.iteration[b]) for b in edited]} (oracle {ref.iteration})")
    for b in edited:
        assert np.array_equal(typ[b], tp)
        assert an.status[b] == 0 and an.method.iteration[b] == ref.iteration, b
    assert dv <= 1e-8
    assert _mx(an.voltage.magnitude[63] - an.voltage.magnitude[0]) > 1e-6            # the edit did change the lane
    others = [b for b in range(B) if b not in edited]
    assert np.array_equal(an.voltage.magnitude[others], plain.voltage.magnitude[others]) and np.array_equal(an.voltage.angle[others], plain.voltage.angle[others])
    assert np.array_equal(an.method.iteration[others], plain.method.iteration[others]) and np.all(an.status[others] == 0)
    base = N.run(name, 0)
    assert an.method.iteration[0] == base.iteration and max(_mx(an.voltage.magnitude[0] - base.vm), _mx(an.voltage.angle[0] - base.va)) <= 1e-8
    an.close(); plain.close()


FAST_LIMIT = 100


def _fast(jg, name, bx):
    return (jg.fastNewtonRaphsonBX if bx else jg.fastNewtonRaphsonXB)(N.system(name, jg))


@pytest.mark.parametrize("bx", [True, False])
@pytest.mark.parametrize("name", ORDER)
def test_fast_decoupled_model_mismatch_and_step(jg, oracle, name, bx):
    """fastNewtonRaphsonBX / XB on every family, as tests/test_fast_gpu.py::test_model_mismatch_and_step_match_oracle: B', B'' element by element,
    mismatches 1e-12, V and theta after one solve_ 1e-9.  The families without a PQ bus have an EMPTY B'': the device factorises the block matrix
    diag(B', B'') with identity blocks where a bus is in neither (jg_nr_fast_setup: "the caller pads slack / PV rows and columns with identity"), so the
    Q half is a solve with the identity on a zero right-hand side -- a correct solve, pinned here: the magnitudes stay bitwise at their start."""
    an = _fast(jg, name, bx)
    o = oracle.OracleFastNR(oracle.OracleSystem(N.family(name)), bx)
    assert np.array_equal(an.method.pq, o.pq) and np.array_equal(an.method.pvpq, o.pvpq)
    dm = 0.0
    for M, R in ((an.method.active.jacobian, o.P), (an.method.reactive.jacobian, o.Q)):
        assert M.toscipy().shape == R.shape
        if R.shape[0]:
            dm = max(dm, abs(M.toscipy() - R).max() / max(1.0, abs(R).max()))
    vm0 = np.array(an.voltage.magnitude)
    dp, dq = jg.mismatch_(an)
    op, oq = o.mismatch()
    scale = max(1.0, op, oq)
    f = an.mismatch
    df = max(abs(dp - op), abs(dq - oq), _mx(f[:o.mismP.size] - o.mismP), _mx(f[o.mismP.size:] - o.mismQ)) / scale
    jg.solve_(an)
    o.solve()
    dv = max(_mx(an.voltage.magnitude - o.vm), _mx(an.voltage.angle - o.va))
    print(f"\n[{name}, {'BX' if bx else 'XB'}] B', B'' {dm:.2e}, mismatch {df:.2e}, V / theta after one step {dv:.2e}; npq = {o.npq}")
    assert dm <= 1e-12 and df <= 1e-12 and dv <= 1e-9
    assert f.size == o.mismP.size + o.mismQ.size == an.dims["dimJ"]
    if o.npq == 0:
        assert np.array_equal(an.voltage.magnitude, vm0)
    an.close()


@pytest.mark.parametrize("bx", [True, False])
@pytest.mark.parametrize("name", ["star 33, hub slack", "star 71, hub last", "star 40, hub first PV", "complete 24 AC", "all PV ring 9", "star 17 all PV"])
def test_fast_decoupled_full_runs(jg, oracle, name, bx):
    """the three stars, the clique and the two grids with an empty B'': the oracle's run stops clear of the tolerance (asserted first), then iteration
    count and status are equal and V, theta within 1e-8"""
    o = oracle.OracleFastNR(oracle.OracleSystem(N.family(name)), bx)
    hist = []
    status = 1
    for _ in range(FAST_LIMIT + 1):                                   # OracleFastNR.power_flow, keeping the checks
        dp, dq = o.mismatch()
        hist.append(max(dp, dq))
        if dp < N.TOLERANCE and dq < N.TOLERANCE:
            status = 0
            break
        if o.iteration == FAST_LIMIT:
            break
        o.solve()
    assert status == 0 and hist[-1] * (1.0 + N.MARGIN) <= N.TOLERANCE and hist[-2] >= N.TOLERANCE * (1.0 + N.MARGIN), hist[-2:]
    an = _fast(jg, name, bx)
    jg.powerFlow_(an, iteration=FAST_LIMIT, tolerance=N.TOLERANCE)
    dv = max(_mx(an.voltage.magnitude - o.vm), _mx(an.voltage.angle - o.va))
    print(f"\n[{name}, {'BX' if bx else 'XB'}] {o.iteration} iterations (device {an.method.iteration}), V / theta {dv:.2e}")
    assert an.status == 0 and an.method.iteration == o.iteration
    assert dv <= 1e-8
    an.close()


def test_one_bus_is_solved_before_the_first_iteration(jg, oracle):
    """n = 1, dimJ = 0: the slack alone.  jg_nr_create keeps a block row per BUS (the slack's is an identity block), so no table, launch grid or
    allocation of the handle is empty: the assembly runs one row, the verdict finds no mismatch, and powerFlow_ returns status 0 after 0 iterations with
    the slack at its unit's set-point -- for one lane and for a batch, under Newton-Raphson and under both fast variants."""
    t = N.family("one bus")
    ref = N.run("one bus", 0)
    assert ref.status == 0 and ref.iteration == 0 and ref.vm[0] == t["gen_vg"][0]
    for B in (1, 3, 65):
        s, an = _analysis(jg, "one bus", B)
        assert an.dims["dimJ"] == 0 and an.dims["nnzJ"] == 0
        dp, dq = (np.atleast_1d(x) for x in jg.mismatch_(an))
        assert np.all(dp == 0.0) and np.all(dq == 0.0)
        assert np.atleast_2d(an.mismatch).shape == (B, 0)
        jg.powerFlow_(an, iteration=N.ITERATION, tolerance=N.TOLERANCE)
        assert np.all(np.atleast_1d(an.status) == 0) and np.all(np.atleast_1d(an.method.iteration) == 0)
        assert np.all(np.atleast_2d(an.voltage.magnitude) == ref.vm[0]) and np.all(np.atleast_2d(an.voltage.angle) == ref.va[0])
        an.close()
    for bx in (True, False):
        an = _fast(jg, "one bus", bx)
        jg.powerFlow_(an, iteration=FAST_LIMIT, tolerance=N.TOLERANCE)
        assert an.status == 0 and an.method.iteration == 0 and an.voltage.magnitude[0] == ref.vm[0]
        an.close()
