"""gaussNewton(monitoring, Orthogonal) -- jg_gn_set_method(h, 1): the correction pass of launch_increment (k_gn_hdelta, the k_gn_gain launch over the
right-hand-side records alone, Engine::forward + the plain-row backsolve on a factor built with Jordan rows off, k_gn_add) -- past 30 buses and 5 lanes:
the 118- and 300-bus grids (slack = bus 69 / 257, bus rows with up to 143 / 147 contributions = 36 / 37 GainRec records), batches of 1, 64, 65 and 130
lanes with readings of their own, lanes and lane groups that stop at different iterations, rows out of service and removed, the tag switched on a live
handle, the PMU-only model at 70 lanes.  The reference is the oracle's dense QR (OracleGN.increment_orthogonal, numpy) on the lane's own table.

Yardstick, measured on the CPU by tests/test_oracle_methods.py (dense QR against dense Peters-Wilkinson at the start point, max|orth - pw| / max|orth|):
    dev_ref(case118) = 2.5e-15        dev_ref(case300) = 4.2e-15
Bounds (tests/methods_reference.py): first increment 10 x dev_ref relative to max|ref| (2.5e-14 / 4.2e-14); V and theta after stateEstimation_
10 x dev_ref absolute, floored at 1e-9 (the runs stop at a step of 1e-8); iteration counts and status equal; lanes with the same readings equal bit for bit.

Worst values measured on one MI355X (printed by every test; `pytest -s`):
    first increment vs dense QR .......... 6.41e-15 (case118, every batch size, lanes 0 / 63 / 64 / 65 / B - 1), 1.04e-15 (case300), 6.63e-15 (353 rows out)
    LU vs Orthogonal increment ........... 5.17e-13 (case118), 1.44e-13 (case300): the size of the whole correction pass on these grids
    V / theta vs the oracle's run ........ 3.33e-16 (lane edges, rows out), 2.17e-13 / 8.55e-15 (lanes that stop at 2 and 3 iterations)
    bad data ............................. 499.994721 under both tags, vector vs oracle 1.64e-11, re-estimate 5.36e-11 from the power flow (bound 2.86e-8)
    PMU-only model, 70 lanes ............. 1.51e-11

What these tests can and cannot see (reasoned from the code and a numpy replica of the pass, not by running a broken kernel).  The correction is
G^-1 H'W (r - H d): as large as the error of the normal-equations step, 5e-13 of the step on the 118-bus grid.  Reading d_res in place of d_rho in the
second k_gn_gain launch doubles the step: every test here fails.  A record missing at the END of the right-hand-side table (the last rwave entry dropped)
leaves one bus row of H'W rho unwritten; in the replica that moves the increment past the 2.5e-14 bound for 4 of the 118 bus rows only (2 of 300), so
such a fault in the last bus rows of the pivot order can pass these tests -- no comparison of increments on a well-conditioned set can do better."""
import numpy as np
import pytest

import methods_reference as R
from test_se_gpu import _mirror, _system_like

pytestmark = pytest.mark.gpu

def _analysis(jg, oracle, case, tab, tag="Orthogonal", batch=1):
    t, s, vm, va = R.grid(oracle, case)
    sysm = _system_like(jg, t, s)
    return jg.gaussNewton(_mirror(jg, sysm, tab), getattr(jg, tag), batch=batch), sysm


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _state_gap(an, b, answer):
    vm, va = np.atleast_2d(an.voltage.magnitude)[b], np.atleast_2d(an.voltage.angle)[b]
    return float(max(np.abs(vm - answer.magnitude).max(), np.abs(va - answer.angle).max()))


@pytest.mark.parametrize("case", ["case118", "case300"])
def test_first_increment_against_the_dense_qr(jg, oracle, case):
    t, s, vm, va = R.grid(oracle, case)
    assert s.slack != 1
    tab = R.all_families(oracle, s, vm, va)
    an, sysm = _analysis(jg, oracle, case, tab)
    gn = oracle.OracleGN(s, tab)
    J = an.jacobian
    assert np.array_equal(J.colptr, gn.hcolptr) and np.array_equal(J.rowval, gn.hrowval)
    longest = int(R.contributions_per_bus(J.colptr, J.rowval, s.n).max())
    assert longest > 16                                          # a continued item of >= 5 records crosses a wave's share of 4 records
    ref = gn.increment_orthogonal()
    scale = np.abs(ref).max()
    mx = jg.incrementSE_(an)
    err = _rel(an.increment, ref)
    plain = jg.gaussNewton(_mirror(jg, sysm, tab))
    jg.incrementSE_(plain)
    gap = float(np.abs(plain.increment - an.increment).max() / scale)
    print(f"\n[{case}] longest contribution list {longest}; Orthogonal vs dense QR {err:.2e} (bound {R.increment_bound(case):.1e}); LU vs Orthogonal {gap:.2e}")
    assert err <= R.increment_bound(case)
    assert abs(mx - scale) <= R.increment_bound(case) * scale
    assert an.increment[s.slack - 1] == 0.0
    assert gap <= 1e-7                                           # what the plain normal equations are allowed (tests/test_oracle_methods.py)
    an.close(); plain.close()


REPEATS = {1: (), 64: ((62, 1),), 65: ((64, 1),), 130: ((64, 1), (129, 63))}       # (lane, lane whose readings it repeats): across the wave boundary where there is one


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_lane_edges_with_readings_per_lane(jg, oracle, B):
    """Lane b reads z + 0.25 (b % 5) sigma N(0, 1) from its own generator (lanes 0, 5, 10, ... exactly).  Lanes {0, 63, 64, 65 % B, B - 1} against the
    dense QR on a fresh table of the lane's readings.  B = 1 is the handle with lanes == 1, ld == 64: the one-scenario kernels of the engine, here with
    Jordan rows off (the forward elimination of the correction pass reads the plain triangle)."""
    case = "case118"
    t, s, vm, va = R.grid(oracle, case)
    tab = R.all_families(oracle, s, vm, va)
    src = dict(REPEATS[B])
    n1, n2 = R.lane_readings(tab, list(range(B)), repeats=REPEATS[B])
    an, _ = _analysis(jg, oracle, case, tab, batch=B)
    R.upload_lanes(an, n1, n2)
    checked = sorted({b for b in (0, 63, 64, 65 % B, B - 1) if b < B})
    assert len(checked) <= 6
    answers = {b: R.lane_answer(oracle, case, src.get(b, b)) for b in checked}
    jg.incrementSE_(an)
    inc = np.atleast_2d(an.increment).copy()
    jg.stateEstimation_(an)
    it, st = np.atleast_1d(an.method.iteration), np.atleast_1d(an.status)
    worst_inc = max(_rel(inc[b], answers[b].first) for b in checked)
    worst_state = max(_state_gap(an, b, answers[b]) for b in checked)
    print(f"\n[B = {B}] lanes {checked}: first increment vs dense QR {worst_inc:.2e} (bound {R.increment_bound(case):.1e}); "
          f"V / theta {worst_state:.2e} (bound {R.state_bound(case):.1e}); iterations {[int(it[b]) for b in checked]}")
    for b in checked:
        a = answers[b]
        assert _rel(inc[b], a.first) <= R.increment_bound(case), b
        assert a.ok and st[b] == 0 and it[b] == a.iteration, b
        assert _state_gap(an, b, a) <= R.state_bound(case), b
    vmag, vang = np.atleast_2d(an.voltage.magnitude), np.atleast_2d(an.voltage.angle)
    same = list(REPEATS[B]) + [(b, 0) for b in range(5, B, 5)]                       # the exact lanes repeat lane 0
    for b, a in same:
        assert np.array_equal(inc[b], inc[a]) and it[b] == it[a], (b, a)
        assert np.array_equal(vmag[b], vmag[a]) and np.array_equal(vang[b], vang[a]), (b, a)
    an.close()


@pytest.mark.parametrize("which", list(R.SPREAD))
def test_lanes_and_groups_that_stop_at_different_iterations(jg, oracle, which):
    """65 lanes with noise 100 (b % 5) sigma: the exact lanes stop after 2 iterations, the noisy ones after 3, so one wavefront group of the batch is
    finished while the other goes on (GroupSel{group} under method 1: factor, forward and both backsolves skip it; k_gn_hdelta, the gain launches and
    k_gn_add do not).  The conditions on the reference alone come first."""
    case, B = "case118", 65
    repeats, checked = R.SPREAD[which]
    src = dict(repeats)
    answers = {b: R.lane_answer(oracle, case, src.get(b, b), R.SPREAD_SEED, R.SPREAD_STEP) for b in checked}
    assert len({a.iteration for a in answers.values()}) >= 2
    assert all(R.margins_hold(a) for a in answers.values())
    assert answers[64].iteration != max(answers[b].iteration for b in checked if b < 64)     # the two groups stop apart
    t, s, vm, va = R.grid(oracle, case)
    tab = R.all_families(oracle, s, vm, va)
    n1, n2 = R.lane_readings(tab, list(range(B)), R.SPREAD_SEED, repeats, R.SPREAD_STEP)
    an, _ = _analysis(jg, oracle, case, tab, batch=B)
    R.upload_lanes(an, n1, n2)
    jg.stateEstimation_(an)
    worst = max(_state_gap(an, b, answers[b]) for b in checked)
    print(f"\n[{which}] lanes {checked}: iterations {[int(an.method.iteration[b]) for b in checked]}, V / theta {worst:.2e} (bound {R.state_bound(case):.1e})")
    for b in checked:
        assert an.status[b] == 0 and an.method.iteration[b] == answers[b].iteration, b
        assert _state_gap(an, b, answers[b]) <= R.state_bound(case), b
    for b, a in repeats:
        assert np.array_equal(an.voltage.magnitude[b], an.voltage.magnitude[a]) and np.array_equal(an.voltage.angle[b], an.voltage.angle[a]), (b, a)
    an.close()


def test_rows_out_of_service(jg, oracle):
    """every seventh meter out of service; rows 15, 16 (the last row of the first workgroup of the row kernels, the first of the second) and m - 1 in
    service between neighbours that are out"""
    case = "case118"
    t, s, vm, va = R.grid(oracle, case)
    tab = R.masked_table(oracle, s, vm, va)
    gn = oracle.OracleGN(s, tab)
    assert list(gn.type[R.GN_ROWS - 2:R.GN_ROWS + 2] != 0) == [False, True, True, False]
    assert list(gn.type[-4:] != 0) == [False, False, True, True] and 0.1 < np.mean(gn.type == 0) < 0.2
    an, _ = _analysis(jg, oracle, case, tab)
    assert np.array_equal(an.method.type, gn.type)
    a = R.LaneAnswer(oracle, s, tab)
    jg.incrementSE_(an)
    err = _rel(an.increment, a.first)
    jg.stateEstimation_(an)
    gap = _state_gap(an, 0, a)
    print(f"\n[{int((gn.type == 0).sum())} of {gn.m} rows out] first increment vs dense QR {err:.2e} (bound {R.increment_bound(case):.1e}); V / theta {gap:.2e}")
    assert err <= R.increment_bound(case)
    assert a.ok and an.status == 0 and an.method.iteration == a.iteration
    assert gap <= R.state_bound(case)
    an.close()


def test_a_gross_error_is_removed_under_the_tag(jg, oracle):
    """residualTest_ on an Orthogonal analysis: the same row and the same largest normalised residual as an LU analysis of the same data (1e-7 relative,
    as tests/test_baddata_gpu.py), the whole vector against the dense oracle, and after removal the power-flow state -- within 10 x what the oracle's own
    Orthogonal run leaves on the table without that row (tests/test_oracle_methods.py prints it: 2.9e-9), floored at 1e-10."""
    case = "case118"
    t, s, vm, va = R.grid(oracle, case)
    tab, row = R.bad_table(oracle, s, vm, va)
    out = {}
    for tag in ("Orthogonal", "LU"):
        an, _ = _analysis(jg, oracle, case, tab, tag)
        jg.stateEstimation_(an)
        assert an.status == 0
        out[tag] = (an, jg.residualTest_(an))
    (an, o), (lu, l) = out["Orthogonal"], out["LU"]
    assert o.detect and l.detect and o.index == l.index == row + 1 and o.label == l.label == f"Wattmeter {R.BAD_WATTMETER}"
    assert abs(o.maxNormalizedResidual - l.maxNormalizedResidual) <= 1e-7 * l.maxNormalizedResidual
    gn = oracle.OracleGN(s, tab)
    assert gn.state_estimation(40, 1e-8) == 0
    gn.increment()
    ref = oracle.gn_normalized_residuals(gn)
    assert int(np.argmax(ref)) == row
    vec = float(np.abs(jg.normalizedResidual(an) - ref).max() / ref.max())
    assert vec <= 1e-7
    assert an.method.type[row] == 0 and an.method.iteration == 0
    jg.stateEstimation_(an)
    bound = max(10.0 * R.reestimate_deviation(oracle, case), 1e-10)
    gap = float(max(np.abs(an.voltage.magnitude - vm).max(), np.abs(an.voltage.angle - va).max()))
    print(f"\nlargest normalised residual {o.maxNormalizedResidual:.6f} (LU {l.maxNormalizedResidual:.6f}), vector vs oracle {vec:.2e}; "
          f"re-estimate vs power flow {gap:.2e} (bound {bound:.2e})")
    assert an.status == 0 and gap <= bound
    assert not jg.residualTest_(an).detect
    an.close(); lu.close()


def test_the_tag_switched_on_a_live_handle(jg, oracle):
    """jg_gn_set_method on a handle that has run: the captured iteration is dropped and Engine::jordan follows the method.  Each mode runs twice, so its
    graph is replayed at least once; everything compared is compared bit for bit."""
    case, lanes = "case118", [0, 2, 4]                               # under the spread rule: 2, 3 and 3 iterations
    t, s, vm, va = R.grid(oracle, case)
    tab = R.all_families(oracle, s, vm, va)
    n1, n2 = R.lane_readings(tab, lanes, R.SPREAD_SEED, step=R.SPREAD_STEP)

    def run(an, sysm):
        an.setVoltage(sysm.bus.voltage.magnitude, sysm.bus.voltage.angle)
        jg.stateEstimation_(an)
        assert np.all(an.status == 0)
        return an.voltage.magnitude.copy(), an.voltage.angle.copy(), an.method.iteration.copy(), an.increment.copy()

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    an, sysm = _analysis(jg, oracle, case, tab, "LU", batch=3)
    R.upload_lanes(an, n1, n2)
    lu1, lu2 = run(an, sysm), run(an, sysm)
    assert same(lu1, lu2)
    jg._lib.check(jg._lib.lib().jg_gn_set_method(an._h, 1))
    or1, or2 = run(an, sysm), run(an, sysm)
    fresh, fsys = _analysis(jg, oracle, case, tab, "Orthogonal", batch=3)
    R.upload_lanes(fresh, n1, n2)
    ref = run(fresh, fsys)
    assert same(or1, ref) and same(or2, ref)
    assert not np.array_equal(or1[3], lu1[3])                        # the correction pass ran: the last increments differ in their last bits
    jg._lib.check(jg._lib.lib().jg_gn_set_method(an._h, 0))
    back1, back2 = run(an, sysm), run(an, sysm)
    assert same(back1, lu1) and same(back2, lu1)
    print(f"\niterations LU {lu1[2].tolist()} Orthogonal {or1[2].tolist()}; max |V(Orthogonal) - V(LU)| {np.abs(or1[0] - lu1[0]).max():.2e}")
    an.close(); fresh.close()


def test_pmu_only_model_with_the_tag_beyond_one_wave(jg, oracle):
    """pmuStateEstimation(monitoring, Orthogonal, batch=70) on IEEE 30, uncorrelated PMUs with noise of their own per lane (mean AND precision differ
    from lane to lane); lanes 0, 63, 64 and 69 against the linear WLS oracle on the lane's own table at 1e-9, as tests/test_pmu_gpu.py does under LU."""
    from test_oracle_pmu import case30, pmu_table
    t, osys, vm, va = case30(oracle)
    tab = pmu_table(oracle, osys, vm, va, variance=1e-6, correlated=False)
    an = jg.pmuStateEstimation(_mirror(jg, _system_like(jg, t, osys), tab), jg.Orthogonal, batch=70)
    jg.setNoise_(an, np.random.default_rng(11))
    jg.stateEstimation_(an)
    z1, v1, s1, z2, v2, s2 = an._z
    rng = np.random.default_rng(11)                                 # the draws of setNoise_, repeated
    n1 = z1[None, :] + np.sqrt(v1)[None, :] * rng.standard_normal((70, z1.size))
    n2 = z2[None, :] + np.sqrt(v2)[None, :] * rng.standard_normal((70, z2.size))
    worst = 0.0
    for b in (0, 63, 64, 69):
        om, oa = oracle.OraclePmuWLS(osys, R.lane_table(oracle, tab, n1[b], n2[b])).solve()
        worst = max(worst, np.abs(an.voltage.magnitude[b] - om).max(), np.abs(an.voltage.angle[b] - oa).max())
    print(f"\nlanes 0, 63, 64, 69 vs the linear WLS oracle {worst:.2e} (bound 1e-9)")
    assert worst <= 1e-9
    assert 1e-6 < np.abs(an.voltage.magnitude - vm).max() < 0.05        # the lanes scatter around the truth
    an.close()
