"""Batched DC least-absolute-value estimation on the device (csrc/jg_dclav.hip, csrc/jg_dc_lanefactor.hip) against the numpy restatement of the same
method (tests/dclav_reference.py: same statements, dense, one lane) and against scipy's HiGHS on the same LP.

What is compared with what.  Objectives go against linprog's, per lane.  Angles go against linprog only where the test shows on the CPU that the
optimum is the true state (exact readings, gross errors off the leverage points); on noisy lanes the LP can have a flat optimal face (a branch metered
at both ends), of which linprog returns a vertex and an interior-point method a centre, so angles, duals and iteration counts go against the
restatement there: same method, same iterates.

Tolerances.
  OBJECTIVE_TOL   restatement against linprog, from tests/test_dclav_host.py (10 x the largest deviation measured on the CPU).
  DEVICE_*        device against restatement: the same arithmetic in another summation order, amplified by the conditioning of H' Q H near the
                  solution where Q spans many decades.  Measured on one MI355X, the largest over the lanes of test_noisy_lanes (printed by it: angles 1.27e-13, objective
                  1.78e-15, duals 8.04e-11) and over ten more noisy lanes of other seeds on the same two grids (angles 1.71e-11, objective 7.8e-15,
                  duals 7.8e-11); the objective relative to 1 + objective.  The bounds are 10 x the largest.
  known answers   the reference's own criterion (dc_reference.isapprox), as in tests/test_dcse_gpu.py.
  lane factor     relative error <= cond(H' Q H) x 2^-52 per lane: the bound of a backward-stable solve, which both the device's factor and numpy's
                  dense solve carry; the project's linear-step bound 1e-9 (tests/test_dc_gpu.py) where the lane factor repeats the shared one.
  Iteration counts are equal; bitwise claims are np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
import dclav_reference as L
from conftest import load_case
from test_dclav_host import OBJECTIVE_TOL, TOL
from test_dcse_host import monitoring_of

pytestmark = pytest.mark.gpu

MEASURED_ANGLE, MEASURED_OBJECTIVE, MEASURED_DUAL = 1.71e-11, 7.8e-15, 8.04e-11
DEVICE_ANGLE, DEVICE_OBJECTIVE, DEVICE_DUAL = 10 * MEASURED_ANGLE, 10 * MEASURED_OBJECTIVE, 10 * MEASURED_DUAL
GROSS_SEED = 20260                    # picks the rows of the gross errors of the known-answer lanes
LINEAR_TOL = 1e-9

_GRID = {}


def grid(case):
    """table, power-flow angles, full measurement set, H, z (exact), in-service mask, slack, the slack's angle"""
    if case not in _GRID:
        t = load_case(case)
        th, _ = R.solve(t)
        ms = S.full_set(t, th)
        H, z, on, slack = L.lav_rows(t, ms)
        _GRID[case] = (t, th, ms, H, z, on, slack, float(np.asarray(t["bus_va"], dtype=np.float64)[slack]))
    return _GRID[case]


def lav(jg):
    return jg.dclavstateestimation


def handle(jg, case, batch, ms=None, **kw):
    t, _, ms0 = grid(case)[:3]
    return jg.dcLavStateEstimation(monitoring_of(jg, t, ms0 if ms is None else ms), batch=batch, **kw)


def mixed_readings(case, count, seed=7):
    """lanes that finish at different iterations: exact, gross errors only, noisy, noisy with gross errors, in turn"""
    z = grid(case)[4]
    rng = np.random.default_rng(seed)
    kinds = [z.copy() for _ in range(4)]
    kinds[1][rng.choice(z.size, 3, replace=False)] += 5.0
    kinds[2] += 1e-2 * rng.standard_normal(z.size)
    kinds[3] += 1e-2 * rng.standard_normal(z.size)
    kinds[3][rng.choice(z.size, 2, replace=False)] -= 4.0
    return np.stack([kinds[s % 4] for s in range(count)]), kinds


def solve(jg, an, Z):
    lav(jg).setReadings_(an, Z)
    lav(jg).solve_(an)
    return np.atleast_2d(an.voltage.angle).copy(), np.atleast_1d(an.status).copy(), np.atleast_1d(an.iterations).copy()


_SINGLE = {}


def singles(jg, case):
    """the four kinds of mixed_readings, each solved alone in a batch of 1: angles, dual, objective, iterations"""
    if case not in _SINGLE:
        out = []
        for z in mixed_readings(case, 4)[1]:
            an = handle(jg, case, 1)
            solve(jg, an, z[None, :])
            out.append((an.voltage.angle.copy(), an.dual.copy(), an.objective, an.iterations))
            an.close()
        _SINGLE[case] = out
    return _SINGLE[case]


@pytest.mark.parametrize("case", ["case14test", "case118"])
def test_known_answers(jg, case):
    """exact readings of the DC power flow give its angles; so do 1, 2 and 3 gross errors on rows that are not leverage points (the rows come from
    GROSS_SEED; linprog confirms on the CPU that the optimum is the true state and costs exactly the errors)"""
    t, th, ms, H, z, on, slack, va = grid(case)
    rng = np.random.default_rng(GROSS_SEED)
    Z = np.tile(z, (4, 1))
    for k in (1, 2, 3):
        Z[k, rng.choice(z.size, k, replace=False)] += 5.0
        lp = L.lav_linprog(H, Z[k], on, slack)
        assert R.isapprox(lp.theta + va, th) and abs(lp.objective - 5.0 * k) <= 1e-9, k
    an = handle(jg, case, 4)
    ang, st, it = solve(jg, an, Z)
    print(case, "iterations", it, "worst", [float(np.abs(ang[k] - th).max()) for k in range(4)])
    assert (st == 0).all() and it[0] <= 3
    for k in range(4):
        assert R.isapprox(ang[k], th), k
        assert abs(an.objective[k] - 5.0 * k) <= OBJECTIVE_TOL
    an.close()


@pytest.mark.parametrize("case", ["case14test", "case118"])
def test_noisy_lanes(jg, case):
    t, th, ms, H, z, on, slack, va = grid(case)
    rng = np.random.default_rng(3)
    T = 6
    Z = z[None, :] + 1e-2 * rng.standard_normal((T, z.size))
    for s in range(T):
        Z[s, rng.choice(z.size, s, replace=False)] += 5.0 * rng.choice([-1.0, 1.0], s)
    an = handle(jg, case, T)
    ang, st, it = solve(jg, an, Z)
    assert (st == 0).all()
    m, hnorm = int(on.sum()), np.abs(H).sum(axis=0).max()
    wa = wo = wd = 0.0
    for s in range(T):
        ref = L.lav_ipm(H, Z[s], on, slack, tolerance=TOL)
        lp = L.lav_linprog(H, Z[s], on, slack)
        y, r, obj = an.dual[s], an.residual[s], an.objective[s]
        a, o, d = np.abs(ang[s] - va - ref.theta).max(), abs(obj - ref.objective) / (1.0 + ref.objective), np.abs(y - ref.y).max()
        wa, wo, wd = max(wa, a), max(wo, o), max(wd, d)
        print(case, s, "iterations", it[s], ref.iterations, "angle", a, "objective", o, "dual", d, "objective - linprog's", obj - lp.objective)
        assert it[s] == ref.iterations
        assert abs(obj - lp.objective) <= OBJECTIVE_TOL
        assert a <= DEVICE_ANGLE and o <= DEVICE_OBJECTIVE and d <= DEVICE_DUAL
        # the certificate, from dual / residual (bounds: tests/test_dclav_host.py)
        gap_max, rp_max, rd_max = TOL * (1.0 + obj), TOL * (1.0 + np.abs(Z[s]).max()), TOL * hnorm
        assert np.abs(y).max() < 1.0 and np.abs(H.T @ y).max() <= rd_max * (1.0 + 1e-6)     # (numpy's H'y is the device's up to 1e-8 of the bound)
        assert an.gap[s] <= gap_max
        clear = np.abs(r) > 1e-3
        assert (np.abs(y[clear] - np.sign(r[clear])) <= 2.0 * gap_max / np.abs(r[clear])).all()
        assert abs(Z[s] @ y - obj) <= 2.0 * gap_max + 2.0 * m * rp_max + np.abs(ang[s] - va).sum() * rd_max
        assert abs(np.abs(r).sum() - obj) <= 1e-12 * (1.0 + obj)
    print(case, "largest: angle", wa, "objective", wo, "dual", wd)
    an.close()


@pytest.mark.parametrize("batch", [1, 3, 64, 65, 130])
def test_lane_edges(jg, batch):
    """exact, gross-only and noisy lanes interleaved finish at different iterations inside one group of 64; every lane, frozen early or late, padded
    group or full, is bitwise what it is when solved alone in a batch of 1"""
    case = "case14test"
    Z, _ = mixed_readings(case, batch)
    one = singles(jg, case)
    an = handle(jg, case, batch)
    ang, st, it = solve(jg, an, Z)
    assert (st == 0).all()
    assert len({one[k][3] for k in range(4)}) >= 3                  # the lanes of a group do leave at different iterations
    dual, obj = np.atleast_2d(an.dual), np.atleast_1d(an.objective)
    for s in range(batch):
        a, y, o, i = one[s % 4]
        assert it[s] == i and np.array_equal(ang[s], a) and np.array_equal(dual[s], y) and obj[s] == o, s
    assert an.dims()["lastIterations"] == max(one[k][3] for k in range(min(batch, 4)))
    an.close()


def test_a_whole_group_finishes_before_the_next(jg):
    case = "case118"
    _, kinds = mixed_readings(case, 4)
    one = singles(jg, case)
    assert one[0][3] + 3 <= one[2][3]
    Z = np.stack([kinds[0]] * 64 + [kinds[2]] * 64)
    an = handle(jg, case, 128)
    ang, st, it = solve(jg, an, Z)
    assert (st == 0).all() and (it[:64] == one[0][3]).all() and (it[64:] == one[2][3]).all()
    for s in (0, 63, 64, 127):
        k = 0 if s < 64 else 2
        assert np.array_equal(ang[s], one[k][0]) and np.array_equal(an.dual[s], one[k][1])
    an.close()


def test_row_status(jg):
    case = "case14test"
    t, th, ms, H, z, on, slack, va = grid(case)
    Z, _ = mixed_readings(case, 3)
    an = handle(jg, case, 3)
    first = solve(jg, an, Z)
    lav(jg).updateWattmeter_(an, 20, status=0)                      # row 20 leaves: equal to an analysis built with the row out of service
    gone = solve(jg, an, Z)
    ms2 = S.full_set(t, th)
    ms2.w_status[19] = 0
    other = handle(jg, case, 3, ms=ms2)
    built = solve(jg, other, Z)
    assert an.method.inservice == other.method.inservice == z.size - 1
    assert np.array_equal(gone[0], built[0]) and np.array_equal(gone[2], built[2]) and np.array_equal(an.residual, other.residual)
    assert (an.residual[:, 19] == 0.0).all() and not np.array_equal(gone[0], first[0])
    on2 = on.copy()
    on2[19] = False
    ref = L.lav_ipm(H, Z[2] * on2, on2, slack, tolerance=TOL)
    assert gone[2][2] == ref.iterations and np.abs(gone[0][2] - va - ref.theta).max() <= DEVICE_ANGLE
    other.close()
    # bus 8 hangs on bus 7 alone: without the rows that touch it no in-service row observes it
    rows = [i for i in range(z.size) if H[i, 7] != 0.0 and i != 19]
    nw = ms.w_index.size
    for i in rows:
        if i < nw:
            lav(jg).updateWattmeter_(an, i + 1, status=0)
        else:
            lav(jg).updatePmu_(an, i - nw + 1, statusAngle=0)
    ang, st, _ = solve(jg, an, Z)
    assert (st == 1).all() and np.isnan(ang).all() and np.isnan(an.objective).all()
    for i in rows + [19]:
        if i < nw:
            lav(jg).updateWattmeter_(an, i + 1, status=1)
        else:
            lav(jg).updatePmu_(an, i - nw + 1, statusAngle=1)
    again = solve(jg, an, Z)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    an.close()


def test_weighted_equals_rows_scaled_by_hand(jg):
    case = "case14test"
    t, th, ms, H, z, on, slack, va = grid(case)
    Z, _ = mixed_readings(case, 3)
    an = handle(jg, case, 3, weighted=True)
    ang, st, it = solve(jg, an, Z)
    scale = 1.0 / np.sqrt(np.r_[ms.w_variance, ms.p_variance])
    # the same rows, scaled by hand, through the C ABI of the unweighted model
    lib, h = jg._lib.lib(), C.c_int64(0)
    val = np.ascontiguousarray(an._val * np.repeat(scale, np.diff(an._ptr)))
    jg._lib.check(lib.jg_dclav_create(C.byref(h), 14, z.size, an._ptr, an._col, val, np.ones(z.size, dtype=np.int32), slack + 1, va, 3, 0))
    jg._lib.check(lib.jg_dclav_set_readings(h.value, 0, 3, np.ascontiguousarray(Z * scale[None, :]).reshape(-1)))
    jg._lib.check(lib.jg_dclav_solve(h.value, 50, TOL))
    ang2, it2 = np.zeros((3, 14)), np.zeros(3, dtype=np.int32)
    jg._lib.check(lib.jg_dclav_get_angle(h.value, ang2.ctypes.data_as(jg._lib.VP), None, None, it2.ctypes.data_as(jg._lib.VP)))
    lib.jg_dclav_destroy(h.value)
    assert (st == 0).all() and np.array_equal(ang, ang2) and np.array_equal(it, it2)
    ref = L.lav_ipm(H * scale[:, None], Z[2] * scale, on, slack, tolerance=TOL)
    assert it[2] == ref.iterations and abs(an.objective[2] - ref.objective) <= DEVICE_OBJECTIVE * (1.0 + ref.objective)
    plain = handle(jg, case, 3)
    assert not np.array_equal(solve(jg, plain, Z)[0][2], ang[2])    # the weights do move the estimate
    plain.close()
    an.close()


def test_flows_second_solve_and_iteration_limit(jg):
    case = "case14test"
    t, th, ms, H, z, on, slack, va = grid(case)
    Z, _ = mixed_readings(case, 3)
    an = handle(jg, case, 3)
    lav(jg).setReadings_(an, Z[::-1])
    lav(jg).stateEstimation_(an, power=True)
    f, to = np.asarray(t["br_from"]).astype(int) - 1, np.asarray(t["br_to"]).astype(int) - 1
    y = an.system.model.dc.admittance
    flows = y[None, :] * (an.voltage.angle[:, f] - an.voltage.angle[:, to] - np.asarray(t["br_shift"], dtype=np.float64)[None, :])
    assert np.abs(an.power.from_.active - flows).max() <= 1e-12 * max(1.0, np.abs(flows).max())
    assert np.array_equal(an.power.to.active, -an.power.from_.active)
    second = solve(jg, an, Z)                                       # a second solve after other readings starts anew: equal to a fresh analysis
    fresh = handle(jg, case, 3)
    new = solve(jg, fresh, Z)
    assert all(np.array_equal(a, b) for a, b in zip(second, new)) and np.array_equal(an.dual, fresh.dual)
    fresh.close()
    an.close()
    short = handle(jg, case, 3, iteration=3)
    ang, st, it = solve(jg, short, Z)
    assert st[0] == 0 and (st[1:] == 5).all() and (it[1:] == 3).all() and np.isfinite(ang).all()
    short.close()


def test_initial_point_from_another_analysis(jg):
    """setInitialPoint_ replaces the start's least-squares estimate once: from the WLS estimate the lane still reaches the LAV optimum"""
    case = "case14test"
    t, th, ms, H, z, on, slack, va = grid(case)
    Z, _ = mixed_readings(case, 4)
    wls = jg.dcStateEstimation(monitoring_of(jg, t, ms))
    jg.setReadings_(wls, Z[3][None, :])
    jg.stateEstimation_(wls)
    an = handle(jg, case, 1)
    lav(jg).setReadings_(an, Z[3][None, :])
    lav(jg).setInitialPoint_(an, wls)
    lav(jg).solve_(an)
    ref = L.lav_ipm(H, Z[3], on, slack, tolerance=TOL, theta0=wls.voltage.angle - va)
    assert an.status == 0 and an.iterations == ref.iterations and np.abs(an.voltage.angle - va - ref.theta).max() <= DEVICE_ANGLE
    lp = L.lav_linprog(H, Z[3], on, slack)
    assert abs(an.objective - lp.objective) <= OBJECTIVE_TOL
    lav(jg).solve_(an)                                              # the point is used once
    assert np.array_equal(an.voltage.angle, singles(jg, case)[3][0])
    wls.close()
    an.close()


@pytest.mark.parametrize("case", ["case14test", "case118"])
def test_the_lane_valued_factor_alone(jg, case):
    t, th, ms, H, z, on, slack, va = grid(case)
    rng = np.random.default_rng(11)
    T = 65
    an = handle(jg, case, T)
    # every lane's Q = 1: the unit-weight estimate of the WLS analysis (its shared factor, all variances 1)
    unit = S.full_set(t, th, 1.0, 1.0)
    wls = jg.dcStateEstimation(monitoring_of(jg, t, unit))
    jg.stateEstimation_(wls)
    x, bad = an.factor_solve(np.ones((T, z.size)), np.tile(H.T @ z, (T, 1)))
    assert not bad.any() and (x == x[0]).all()
    assert np.abs(x[0] + va - wls.voltage.angle).max() <= LINEAR_TOL * max(1.0, np.abs(wls.voltage.angle).max())
    wls.close()
    # a random Q per lane over twelve decades against numpy's dense solve of that lane's H' Q H
    q = 10.0 ** rng.uniform(-6.0, 6.0, (T, z.size))
    rhs = rng.standard_normal((T, H.shape[1]))
    rhs[:, slack] = 0.0
    x, bad = an.factor_solve(q, rhs)
    assert not bad.any()
    worst = 0.0
    for s in (0, 1, 31, 63, 64):
        G = H.T @ (q[s][:, None] * H)
        G[slack, slack] = 1.0
        ref = np.linalg.solve(G, rhs[s])
        err, bound = np.abs(x[s] - ref).max() / np.abs(ref).max(), np.linalg.cond(G) * 2.0 ** -52
        worst = max(worst, err / bound)
        assert err <= bound, (s, err, bound)
    print(case, "largest error / bound", worst)
    # a lane whose weights leave a state unobserved reports its own bad pivot; the others do not
    q[5, np.abs(H[:, 7]) > 0] = 0.0
    x, bad = an.factor_solve(q, rhs)
    assert bad[5] == 1 and bad.sum() == 1
    an.close()
