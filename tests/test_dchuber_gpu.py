"""Batched DC Huber / Schweppe-Huber estimation on the device (csrc/jg_dchuber.hip on csrc/jg_dc_lanefactor.hip) against the numpy restatement of the same
method (tests/dchuber_reference.py: same statements, dense, one lane), whose optimality tests/test_dchuber_host.py certifies on the CPU.

Tolerances.
  DEVICE_*        device against restatement: the same arithmetic in another summation order, amplified by the conditioning of H~' Q H~ near the
                  solution.  Q = 1 / d with d >= 1 (the 1 of the quadratic part), so H~' Q H~ stays as well conditioned as the WLS gain and the
                  deviations are a few units in the last place, where LAV's reach 1e-11.  Measured on one MI355X, the largest over the lanes of
                  test_mixed_lanes_against_the_restatement and test_per_row_bounds (printed by them: angles 1.11e-16, objective 5.13e-16, duals
                  7.31e-14, weights 2.71e-14) and over 240 more lanes of ten other seeds on the same two grids with omega = 1, an omega array and
                  Schweppe's weights (angles 2.22e-16, objective 9.62e-16 relative to 1 + objective, duals 7.02e-14, weights 1.70e-13; equal
                  iteration counts on all of them).  The bounds are 10 x the largest.
  LINEAR_TOL      the project's linear-step bound 1e-9 (tests/test_dc_gpu.py): a threshold no residual reaches against the device's WLS estimate.
  known answers   the reference's own criterion (dc_reference.isapprox), as in tests/test_dcse_gpu.py.
  Iteration counts are equal; the seeds are such that no verdict of a compared lane lies within 1 +- 1e-6 of its bound in the restatement
  (test_dchuber_host.fair, asserted here on the CPU before the comparison), so equal counts are a fair claim.  Bitwise claims are np.array_equal."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
import dchuber_reference as U
from test_dchuber_host import THRESHOLD, TOL, fair, grid, mixed_readings, row_omega
from test_dcse_host import monitoring_of

pytestmark = pytest.mark.gpu

MEASURED_ANGLE, MEASURED_OBJECTIVE, MEASURED_DUAL, MEASURED_WEIGHT = 2.22e-16, 9.62e-16, 7.31e-14, 1.70e-13
DEVICE_ANGLE, DEVICE_OBJECTIVE, DEVICE_DUAL, DEVICE_WEIGHT = 10 * MEASURED_ANGLE, 10 * MEASURED_OBJECTIVE, 10 * MEASURED_DUAL, 10 * MEASURED_WEIGHT
LINEAR_TOL = 1e-9


def hub(jg):
    return jg.dchuberstateestimation


def handle(jg, case, batch, ms=None, **kw):
    t, _, ms0 = grid(case)[:3]
    return jg.dcHuberStateEstimation(monitoring_of(jg, t, ms0 if ms is None else ms), batch=batch, **kw)


def unscaled(case, count, seed=None):
    """[count, m] readings as the analysis takes them: the four kinds of test_dchuber_host.mixed_readings in turn, times sigma"""
    kinds = mixed_readings(case, seed) * grid(case)[7][None, :]
    return np.stack([kinds[s % 4] for s in range(count)]), kinds


def solve(jg, an, Z):
    hub(jg).setReadings_(an, Z)
    hub(jg).solve_(an)
    return np.atleast_2d(an.voltage.angle).copy(), np.atleast_1d(an.status).copy(), np.atleast_1d(an.iterations).copy()


def results(an):
    return (np.atleast_2d(an.voltage.angle).copy(), np.atleast_2d(an.dual).copy(), np.atleast_2d(an.weight).copy(), np.atleast_2d(an.residual).copy(),
            np.atleast_1d(an.objective).copy(), np.atleast_1d(an.iterations).copy(), np.atleast_1d(an.status).copy())


def equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def restated(case, an, z, **kw):
    """the restatement of one lane on what the device sees: the reading times the analysis' scale, the analysis' bounds"""
    H, on, slack = grid(case)[3], grid(case)[5], grid(case)[6]
    ref = U.huber_ipm(H, z * an._scale, an.kappa, on, slack, **{"tolerance": TOL, **kw})
    return ref


def deviations(case, an, s, ref):
    va = grid(case)[8]
    ang, y, w, obj = np.atleast_2d(an.voltage.angle)[s], np.atleast_2d(an.dual)[s], np.atleast_2d(an.weight)[s], np.atleast_1d(an.objective)[s]
    return (np.abs(ang - va - ref.theta).max(), abs(obj - ref.objective) / (1.0 + ref.objective), np.abs(y - ref.y).max(), np.abs(w - ref.weight).max())


def compare(case, an, Z, lanes, name):
    """iteration counts equal, angles, objective, duals and weights within the DEVICE bounds; prints each figure before it asserts"""
    worst = np.zeros(4)
    it, st = np.atleast_1d(an.iterations), np.atleast_1d(an.status)
    for s in lanes:
        ref = restated(case, an, Z[s])
        assert fair(ref), (s, ref.margins)
        d = deviations(case, an, s, ref)
        worst = np.maximum(worst, d)
        print(name, case, s, "iterations", it[s], ref.iterations, "angle", d[0], "objective", d[1], "dual", d[2], "weight", d[3])
        assert st[s] == ref.status == 0 and it[s] == ref.iterations, s
        # the unscaled residual sigma (z~ - h~ theta): the angles' deviation through a row of H~, plus 16 units in the last place of the row's terms
        rowsum = np.abs(grid(case)[3]).sum(axis=1).max()
        bound = an._sigma.max() * (DEVICE_ANGLE * rowsum + 16 * 2.0 ** -52 * (np.abs(Z[s] * an._scale).max() + rowsum * np.abs(ref.theta).max()))
        assert np.abs(np.atleast_2d(an.residual)[s] - ref.residual * an._sigma).max() <= bound
        assert np.atleast_1d(an.suspect)[s] == (np.atleast_2d(an.weight)[s] < 1.0).sum()
    print(name, case, "largest: angle", worst[0], "objective", worst[1], "dual", worst[2], "weight", worst[3])
    assert worst[0] <= DEVICE_ANGLE and worst[1] <= DEVICE_OBJECTIVE and worst[2] <= DEVICE_DUAL and worst[3] <= DEVICE_WEIGHT


_SINGLE = {}


def singles(jg, case):
    """the four kinds, each solved alone in a batch of 1"""
    if case not in _SINGLE:
        out = []
        for z in unscaled(case, 4)[1]:
            an = handle(jg, case, 1)
            solve(jg, an, z[None, :])
            out.append(results(an))
            an.close()
        _SINGLE[case] = out
    return _SINGLE[case]


def same_as_single(res, s, one):
    return all(np.array_equal(x[s], y[0]) for x, y in zip(res, one))


@pytest.mark.parametrize("case", ["case14test", "case118"])
def test_known_answers(jg, case):
    """exact readings of the DC power flow give its angles, a zero loss and unit weights; of four gross errors of 40 sigma a lane suspects those off the
    leverage points (omega = 1 lets a row the estimate leans on pull the estimate to itself: what Schweppe's weights are for)"""
    t, th = grid(case)[:2]
    Z, kinds = unscaled(case, 2)
    an = handle(jg, case, 2)
    ang, st, it = solve(jg, an, Z)
    print(case, "iterations", it, "worst", np.abs(ang[0] - th).max(), "loss", an.objective, "suspect", an.suspect)
    assert (st == 0).all() and it[0] <= 3 and R.isapprox(ang[0], th)
    assert an.objective[0] <= 1e-12 and (an.weight[0] == 1.0).all() and an.suspect[0] == 0
    gross = np.flatnonzero(kinds[1] != kinds[0])
    off = gross[U.schweppe_omega(grid(case)[3], grid(case)[5], grid(case)[6])[gross] > 0.5]
    assert gross.size == 4 and off.size >= 2 and (an.weight[1, off] < 0.1).all() and an.suspect[1] >= off.size and ((an.weight > 0) & (an.weight <= 1)).all()
    an.close()


@pytest.mark.parametrize("case", ["case14test", "case118"])
def test_a_threshold_no_residual_reaches_is_the_wls_estimate(jg, case):
    t, th, ms = grid(case)[:3]
    Z, _ = unscaled(case, 4)
    an = handle(jg, case, 4, threshold=1e6)
    ang, st, it = solve(jg, an, Z)
    wls = jg.dcStateEstimation(monitoring_of(jg, t, ms), batch=4)
    jg.setReadings_(wls, Z)
    jg.stateEstimation_(wls)
    worst = np.abs(ang - wls.voltage.angle).max()
    print(case, "iterations", it, "against the device's WLS estimate", worst)
    assert (st == 0).all() and (an.weight == 1.0).all() and (an.suspect == 0).all()
    assert worst <= LINEAR_TOL * max(1.0, np.abs(wls.voltage.angle).max())
    wls.close()
    an.close()


@pytest.mark.parametrize("case", ["case14test", "case118"])
def test_mixed_lanes_against_the_restatement(jg, case):
    Z = np.concatenate([unscaled(case, 4)[0], unscaled(case, 4, seed=11)[0]])
    an = handle(jg, case, 8)
    solve(jg, an, Z)
    compare(case, an, Z, range(8), "mixed")
    an.close()


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 130])
def test_lane_edges(jg, batch):
    """exact, gross-only and noisy lanes interleaved finish at different iterations inside one group of 64; every lane, frozen early or late, padded
    group or full, is bitwise what it is when solved alone in a batch of 1"""
    case = "case14test"
    Z, _ = unscaled(case, batch)
    one = singles(jg, case)
    assert len({int(one[k][5][0]) for k in range(4)}) >= 3          # the lanes of a group do leave at different iterations
    an = handle(jg, case, batch)
    _, st, _ = solve(jg, an, Z)
    res = results(an)
    assert (st == 0).all()
    for s in range(batch):
        assert same_as_single(res, s, one[s % 4]), s
    assert an.dims()["lastIterations"] == max(int(one[k][5][0]) for k in range(min(batch, 4)))
    an.close()


def test_whole_groups_leave(jg):
    """192 lanes, the first 128 exact readings: their two groups leave after the first verdicts, the launches follow the slow lanes to the end"""
    case = "case14test"
    _, kinds = unscaled(case, 4)
    one = singles(jg, case)
    fast, slow = int(one[0][5][0]), int(one[3][5][0])
    assert fast + 3 <= slow
    Z = np.stack([kinds[0]] * 128 + [kinds[3]] * 64)
    an = handle(jg, case, 192)
    _, st, it = solve(jg, an, Z)
    res = results(an)
    assert (st == 0).all() and (it[:128] == fast).all() and (it[128:] == slow).all() and an.dims()["lastIterations"] == slow
    for s in (0, 63, 64, 127):
        assert same_as_single(res, s, one[0]), s
    for s in (128, 191):
        assert same_as_single(res, s, one[3]), s
    an.close()


def test_per_row_bounds(jg):
    """an omega array, then Schweppe's weights from the residual variances of the WLS path: both against the restatement fed the same omega"""
    case = "case14test"
    Z, _ = unscaled(case, 4)
    om = row_omega(case)
    an = handle(jg, case, 4, leverage=om)
    assert np.array_equal(an.omega, om) and np.array_equal(an.kappa, THRESHOLD * om)
    solve(jg, an, Z)
    compare(case, an, Z, range(4), "omega")
    an.close()
    an = handle(jg, case, 4, leverage="schweppe")
    H, on, slack = grid(case)[3], grid(case)[5], grid(case)[6]
    print("Schweppe's omega against numpy's", np.abs(an.omega - U.schweppe_omega(H, on, slack)).max(), "smallest", an.omega.min())
    assert (an.omega > 1e-3).all() and (an.omega <= 1.0).all() and an.omega.min() < 0.5
    solve(jg, an, Z)
    compare(case, an, Z, range(4), "schweppe")
    an.close()


def test_statuses(jg):
    case = "case14test"
    t, th, ms, H, z, on, slack, sigma, va = grid(case)
    Z, _ = unscaled(case, 4)
    # the iteration limit: status 5 on the noisy lanes with the restatement's iterate after two iterations
    short = handle(jg, case, 4, iteration=2)
    ang, st, it = solve(jg, short, Z)
    for s in (2, 3):
        ref = restated(case, short, Z[s], iteration=2)
        d = deviations(case, short, s, ref)
        print("iteration limit", s, d)
        assert st[s] == ref.status == 5 and it[s] == ref.iterations == 2
        assert d[0] <= DEVICE_ANGLE and d[2] <= DEVICE_DUAL
    short.close()
    # bus 8 hangs on bus 7 alone: without the rows that touch it no in-service row observes it
    an = handle(jg, case, 4)
    first = solve(jg, an, Z)
    rows = [i for i in range(z.size) if H[i, 7] != 0.0]
    nw = ms.w_index.size
    for i in rows:
        if i < nw:
            hub(jg).updateWattmeter_(an, i + 1, status=0)
        else:
            hub(jg).updatePmu_(an, i - nw + 1, statusAngle=0)
    ang, st, _ = solve(jg, an, Z)
    assert (st == 1).all() and np.isnan(ang).all() and np.isnan(an.objective).all() and np.isnan(an.weight).all() and np.isnan(an.residual).all()
    for i in rows:
        if i < nw:
            hub(jg).updateWattmeter_(an, i + 1, status=1)
        else:
            hub(jg).updatePmu_(an, i - nw + 1, statusAngle=1)
    assert equal(solve(jg, an, Z), first)
    # one row out of service: the restatement without that row
    hub(jg).updateWattmeter_(an, 20, status=0)
    ang, st, it = solve(jg, an, Z)
    on2 = on.copy()
    on2[19] = False
    ref = U.huber_ipm(H, Z[3] * an._scale * on2, an.kappa, on2, slack, tolerance=TOL)
    assert fair(ref) and st[3] == 0 and it[3] == ref.iterations and np.abs(ang[3] - va - ref.theta).max() <= DEVICE_ANGLE
    assert (an.residual[:, 19] == 0.0).all() and (an.weight[:, 19] == 1.0).all() and an.method.inservice == z.size - 1
    an.close()


def test_new_readings_a_new_mean_and_a_new_threshold_equal_a_fresh_handle(jg):
    case = "case14test"
    t, th, ms = grid(case)[:3]
    Z, _ = unscaled(case, 3)
    an = handle(jg, case, 3)
    solve(jg, an, Z[::-1])
    # other readings
    solve(jg, an, Z)
    fresh = handle(jg, case, 3)
    solve(jg, fresh, Z)
    assert equal(results(an), results(fresh))
    fresh.close()
    # the mean of wattmeter 5
    hub(jg).updateWattmeter_(an, 5, active=float(ms.w_mean[4]) + 0.7)
    hub(jg).solve_(an)
    ms2 = S.full_set(t, th)
    ms2.w_mean[4] += 0.7
    fresh = handle(jg, case, 3, ms=ms2)
    Z2 = Z.copy()
    Z2[:, 4] = fresh.method.mean[4]
    assert np.array_equal(an.readings, Z2)
    solve(jg, fresh, Z2)
    assert equal(results(an), results(fresh))
    moved = results(an)
    # a new threshold
    hub(jg).setThreshold_(an, 2.0)
    hub(jg).solve_(an)
    other = handle(jg, case, 3, ms=ms2, threshold=2.0)
    solve(jg, other, Z2)
    assert equal(results(an), results(other)) and not np.array_equal(results(an)[0], moved[0])
    other.close()
    # and back, with an omega array
    om = row_omega(case)
    hub(jg).setThreshold_(an, THRESHOLD, leverage=om)
    hub(jg).solve_(an)
    hub(jg).setThreshold_(fresh, leverage=om)
    hub(jg).solve_(fresh)
    assert equal(results(an), results(fresh)) and np.array_equal(an.kappa, THRESHOLD * om)
    fresh.close()
    an.close()


def test_power_follows_the_angles(jg):
    case = "case14test"
    t = grid(case)[0]
    Z, _ = unscaled(case, 3)
    an = handle(jg, case, 3)
    hub(jg).setReadings_(an, Z)
    hub(jg).stateEstimation_(an, power=True)
    f, to = np.asarray(t["br_from"]).astype(int) - 1, np.asarray(t["br_to"]).astype(int) - 1
    y = an.system.model.dc.admittance
    flows = y[None, :] * (an.voltage.angle[:, f] - an.voltage.angle[:, to] - np.asarray(t["br_shift"], dtype=np.float64)[None, :])
    assert np.abs(an.power.from_.active - flows).max() <= 1e-12 * max(1.0, np.abs(flows).max())
    assert np.array_equal(an.power.to.active, -an.power.from_.active)
    for s in range(3):
        ref = R.power(t, an.voltage.angle[s])
        assert np.abs(an.power.from_.active[s] - ref["from_"]).max() <= 1e-12 * max(1.0, np.abs(ref["from_"]).max())
    an.close()
