"""DC Huber / Schweppe-Huber estimation, host side: the numpy restatement of the device's interior-point method (tests/dchuber_reference.py) is held
against an independent certificate, against the WLS solve of tests/dcse_reference.py and against the power flow.

The problem is convex, so the gradient of the objective, H~' clip(z~ - H~ theta, +-kappa), vanishes at the optimum and only there: huber_certificate is
its largest entry over max_j sum_i |H~_ij| max kappa, the scale of the method's dual stopping test.  The method stops on ITS dual residual H~'y with y
strictly inside the bounds; the certificate clips the residual itself, so it is not bounded by the tolerance alone: on a row near the kink y and
clip(r) still differ when the gap test passes.  It is therefore measured.

CERTIFICATE_TOL   10 x MEASURED_CERTIFICATE, the largest certificate of the 15 seeded lanes below at tolerance TOL (printed by
                  test_the_restatement_converges_to_the_optimum: 1.5e-7 / 3.2e-6 / 7.15e-6 on 14 / 30 / 118 buses), the project's rule for OBJECTIVE_TOL (tests/test_dclav_host.py).
"""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
import dchuber_reference as U
from conftest import load_case

TOL = 1e-8
THRESHOLD = 1.345
MEASURED_CERTIFICATE = 7.15e-6
CERTIFICATE_TOL = 10 * MEASURED_CERTIFICATE
CASES = ["case14test", "case30test", "case118"]
SEED = {"case14test": 1, "case30test": 2, "case118": 3}
FAIR = 1e-6                          # no verdict of a compared lane lies within 1 +- FAIR of its bound: equal iteration counts are a fair claim

_GRID = {}


def grid(case):
    """table, power-flow angles, full measurement set, H~, z~ (exact), in-service mask, slack, sigma, the slack's angle"""
    if case not in _GRID:
        t = load_case(case)
        th, _ = R.solve(t)
        ms = S.full_set(t, th)
        H, z, on, slack, sigma = U.huber_rows(t, ms)
        _GRID[case] = (t, th, ms, H, z, on, slack, sigma, float(np.asarray(t["bus_va"], dtype=np.float64)[slack]))
    return _GRID[case]


def mixed_readings(case, seed=None):
    """the four kinds of lanes, SCALED readings [4, m]: exact, gross errors only (four of 40 sigma), noisy (one sigma), noisy with three gross errors"""
    z = grid(case)[4]
    rng = np.random.default_rng(SEED[case] if seed is None else seed)
    kinds = [z.copy() for _ in range(4)]
    kinds[1][rng.choice(z.size, 4, replace=False)] += 40.0 * rng.choice([-1.0, 1.0], 4)
    kinds[2] += rng.standard_normal(z.size)
    kinds[3] += rng.standard_normal(z.size)
    kinds[3][rng.choice(z.size, 3, replace=False)] -= 40.0
    return np.stack(kinds)


def row_omega(case):
    """a per-row omega drawn from [0.3, 1]"""
    return np.random.default_rng(100 + SEED[case]).uniform(0.3, 1.0, grid(case)[4].size)


def lanes(case):
    """five lanes (z~, kappa): exact, gross only, noisy with a per-row omega, noisy with gross errors, the same with a per-row omega"""
    Z, om = mixed_readings(case), row_omega(case)
    return [(Z[0], THRESHOLD), (Z[1], THRESHOLD), (Z[2], THRESHOLD * om), (Z[3], THRESHOLD), (Z[3], THRESHOLD * om)]


def fair(ref):
    return all(abs(g - 1.0) > FAIR for g in ref.margins)


_SOLVED = {}


def solved(case):
    if case not in _SOLVED:
        H, on, slack = grid(case)[3], grid(case)[5], grid(case)[6]
        _SOLVED[case] = [(z, k, U.huber_ipm(H, z, k, on, slack, iteration=50, tolerance=TOL)) for z, k in lanes(case)]
    return _SOLVED[case]


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_converges_to_the_optimum(case):
    H = grid(case)[3]
    worst = 0.0
    for s, (z, k, a) in enumerate(solved(case)):
        c = U.huber_certificate(H, z, a.theta, k)
        print(case, s, "status", a.status, "iterations", a.iterations, "certificate", c, "objective", a.objective, "gap", a.gap)
        worst = max(worst, c)
        assert a.status == 0 and a.iterations <= 50, s
        assert c <= CERTIFICATE_TOL, s
        assert np.abs(a.y).max() < np.max(k) and (a.u > 0).all() and (a.v > 0).all()
        assert ((a.weight > 0) & (a.weight <= 1)).all()
    print(case, "largest certificate", worst)
    assert solved(case)[0][2].iterations + 3 <= solved(case)[3][2].iterations          # exact lanes finish early, noisy ones late


@pytest.mark.parametrize("case", CASES)
def test_a_large_threshold_is_least_squares(case):
    t, th, ms, H, z, on, slack, sigma, va = grid(case)
    Z = mixed_readings(case)
    for s in (2, 3):
        a = U.huber_ipm(H, Z[s], 1e6, on, slack, tolerance=TOL)
        wls = S.solve(t, ms, Z[s] * sigma)
        assert a.status == 0 and (a.weight == 1.0).all()
        assert np.abs(a.theta + va - wls).max() <= 1e-10, s


@pytest.mark.parametrize("case", CASES)
def test_exact_readings_give_the_power_flow(case):
    t, th, ms, H, z, on, slack, sigma, va = grid(case)
    for k in (THRESHOLD, THRESHOLD * row_omega(case)):
        a = U.huber_ipm(H, z, k, on, slack, tolerance=TOL)
        assert a.status == 0 and a.iterations <= 3 and R.isapprox(a.theta + va, th)
        assert a.objective <= 1e-12 and (a.weight == 1.0).all()


def test_schweppe_bounds_hold_a_gross_error_at_a_leverage_point():
    """the row the estimate leans on most (the smallest omega) reads 50 sigma too much on a noisy lane: with omega = 1 the row keeps a bound of 1.345
    on a residual it shrinks itself; Schweppe's bound is omega times that, and the angle error is smaller"""
    case = "case14test"
    t, th, ms, H, z, on, slack, sigma, va = grid(case)
    om = U.schweppe_omega(H, on, slack)
    row = int(np.argmin(om))
    assert om[row] < 0.5 and np.all(om > 1e-3) and np.all(om <= 1.0)
    zz = mixed_readings(case)[2].copy()
    zz[row] += 50.0
    plain = U.huber_ipm(H, zz, THRESHOLD, on, slack, tolerance=TOL)
    schweppe = U.huber_ipm(H, zz, THRESHOLD * om, on, slack, tolerance=TOL)
    e0, e1 = np.abs(plain.theta + va - th).max(), np.abs(schweppe.theta + va - th).max()
    print("row", row, "omega", om[row], "angle error: omega = 1", e0, "Schweppe", e1)
    assert plain.status == 0 and schweppe.status == 0 and e1 < e0
    assert schweppe.weight[row] < plain.weight[row]                 # with omega = 1 the row pulls the estimate until its residual passes for clean


def test_unobservable_and_iteration_limit():
    case = "case14test"
    t, th, ms, H, z, on, slack, sigma, va = grid(case)
    zz = mixed_readings(case)[3]
    a = U.huber_ipm(H, zz, THRESHOLD, on, slack, iteration=2)
    assert a.status == 5 and a.iterations == 2 and np.isfinite(a.theta).all()
    on = on.copy()
    on[np.abs(H[:, 7]) > 0] = False                                 # no in-service row touches bus 8
    a = U.huber_ipm(H, zz, THRESHOLD, on, slack)
    assert a.status == 1 and np.isnan(a.theta).all()


def test_the_package_exports_the_estimator():
    import juliagrid.jl_amd as jg
    assert callable(jg.dcHuberStateEstimation) and hasattr(jg.dchuberstateestimation, "setThreshold_")
