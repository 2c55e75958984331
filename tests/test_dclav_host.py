"""DC least-absolute-value estimation, host side: the library's host model equals the WLS model's rows, and the numpy restatement of the device's
interior-point method (tests/dclav_reference.py) is held against scipy's HiGHS on the same LP and against its own optimality certificate.

Bounds.  OBJECTIVE_TOL: the restatement's objective against linprog's, absolute, over the seeded cases below; the largest deviation measured on the CPU
is MEASURED_OBJECTIVE, the bound 10 x that (both are f64 solvers stopped near 1e-8 .. 1e-9: the factor covers another seed and no more).  The
certificate's bounds follow from the method's three stopping tests at tolerance TOL and are derived in test_the_restatements_certificate."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
import dclav_reference as L
from conftest import load_case
from test_dcse_host import monitoring_of

TOL = 1e-8
MEASURED_OBJECTIVE = 1.145e-8        # the largest of the 15 seeded lanes, on case14test (printed by test_the_restatement_against_linprog)
OBJECTIVE_TOL = 10 * MEASURED_OBJECTIVE
CASES = ["case14test", "case30test", "case118"]


def noisy_lanes(case, seed, gross):
    """(H, z, on, slack, true angles relative to the slack) of the full set of `case` with noise of 1e-2 on every reading and `gross` errors of +-5"""
    t = load_case(case)
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    H, z, on, slack = L.lav_rows(t, ms)
    rng = np.random.default_rng(seed)
    z = z + 1e-2 * rng.standard_normal(z.size)
    rows = rng.choice(z.size, gross, replace=False)
    z[rows] += 5.0 * rng.choice([-1.0, 1.0], gross)
    return H, z, on, slack, th - th[slack]


@pytest.mark.parametrize("case", ["case14test", "case30test"])
def test_the_host_model_has_the_rows_of_the_wls_model(case):
    import juliagrid.jl_amd as jg
    t = load_case(case)
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    ms.w_status[[3, 11]] = 0
    ms.p_status[2] = 0
    mon = monitoring_of(jg, t, ms)
    lav, wls = jg.dcLavModel(mon), jg.dcstateestimation.dcWlsModel(mon)
    for key in ("colptr", "rowval", "nzval"):
        assert np.array_equal(getattr(lav.coefficient, key), getattr(wls.coefficient, key)), key
    assert np.array_equal(lav.mean, wls.mean) and lav.index == wls.index
    assert lav.number == wls.number and lav.inservice == wls.inservice == wls.number - 3
    assert not hasattr(lav, "precision")                            # the reference's LAV model is unweighted


_SOLVED = {}


def solved(case, seed, gross):
    key = (case, seed, gross)
    if key not in _SOLVED:
        H, z, on, slack, th = noisy_lanes(case, seed, gross)
        _SOLVED[key] = (H, z, on, slack, L.lav_ipm(H, z, on, slack, tolerance=TOL))
    return _SOLVED[key]


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_against_linprog(case):
    worst = 0.0
    for seed, gross in enumerate([1, 2, 3, 4, 5]):
        H, z, on, slack, a = solved(case, seed, gross)
        b = L.lav_linprog(H, z, on, slack)
        print(case, seed, gross, "iterations", a.iterations, "objective", a.objective, "minus linprog's", a.objective - b.objective)
        assert a.status == 0 and a.iterations <= 30
        worst = max(worst, abs(a.objective - b.objective))
        assert abs(a.objective - b.objective) <= OBJECTIVE_TOL, (seed, gross)
    print(case, "largest deviation", worst)


@pytest.mark.parametrize("case", CASES)
def test_the_restatements_certificate(case):
    """y is dual feasible up to the stopping tests and certifies the objective.  With gap = sum u (1 - y) + v (1 + y) <= TOL (1 + obj), |rp| <= TOL (1 + max |z|)
    and |rd| <= TOL hnorm at the end:
      * a row with r_i > 2 |rp|_max has u_i >= r_i / 2, so 1 - y_i <= gap / u_i <= 2 gap / r_i (and the mirror image for r_i < 0);
      * gap = sum (u + v) - y'(r - rp), y'r = z'y + theta'rd and |sum |r| - sum (u + v)| <= sum |rp| + sum 2 min(u, v) <= m |rp|_max + gap give
        |z'y - obj| <= 2 gap + 2 m |rp|_max + |theta|_1 |rd|_max."""
    for seed, gross in enumerate([1, 2, 3, 4, 5]):
        H, z, on, slack, a = solved(case, seed, gross)
        m = int(on.sum())
        gap_max = TOL * (1.0 + a.objective)
        rp_max = TOL * (1.0 + np.abs(z).max())
        rd_max = TOL * np.abs(H).sum(axis=0).max()
        y, r = a.y, a.residual
        assert np.abs(y).max() < 1.0
        assert np.abs(H.T @ y).max() <= rd_max
        clear = np.abs(r) > 1e-3
        assert clear.sum() > m // 2
        assert (np.abs(y[clear] - np.sign(r[clear])) <= 2.0 * gap_max / np.abs(r[clear])).all()
        bound = 2.0 * gap_max + 2.0 * m * rp_max + np.abs(a.theta).sum() * rd_max
        print(case, seed, "z'y - objective", z @ y - a.objective, "bound", bound)
        assert abs(z @ y - a.objective) <= bound


def test_exact_readings_and_gross_errors_give_the_true_state():
    """the reference's own LAV test idea: exact readings return the power-flow angles, also with gross errors on rows that are not leverage points"""
    t = load_case("case14test")
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    H, z, on, slack = L.lav_rows(t, ms)
    a = L.lav_ipm(H, z, on, slack)
    assert a.status == 0 and a.iterations <= 3 and np.abs(a.theta - (th - th[slack])).max() <= 1e-12
    z2 = z.copy()
    z2[[5, 20, 40]] += 5.0
    a = L.lav_ipm(H, z2, on, slack)
    assert a.status == 0 and np.abs(a.theta - (th - th[slack])).max() <= 1e-9
    assert abs(a.objective - 15.0) <= 1e-8


def test_unobservable_and_iteration_limit():
    H, z, on, slack, _ = noisy_lanes("case14test", 0, 2)
    a = L.lav_ipm(H, z, on, slack, iteration=3)
    assert a.status == 5 and a.iterations == 3 and np.isfinite(a.theta).all()
    on = on.copy()
    on[np.abs(H[:, 7]) > 0] = False                                 # no in-service row touches bus 8
    a = L.lav_ipm(H, z, on, slack)
    assert a.status == 1 and np.isnan(a.theta).all()
