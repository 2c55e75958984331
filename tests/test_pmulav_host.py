"""PMU least-absolute-value estimation, host side: the numpy restatement of the device's interior-point method without a fixed state
(tests/pmulav_reference.py on the iteration of tests/dclav_reference.py) is held against scipy's HiGHS on the same LP, the lanes with gross phasor errors
that the GPU known-answer test uses are shown to have the power-flow state as their optimum, and the library's host model equals the restatement's.

Grids: case14test and case30test, a bus PMU at every bus plus both ends of every in-service branch (18 of case14test's 20 branches are in service: 50 PMUs, 100 rows on 28 states).  The state is
the recorded Newton-Raphson solution (tests/golden/results_*.npz); the readings are computed from it, so they are exact for it whatever its own residual.

Bounds.  OBJECTIVE_TOL: the restatement's objective against linprog's, absolute, over the seeded lanes below (exact, noisy with sigma = 1e-2 on magnitude and
angle, 1 to 3 gross phasor errors of magnitude x 1.5 and angle + 0.5 rad); the largest deviation measured on the CPU is MEASURED_OBJECTIVE (printed by
test_the_restatement_against_linprog), the bound 10 x that.  KNOWN_TOL = 1e-8 is the reference's own atol for this estimator
(test/utility/utility.jl:298-300).  The coefficient matrix is compared at 1e-12 relative."""
import numpy as np
import pytest

import pmulav_reference as P
from conftest import load_case, load_golden

TOL = 1e-8
MEASURED_OBJECTIVE = 9.30e-10        # the largest of the seeded lanes of both grids (printed by test_the_restatement_against_linprog)
OBJECTIVE_TOL = 10 * MEASURED_OBJECTIVE
KNOWN_TOL = 1e-8
GROSS_SEED = 2026                    # picks the devices of the gross errors of the known-answer lanes
CASES = ["case14test", "case30test"]

_GRID = {}


def grid(case):
    """table, power-flow magnitudes and angles, the full PMU table, H, z (exact), in-service mask"""
    if case not in _GRID:
        t, g = load_case(case), load_golden(case)
        vm, va = np.asarray(g["newtonRaphson_voltageMagnitude"], dtype=np.float64), np.asarray(g["newtonRaphson_voltageAngle"], dtype=np.float64)
        pmus = P.pmu_table(t, vm, va)
        H, z, on = P.pmulav_rows(t, pmus)
        _GRID[case] = (t, vm, va, pmus, H, z, on)
    return _GRID[case]


def corrupt(mag, ang, devices):
    mag, ang = mag.copy(), ang.copy()
    mag[devices] *= 1.5
    ang[devices] += 0.5
    return mag, ang


def gross_lanes(case):
    """the known-answer lanes: exact readings, then 1, 2 and 3 gross phasor errors on devices drawn from GROSS_SEED -> magnitude, angle [4, pmus], the
    devices of every lane"""
    pmus = grid(case)[3]
    rng = np.random.default_rng(GROSS_SEED)
    mags, angs, devs = [pmus.magnitude], [pmus.angle], [np.zeros(0, dtype=int)]
    for k in (1, 2, 3):
        d = np.sort(rng.choice(pmus.kind.size, k, replace=False))
        m, a = corrupt(pmus.magnitude, pmus.angle, d)
        mags.append(m); angs.append(a); devs.append(d)
    return np.stack(mags), np.stack(angs), devs


def mixed_readings(case, count, seed=7):
    """lanes that finish at different iterations: exact, gross errors only, noisy, noisy with gross errors, in turn -> magnitude, angle [count, pmus]"""
    pmus = grid(case)[3]
    rng = np.random.default_rng(seed)
    P_ = pmus.kind.size
    kinds = [(pmus.magnitude.copy(), pmus.angle.copy())]
    kinds.append(corrupt(pmus.magnitude, pmus.angle, rng.choice(P_, 3, replace=False)))
    noisy = lambda: (pmus.magnitude + 1e-2 * rng.standard_normal(P_), pmus.angle + 1e-2 * rng.standard_normal(P_))
    kinds.append(noisy())
    m, a = noisy()
    kinds.append(corrupt(m, a, rng.choice(P_, 2, replace=False)))
    return np.stack([kinds[s % 4][0] for s in range(count)]), np.stack([kinds[s % 4][1] for s in range(count)])


def seeded_lanes(case):
    """the lanes of the linprog comparison: exact, three noisy, and noisy with 1, 2, 3 gross errors"""
    t, vm, va, pmus, H, z, on = grid(case)
    P_ = pmus.kind.size
    yield "exact", pmus.magnitude, pmus.angle
    for seed in range(3):
        rng = np.random.default_rng(seed)
        yield f"noisy{seed}", pmus.magnitude + 1e-2 * rng.standard_normal(P_), pmus.angle + 1e-2 * rng.standard_normal(P_)
    for gross in (1, 2, 3):
        rng = np.random.default_rng(10 + gross)
        m, a = pmus.magnitude + 1e-2 * rng.standard_normal(P_), pmus.angle + 1e-2 * rng.standard_normal(P_)
        yield f"gross{gross}", *corrupt(m, a, rng.choice(P_, gross, replace=False))
    mags, angs, _ = gross_lanes(case)
    for k in (1, 2, 3):
        yield f"known{k}", mags[k], angs[k]


def monitoring_of(jg, t, pmus, magnitude=None, angle=None):
    """the same set in the library's Measurement container"""
    mon = jg.measurement(jg.powerSystem(t))
    mag = pmus.magnitude if magnitude is None else magnitude
    ang = pmus.angle if angle is None else angle
    for i in range(pmus.kind.size):
        where = {0: "bus", 1: "from_", 2: "to"}[int(pmus.kind[i])]
        jg.addPmu_(mon, **{where: int(pmus.index[i])}, magnitude=float(mag[i]), angle=float(ang[i]), statusMagnitude=int(pmus.status_magnitude[i]),
                   statusAngle=int(pmus.status_angle[i]))
    return mon


def test_the_sets_are_the_issues():
    assert grid("case14test")[4].shape == (2 * (14 + 2 * 18), 28)
    t = grid("case30test")[0]
    assert grid("case30test")[4].shape == (2 * (30 + 2 * int((np.asarray(t["br_status"]) == 1).sum())), 60)


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_against_linprog(case):
    t, vm, va, pmus, H, _, on = grid(case)
    worst = 0.0
    for name, mag, ang in seeded_lanes(case):
        z = P.pmulav_rows(t, pmus, mag, ang)[1]
        a = P.pmulav_ipm(H, z, on, tolerance=TOL)
        b = P.pmulav_linprog(H, z, on)
        print(case, name, "iterations", a.iterations, "objective", a.objective, "minus linprog's", a.objective - b.objective)
        assert a.status == 0 and a.iterations <= 30
        worst = max(worst, abs(a.objective - b.objective))
        assert abs(a.objective - b.objective) <= OBJECTIVE_TOL, name
    print(case, "largest deviation", worst)


@pytest.mark.parametrize("case", CASES)
def test_the_known_answer_lanes_have_the_power_flow_state_as_their_optimum(case):
    """what tests/test_pmulav_gpu.py relies on: with 1, 2 and 3 gross phasor errors on the devices of GROSS_SEED, linprog's optimum is the power-flow state
    within the reference's atol and costs exactly the errors of the corrupted rows"""
    t, vm, va, pmus, H, z0, on = grid(case)
    mags, angs, devs = gross_lanes(case)
    for k in range(4):
        z = P.pmulav_rows(t, pmus, mags[k], angs[k])[1]
        lp = P.pmulav_linprog(H, z, on)
        m, a = P.polar(lp.x)
        cost = np.abs(z - z0).sum()
        print(case, k, "devices", devs[k], "magnitude", np.abs(m - vm).max(), "angle", np.abs(a - va).max(), "objective", lp.objective, "errors", cost)
        assert np.abs(m - vm).max() <= KNOWN_TOL and np.abs(a - va).max() <= KNOWN_TOL, k
        assert abs(lp.objective - cost) <= KNOWN_TOL, k
        assert set(np.flatnonzero(np.abs(z - z0) > 0) // 2) == set(devs[k])
        ref = P.pmulav_ipm(H, z, on, tolerance=TOL)
        m, a = P.polar(ref.x)
        assert ref.status == 0 and np.abs(m - vm).max() <= KNOWN_TOL and np.abs(a - va).max() <= KNOWN_TOL


@pytest.mark.parametrize("case", CASES)
def test_the_host_model_equals_the_restatement(case):
    """pattern and values of the library's coefficient matrix as scipy.sparse reads them, the rectangular means, and the status pairing"""
    import scipy.sparse as sp
    import juliagrid.jl_amd as jg
    t, vm, va, pmus, H, z, on = grid(case)
    pm = P.pmu_table(t, vm, va)
    pm.status_magnitude[3] = 0                                      # magnitude channel only
    pm.status_angle[20] = 0                                         # angle channel only
    pm.status_magnitude[21] = pm.status_angle[21] = 0
    H2, z2, on2 = P.pmulav_rows(t, pm)
    assert not on2[[6, 7, 40, 41, 42, 43]].any() and on2.sum() == on2.size - 6
    model = jg.pmuLavModel(monitoring_of(jg, t, pm))
    c = model.coefficient
    A = sp.csc_matrix((c.nzval, c.rowval - 1, c.colptr - 1), shape=H.shape)
    assert np.abs(A.toarray() - H2 * on2[:, None]).max() <= 1e-12 * np.abs(H).max()
    assert np.abs(model.mean - z2 * on2).max() <= 1e-15 and model.number == on2.size and model.inservice == int(on2.sum())
    assert not hasattr(model, "precision")                          # the reference's LAV model is unweighted
    # the full set: the pattern as scipy.sparse reads it (a lossless branch stores a zero conductance term, which scipy drops on both sides)
    c = jg.pmuLavModel(monitoring_of(jg, t, pmus)).coefficient
    A = sp.csc_matrix((c.nzval, c.rowval - 1, c.colptr - 1), shape=H.shape)
    A.eliminate_zeros()
    ref = sp.csc_matrix(H)
    ref.sort_indices()
    assert np.array_equal(A.indptr, ref.indptr) and np.array_equal(A.indices, ref.indices)
    assert np.abs(A.data - ref.data).max() <= 1e-12 * np.abs(ref.data).max()
    ptr, col, val = jg.pmuCoefficient(monitoring_of(jg, t, pmus))
    B = sp.csr_matrix((val, col - 1, ptr), shape=H.shape)
    assert np.abs(B.toarray() - H).max() <= 1e-12 * np.abs(H).max() and all(np.all(np.diff(col[ptr[i]:ptr[i + 1]]) > 0) for i in range(ptr.size - 1))


def test_a_set_without_a_pmu_is_refused():
    import juliagrid.jl_amd as jg
    mon = jg.measurement(jg.powerSystem(load_case("case14test")))
    with pytest.raises(ValueError):
        jg.pmuLavModel(mon)
    with pytest.raises(ValueError):
        jg.pmuLavStateEstimation(mon)


def test_iteration_limit_of_the_restatement():
    t, vm, va, pmus, H, _, on = grid("case14test")
    mag, ang = mixed_readings("case14test", 4)
    z = P.pmulav_rows(t, pmus, mag[3], ang[3])[1]
    a = P.pmulav_ipm(H, z, on, iteration=3)
    assert a.status == 5 and a.iterations == 3 and np.isfinite(a.x).all()


@pytest.mark.parametrize("which", ["case14", "case30"])
def test_the_coefficient_is_the_wls_models(oracle, which):
    """H of the LAV model against the coefficient of the oracle's restatement of pmuStateEstimation (oracle.OraclePmuWLS, the reference of
    tests/test_pmu_gpu.py for the WLS analysis' own coefficient) as scipy.sparse reads it: same pattern, values within 1e-12 relative.  The library's
    WLS analysis forms its values on the device, so the comparison with pmuStateEstimation(...).coefficient itself is in tests/test_pmulav_gpu.py."""
    import scipy.sparse as sp
    import juliagrid.jl_amd as jg
    from test_oracle_pmu import case30, pmu_table
    from test_oracle_se import se_case14
    from test_se_gpu import _mirror, _system_like
    t, osys, vm, va = se_case14(oracle) if which == "case14" else case30(oracle)
    tab = pmu_table(oracle, osys, vm, va)
    ref = sp.csc_matrix(oracle.OraclePmuWLS(osys, tab).coefficient)
    c = jg.pmuLavModel(_mirror(jg, _system_like(jg, t, osys), tab)).coefficient
    A = sp.csc_matrix((c.nzval, c.rowval - 1, c.colptr - 1), shape=ref.shape)
    for M in (A, ref):
        M.eliminate_zeros()
        M.sort_indices()
    assert np.array_equal(A.indptr, ref.indptr) and np.array_equal(A.indices, ref.indices)
    assert np.abs(A.data - ref.data).max() <= 1e-12 * np.abs(ref.data).max()
