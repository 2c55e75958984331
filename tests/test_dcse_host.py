"""DC state estimation, host side: the numpy / scipy restatement (tests/dcse_reference.py) is pinned to the reference's known answers
(test/stateEstimation/analysis.jl:458-575) and recorded bad-data results (test/stateEstimation/badData.jl:245-370), and the library's host model equals
the restatement's element for element.  The restatement rebuilds H and refactorises for every removed row; the library never does."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
from conftest import load_case
from test_dc_host import dc_golden


def case14_moved_slack():
    """case14test with bus 1 as type 2 and bus 3 as the slack at -0.17 (analysis.jl:466-467, badData.jl:255-256)"""
    t = load_case("case14test")
    t["bus_type"] = np.array(t["bus_type"]).copy()
    t["bus_type"][0], t["bus_type"][2] = 2, 3
    t["bus_va"] = np.asarray(t["bus_va"], dtype=np.float64).copy()
    t["bus_va"][2] = -0.17
    return t


def configurations(t, th, pw):
    """the three measurement configurations of the reference's test: bus wattmeters + PMUs, branch wattmeters + PMUs, all wattmeters"""
    n, nb = t["bus_type"].size, np.asarray(t["br_from"]).size
    fr = pw["from_"]
    bus = (np.zeros(n), np.arange(1, n + 1), pw["injection"])
    brn = (np.tile([1, 2], nb), np.repeat(np.arange(1, nb + 1), 2), np.stack([fr, -fr], axis=1).reshape(-1))
    pmu = dict(p_index=np.arange(1, n + 1), p_angle=th, p_variance=np.full(n, 1e-8))
    yield "bus", S.meters(bus[0], bus[1], bus[2], np.full(n, 1e-4), **pmu)
    yield "branch", S.meters(brn[0], brn[1], brn[2], np.full(2 * nb, 1e-4), **pmu)
    yield "all", S.meters(np.r_[bus[0], brn[0]], np.r_[bus[1], brn[1]], np.r_[bus[2], brn[2]], np.full(n + 2 * nb, 1e-4))


def monitoring_of(jg, t, ms):
    """the same set in the library's Measurement container"""
    s = jg.powerSystem(t)
    mon = jg.measurement(s)
    for k in range(ms.w_index.size):
        where = {0: "bus", 1: "from_", 2: "to"}[int(ms.w_kind[k])]
        jg.addWattmeter_(mon, **{where: int(ms.w_index[k])}, active=float(ms.w_mean[k]), variance=float(ms.w_variance[k]), status=int(ms.w_status[k]))
    for k in range(ms.p_index.size):
        jg.addPmu_(mon, **{"bus" if ms.p_bus[k] else "from_": int(ms.p_index[k])}, magnitude=1.0, angle=float(ms.p_angle[k]),
                   varianceAngle=float(ms.p_variance[k]), statusAngle=int(ms.p_status[k]))
    return mon


@pytest.mark.parametrize("case", ["case14moved", "case30test"])
def test_known_answers_of_the_reference(case):
    """exact readings of the DC power flow: the estimate equals its angles by the reference's own criterion, the powers within its atol of 1e-10"""
    if case == "case30test":
        t, g = load_case(case), dc_golden(case)
        th = g["voltage"]                                           # the golden vectors apply directly
        pw = dict(injection=g["injection"], from_=g["from"])
    else:
        t = case14_moved_slack()
        th, _ = R.solve(t)
        pw = R.power(t, th)
    for name, ms in configurations(t, th, pw):
        if case == "case30test" and name != "all":
            continue                                                # analysis.jl:533-545 runs the 30-bus grid with all wattmeters only
        est = S.solve(t, ms)
        print(case, name, float(np.abs(est - th).max()))
        assert R.isapprox(est, th), name
        got = R.power(t, est)
        for key in ("injection", "from_"):
            assert np.abs(got[key] - pw[key]).max() <= 1e-10, (name, key)


def bad_data_set(t):
    th, _ = R.solve(t)
    return th, S.full_set(t, th, 1e-2, 1e-5)                        # badData.jl:262-274: bus, from / to wattmeters at 1e-2, then bus PMUs at 1e-5


def run_rounds(t, ms, rounds):
    """the reference's loop: estimate, residual test (threshold 3), remove; returns [(row, maximum)], the last estimate"""
    removed, seen = [], []
    for _ in range(rounds):
        est = S.solve(t, ms, removed=removed)
        _, nr = S.residuals(t, ms, est, removed=removed)
        i = int(np.argmax(nr))
        seen.append((i, float(nr[i])))
        assert nr[i] > 3.0
        removed.append(i)
    return seen, S.solve(t, ms, removed=removed)


def test_recorded_bad_data_results_one_outlier():
    from scipy.stats import chi2
    t = case14_moved_slack()
    th, ms = bad_data_set(t)
    ms.w_mean[1] = 100.0                                            # "Wattmeter 2"
    est = S.solve(t, ms)
    mo = S.model(t, ms)
    assert S.objective(t, ms, est) >= chi2.ppf(0.95, mo.inservice - 14 + 1)          # chiTest detects
    seen, last = run_rounds(t, ms, 1)
    assert seen[0][0] == 1 and abs(seen[0][1] - 829.9) <= 0.1, seen
    assert R.isapprox(last, th)


def test_recorded_bad_data_results_two_outliers():
    t = case14_moved_slack()
    th, ms = bad_data_set(t)
    ms.w_mean[1] = 100.0
    ms.p_angle[9] = 10 * np.pi                                      # "PMU 10"
    row_pmu10 = S.model(t, ms).index[10] - 1
    seen, last = run_rounds(t, ms, 2)
    assert seen[0][0] == row_pmu10 and abs(seen[0][1] - 5186.3) <= 0.1, seen
    assert seen[1][0] == 1 and abs(seen[1][1] - 829.9) <= 0.1, seen
    assert R.isapprox(last, th)


def test_a_removal_of_the_restatement_rebuilds_the_gain():
    """the check must not share the library's shortcut: the reduced gain differs from the full one and is factorised anew"""
    t = load_case("case14")
    th, ms = bad_data_set(t)
    G0, G1 = S.gain(t, ms), S.gain(t, ms, removed=[5])
    assert abs(G0 - G1).max() > 1.0
    ms.w_mean[5] += 1.0
    a, b = S.solve(t, ms), S.solve(t, ms, removed=[5])
    assert np.abs(a - th).max() > 1e-4 and R.isapprox(b, th)
    src = open(S.__file__).read().split('"""', 2)[2]
    assert "Omega" not in src and "omega" not in src


@pytest.mark.parametrize("case", ["case14", "case118", "case300", "case_ACTIVSg10k"])
def test_the_host_model_equals_the_restatement_element_for_element(case):
    import juliagrid.jl_amd as jg
    t = load_case(case)
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    ms.w_status[[3, 11]] = 0                                        # out-of-service rows keep their pattern as stored zeros
    ms.p_status[2] = 0
    ms.w_variance[7] = 3e-3
    mo = S.model(t, ms)
    se = jg.dcstateestimation.dcWlsModel(monitoring_of(jg, t, ms))
    H = se.coefficient
    assert np.array_equal(H.colptr, mo.colptr) and np.array_equal(H.rowval, mo.rowval)
    assert np.array_equal(H.nzval, mo.nzval)                        # same values, stored zeros included
    assert np.array_equal(se.mean, mo.mean) and np.array_equal(se.precision, mo.precision)
    assert se.index == mo.index and se.number == mo.number and se.inservice == mo.inservice
    assert np.count_nonzero(H.nzval == 0.0) >= 5


def test_branch_pmus_are_skipped_and_index_maps_pmu_to_row():
    import juliagrid.jl_amd as jg
    t = load_case("case14")
    th, _ = R.solve(t)
    ms = S.meters([0, 1], [1, 2], [0.1, 0.2], [1e-2, 1e-2], None, [4, 3, 9], [True, False, True], [th[3], 0.0, th[8]], [1e-5] * 3)
    mo = S.model(t, ms)
    se = jg.dcstateestimation.dcWlsModel(monitoring_of(jg, t, ms))
    assert mo.index == {1: 3, 3: 4} == se.index and se.number == 4


def test_arguments_without_a_meaning_for_a_dc_analysis_are_refused():
    """checked before anything touches the device"""
    import juliagrid.jl_amd as jg
    t = load_case("case14")
    th, ms = bad_data_set(t)
    mon = monitoring_of(jg, t, ms)
    for kw in (dict(iteration=5), dict(tolerance=1e-6), dict(start=None)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            jg.dcStateEstimation(mon, **kw)
    with pytest.raises(TypeError):
        jg.dcStateEstimation(mon, method=float)
