"""Pins the oracle's restatement of the reference's two non-normal Gauss-Newton solvers -- increment! for
GaussNewton{Orthogonal} (acStateEstimation.jl:906-932) and GaussNewton{PetersWilkinson} (:934-971) -- on the reference's own
acceptance rule for them (test/stateEstimation/analysis.jl:219-232, 284-297): with noise-free measurements of all
families the estimate equals the power-flow state (IEEE 14: atol 1e-10; IEEE 30 with tolerance 1e-10: atol 1e-8), and
on the fact that all three increments solve the same least-squares problem.

The same on the 118- and 300-bus grids (slack = bus 69 / 257; 2 450 / 5 610 rows of all five families, ammeters and branch PMUs only where the current
is at least 1e-6), where the dense restatement is the reference of tests/test_methods_grids_gpu.py: the gap between its two solvers is measured and
printed here (methods_reference.DEV_REF records it), and every condition that file puts on the reference alone -- long contribution lists, lanes that
stop at different iterations clear of the tolerance, the planted gross error -- is asserted here first, without a GPU."""
import numpy as np
import pytest

import methods_reference as R
from conftest import load_case
from test_oracle_se import se_case14


def all_families(oracle, s, vm, va):
    tab = oracle.MeterTable()
    for fam in ("voltmeter", "ammeter", "wattmeter", "varmeter", "pmu"):
        oracle.add_from_power_flow(tab, s, vm, va, fam)
    return tab


def case30(oracle):
    t = load_case("case30test")
    s = oracle.OracleSystem(t)
    pf = oracle.OracleNR(s)
    assert pf.power_flow() == 0
    vm, va = pf.voltage()
    s.type = pf.type.copy(); s.slack = pf.slack
    return t, s, vm, va


@pytest.mark.parametrize("method", ["increment_orthogonal", "increment_peters_wilkinson"])
def test_ieee14_known_answer(oracle, method):
    t, s, vm, va = se_case14(oracle)
    gn = oracle.OracleGN(s, all_families(oracle, s, vm, va))
    ok, it = gn.state_estimation_with(getattr(gn, method))             # defaults: 40 iterations, 1e-8 (analysis.jl:221, 229)
    v = gn.vectors()
    assert ok and it <= 10
    assert np.abs(v["magnitude"] - vm).max() <= 1e-10
    assert np.abs(v["angle"] - va).max() <= 1e-10


@pytest.mark.parametrize("method", ["increment_orthogonal", "increment_peters_wilkinson"])
def test_ieee30_known_answer(oracle, method):
    t, s, vm, va = case30(oracle)
    gn = oracle.OracleGN(s, all_families(oracle, s, vm, va))
    ok, it = gn.state_estimation_with(getattr(gn, method), tolerance=1e-10)     # analysis.jl:286, 294
    v = gn.vectors()
    assert ok
    assert np.abs(v["magnitude"] - vm).max() <= 1e-8
    assert np.abs(v["angle"] - va).max() <= 1e-8


def test_three_increments_solve_the_same_least_squares_problem(oracle):
    t, s, vm, va = se_case14(oracle)
    gn = oracle.OracleGN(s, all_families(oracle, s, vm, va))
    gn.increment()
    normal = gn.vectors()["increment"].copy()
    orth = gn.increment_orthogonal()
    pw = gn.increment_peters_wilkinson()
    scale = np.abs(orth).max()
    assert np.abs(orth - pw).max() <= 1e-9 * scale
    assert np.abs(orth - normal).max() <= 1e-7 * scale
    assert orth[s.slack - 1] == 0.0 and pw[s.slack - 1] == 0.0


GRIDS = ["case118", "case300"]


@pytest.mark.parametrize("case", GRIDS)
def test_grids_have_an_inner_slack_and_long_contribution_lists(oracle, case):
    """what IEEE 14 / 30 do not have: a slack that is not bus 1, and bus rows whose right-hand-side list runs over 5 and more records of 4 contributions"""
    t, s, vm, va = R.grid(oracle, case)
    assert s.slack != 1
    tab = R.all_families(oracle, s, vm, va)
    assert not any((r[0] == 2 or (r[0] == 5 and r[1] != 0)) and r[3] < R.MIN_CURRENT for r in tab.rows)
    gn = oracle.OracleGN(s, tab)
    c = R.contributions_per_bus(gn.hcolptr, gn.hrowval, s.n)
    print(f"\n[{case}] slack {s.slack}, {gn.m} rows, contributions per bus row {c.min()} ... {c.max()}")
    assert c.max() > 16


@pytest.mark.parametrize("case", GRIDS)
def test_dense_increments_agree_on_the_grids(oracle, case):
    """dev_ref(case) = max|orth - pw| / max|orth| at the start point: measured here, recorded in methods_reference.DEV_REF (measured: 2.48e-15 on the
    118-bus grid, 4.23e-15 on the 300-bus grid).  The recorded value may not understate what this machine measures by more than 3 bits."""
    t, s, vm, va = R.grid(oracle, case)
    gn = oracle.OracleGN(s, R.all_families(oracle, s, vm, va))
    gn.increment()
    normal = gn.vectors()["increment"].copy()
    orth = gn.increment_orthogonal()
    pw = gn.increment_peters_wilkinson()
    scale = np.abs(orth).max()
    dev = np.abs(orth - pw).max() / scale
    print(f"\n[{case}] dev_ref = {dev:.3e} (recorded {R.DEV_REF[case]:.1e}); normal equations vs QR {np.abs(orth - normal).max() / scale:.2e}")
    assert dev <= 1e-9 and dev <= 8.0 * R.DEV_REF[case]
    assert np.abs(orth - normal).max() <= 1e-7 * scale
    assert orth[s.slack - 1] == 0.0 and pw[s.slack - 1] == 0.0


@pytest.mark.parametrize("method", ["increment_orthogonal", "increment_peters_wilkinson"])
@pytest.mark.parametrize("case", GRIDS)
def test_grids_known_answer(oracle, case, method):
    """the IEEE 30 rule of the reference (tolerance 1e-10: atol 1e-8) from the case's stored start point"""
    t, s, vm, va = R.grid(oracle, case)
    gn = oracle.OracleGN(s, R.all_families(oracle, s, vm, va))
    ok, it = gn.state_estimation_with(getattr(gn, method), tolerance=1e-10)
    v = gn.vectors()
    assert ok and it <= 10
    assert np.abs(v["magnitude"] - vm).max() <= 1e-8
    assert np.abs(v["angle"] - va).max() <= 1e-8


def test_spread_lanes_stop_clear_of_the_tolerance(oracle):
    """the reference side of test_methods_grids_gpu.test_lanes_and_groups_that_stop_at_different_iterations: under the committed seed the checked lanes
    take two distinct iteration counts, and every one of them stops a factor 2 clear of the tolerance on both sides (last check <= 5e-9, the check before
    >= 2e-8), so no lane's count hangs on the last bits of an increment"""
    for repeats, checked in R.SPREAD.values():
        src = dict(repeats)
        answers = {b: R.lane_answer(oracle, "case118", src.get(b, b), R.SPREAD_SEED, R.SPREAD_STEP) for b in checked}
        print("\n", {b: (a.iteration, f"{a.checks[-2]:.1e}", f"{a.checks[-1]:.1e}") for b, a in answers.items()})
        assert len({a.iteration for a in answers.values()}) >= 2
        assert all(R.margins_hold(a) for a in answers.values())
        assert answers[64].iteration != max(answers[b].iteration for b in checked if b < 64)


def test_lane_rule_is_seeded_and_independent_of_the_batch(oracle):
    t, s, vm, va = R.grid(oracle, "case118")
    tab = R.all_families(oracle, s, vm, va)
    a1, a2 = R.lane_readings(tab, list(range(66)), repeats=((64, 1),))
    b1, b2 = R.lane_readings(tab, [1, 5, 65])
    rows = R.device_rows(tab)
    assert np.array_equal(a1[[1, 5, 65]], b1) and np.array_equal(a2[[1, 5, 65]], b2)
    assert np.array_equal(a1[64], a1[1]) and np.array_equal(a2[64], a2[1]) and not np.array_equal(a1[1], a1[2])
    assert np.array_equal(a1[0], [r[3] for r in rows]) and np.array_equal(a1[5], a1[0]) and np.array_equal(a2[65], [r[6] for r in rows])
    pmu = np.array([r[0] == 5 for r in rows])
    assert np.array_equal(a2[3, ~pmu], np.zeros((~pmu).sum()))                  # the second reading belongs to the PMUs alone
    sd = (a1[4] - a1[0]) / np.sqrt([r[4] for r in rows])
    assert 0.9 < sd.std() / (4 * R.NOISE_STEP) < 1.1                            # noise scale rises with b % 5


def test_masked_table_keeps_the_edge_rows_and_returns_the_power_flow(oracle):
    t, s, vm, va = R.grid(oracle, "case118")
    gn = oracle.OracleGN(s, R.masked_table(oracle, s, vm, va))
    assert list(gn.type[R.GN_ROWS - 2:R.GN_ROWS + 2] != 0) == [False, True, True, False]
    assert list(gn.type[-4:] != 0) == [False, False, True, True] and 0.1 < np.mean(gn.type == 0) < 0.2
    ok, it = gn.state_estimation_with(gn.increment_orthogonal, tolerance=1e-10)
    v = gn.vectors()
    assert ok and np.abs(v["magnitude"] - vm).max() <= 1e-8 and np.abs(v["angle"] - va).max() <= 1e-8


def test_planted_error_is_the_largest_residual_and_its_removal_returns_the_power_flow(oracle):
    """the reference side of test_methods_grids_gpu.test_a_gross_error_is_removed_under_the_tag; prints the deviation the oracle's own Orthogonal
    re-estimate (default loop: 40 iterations, 1e-8) leaves on the table without the flagged row -- 2.86e-9 measured -- which that test takes 10 x of"""
    t, s, vm, va = R.grid(oracle, "case118")
    tab, row = R.bad_table(oracle, s, vm, va)
    gn = oracle.OracleGN(s, tab)
    assert gn.state_estimation(40, 1e-8) == 0
    gn.increment()
    nr = oracle.gn_normalized_residuals(gn)
    assert int(np.argmax(nr)) == row and gn.type[row] in (7, 8) and nr.max() > 100 * np.sort(nr)[-2]
    dev = R.reestimate_deviation(oracle)
    print(f"\nlargest normalised residual {nr.max():.3f} at row {row}; re-estimate without it: {dev:.3e} from the power flow")
    assert dev <= 1e-8
