"""DC state estimation and its batched bad-data removal on the device against the numpy / scipy restatement (tests/dcse_reference.py), which REBUILDS H
and refactorises the gain for every set of removed rows -- the library never does (one shared factor + a low-rank compensation per lane,
csrc/jg_dcse.hpp).

Tolerances.  Lane-by-lane angles of the full set: max |got - ref| <= 1e-9 * max(1, max |ref|), the project's linear-step bound (tests/test_dc_gpu.py).
Removal lanes: REMOVAL_TOL below, see test_removal_rounds_on_the_10k_bus_grid.  Normalised residuals and objectives compare relatively by the same rule.
On the 10k-bus grid the restatement normalises every row of the FULL set (a dense inverse of the gain, once), so the first round compares over all
45 412 rows.  The rows of a REDUCED set are normalised on candidate rows only (a solve per row and lane is minutes there): the planted rows and the 64
rows whose residual in the reduced set is largest over the full set's variance.  A removal lowers a row's variance only where the row is coupled to the
removed ones; the test asserts that the 64th candidate is below half the maximum, so a row outside them would have to lose three quarters of its variance."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
from conftest import load_case
from test_dcse_host import bad_data_set, case14_moved_slack, configurations, monitoring_of

pytestmark = pytest.mark.gpu

TOL = 1e-9
# Largest deviation of a removal lane's angles from the rebuild-and-refactorise restatement, measured on one MI355X on the 10k-bus grid (64 lanes, one
# and two removed rows, scaled as above): 1.122e-10.  The bound is that x 10 because the restatement's own splu ordering moves it by about as much.  The
# lanes WITHOUT a removed row deviate by 1.12e-10 .. 1.67e-10 there (normal equations on a gain of 10 000 states): the compensation adds nothing visible.
MEASURED_REMOVAL = 1.122e-10
REMOVAL_TOL = 10 * MEASURED_REMOVAL
TAGS = ["LU", "KLU", "QR", "LDLt", "LL", "Orthogonal", "PetersWilkinson"]


def at_zero(t):
    """the table with the slack's angle at 0.  The reference's residualTest! multiplies the coefficient without its slack column by voltage.angle, the
    slack's angle included (badData.jl:66-73; its recorded 5186.3 comes out only so): with a slack at 0.52 rad (case118) or -0.86 rad (10k-bus grid) every
    PMU row then carries that angle as a residual, 165 and 273 normalised units at a variance of 1e-5, and names one healthy PMU after the other.  The
    removal tests plant their errors on grids where the test can see them; the noise-only batches keep the angle and compare the same numbers"""
    t = dict(t)
    t["bus_va"] = np.asarray(t["bus_va"], dtype=np.float64).copy()
    t["bus_va"][R.slack_of(t)] = 0.0
    return t


def full(jg, case, batch, method="LU", t=None):
    t = load_case(case) if t is None else t
    th, ms = bad_data_set(t)
    an = jg.dcStateEstimation(monitoring_of(jg, t, ms), getattr(jg, method), batch=batch)
    return t, th, ms, an


@pytest.mark.parametrize("tag", TAGS)
def test_known_answers_on_the_device(jg, tag):
    """analysis.jl:458-575: exact readings of the DC power flow, three configurations on the 14-bus grid with the slack moved to bus 3 at -0.17, all
    wattmeters on the 30-bus grid; estimate = power-flow angles by the reference's criterion, powers within 1e-10"""
    from test_dc_host import dc_golden
    for case in ("case14moved", "case30test"):
        if case == "case30test":
            t, g = load_case(case), dc_golden(case)
            th, pw = g["voltage"], dict(injection=g["injection"], from_=g["from"], supply=g["supply"], generator=g["generator"])
        else:
            t = case14_moved_slack()
            th, _ = R.solve(t)
            pw = R.power(t, th)
        for name, ms in configurations(t, th, pw):
            if case == "case30test" and name != "all":
                continue
            an = jg.dcStateEstimation(monitoring_of(jg, t, ms), getattr(jg, tag))
            jg.stateEstimation_(an, power=True)
            print(case, name, tag, float(np.abs(an.voltage.angle - th).max()))
            assert an.status == 0 and R.isapprox(an.voltage.angle, th), (case, name)
            for key in ("injection", "supply", "generator", "from_"):
                assert np.abs(getattr(an.power, key).active - pw[key]).max() <= 1e-10, (case, name, key)
            assert np.array_equal(an.power.to.active, -an.power.from_.active)
            an.close()


@pytest.mark.parametrize("tag", TAGS)
def test_recorded_bad_data_results_on_the_device(jg, tag):
    """badData.jl:245-370, batch 1 (the reference's route: status 0, re-assembly, refactorisation)"""
    t = case14_moved_slack()
    th, ms = bad_data_set(t)
    mon = monitoring_of(jg, t, ms)
    jg.updateWattmeter_(mon, 2, active=100.0)
    an = jg.dcStateEstimation(mon, getattr(jg, tag))
    jg.stateEstimation_(an)
    assert jg.chiTest(an).detect
    out = jg.residualTest_(an, threshold=3.0)
    print(tag, out)
    assert out.detect and out.label == "Wattmeter 2" and abs(out.maxNormalizedResidual - 829.9) <= 0.1
    assert mon.wattmeter.active.status[1] == 0 and an.method.mean[1] == 0.0
    jg.stateEstimation_(an)
    assert R.isapprox(an.voltage.angle, th) and an.dims()["refactorizations"] == 1
    an.close()
    jg.updateWattmeter_(mon, 2, status=1)
    jg.updatePmu_(mon, 10, angle=10 * np.pi)
    an = jg.dcStateEstimation(mon, getattr(jg, tag))
    jg.stateEstimation_(an)
    out = jg.residualTest_(an, threshold=3.0)
    assert out.label == "PMU 10" and abs(out.maxNormalizedResidual - 5186.3) <= 0.1, out
    jg.stateEstimation_(an)
    out = jg.residualTest_(an, threshold=3.0)
    assert out.label == "Wattmeter 2" and abs(out.maxNormalizedResidual - 829.9) <= 0.1, out
    jg.stateEstimation_(an)
    assert R.isapprox(an.voltage.angle, th)
    an.close()


def check_full_set_lanes(jg, t, ms, an, variances, lanes=None):
    """angles, objective, arg-max row and normalised maximum of the lanes of a solved batch without removed rows"""
    rb = S.Rebuilt(t, ms)
    out = jg.residualTest_(an, threshold=1e300)                      # nothing is removed
    th = np.atleast_2d(an.voltage.angle)
    obj = np.atleast_1d(an.objective)
    wa = wo = wn = 0.0
    for s in (range(an.batch) if lanes is None else lanes):
        z = an.readings[s]
        ref = rb.solve(z)
        a = R.worst(th[s], ref)
        o = abs(obj[s] - rb.objective(z, ref)) / max(1.0, rb.objective(z, ref))
        nr = rb.normalized(z, ref, variances)
        i = int(np.argmax(nr))
        top = np.sort(nr)[-2:]
        assert top[1] > top[0] * (1 + 1e-6), (s, top)                # no tie in the restatement
        idx, mx = (out.index, out.maxNormalizedResidual) if an.batch == 1 else (out.index[s], out.maxNormalizedResidual[s])
        assert a <= TOL and o <= TOL, (s, a, o)
        assert int(idx) == i + 1, (s, int(idx), i + 1, top)
        wn = max(wn, abs(mx - nr[i]) / max(1.0, nr[i]))
        assert wn <= TOL, (s, mx, nr[i])
        wa, wo = max(wa, a), max(wo, o)
    print("worst angle", wa, "objective", wo, "normalised maximum", wn)
    return rb


@pytest.mark.parametrize("case", ["case118", "case_ACTIVSg10k"])
def test_a_batch_of_512_noisy_realisations(jg, case):
    t, th, ms, an = full(jg, case, 512)
    jg.setNoise_(an, np.random.default_rng(20261016))
    jg.solveSE_(an)
    assert np.all(an.status == 0)
    print(case, an.dims())
    variances = S.Rebuilt(t, ms).variances(dense=case != "case118")
    check_full_set_lanes(jg, t, ms, an, variances)
    an.close()


def plantable_rows(t, ms, variances, w):
    """bus wattmeters and bus PMUs (a from / to pair of one branch has the same row up to its sign, so an error on one of the two cannot be told apart)
    whose residual keeps at least 5 % of the reading's variance"""
    n = t["bus_type"].size
    m = w.size
    rows = np.r_[np.arange(n), np.arange(m - n, m)]
    return rows[(w * variances)[rows] >= 0.05]


def plant(t, ms, base, variances, readings, rounds, seed=7):
    """every lane gets gross errors of its own on rows of its own, sized by the share of the variance the residual keeps so that they show as about 60
    and (second row, two rounds) 30 normalised units: 60 to 270 sigma and 30 to 135 sigma"""
    rng = np.random.default_rng(seed)
    pool = plantable_rows(t, ms, variances, base.w)
    sigma = 1.0 / np.sqrt(base.w)
    planted = np.stack([rng.choice(pool, size=2, replace=False) for _ in range(readings.shape[0])])[:, :rounds]
    z = readings.copy()
    for s in range(z.shape[0]):
        share = np.sqrt((base.w * variances)[planted[s]])
        z[s, planted[s, 0]] += 60.0 * sigma[planted[s, 0]] / share[0]
        if rounds > 1:
            z[s, planted[s, 1]] -= 30.0 * sigma[planted[s, 1]] / share[1]
    return z, planted


def expected_rounds(t, ms, base, z, planted, candidates, variances):
    """what the reference's loop (estimate, residual test, remove, again) gives for ONE lane by rebuilding and refactorising: per round the estimate, the
    arg-max row and the maximum; then the last estimate.  Asserted on the restatement: the two largest normalised residuals differ by more than 1 % (no
    tie can hide a wrong answer), the arg-max is one of the planted rows, and no row outside the candidates can hold the maximum"""
    rem, seen = [], []
    for _ in range(len(planted)):
        rb = base if not rem else S.Rebuilt(t, ms, rem)
        assert not rb.singular
        ref = rb.solve(z)
        if not rem:
            nr = rb.normalized(z, ref, variances)                    # the full set: every row
        else:
            by_full = rb.normalized(z, ref, variances)               # the reduced set's residuals over the FULL set's variances: picks the candidates
            rows = None if candidates is None else np.r_[np.argsort(by_full)[-candidates:], planted]
            nr = rb.normalized(z, ref, rb.variances(rows))
        i = int(np.nanargmax(nr))
        top = np.sort(nr[~np.isnan(nr)])[-2:]
        assert top[1] > 1.01 * top[0], (rem, top)
        assert i in [int(x) for x in planted] and i not in rem and top[1] > 20.0, (i, planted, top)
        if candidates is not None and rem:
            assert np.sort(by_full)[-candidates] < top[1] / 2, (rem, np.sort(by_full)[-candidates], top[1])
        seen.append((ref, i, float(nr[i])))
        rem.append(i)
    return seen, S.Rebuilt(t, ms, rem).solve(z), rem


def removal_rounds(jg, case, batch, lanes, rounds, candidates=None):
    """after each round the removed rows equal the planted ones (in the restatement's order) and the angles equal the rebuild-and-refactorise
    restatement; returns the worst scaled deviation of the angles of lanes with removed rows"""
    t, th, ms, an = full(jg, case, batch, t=at_zero(load_case(case)))
    jg.setNoise_(an, np.random.default_rng(7))
    base = S.Rebuilt(t, ms)
    variances = base.variances(dense=candidates is not None)
    z, planted = plant(t, ms, base, variances, an.readings, rounds)
    jg.setReadings_(an, z)
    want = {s: expected_rounds(t, ms, base, z[s], planted[s], candidates, variances) for s in lanes}
    worst = 0.0
    for rnd in range(rounds):
        jg.solveSE_(an)
        out = jg.residualTest_(an, threshold=3.0, labels=True)
        gone = jg.removed(an)
        assert np.all(gone.status == 0)
        for s in lanes:
            ref, i, mx = want[s][0][rnd]
            d = R.worst(an.voltage.angle[s], ref)
            print("round", rnd, "lane", s, "deviation", d)
            worst = max(worst, d) if rnd else worst
            assert d <= (REMOVAL_TOL if rnd else TOL), (rnd, s, d)
            assert int(out.index[s]) == i + 1 and out.detect[s], (rnd, s, i, planted[s], int(out.index[s]))
            assert abs(out.maxNormalizedResidual[s] - mx) <= (REMOVAL_TOL if rnd else TOL) * max(1.0, mx), (rnd, s, out.maxNormalizedResidual[s], mx)
            assert [int(x) - 1 for x in gone.rows[s]] == want[s][2][:rnd + 1], (rnd, s, gone.rows[s], want[s][2])
    jg.solveSE_(an)
    assert np.all(an.status == 0)
    for s in lanes:
        d = R.worst(an.voltage.angle[s], want[s][1])
        print("after", rounds, "rounds, lane", s, "deviation", d)
        worst = max(worst, d)
        assert d <= REMOVAL_TOL, (s, d)
    assert an.dims()["refactorizations"] == 0                        # the factor was never redone
    print(case, "rounds", rounds, "lanes", len(lanes), "worst removal-lane deviation", worst)
    an.close()
    return worst


@pytest.mark.parametrize("rounds", [1, 2])
def test_removal_rounds_on_case118(jg, rounds):
    removal_rounds(jg, "case118", 512, range(512), rounds)


@pytest.mark.parametrize("rounds", [1, 2])
def test_removal_rounds_on_the_10k_bus_grid(jg, rounds):
    """64 lanes, 8 of every lane group of the 512.  Largest deviation of a removal lane's angles from the restatement measured here on one MI355X:
    1.122e-10 after one round and after two (MEASURED_REMOVAL); the bound REMOVAL_TOL is that x 10 = 1.122e-9.  On case118 the same figure is 4.9e-15."""
    lanes = [g * 64 + k for g in range(8) for k in (0, 9, 18, 27, 36, 45, 54, 63)]
    removal_rounds(jg, "case_ACTIVSg10k", 512, lanes, rounds, candidates=64)


def test_a_planted_critical_measurement(jg):
    """a leaf bus seen by exactly one meter: without that meter the grid is unobservable.  Its residual is 0 up to rounding, so no test ever names it; the
    lane drops it through removeMeasurement_.  That lane gets a non-zero status and NaN angles, the other lanes stay bitwise what they were"""
    t = load_case("case14")
    th, _ = R.solve(t)
    f, to = np.asarray(t["br_from"]).astype(int), np.asarray(t["br_to"]).astype(int)
    n = t["bus_type"].size
    deg = np.bincount(np.r_[f, to], minlength=n + 1)
    leaf = int(np.flatnonzero(deg[1:] == 1)[0]) + 1
    k = int(np.flatnonzero((f == leaf) | (to == leaf))[0])
    neighbour = int(to[k] if f[k] == leaf else f[k])
    pw = R.power(t, th)
    buses = [b for b in range(1, n + 1) if b not in (leaf, neighbour)]      # injections that do not see the leaf
    seen = [b for b in range(1, n + 1) if b != leaf]                         # PMUs everywhere but at the leaf
    ms = S.meters([1] + [0] * len(buses), [k + 1] + buses, [pw["from_"][k]] + [pw["injection"][b - 1] for b in buses], [1e-2] * (1 + len(buses)), None,
                  seen, None, [th[b - 1] for b in seen], [1e-5] * len(seen))
    assert S.Rebuilt(t, ms, [0]).singular and not S.Rebuilt(t, ms).singular and not S.Rebuilt(t, ms, [2]).singular
    an = jg.dcStateEstimation(monitoring_of(jg, t, ms), batch=70)
    jg.setNoise_(an, np.random.default_rng(3))
    jg.solveSE_(an)
    before = an.voltage.angle.copy()
    rows = np.zeros(70, dtype=np.int32)
    rows[5], rows[7] = 1, 3                                                   # lane 5: the critical meter; lane 7: a redundant one
    jg.removeMeasurement_(an, rows)
    jg.solveSE_(an)
    assert an.status[5] == 1 and np.all(np.isnan(an.voltage.angle[5])) and np.all(np.delete(an.status, 5) == 0)
    keep = np.delete(np.arange(70), [5, 7])
    assert np.array_equal(an.voltage.angle[keep], before[keep])
    assert R.worst(an.voltage.angle[7], S.Rebuilt(t, ms, [2]).solve(an.readings[7])) <= REMOVAL_TOL
    gone = jg.removed(an)
    assert list(gone.rows[7]) == [3] and list(gone.rows[5]) == [] and gone.status[5] == 1
    an.close()


def test_a_fifth_removed_row_gives_status_2(jg):
    """a lane keeps at most dims()["maxRemoved"] rows: four are compensated (against the rebuild), the fifth gives status 2 and NaN angles; the others stay"""
    t, th, ms, an = full(jg, "case118", 3, t=at_zero(load_case("case118")))
    assert an.dims()["maxRemoved"] == 4
    jg.setNoise_(an, np.random.default_rng(2))
    jg.solveSE_(an)
    before = an.voltage.angle.copy()
    base = S.Rebuilt(t, ms)
    pool = plantable_rows(t, ms, base.variances(), base.w)[::17][:5]
    for k, row in enumerate(pool):
        jg.removeMeasurement_(an, np.array([0, row + 1, 0], dtype=np.int32))
        jg.solveSE_(an)
        assert np.array_equal(an.voltage.angle[[0, 2]], before[[0, 2]])
        if k < 4:
            ref = S.Rebuilt(t, ms, [int(r) for r in pool[:k + 1]]).solve(an.readings[1])
            assert an.status[1] == 0 and R.worst(an.voltage.angle[1], ref) <= REMOVAL_TOL, k
    assert an.status[1] == 2 and np.all(np.isnan(an.voltage.angle[1])) and an.status[0] == 0 and an.status[2] == 0
    assert [int(x) - 1 for x in jg.removed(an).rows[1]] == [int(r) for r in pool[:4]]
    an.close()


def test_updates_against_a_freshly_built_analysis(jg):
    """a reading: no refactorisation; a status or a variance: one.  Results equal a freshly built analysis bitwise"""
    t, th, ms, an = full(jg, "case118", 3)
    jg.solveSE_(an)
    jg.updateWattmeter_(an, 7, active=0.3)
    jg.updatePmu_(an, 4, angle=0.01)
    jg.solveSE_(an)
    assert an.dims()["refactorizations"] == 0
    fresh = jg.dcStateEstimation(an.monitoring, batch=3)
    jg.solveSE_(fresh)
    assert np.array_equal(fresh.voltage.angle, an.voltage.angle) and np.array_equal(fresh.objective, an.objective)
    fresh.close()
    jg.updateWattmeter_(an, 9, status=0)
    jg.solveSE_(an)
    assert an.dims()["refactorizations"] == 1
    jg.updatePmu_(an, 11, varianceAngle=1e-4)
    jg.solveSE_(an)
    assert an.dims()["refactorizations"] == 2
    fresh = jg.dcStateEstimation(an.monitoring, batch=3)
    jg.solveSE_(fresh)
    assert np.array_equal(fresh.method.coefficient.nzval, an.method.coefficient.nzval) and np.array_equal(fresh.method.mean, an.method.mean)
    assert np.array_equal(fresh.voltage.angle, an.voltage.angle) and np.array_equal(fresh.objective, an.objective)
    a, b = jg.residualTest_(an, threshold=1e300), jg.residualTest_(fresh, threshold=1e300)
    assert np.array_equal(a.index, b.index) and np.array_equal(a.maxNormalizedResidual, b.maxNormalizedResidual)
    ms.w_status[8], ms.p_variance[10] = 0, 1e-4
    ms.w_mean[6], ms.p_angle[3] = 0.3, 0.01
    assert R.worst(an.voltage.angle[0], S.solve(t, ms)) <= TOL
    fresh.close()
    an.close()


def test_batch_sizes_that_are_not_multiples_of_64(jg):
    t = at_zero(load_case("case118"))
    th, ms = bad_data_set(t)
    mon = monitoring_of(jg, t, ms)
    big = jg.dcStateEstimation(mon, batch=512)
    jg.setNoise_(big, np.random.default_rng(11))
    z = big.readings.copy()
    base = S.Rebuilt(t, ms)
    pool = plantable_rows(t, ms, base.variances(), base.w)
    z[np.arange(512), pool[np.arange(512) % pool.size]] += 2.0
    jg.setReadings_(big, z)
    res = {}
    for batch in (1, 3, 70, 512):
        an = jg.dcStateEstimation(mon, batch=batch)
        jg.setReadings_(an, z[:batch])
        jg.solveSE_(an)
        nr = np.atleast_2d(jg.normalizedResidual(an))
        if batch > 1:
            jg.residualTest_(an, threshold=3.0)
            jg.solveSE_(an)
        res[batch] = (np.atleast_2d(an.voltage.angle).copy(), np.atleast_1d(an.objective).copy(), nr)
        for s in range(min(batch, 3)):
            rb = S.Rebuilt(t, ms, [int(pool[s % pool.size])] if batch > 1 else [])
            assert R.worst(res[batch][0][s], rb.solve(z[s])) <= (REMOVAL_TOL if batch > 1 else TOL), (batch, s)
        an.close()
    for k in range(3):
        assert np.array_equal(res[70][k], res[512][k][:70]), k       # a lane's result does not depend on the batch it runs in
        assert np.array_equal(res[3][k], res[512][k][:3]), k
    assert np.array_equal(res[1][2], res[512][2][:1])
    big.close()


@pytest.mark.parametrize("tag", ["Orthogonal", "PetersWilkinson"])
def test_the_corrected_methods_against_lu_and_the_restatement(jg, tag):
    t, th, ms, lu = full(jg, "case300", 70)
    jg.setNoise_(lu, np.random.default_rng(5))
    an = jg.dcStateEstimation(lu.monitoring, getattr(jg, tag), batch=70)
    jg.setReadings_(an, lu.readings)
    jg.solveSE_(lu)
    jg.solveSE_(an)
    rb = S.Rebuilt(t, ms)
    for s in range(70):
        ref = rb.solve(lu.readings[s])
        assert R.worst(an.voltage.angle[s], ref) <= TOL and R.worst(lu.voltage.angle[s], ref) <= TOL and R.worst(an.voltage.angle[s], lu.voltage.angle[s]) <= TOL
    an.close()
    lu.close()


def test_an_unobservable_set_raises(jg):
    t = load_case("case14")
    th, _ = R.solve(t)
    ms = S.meters([0], [1], [0.0], [1e-2], None, [1, 2], None, th[:2], [1e-5, 1e-5])
    with pytest.raises(Exception, match="observable"):
        jg.dcStateEstimation(monitoring_of(jg, t, ms))
    with pytest.raises(ValueError, match="drawNoise_"):
        t, th, ms, an = full(jg, "case14", 2)
        jg.drawNoise_(an, 1)
