"""The critical-measurement and critical-pair screen (dcCriticalScreen, csrc/jg_dcse_critical.hip) on the device against the dense restatement
(tests/dcse_critical_reference.py: one dense inverse of the gain, all of Omega at once -- never the device's blocks of 512 columns on the sparse factor).

The sets are the smallest at which the kernel can go wrong (tests/test_dcse_critical_host.py pins them): 58 rows on the 14-bus grid (one partial wave),
598 rows on case118 (two blocks of columns, the second partial, no multiple of 32; one critical pair across the blocks, one inside a group of 64 columns)
and 523 rows of a seeded grid thinned at random.  What is critical is compared for EQUALITY: the host test shows three decades on either side of the
threshold.  gamma, partnerCorrelation and variance: |got - ref| <= 1e-9 * max(1, |ref|), the bound of tests/test_dcse_gpu.py for the diagonal path."""
import numpy as np
import pytest

import dc_reference as R
import dcse_critical_reference as C
from test_dcse_critical_host import SETS, reference
from test_dcse_host import monitoring_of

pytestmark = pytest.mark.gpu

TOL = 1e-9
_GOT = {}


def scaled(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0


def screened(jg, name, correlation=None):
    """the device's screen of a set, run once per correlation and shared"""
    if (name, correlation) not in _GOT:
        t, ms, _ = reference(name, correlation)
        an = jg.dcStateEstimation(monitoring_of(jg, t, ms), batch=3)
        _GOT[name, correlation] = jg.dcCriticalScreen(an, correlation=correlation)
        an.close()
    return _GOT[name, correlation]


@pytest.mark.parametrize("name", list(SETS))
def test_singles_pairs_totals_and_partners_against_the_restatement(jg, name):
    ref = reference(name)[2]
    got = screened(jg, name)
    assert np.array_equal(got.critical, ref.critical + 1)
    assert (got.totalSingles, got.totalPairs, got.totalCorrelated) == ref.totals and got.totalCorrelated == 0
    assert np.array_equal(got.pairs[:, :2], ref.records[:, :2] + 1) and np.array_equal(got.pairs[:, 2], ref.records[:, 2])     # sorted by (i, j); +-1
    clear = ref.gap > 1e-9                                            # best and second best of the restatement apart
    assert np.array_equal(got.partner[clear], np.where(ref.partner >= 0, ref.partner + 1, -1)[clear]) and clear.sum() > ref.w.size // 2
    dead = ~ref.live
    assert np.all(got.partner[dead] == -1) and np.all(np.isnan(got.partnerCorrelation[dead]))
    has = clear & (ref.partner >= 0)
    dg, dv = scaled(got.partnerCorrelation[has], ref.partner_gamma[has]), scaled(got.variance, ref.variance)
    # where two partners tie within 1e-9 the device may name either: its |gamma| still equals the restatement's best
    tie = ~clear & (ref.partner >= 0)
    dt = scaled(np.abs(got.partnerCorrelation[tie]), np.abs(ref.partner_gamma[tie]))
    print(name, "rows", ref.w.size, "worst scaled deviation: partnerCorrelation", dg, "on ties", dt, "variance", dv)
    assert dg <= TOL and dv <= TOL and dt <= TOL


@pytest.mark.parametrize("name", list(SETS))
def test_the_records_of_correlation_0_9(jg, name):
    """the host test asserts that no |gamma| of the restatement is within 1e-9 of 0.9, so the lists are compared whole"""
    ref = reference(name, 0.9)[2]
    got = screened(jg, name, 0.9)
    assert (got.totalSingles, got.totalPairs, got.totalCorrelated) == ref.totals
    assert np.array_equal(got.pairs[:, :2], ref.records[:, :2] + 1)
    crit = np.abs(ref.records[:, 2]) == 1.0
    assert np.array_equal(got.pairs[crit, 2], ref.records[crit, 2]) and np.all(np.abs(got.pairs[~crit, 2]) < 1.0)
    d = scaled(got.pairs[:, 2], ref.records[:, 2])
    print(name, "records", len(ref.records), "worst scaled deviation of gamma", d)
    assert d <= TOL
    base = screened(jg, name)                                         # per-row results do not depend on the correlation
    assert np.array_equal(base.partner, got.partner) and np.array_equal(base.partnerCorrelation, got.partnerCorrelation, equal_nan=True)


def test_a_capacity_below_the_total(jg):
    t, ms, ref = reference("seeded", 0.9)
    total = ref.totals[1] + ref.totals[2]
    full = screened(jg, "seeded", 0.9)
    an = jg.dcStateEstimation(monitoring_of(jg, t, ms))
    for cap in (0, 1, 7, total - 1, total, total + 5):
        got = jg.dcCriticalScreen(an, correlation=0.9, capacity=cap)
        assert (got.totalSingles, got.totalPairs, got.totalCorrelated) == ref.totals, cap
        assert got.pairs.shape == (min(cap, total), 3) and np.array_equal(got.pairs[:, :2], ref.records[:cap, :2] + 1), cap
        assert np.array_equal(got.pairs, full.pairs[:cap]), cap        # bit for bit the prefix of the whole list
    an.close()


@pytest.mark.parametrize("name", ["case118", "seeded"])
def test_reported_pairs_against_the_removal_path(jg, name):
    """a lane that removes i and then j of a reported critical pair meets the zero pivot (status 1); a lane that removes the most correlated pair that
    is not reported keeps status 0.  Afterwards the handle has removed rows: the screen is refused with a message, not a fault."""
    t, ms, ref = reference(name)
    an = jg.dcStateEstimation(monitoring_of(jg, t, ms), batch=3)
    got = jg.dcCriticalScreen(an)
    ag = np.where(ref.is_candidate & ~ref.is_pair, np.abs(ref.gamma), 0.0)
    other = np.unravel_index(int(np.argmax(ag)), ag.shape)
    lanes = [tuple(int(x) for x in got.pairs[0, :2]), tuple(int(x) for x in got.pairs[-1, :2]), (int(other[0]) + 1, int(other[1]) + 1)]
    assert lanes[0] != lanes[1]
    jg.solveSE_(an)
    for k in range(2):
        jg.removeMeasurement_(an, np.array([p[k] for p in lanes], dtype=np.int32))
        jg.solveSE_(an)
        assert list(an.status) == ([0, 0, 0] if k == 0 else [1, 1, 0]), (k, an.status)
    with pytest.raises(Exception, match="removed rows"):
        jg.dcCriticalScreen(an)
    an.close()


def test_the_estimator_and_a_dc_handle_are_left_as_they_were(jg):
    """after the screen, normalizedResidual and residualTest_ on the same handle are bit for bit those of a fresh analysis, and a DC power-flow handle run
    before and after it gives the same bits: the shared sweep keeps no state"""
    t, ms, ref = reference("case118")
    mon = monitoring_of(jg, t, ms)
    dc = jg.dcPowerFlow(jg.powerSystem(t), batch=70)
    jg.dcpowerflow.solve_(dc)
    before = dc.voltage.angle.copy()
    out = []
    for with_screen in (True, False):
        an = jg.dcStateEstimation(mon, batch=3)
        jg.setNoise_(an, np.random.default_rng(4))
        jg.solveSE_(an)
        if with_screen:
            got = jg.dcCriticalScreen(an, correlation=0.9)
            assert got.totalPairs == ref.totals[1]
            jg.dcpowerflow.solve_(dc)
            assert np.array_equal(dc.voltage.angle, before)
        nr = jg.normalizedResidual(an)
        test = jg.residualTest_(an, threshold=1e300)
        out.append((nr, test.maxNormalizedResidual, test.index, an.voltage.angle.copy()))
        assert an.dims()["omegaRuns"] == 1                             # the screen formed the diagonal, or the test did: once
        an.close()
    dc.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert R.worst(before[0], R.solve(t)[0]) <= TOL


def test_new_weights_give_the_screen_of_the_new_set(jg):
    """one wattmeter of the leaf's critical pair goes out of service: the other becomes a critical measurement and the pair is gone.  Also: a Measurement
    container instead of an analysis, and labels"""
    t, ms, plan = C.thinned_case14(__import__("conftest").load_case)
    ref = C.screen(t, ms)
    (i, j), = ref.critical_pairs
    mon = monitoring_of(jg, t, ms)
    assert jg.dcCriticalScreen(mon, labels=True).critical == [f"PMU {int(r) - ms.w_index.size + 1}" for r in ref.critical]
    an = jg.dcStateEstimation(mon)
    first = jg.dcCriticalScreen(an)
    assert np.array_equal(first.pairs[:, :2], [[i + 1, j + 1]])
    jg.updateWattmeter_(an, int(i) + 1, status=0)
    ms.w_status[i] = 0
    new = C.screen(t, ms)
    assert j in new.critical and not new.critical_pairs
    got = jg.dcCriticalScreen(an)
    assert np.array_equal(got.critical, new.critical + 1) and got.pairs.shape == (0, 3) and (got.totalSingles, got.totalPairs) == new.totals[:2]
    assert scaled(got.variance, new.variance) <= TOL and an.dims()["refactorizations"] == 1
    an.close()
