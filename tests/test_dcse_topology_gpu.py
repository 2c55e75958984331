"""The branch status tests (dcTopologyScreen, csrc/jg_dcse_topology.hip) on the device against the dense restatement (tests/dcse_topology_reference.py: a
dense inverse of the gain and, independently, least squares on the widened matrix -- never the device's blocks of 512 candidates on the sparse factor).

The sets are the smallest at which a kernel can go wrong (tests/test_dcse_topology_host.py pins them and their margins): 20 candidates x 1 and 5 lanes
(partial waves everywhere), 186 x 70 (neither a multiple of 64), 1 300 x 3 (three blocks of 512 candidates, the last of 276), and two hand-made grids with
critical branches, twins, shifts and a slack angle.  Status is compared for EQUALITY (three decades on either side of the limit); D / norm within 1e-9
absolute; t, phi and angles within 1e-9 * max(1, |ref|), the bound the project holds its DC parity to.

Worst deviations seen on an MI355X (scaled as above; printed by every test): D / norm 4.0e-15, t 9.3e-12, phi 1.8e-12, corrected angles 1.2e-14, the
noise-free known answer 8.7e-16."""
import numpy as np
import pytest

import dcse_topology_reference as T
from conftest import load_case
from test_dcse_host import monitoring_of
from test_dcse_topology_host import lanes_of, scaled

pytestmark = pytest.mark.gpu

TOL = 1e-9
NAMES = list(T.FIXTURES)
_GOT = {}


def analysis_of(jg, name):
    fx, Z, roles, st, thr = lanes_of(name)
    an = jg.dcStateEstimation(monitoring_of(jg, fx.t, fx.ms), batch=fx.batch)
    jg.setReadings_(an, Z)
    jg.solveSE_(an)
    return an


def screened(jg, name):
    """the device's screen of a set's lanes (dense, corrected), run once and shared with what the handle gave before and after it"""
    if name not in _GOT:
        fx, Z, roles, st, thr = lanes_of(name)
        an = analysis_of(jg, name)
        before = (np.atleast_2d(jg.normalizedResidual(an)).copy(), np.atleast_2d(an.voltage.angle).copy())
        got = jg.dcTopologyScreen(an, candidates=fx.cand + 1, threshold=thr, dense=True, correct=True)
        runs = jg.topologyRuns(an)
        again = jg.dcTopologyScreen(an, candidates=None if name == "case118" else fx.cand + 1, threshold=thr)
        after = (np.atleast_2d(jg.normalizedResidual(an)).copy(), jg.residualTest_(an, threshold=1e300) if fx.batch > 1 else None)
        _GOT[name] = NS(got=got, again=again, runs=(runs, jg.topologyRuns(an)), before=before, after=after, largest=before[0].max(axis=1))
        an.close()
    return _GOT[name]


from types import SimpleNamespace as NS  # noqa: E402


@pytest.mark.parametrize("name", NAMES)
def test_denominators_and_status_against_the_restatement(jg, name):
    fx = T.fixture(name, load_case)
    got = screened(jg, name).got
    sc = fx.sc
    assert np.array_equal(got.candidates, fx.cand + 1) and np.array_equal(got.status, sc.status)
    seen = sc.status != 2
    d = float(np.abs(got.denominator[seen] / got.norm[seen] - sc.D[seen] / sc.norm[seen]).max())
    dn = scaled(got.norm, sc.norm)
    print(name, "candidates", sc.cand.size, "worst |D / norm - ref|", d, "norm scaled", dn)
    assert d <= TOL and dn <= TOL
    assert np.array_equal(got.critical, fx.cand[sc.status == 1] + 1) and np.array_equal(got.unseen, fx.cand[sc.status == 2] + 1)


@pytest.mark.parametrize("name", NAMES)
def test_statistics_best_counts_and_records_against_the_restatement(jg, name):
    fx, Z, roles, st, thr = lanes_of(name)
    g = screened(jg, name)
    got = g.got
    ok = fx.sc.status == 0
    assert np.all(np.isnan(got.statisticAll[~ok])) and got.statisticAll.shape == st.t.shape
    dt = scaled(got.statisticAll[ok], st.t[ok])
    a = np.abs(np.where(np.isnan(st.t), 0.0, st.t))
    order = np.sort(a, axis=0)
    clear = order[-1] - order[-2] > 1e-6 * order[-1]                  # the restatement's two largest |t| of a lane apart
    ref_best = fx.cand[np.argmax(a, axis=0)] + 1
    assert np.array_equal(got.best[clear], ref_best[clear]) and (~clear).sum() <= 0.05 * fx.batch
    pos = {int(k): q for q, k in enumerate(fx.cand)}
    for l, (kind, k) in enumerate(roles):
        if kind in ("open", "close"):
            assert clear[l]                                            # no planted lane is left out of the comparison of `best`
            q = pos[int(got.best[l]) - 1]
            assert got.best[l] == k + 1 or a[q, l] >= a[pos[k], l] * (1.0 - 1e-9), (l, kind, k, got.best[l])     # the planted branch, or its twin
            # one branch explains the lane at least as well as any single meter (with a slack angle residualTest_ follows the reference's variant of the
            # residual, tests/dcse_reference.py: residuals, which is not the least-squares one: no statement there)
            # (a critical PMU's residual is rounding over a variance of zero: infinite, as residualTest_ reports it)
            assert fx.dense.va != 0.0 or not np.isfinite(g.largest[l]) or abs(got.statistic[l]) >= g.largest[l] * (1.0 - 1e-9)
        if kind == "meter":
            assert g.largest[l] >= abs(got.statistic[l]) and np.array_equal(got.largestResidual, g.largest)
    lane = np.arange(fx.batch)
    qb = np.array([pos[int(b) - 1] for b in got.best])
    ds, dp = scaled(got.statistic, st.t[qb, lane]), scaled(got.flowError, st.phi[qb, lane])
    hits = a >= thr
    assert np.array_equal(got.count, hits.sum(axis=0)) and got.total == int(hits.sum())
    ll, qq = np.nonzero(hits.T)                                       # lane-major: sorted by (lane, candidate)
    assert np.array_equal(got.records[:, 0], ll + 1) and np.array_equal(got.records[:, 1], fx.cand[qq] + 1)
    dr = max(scaled(got.records[:, 2], st.t[qq, ll]), scaled(got.records[:, 3], st.phi[qq, ll]))
    print(name, "lanes", fx.batch, "records", got.total, "worst scaled deviation: statisticAll", dt, "statistic", ds, "flowError", dp, "records", dr)
    assert max(dt, ds, dp, dr) <= TOL


def test_the_known_answer_without_noise(jg):
    """exact readings of the grid with branch k open against a model that holds it closed: |phi^ + f_k| <= 1e-9 scaled, the corrected angles are the
    true ones"""
    for name in ("case14", "mesh"):
        fx = T.fixture(name, load_case)
        ks = T.plantable(fx, True, 2) + T.plantable(fx, False, 1)
        truth = [T.readings(fx, k) for k in ks]
        Z = np.array([truth[l % len(ks)][0] for l in range(fx.batch)])
        an = jg.dcStateEstimation(monitoring_of(jg, fx.t, fx.ms), batch=fx.batch)
        jg.setReadings_(an, Z)
        jg.solveSE_(an)
        got = jg.dcTopologyScreen(an, candidates=fx.cand + 1, threshold=1e-3, correct=True)
        an.close()
        y = __import__("dc_reference").admittance(fx.t)
        f, to = fx.t["br_from"].astype(int) - 1, fx.t["br_to"].astype(int) - 1
        worst = 0.0
        for l in range(fx.batch):
            k = ks[l % len(ks)]
            z, th_true, flow = truth[l % len(ks)]
            th = got.angle[l]
            fk = y[k] * (th[f[k]] - th[to[k]] - float(fx.t["br_shift"][k])) if fx.t["br_status"][k] else -flow[k]
            worst = max(worst, scaled(got.flowError[l], -fk), scaled(th, th_true))
        print(name, "worst scaled deviation of phi^ + f_k and of the corrected angles", worst)
        assert worst <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_corrected_angles_and_an_untouched_handle(jg, name):
    fx, Z, roles, st, thr = lanes_of(name)
    g = screened(jg, name)
    got = g.got
    angle = np.atleast_2d(got.angle)
    worst, corrected = 0.0, 0
    for l in range(fx.batch):
        if abs(got.statistic[l]) >= thr:
            k = int(got.best[l]) - 1
            worst = max(worst, scaled(angle[l], fx.dense.augmented(Z[l], k)[1]))
            corrected += 1
        else:
            assert np.array_equal(angle[l], g.before[1][l])            # bit for bit the analysis' angles
    print(name, "lanes corrected", corrected, "worst scaled deviation of the corrected angles from least squares", worst)
    assert worst <= TOL and corrected >= 1
    assert np.array_equal(g.before[0], g.after[0])                     # normalizedResidual after the screen: the same bits
    if g.after[1] is not None:
        assert np.array_equal(g.after[1].maxNormalizedResidual, g.largest)


@pytest.mark.parametrize("name", ["case14", "case118"])
def test_a_second_call_sweeps_nothing_and_new_weights_sweep_again(jg, name):
    fx, Z, roles, st, thr = lanes_of(name)
    g = screened(jg, name)
    assert g.runs == (1, 1)                                            # the second call found the denominators on the handle
    for field in ("status", "denominator", "norm", "best", "statistic", "count", "records"):
        assert np.array_equal(getattr(g.again, field), getattr(g.got, field), equal_nan=True), field
    if name != "case14":
        return
    an = analysis_of(jg, name)
    jg.dcTopologyScreen(an, candidates=fx.cand + 1, threshold=thr)
    k = next(k for kind, k in roles if kind == "open")
    row = int(np.flatnonzero((fx.ms.w_kind > 0) & (fx.ms.w_index == k + 1) & (fx.ms.w_status == 1))[0])
    jg.updateWattmeter_(an, row + 1, status=0)
    jg.solveSE_(an)
    got = jg.dcTopologyScreen(an, candidates=fx.cand + 1, threshold=thr)
    assert jg.topologyRuns(an) == 2 and an.dims()["refactorizations"] == 1
    an.close()
    ms = T.S.meters(fx.ms.w_kind, fx.ms.w_index, fx.ms.w_mean, fx.ms.w_variance, fx.ms.w_status, fx.ms.p_index, fx.ms.p_bus, fx.ms.p_angle, fx.ms.p_variance,
                    fx.ms.p_status)
    ms.w_status[row] = 0
    sc = T.Dense(fx.t, ms).screen(fx.cand)
    seen = sc.status != 2
    assert np.array_equal(got.status, sc.status) and not np.array_equal(sc.D, fx.sc.D)
    assert float(np.abs(got.denominator[seen] / got.norm[seen] - sc.D[seen] / sc.norm[seen]).max()) <= TOL


def test_the_block_a_candidate_falls_in_does_not_matter(jg):
    fx, Z, roles, st, thr = lanes_of("pegase777")
    an = analysis_of(jg, "pegase777")
    rev = jg.dcTopologyScreen(an, candidates=(fx.cand + 1)[::-1], threshold=thr)
    an.close()
    got = screened(jg, "pegase777").got
    assert np.array_equal(rev.status[::-1], got.status) and np.array_equal(rev.norm[::-1], got.norm)
    d = float(np.abs(rev.denominator[::-1] - got.denominator).max() / got.norm.max())
    print("reversed candidates: worst |D - D| / norm", d)
    assert d <= 1e-12 and rev.total == got.total and np.array_equal(rev.count, got.count)


def test_a_capacity_below_the_total(jg):
    fx, Z, roles, st, thr = lanes_of("mesh")
    full = screened(jg, "mesh").got
    assert full.total >= 3
    an = analysis_of(jg, "mesh")
    for cap in (0, 1, full.total - 1, full.total):
        got = jg.dcTopologyScreen(an, candidates=fx.cand + 1, threshold=thr, capacity=cap)
        assert got.total == full.total and np.array_equal(got.count, full.count), cap
        assert got.records.shape == (min(cap, full.total), 4) and np.array_equal(got.records, full.records[:cap]), cap
    an.close()


def test_refusals_are_exceptions(jg):
    fx, Z, roles, st, thr = lanes_of("case14")
    mon = monitoring_of(jg, fx.t, fx.ms)
    an = jg.dcStateEstimation(mon, batch=fx.batch)
    with pytest.raises(ValueError, match="dcTopologyScreen: solve"):
        jg.dcTopologyScreen(an)
    jg.setReadings_(an, Z)
    jg.solveSE_(an)
    with pytest.raises(ValueError, match="label 21"):
        jg.dcTopologyScreen(an, candidates=[1, 21])
    with pytest.raises(ValueError, match="threshold"):
        jg.dcTopologyScreen(an, threshold=0.0)
    with pytest.raises(ValueError, match="capacity"):
        jg.dcTopologyScreen(an, capacity=-1)
    with pytest.raises(TypeError, match="dcTopologyScreen"):
        jg.dcTopologyScreen(fx.t)
    rows = np.zeros(fx.batch, dtype=np.int32)
    rows[1] = 1
    jg.removeMeasurement_(an, rows)
    jg.solveSE_(an)
    with pytest.raises(Exception, match="removed rows"):
        jg.dcTopologyScreen(an)
    an.close()
    got = jg.dcTopologyScreen(mon, labels=True)                       # a Measurement container: built, solved and closed here
    assert got.critical == [f"Branch {int(k) + 1}" for k in fx.cand[fx.sc.status == 1]] and got.best.shape == (1,)
