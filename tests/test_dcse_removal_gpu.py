"""DC bad-data removal with two to four COUPLED rows per lane on the device, against the rebuild-and-refactorise restatement (tests/dcse_reference.py).

The rows are the clusters of tests/test_dcse_removal_host.py (four meters round one bus), whose Omega_SS has large off-diagonal terms: the host file
shows that a compensation without them is off by more than 1e-3 on every cluster used here, six decades above the bound below.  `checked` compares,
per lane with removed rows S and rb = Rebuilt(t, ms, S), ref = rb.solve(z):

  angles                          R.worst(angle, ref) <= REMOVAL_TOL (TOL where nothing is removed)
  every normalised residual       |got - nr| <= REMOVAL_TOL * max(1, nr), nr = rb.normalized(z, ref, rb.variances()), all m rows;
                                  removed and out-of-service rows exactly 0
  maximum and index               residualTest_(threshold=1e300): the index exact (the restatement's two largest differ by more than 1 %), the
                                  maximum at the same bound
  objective                       relative, |got - ref| / max(1, ref) <= the same bound

Asserted on the restatement before any comparison: the rebuilt gain is not singular and every kept in-service row keeps w_i Omega'_ii >= 1e-3 (the
relative error of a normalised residual grows like the inverse of that).  The readings are the model's means plus N(0, sigma) from a fixed seed, drawn
here so that the restatement's side can be evaluated without a device; every lane also carries 8 sigma (over the share of variance its residual keeps)
on the PMU at the far end of its cluster's branch, a kept row next to the removed ones, so that the largest normalised residual is no near-tie of two
noise values.  The restatement of a (grid, removed rows) pair is built once and shared by the tests.

TOL and REMOVAL_TOL are tests/test_dcse_gpu.py's (MEASURED_REMOVAL = 1.122e-10 on the 10k-bus grid, x 10; 4.9e-15 on case118 with two far-apart rows).
Worst deviations seen on one MI355X in this file, lanes with removed rows, next to that MEASURED_REMOVAL: angles 5.6e-15 (MEASURED_ANGLE),
normalised residuals, relative over all rows, 1.8e-12 (MEASURED_NORMALISED), objective 3.0e-15 (MEASURED_OBJECTIVE); per test in the docstrings
below.  The coupled rows cost the angles nothing against two far-apart ones; the normalised residuals sit three decades below the bound and nine
below what a compensation without the coupling would show."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
from conftest import load_case
from test_dcse_gpu import REMOVAL_TOL, TOL
from test_dcse_host import monitoring_of
from test_dcse_removal_host import CONDITION, gpu_clusters, grid, kept, measurement_set, outage_rows, twice_metered_leaf

pytestmark = pytest.mark.gpu

MEASURED_ANGLE = 5.552e-15                                           # case118 with the slack's angle kept, four rows
MEASURED_NORMALISED = 1.764e-12                                      # case118, zero to four rows in one wavefront
MEASURED_OBJECTIVE = 3.018e-15                                       # case14, the twice-metered leaf, one row

_GRIDS, _REBUILT = {}, {}


def setting(name):
    """(table, measurement set, clusters) of a grid of test_dcse_removal_host.GPU_GRIDS, built once"""
    if name not in _GRIDS:
        t = grid(name)
        _GRIDS[name] = (t, measurement_set(name, t)[1], gpu_clusters(name, t))
    return _GRIDS[name]


def rebuilt(name, rows):
    """(Rebuilt, its variances) of the grid without `rows`, once per set of rows; observable and conditioned, or the inputs are wrong"""
    key = (name, tuple(int(r) for r in rows))
    if key not in _REBUILT:
        t, ms, _ = setting(name)
        rb = S.Rebuilt(t, ms, key[1])
        assert not rb.singular, key
        var = rb.variances()
        share = (rb.w * var)[kept(rb)]
        assert share.min() >= CONDITION, (key, float(share.min()))
        _REBUILT[key] = (rb, var)
    return _REBUILT[key]


def cluster_of(name, s):
    """lane s takes the cluster of the (s mod 65)-th eligible bus (round again where a grid has fewer): lanes s and s + 65 share one"""
    clusters = setting(name)[2]
    return clusters[(s % 65) % len(clusters)]


def readings_of(name, batch, seed, scale=1.0, amplitude=8.0, clusters=None):
    """[batch, m] se.mean of every lane: the model's means + scale * sigma * N(0, 1) on the in-service rows (what setNoise_ draws), lanes s + 65 a copy
    of lanes s, and `amplitude` sigma over the kept share on the PMU at the far end of the lane's cluster's branch (against the slack's angle, which
    every PMU row carries as a residual where it is not 0: badData.jl:66-73)"""
    t, ms, _ = setting(name)
    mo = S.model(t, ms)
    rb, var = rebuilt(name, ())
    z = mo.mean[None, :] + rb.status[None, :] * scale / np.sqrt(mo.precision)[None, :] * np.random.default_rng(seed).standard_normal((batch, mo.number))
    z[65:] = z[:max(batch - 65, 0)]
    n = t["bus_type"].size
    for s in range(batch):
        c = cluster_of(name, s) if clusters is None else clusters[s]
        row = mo.number - n + c[3]
        assert rb.status[row] == 1.0 and row not in c
        z[s, row] += (-1.0 if rb.va > 0 else 1.0) * amplitude / np.sqrt(mo.precision[row] * (mo.precision * var)[row])
    return z


def expected(name, z, rows):
    """the restatement of one lane: angles, all normalised residuals, the arg-max and the maximum (the two largest differ by more than 1 %), objective"""
    rb, var = rebuilt(name, rows)
    ref = rb.solve(z)
    nr = rb.normalized(z, ref, var)
    i = int(np.argmax(nr))
    top = np.sort(nr)[-2:]
    assert top[1] > 1.01 * top[0], (name, rows, top)
    return ref, nr, i, rb.objective(z, ref), rb


def checked(jg, name, an, removed_rows, lanes=None, what=""):
    """the full check of the module's docstring on `lanes` of a solved analysis; removed_rows[s]: the 0-based rows lane s has removed, in order.
    Returns the worst deviations (angles, normalised residuals, objective) of the lanes with removed rows"""
    th, obj = np.atleast_2d(an.voltage.angle), np.atleast_1d(an.objective)
    nrm = np.atleast_2d(jg.normalizedResidual(an))
    out = jg.residualTest_(an, threshold=1e300)                      # removes nothing
    worst = np.zeros(3)
    for s in (range(an.batch) if lanes is None else lanes):
        rows = [int(r) for r in removed_rows[s]]
        ref, nr, i, o, rb = expected(name, an.readings[s], rows)
        tol = REMOVAL_TOL if rows else TOL
        assert np.atleast_1d(an.status)[s] == 0, (what, s)
        dev = np.array([R.worst(th[s], ref), float((np.abs(nrm[s] - nr) / np.maximum(1.0, nr)).max()), abs(obj[s] - o) / max(1.0, o)])
        assert dev[0] <= tol, (what, s, "angles", dev[0])
        assert dev[1] <= tol, (what, s, "normalised residuals", dev[1], int(np.argmax(np.abs(nrm[s] - nr) / np.maximum(1.0, nr))))
        assert np.all(nrm[s][rb.status == 0.0] == 0.0), (what, s, "a removed or out-of-service row carries a normalised residual")
        assert int(out.index[s]) == i + 1, (what, s, int(out.index[s]), i + 1)
        assert abs(out.maxNormalizedResidual[s] - nr[i]) <= tol * max(1.0, nr[i]), (what, s, out.maxNormalizedResidual[s], nr[i])
        assert dev[2] <= tol, (what, s, "objective", dev[2])
        if rows:
            worst = np.maximum(worst, dev)
    print(what, "worst of the removal lanes: angles", worst[0], "normalised residuals", worst[1], "objective", worst[2])
    return worst


def analysis(jg, name, batch, method="LU"):
    t, ms, _ = setting(name)
    return jg.dcStateEstimation(monitoring_of(jg, t, ms), getattr(jg, method), batch=batch)


def remove(jg, an, rows_by_lane):
    """one removeMeasurement_ call: {lane: 0-based row}"""
    r = np.zeros(an.batch, dtype=np.int32)
    for s, row in rows_by_lane.items():
        r[s] = row + 1
    jg.removeMeasurement_(an, r)


def test_coupled_clusters_one_to_four_rows_all_residuals(jg):
    """case118, 70 lanes (the second wavefront is partial): lane s drops the rows of its cluster one per call; after every call everything is compared.
    Seen on one MI355X after 1, 2, 3, 4 rows: angles 2.5e-15, 2.7e-15, 2.8e-15, 2.8e-15; normalised residuals 1.02e-12, 9.5e-13, 1.25e-12, 1.04e-12;
    objective at most 1.4e-15"""
    an = analysis(jg, "case118", 70)
    jg.setReadings_(an, readings_of("case118", 70, 20261019))
    for k in range(4):
        remove(jg, an, {s: cluster_of("case118", s)[k] for s in range(70)})
        jg.solveSE_(an)
        checked(jg, "case118", an, [cluster_of("case118", s)[:k + 1] for s in range(70)], what=f"{k + 1} rows")
    gone = jg.removed(an)
    assert all([int(x) - 1 for x in gone.rows[s]] == cluster_of("case118", s) for s in range(70))
    assert an.dims()["refactorizations"] == 0
    an.close()


def test_lanes_of_one_wavefront_with_zero_to_four_rows(jg):
    """case118, 130 lanes: lane s holds the first s mod 5 rows of its cluster, so every guard on a lane's count diverges inside every wavefront.  The
    lanes without a removed row equal an analysis that never removed anything bitwise; lanes s and s + 65 (same cluster, same readings, other
    neighbours, other wavefront) equal each other bitwise.  Seen on one MI355X: angles 3.4e-15, normalised residuals 1.76e-12, objective 1.0e-15"""
    z = readings_of("case118", 130, 20261020)
    an, plain = analysis(jg, "case118", 130), analysis(jg, "case118", 130)
    jg.setReadings_(an, z)
    jg.setReadings_(plain, z)
    for k in range(4):
        remove(jg, an, {s: cluster_of("case118", s)[k] for s in range(130) if s % 5 > k})
    jg.solveSE_(an)
    jg.solveSE_(plain)
    held = [cluster_of("case118", s)[:s % 5] for s in range(130)]
    assert [len(r) for r in jg.removed(an).rows] == [s % 5 for s in range(130)]
    checked(jg, "case118", an, held, what="mixed counts")
    a, b = jg.normalizedResidual(an), jg.normalizedResidual(plain)
    ta, tb = jg.residualTest_(an, threshold=1e300), jg.residualTest_(plain, threshold=1e300)
    none = np.arange(0, 130, 5)
    assert np.array_equal(an.voltage.angle[none], plain.voltage.angle[none]) and np.array_equal(an.objective[none], plain.objective[none])
    assert np.array_equal(a[none], b[none]) and np.array_equal(ta.index[none], tb.index[none])
    assert np.array_equal(ta.maxNormalizedResidual[none], tb.maxNormalizedResidual[none])
    assert np.array_equal(an.voltage.angle[:65], an.voltage.angle[65:]) and np.array_equal(an.objective[:65], an.objective[65:])
    assert np.array_equal(a[:65], a[65:]) and np.array_equal(ta.index[:65], ta.index[65:])
    assert np.array_equal(ta.maxNormalizedResidual[:65], ta.maxNormalizedResidual[65:])
    assert an.dims()["refactorizations"] == 0
    plain.close()
    an.close()


@pytest.mark.parametrize("name", ["case14moved", "case118kept"])
def test_removal_with_the_slack_angle_kept(jg, name):
    """the slack at -0.17 (the 14-bus grid with the slack moved) and at 0.52 rad (case118 as stored): roff_t and roff_c enter the passes over a reduced
    set.  Every PMU row carries the slack's angle as a residual there (at_zero's docstring), so the rows leave by removeMeasurement_.  Seen on one
    MI355X after four rows: angles 5.3e-16 and 5.6e-15, normalised residuals 2.0e-14 and 4.6e-13"""
    an = analysis(jg, name, 3)
    jg.setReadings_(an, readings_of(name, 3, 5, amplitude=1000.0))
    for k in (2, 4):
        rb, var = rebuilt(name, cluster_of(name, 0)[:k])
        ref = rb.solve(an.readings[0])
        with_angle, without = rb.normalized(an.readings[0], ref, var), rb.normalized(an.readings[0], ref - rb.va, var)
        assert np.abs(with_angle - without).max() > 1.0             # the offset of the test's residual matters on these grids
        remove(jg, an, {s: cluster_of(name, s)[k - 2] for s in range(3)})
        remove(jg, an, {s: cluster_of(name, s)[k - 1] for s in range(3)})
        jg.solveSE_(an)
        checked(jg, name, an, [cluster_of(name, s)[:k] for s in range(3)], what=f"{name}, {k} rows")
    assert an.dims()["refactorizations"] == 0
    an.close()


@pytest.mark.parametrize("tag", ["Orthogonal", "PetersWilkinson"])
def test_the_corrected_methods_with_removed_rows(jg, tag):
    """case30test, 70 lanes: the correction step on the shared factor, then the compensation; also against LU with the same removals.  Seen on one
    MI355X, both tags: angles 2.1e-15 (the same against LU), normalised residuals 8.3e-13, objective 1.4e-15"""
    name = "case30test"
    z = readings_of(name, 70, 30)
    an, lu = analysis(jg, name, 70, tag), analysis(jg, name, 70)
    jg.setReadings_(an, z)
    jg.setReadings_(lu, z)
    for k in (2, 4):
        for q in (k - 2, k - 1):
            remove(jg, an, {s: cluster_of(name, s)[q] for s in range(70)})
            remove(jg, lu, {s: cluster_of(name, s)[q] for s in range(70)})
        jg.solveSE_(an)
        jg.solveSE_(lu)
        checked(jg, name, an, [cluster_of(name, s)[:k] for s in range(70)], what=f"{tag}, {k} rows")
        both = max(R.worst(an.voltage.angle[s], lu.voltage.angle[s]) for s in range(70))
        print(tag, k, "rows: against LU", both)
        assert both <= TOL
    lu.close()
    an.close()


def test_out_of_service_rows_in_the_set(jg):
    """case118 with three wattmeters (one at the first cluster's bus, not in the cluster) and one PMU out of service before the monitoring is built.
    Seen on one MI355X: angles 2.7e-15, normalised residuals 5.6e-13"""
    name = "case118outage"
    t, ms, _ = setting(name)
    dead = outage_rows(t)
    an = analysis(jg, name, 3)
    assert an.method.inservice == an.method.number - 4
    jg.setReadings_(an, readings_of(name, 3, 9))
    with pytest.raises(jg._lib.JGridError, match="out of service"):
        remove(jg, an, {1: dead[0]})
    for k in range(4):
        remove(jg, an, {s: cluster_of(name, s)[k] for s in range(3)})
    jg.solveSE_(an)
    checked(jg, name, an, [cluster_of(name, s) for s in range(3)], what="out-of-service rows")
    assert np.all(np.atleast_2d(jg.normalizedResidual(an))[:, dead] == 0.0)
    an.close()


def test_a_lane_turns_critical_at_its_second_removal(jg):
    """case14, a leaf seen by the from- and the to-wattmeter of its branch only (rows 1 and 2): either may leave, the second one is critical, and the
    pivot of k_dcse_extend reaches 0 by cancellation, d = Omega_kk - sum L^2 D, not as Omega_kk.  Angles and objective only: once one of the two has
    left, the other's residual is 0 with variance 0, so the condition of the normalised check cannot hold on these lanes.  Seen on one MI355X:
    angles 2.2e-16, objective 3.0e-15"""
    t = load_case("case14")
    th, ms, leaf, neighbour = twice_metered_leaf(t)
    an = jg.dcStateEstimation(monitoring_of(jg, t, ms), batch=70)
    jg.setNoise_(an, np.random.default_rng(3))
    jg.solveSE_(an)
    before = (an.voltage.angle.copy(), an.objective.copy())
    rest = np.delete(np.arange(70), [5, 6, 7, 8])

    def same(s, rows):
        rb = S.Rebuilt(t, ms, rows)
        assert not rb.singular
        ref = rb.solve(an.readings[s])
        o = rb.objective(an.readings[s], ref)
        dev = (R.worst(an.voltage.angle[s], ref), abs(an.objective[s] - o) / max(1.0, o))
        print("lane", s, "without", rows, "angles", dev[0], "objective", dev[1])
        assert an.status[s] == 0 and dev[0] <= REMOVAL_TOL and dev[1] <= REMOVAL_TOL, (s, rows, dev)

    def critical(s):
        assert an.status[s] == 1 and np.all(np.isnan(an.voltage.angle[s])) and np.isnan(an.objective[s]), s
        out = jg.residualTest_(an, threshold=1e300)                  # removes nothing
        assert np.isnan(out.maxNormalizedResidual[s]) and out.index[s] == 0 and not out.detect[s]

    def untouched():
        assert np.array_equal(an.voltage.angle[rest], before[0][rest]) and np.array_equal(an.objective[rest], before[1][rest])
        assert np.all(an.status[rest] == 0)

    remove(jg, an, {5: 0, 6: 0, 7: 4, 8: 0})
    jg.solveSE_(an)
    for s, rows in ((5, [0]), (6, [0]), (7, [4]), (8, [0])):
        same(s, rows)
    untouched()
    remove(jg, an, {5: 1, 6: 4, 7: 0})
    jg.solveSE_(an)
    critical(5)
    for s, rows in ((6, [0, 4]), (7, [4, 0]), (8, [0])):
        same(s, rows)
    untouched()
    remove(jg, an, {6: 1})
    jg.solveSE_(an)
    critical(5)
    critical(6)
    for s, rows in ((7, [4, 0]), (8, [0])):
        same(s, rows)
    untouched()
    gone = jg.removed(an)
    assert [list(gone.rows[s]) for s in (5, 6, 7, 8)] == [[1], [1, 5], [5, 1], [1]]
    assert all(list(gone.rows[s]) == [] for s in rest) and list(gone.status[[5, 6, 7, 8]]) == [1, 1, 0, 0]
    assert an.dims()["refactorizations"] == 0
    an.close()


SIZES = (240.0, 120.0, 60.0, 30.0)                                   # normalised units of the four planted errors, in the cluster's order
FIFTH = 15.0


def planted(name, batch, seed):
    """readings with gross errors on the four rows of every lane's cluster, sized as test_dcse_gpu.plant does (by the share of the variance the residual
    keeps in the full set), alternating in sign; lane 0 carries a fifth on an injection wattmeter elsewhere.  Noise at half a sigma, so that a lane
    whose errors are all gone stays below the threshold of 3.  The cluster of bus 24 is left out: the restatement's loop names the to-wattmeter of
    its branch there, the twin of the planted from-wattmeter (the same row up to its sign, test_dcse_gpu.plantable_rows)"""
    t, ms, clusters = setting(name)
    usable = [c for c in clusters if c[0] != 23]
    mine = [usable[(s % 65) % len(usable)] for s in range(batch)]
    z = readings_of(name, batch, seed, scale=0.5, amplitude=0.0, clusters=mine)
    rb, var = rebuilt(name, ())
    share = np.sqrt(rb.w * var)
    for s in range(batch):
        for q, row in enumerate(mine[s]):
            z[s, row] += (-1.0) ** q * SIZES[q] / np.sqrt(rb.w[row]) / share[row]
    fifth = clusters[20][0]
    assert fifth not in mine[0]
    z[0, fifth] += FIFTH / np.sqrt(rb.w[fifth]) / share[fifth]
    return z, fifth, mine


def restated_rounds(name, z, rounds):
    """the reference's loop for one lane (estimate, normalise every row, remove the arg-max above 3): [(angles, row or None, maximum)]"""
    rows, seen = [], []
    for _ in range(rounds):
        rb, var = rebuilt(name, rows)
        ref = rb.solve(z)
        nr = rb.normalized(z, ref, var)
        i = int(np.argmax(nr))
        top = np.sort(nr)[-2:]
        if top[1] > 3.0:
            assert top[1] > 1.01 * top[0], (rows, top)
            seen.append((ref, i, float(nr[i])))
            rows = rows + [i]
        else:
            assert top[1] < 2.9                                      # clearly below the threshold: nothing leaves
            seen.append((ref, None, float(nr[i])))
    return seen, rows


def test_four_rounds_of_the_residual_test_then_a_fifth(jg):
    """case118, 70 lanes, four gross errors on every lane's cluster: four rounds of solveSE_ and residualTest_(threshold=3) name the rows the
    restatement's loop names, with its maximum and its angles; lane 0's fifth error asks for a fifth row in the fifth round: status 2.  Seen on one
    MI355X over rounds two to five: angles 3.9e-15, maximum 4.0e-13"""
    name = "case118"
    z, fifth, mine = planted(name, 70, 77)
    want = [restated_rounds(name, z[s], 5) for s in range(70)]
    for s in range(70):                                              # on the restatement: a planted row in each of four rounds, then nothing (lane 0: the fifth)
        seen, rows = want[s]
        assert sorted(rows[:4]) == sorted(mine[s]) and all(x[2] > 20.0 for x in seen[:4]), (s, rows)
        assert rows[4:] == ([fifth] if s == 0 else []), (s, rows)
    an = analysis(jg, name, 70)
    jg.setReadings_(an, z)
    worst = np.zeros(2)
    for rnd in range(5):
        jg.solveSE_(an)
        assert np.all(an.status == 0)
        last = (an.voltage.angle.copy(), an.objective.copy())
        out = jg.residualTest_(an, threshold=3.0)
        tol = REMOVAL_TOL if rnd else TOL
        for s in range(70):
            ref, i, mx = want[s][0][rnd]
            dev = (R.worst(an.voltage.angle[s], ref), abs(out.maxNormalizedResidual[s] - mx) / max(1.0, mx))
            assert dev[0] <= tol and dev[1] <= tol, (rnd, s, dev)
            assert bool(out.detect[s]) == (i is not None) and (i is None or int(out.index[s]) == i + 1), (rnd, s, i, int(out.index[s]))
            worst = np.maximum(worst, dev) if rnd else worst
        gone = jg.removed(an)
        assert all([int(x) - 1 for x in gone.rows[s]] == want[s][1][:min(rnd + 1, 4)] for s in range(70)), rnd
    print("rounds: worst angles", worst[0], "worst maximum", worst[1])
    jg.solveSE_(an)
    assert an.status[0] == 2 and np.all(np.isnan(an.voltage.angle[0])) and np.isnan(an.objective[0]) and np.all(an.status[1:] == 0)
    assert np.array_equal(an.voltage.angle[1:], last[0][1:]) and np.array_equal(an.objective[1:], last[1][1:])
    assert an.dims()["refactorizations"] == 0
    an.close()


def test_powers_and_chi_square_on_lanes_with_removed_rows(jg):
    """case118, 70 lanes, four rows removed on all but the last lane: the branch flows come from the compensated angles, the degrees of freedom of the
    chi-square test lose the removed rows.  Seen on one MI355X: flows 4.1e-14"""
    from scipy.stats import chi2
    name = "case118"
    t, ms, _ = setting(name)
    an = analysis(jg, name, 70)
    jg.setReadings_(an, readings_of(name, 70, 20261019))
    for k in range(4):
        remove(jg, an, {s: cluster_of(name, s)[k] for s in range(69)})
    jg.solveSE_(an)
    held = [cluster_of(name, s) if s < 69 else [] for s in range(70)]
    checked(jg, name, an, held, what="before the powers")
    jg.power_(an)
    worst = 0.0
    for s in range(70):
        ref, nr, i, o, rb = expected(name, an.readings[s], held[s])
        flows = R.power(t, ref)["from_"]
        worst = max(worst, float((np.abs(an.power.from_.active[s] - flows) / np.maximum(1.0, np.abs(flows))).max()))
    print("flows: worst deviation", worst)
    assert worst <= 1e-9
    assert np.array_equal(an.power.to.active, -an.power.from_.active)
    c = jg.chiTest(an)
    n, inservice = t["bus_type"].size, an.method.inservice
    assert inservice == an.method.number
    assert np.array_equal(c.threshold[:69], np.full(69, chi2.ppf(0.95, inservice - 4 - n + 1))) and c.threshold[69] == chi2.ppf(0.95, inservice - n + 1)
    assert np.array_equal(c.objective, an.objective) and np.array_equal(c.detect, an.objective >= c.threshold)
    an.close()


def test_removal_after_a_weight_update(jg):
    """a variance update refactorises and empties every lane's removed rows, but the device keeps the old U and L D L': the first passes after it must
    not read them.  Bitwise against a freshly built analysis with the same two removals.  Seen on one MI355X after the update: angles 1.9e-15,
    normalised residuals 9.7e-13"""
    name = "case118pmu11"
    an = analysis(jg, "case118", 3)
    jg.setReadings_(an, readings_of("case118", 3, 13))
    for k in range(2):
        remove(jg, an, {s: cluster_of("case118", s)[k] for s in range(3)})
    jg.solveSE_(an)
    checked(jg, "case118", an, [cluster_of("case118", s)[:2] for s in range(3)], what="before the update")
    jg.updatePmu_(an, 11, varianceAngle=1e-4)
    jg.solveSE_(an)
    assert an.dims()["refactorizations"] == 1 and all(r.size == 0 for r in jg.removed(an).rows) and np.all(an.status == 0)
    clusters = [setting(name)[2][3 + s] for s in range(3)]
    z = readings_of(name, 3, 13, clusters=clusters)
    fresh = jg.dcStateEstimation(an.monitoring, batch=3)
    for a in (an, fresh):
        jg.setReadings_(a, z)
        for k in range(2):
            remove(jg, a, {s: clusters[s][k] for s in range(3)})
        jg.solveSE_(a)
    checked(jg, name, an, [c[:2] for c in clusters], what="after the update")
    assert an.dims()["refactorizations"] == 1 and fresh.dims()["refactorizations"] == 0
    assert np.array_equal(an.voltage.angle, fresh.voltage.angle) and np.array_equal(an.objective, fresh.objective)
    assert np.array_equal(jg.normalizedResidual(an), jg.normalizedResidual(fresh))
    a, b = jg.residualTest_(an, threshold=1e300), jg.residualTest_(fresh, threshold=1e300)
    assert np.array_equal(a.index, b.index) and np.array_equal(a.maxNormalizedResidual, b.maxNormalizedResidual)
    fresh.close()
    an.close()
