"""Batched PMU least-absolute-value estimation on the device (csrc/jg_pmulav.hip on the iteration of csrc/jg_dclav.hip, without a fixed state) against the
numpy restatement of the same method (tests/pmulav_reference.py: same statements, dense, one lane) and against scipy's HiGHS on the same LP.

What is compared with what.  Voltages go against the power-flow state only on the lanes that tests/test_pmulav_host.py shows on the CPU to have it as
their optimum (exact readings, 1 to 3 gross phasor errors on the devices of GROSS_SEED).  On noisy lanes voltages, duals and iteration counts go against
the restatement: same method, same iterates.

Tolerances.
  KNOWN_TOL       1e-8, the reference's own atol for this estimator (test/utility/utility.jl:298-300).
  OBJECTIVE_TOL   restatement against linprog, from tests/test_pmulav_host.py (10 x the largest deviation measured on the CPU).
  DEVICE_*        device against restatement: the same arithmetic in another summation order, amplified by the conditioning of H' Q H near the solution
                  where Q spans many decades.  Measured on one MI355X, the largest over the lanes of test_device_against_restatement (printed by it) and
                  over ten more seeds of the same four kinds of lanes on the same two grids (worst(...) below run with seeds 8 .. 17): voltage 3.64e-11
                  (magnitude in per unit and angle in rad, whichever is larger; 6.7e-16 / 3.64e-11 on the test's own lanes of the two grids),
                  objective 3.14e-14 relative to 1 + objective, duals of the noisy lanes 4.04e-12.  On the lanes WITHOUT noise (exact, gross errors
                  only) every clean row is fitted exactly, the LP is degenerate there and its dual is not unique on those rows: the two iterations end
                  at different interior points of the dual face, 6.96e-5 apart at most (MEASURED_DUAL_CLEAN), and are held to that, apart from the
                  noisy lanes' bound.  The bounds are 10 x the largest.  A measured voltage deviation above 1e-9 is a defect, not a tolerance.
  RECT_TOL        k_pmu_rect against numpy's m cos(a), m sin(a), relative to the magnitude: 10 x the measured 2.13e-16 (0.96 ulp); anything above 4 ulp
                  is a defect.
  FLOW_TOL        the branch and bus quantities against numpy on the device's own voltages, relative to the largest flow: 10 x the measured 4.93e-15.
  WEIGHTED_*      weighted=True against the restatement on the rows scaled by hand (scales of 1e2 .. 1e3 from variances of 1e-6 .. 1e-4): voltages, the
                  objective relative to 1 + objective, the scaled residual relative to the largest scaled reading, rho in per unit; 10 x the measured
                  MEASURED_WEIGHTED (printed by test_weighted: 6.67e-16, 3.09e-12, 2.31e-15, 3.69e-15 on one MI355X).
  Duals           beside the comparison, every lane's dual is held to the LP's own certificate: |y| < 1, |H'y| <= tol max_j sum_i |H_ij| and
                  |z'y - objective| <= 2 gap + 2 m |rp| + |x|_1 |rd| at the stopping tests' bounds (derived in tests/test_dclav_host.py), so two duals
                  that differ on a degenerate face are both shown feasible and worth the same objective.
  Iteration counts are equal; bitwise claims are np.array_equal."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import pmulav_reference as P
from test_pmulav_host import KNOWN_TOL, OBJECTIVE_TOL, TOL, grid, gross_lanes, mixed_readings, monitoring_of

pytestmark = pytest.mark.gpu

MEASURED_VOLTAGE, MEASURED_OBJECTIVE, MEASURED_DUAL, MEASURED_DUAL_CLEAN = 3.64e-11, 3.14e-14, 4.04e-12, 6.96e-5
MEASURED_RECT, MEASURED_FLOW = 2.13e-16, 4.93e-15
DEVICE_VOLTAGE, DEVICE_OBJECTIVE, DEVICE_DUAL, DEVICE_DUAL_CLEAN = 10 * MEASURED_VOLTAGE, 10 * MEASURED_OBJECTIVE, 10 * MEASURED_DUAL, 10 * MEASURED_DUAL_CLEAN
RECT_TOL, FLOW_TOL = 10 * MEASURED_RECT, 10 * MEASURED_FLOW
MEASURED_WEIGHTED = dict(voltage=6.67e-16, objective=3.09e-12, residual=2.31e-15, rho=3.69e-15)
WEIGHTED_TOL = {k: 10 * v for k, v in MEASURED_WEIGHTED.items()}
ULP = 2.0 ** -52
CASES = ["case14test", "case30test"]


def lav(jg):
    return jg.pmulavstateestimation


def handle(jg, case, batch, pmus=None, t=None, **kw):
    t0, _, _, pmus0 = grid(case)[:4]
    return jg.pmuLavStateEstimation(monitoring_of(jg, t0 if t is None else t, pmus0 if pmus is None else pmus), batch=batch, **kw)


def solve(jg, an, mag, ang):
    lav(jg).setReadings_(an, mag, ang)
    lav(jg).solve_(an)
    return (np.atleast_2d(an.voltage.magnitude).copy(), np.atleast_2d(an.voltage.angle).copy(), np.atleast_1d(an.status).copy(),
            np.atleast_1d(an.iterations).copy())


_SINGLE = {}


def singles(jg, case):
    """the four kinds of mixed_readings, each solved alone in a batch of 1: magnitude, angle, dual, objective, iterations"""
    if case not in _SINGLE:
        mag, ang = mixed_readings(case, 4)
        out = []
        for k in range(4):
            an = handle(jg, case, 1)
            solve(jg, an, mag[k][None, :], ang[k][None, :])
            out.append((an.voltage.magnitude.copy(), an.voltage.angle.copy(), an.dual.copy(), an.objective, an.iterations))
            an.close()
        _SINGLE[case] = out
    return _SINGLE[case]


def certificate(H, z, on, y, objective, gap, x):
    """y is dual feasible up to the stopping tests and certifies the objective (bounds: tests/test_dclav_host.py, test_the_restatements_certificate)"""
    m = int(on.sum())
    gap_max, rp_max, rd_max = TOL * (1.0 + objective), TOL * (1.0 + np.abs(z[on]).max()), TOL * np.abs(H[on]).sum(axis=0).max()
    assert np.abs(y).max() < 1.0 and (y[~on] == 0.0).all()
    assert np.abs(H.T @ y).max() <= rd_max * (1.0 + 1e-6)          # (numpy's H'y is the iteration's own up to 1e-8 of the bound)
    assert gap <= gap_max
    assert abs(z @ y - objective) <= 2.0 * gap_max + 2.0 * m * rp_max + np.abs(x).sum() * rd_max


def worst(jg, case, seed, count=8):
    """device against restatement over `count` mixed lanes of `seed`: the largest voltage, objective and dual deviation, the duals apart for the noisy
    lanes and for the lanes without noise; iteration counts must be equal"""
    t, vm, va, pmus, H, _, on = grid(case)
    mag, ang = mixed_readings(case, count, seed)
    an = handle(jg, case, count)
    dm, da, st, it = solve(jg, an, mag, ang)
    assert (st == 0).all()
    wv = wo = wd = wc = 0.0
    for s in range(4):                                              # lanes s + 4 repeat lane s
        ref = P.pmulav_ipm(H, P.pmulav_rows(t, pmus, mag[s], ang[s])[1], on, tolerance=TOL)
        rm, ra = P.polar(ref.x)
        v = max(np.abs(dm[s] - rm).max(), np.abs(da[s] - ra).max())
        o, d = abs(an.objective[s] - ref.objective) / (1.0 + ref.objective), np.abs(an.dual[s] - ref.y).max()
        print(case, "seed", seed, "lane", s, "iterations", it[s], ref.iterations, "voltage", v, "objective", o, "dual", d)
        assert it[s] == ref.iterations and ref.status == 0
        assert np.array_equal(dm[s + 4], dm[s]) and np.array_equal(an.dual[s + 4], an.dual[s])
        certificate(H, P.pmulav_rows(t, pmus, mag[s], ang[s])[1], on, an.dual[s], an.objective[s], an.gap[s], np.r_[dm[s] * np.cos(da[s]), dm[s] * np.sin(da[s])])
        certificate(H, P.pmulav_rows(t, pmus, mag[s], ang[s])[1], on, ref.y, ref.objective, ref.gap, ref.x)
        wv, wo = max(wv, v), max(wo, o)
        wd, wc = (max(wd, d), wc) if s >= 2 else (wd, max(wc, d))
    an.close()
    return wv, wo, wd, wc


@pytest.mark.parametrize("case", CASES)
def test_known_answers(jg, case):
    """exact readings of the power-flow state give its magnitudes and angles; so do 1, 2 and 3 gross phasor errors (CPU-verified lanes), at the cost of
    exactly those errors; suspect_ at half the smallest injected error flags the corrupted devices and no others"""
    t, vm, va, pmus, H, z0, on = grid(case)
    mags, angs, devs = gross_lanes(case)
    an = handle(jg, case, 4)
    dm, da, st, it = solve(jg, an, mags, angs)
    print(case, "iterations", it, "worst", [float(max(np.abs(dm[k] - vm).max(), np.abs(da[k] - va).max())) for k in range(4)])
    assert (st == 0).all() and it[0] <= 3
    smallest = np.inf
    for k in range(4):
        z = P.pmulav_rows(t, pmus, mags[k], angs[k])[1]
        assert np.abs(dm[k] - vm).max() <= KNOWN_TOL and np.abs(da[k] - va).max() <= KNOWN_TOL, k
        assert abs(an.objective[k] - np.abs(z - z0).sum()) <= OBJECTIVE_TOL, k
        if devs[k].size:
            smallest = min(smallest, P.rho(z - z0, on)[devs[k]].min())
    lav(jg).suspect_(an, 0.5 * smallest)
    for k in range(4):
        assert np.array_equal(an.suspect[k], devs[k]) and an.suspectCount[k] == k, k
        if k:
            assert an.worst[k] in devs[k] and an.rho[k][an.worst[k]] == an.rho[k].max()
    an.close()


@pytest.mark.parametrize("case", CASES)
def test_device_against_restatement(jg, case):
    wv, wo, wd, wc = worst(jg, case, 7)
    print(case, "largest: voltage", wv, "objective", wo, "dual", wd, "dual of the lanes without noise", wc)
    assert wv <= 1e-9                                               # above that: a defect to investigate, not a tolerance to adopt
    assert wv <= DEVICE_VOLTAGE and wo <= DEVICE_OBJECTIVE and wd <= DEVICE_DUAL and wc <= DEVICE_DUAL_CLEAN


def test_batch_independence(jg):
    """130 lanes, three groups: exact, gross-only and noisy lanes interleaved finish at different iterations; every lane is bitwise what it is when solved
    alone in a batch of 1, and the group that finishes first leaves the launches"""
    case = "case14test"
    mag, ang = mixed_readings(case, 130)
    one = singles(jg, case)
    assert len({one[k][4] for k in range(4)}) >= 3
    an = handle(jg, case, 130)
    dm, da, st, it = solve(jg, an, mag, ang)
    assert (st == 0).all()
    for s in range(130):
        m, a, y, o, i = one[s % 4]
        assert it[s] == i and np.array_equal(dm[s], m) and np.array_equal(da[s], a) and np.array_equal(an.dual[s], y) and an.objective[s] == o, s
    assert an.dims()["lastIterations"] == max(one[k][4] for k in range(4))
    # a whole group of exact lanes between two noisy groups finishes first
    order = np.r_[np.full(64, 2), np.full(64, 0), np.full(2, 3)]
    dm, da, st, it = solve(jg, an, mag[order], ang[order])
    for s in (0, 63, 64, 127, 128, 129):
        m, a, y, o, i = one[order[s]]
        assert it[s] == i and np.array_equal(dm[s], m) and np.array_equal(da[s], a) and np.array_equal(an.dual[s], y), s
    an.close()


def test_polar_to_rectangular(jg):
    """k_pmu_rect: the solve's input rows, read back as the residual of a zero-iteration solve from a zero initial point (r = z - H 0)"""
    case = "case14test"
    pmus = grid(case)[3]
    n, Pn, T = 14, pmus.kind.size, 70
    rng = np.random.default_rng(5)
    mag = rng.uniform(0.1, 3.0, (T, Pn))
    ang = rng.uniform(-np.pi, np.pi, (T, Pn))
    ang[:, :8] = np.linspace(-np.pi, np.pi, 8, endpoint=False)[None, :] + 0.1          # all four quadrants in every lane
    mag[3, 5] = mag[69, 0] = 0.0
    ang[7, 2] = ang[64, 9] = np.pi
    ang[8, 2] = -np.pi
    ang[9, 3] = 0.0
    an = handle(jg, case, T, iteration=0)
    lav(jg).setInitialPoint_(an, NS(voltage=NS(magnitude=np.zeros(n), angle=np.zeros(n))))
    lav(jg).setReadings_(an, mag, ang)
    lav(jg).solve_(an)
    assert (np.atleast_1d(an.iterations) == 0).all()
    r = an.residual
    err = np.maximum(np.abs(r[:, 0::2] - mag * np.cos(ang)), np.abs(r[:, 1::2] - mag * np.sin(ang)))
    rel = np.where(mag > 0.0, err / np.where(mag > 0.0, mag, 1.0), err)
    print("k_pmu_rect: largest deviation relative to the magnitude", rel.max(), "=", rel.max() / ULP, "ulp")
    assert r[3, 10] == 0.0 and r[3, 11] == 0.0 and r[69, 0] == 0.0 and r[69, 1] == 0.0
    assert r[7, 4] == -mag[7, 2] and r[9, 6] == mag[9, 3] and r[9, 7] == 0.0
    assert rel.max() <= 4 * ULP
    assert rel.max() <= RECT_TOL
    an.close()


def test_status_pairing(jg):
    """a PMU with only its magnitude channel off, one with only its angle channel off and one with both off leave with both rows: the estimate is that of
    a set built without them (another gain pattern, so within DEVICE_*); status 0 and back to 1 on a live handle returns the first result to the bit"""
    case = "case14test"
    t, vm, va, pmus, H, _, on = grid(case)
    mag, ang = mixed_readings(case, 4)
    off = [3, 20, 21]
    pm = P.pmu_table(t, vm, va)
    pm.status_magnitude[3] = 0
    pm.status_angle[20] = 0
    pm.status_magnitude[21] = pm.status_angle[21] = 0
    an = handle(jg, case, 4, pmus=pm)
    assert an.method.inservice == 2 * (pmus.kind.size - 3)
    got = solve(jg, an, mag, ang)
    assert (got[2] == 0).all() and (an.residual[:, [6, 7, 40, 41, 42, 43]] == 0.0).all()
    keep = np.setdiff1d(np.arange(pmus.kind.size), off)
    cut = NS(**{k: getattr(pmus, k)[keep] for k in ("kind", "index", "magnitude", "angle", "status_magnitude", "status_angle")})
    other = handle(jg, case, 4, pmus=cut)
    ref = solve(jg, other, mag[:, keep], ang[:, keep])
    assert np.array_equal(got[3], ref[3])
    assert np.abs(got[0] - ref[0]).max() <= DEVICE_VOLTAGE and np.abs(got[1] - ref[1]).max() <= DEVICE_VOLTAGE
    assert np.abs(np.atleast_1d(an.objective) - np.atleast_1d(other.objective)).max() <= DEVICE_OBJECTIVE * (1.0 + np.max(other.objective))
    other.close()
    an.close()
    live = handle(jg, case, 4)
    first = solve(jg, live, mag, ang)
    dual = live.dual.copy()
    state = lambda: (np.array(live.voltage.magnitude), np.array(live.voltage.angle), np.array(live.status), np.array(live.iterations))
    lav(jg).updatePmu_(live, 12, status=0)
    lav(jg).updatePmu_(live, 30, statusAngle=0)
    lav(jg).solve_(live)                                            # no setReadings_ in between: a status change leaves the lanes' readings alone
    gone = state()
    assert live.method.inservice == 2 * (pmus.kind.size - 2) and not np.array_equal(gone[0], first[0])
    lav(jg).updatePmu_(live, 12, status=1)
    lav(jg).updatePmu_(live, 30, statusAngle=1)
    lav(jg).solve_(live)
    again = state()
    assert all(np.array_equal(a, b) for a, b in zip(again, first)) and np.array_equal(live.dual, dual)
    live.close()


def test_unobservable(jg):
    """bus 8 of case14test hangs on bus 7 alone: with every PMU that touches it switched off no in-service row touches its two states -- every lane has
    status 1 and NaN voltages; switched back on, the handle solves as before"""
    case = "case14test"
    t, vm, va, pmus, H, _, on = grid(case)
    mag, ang = mixed_readings(case, 4)
    an = handle(jg, case, 4)
    first = solve(jg, an, mag, ang)
    touch = np.flatnonzero((H[0::2, 7] != 0.0) | (H[0::2, 14 + 7] != 0.0) | (H[1::2, 7] != 0.0) | (H[1::2, 14 + 7] != 0.0))
    assert touch.size == 3                                          # its bus PMU and both ends of branch 7 - 8
    for i in touch:
        lav(jg).updatePmu_(an, int(i) + 1, status=0)
    dm, da, st, it = solve(jg, an, mag, ang)
    assert (st == 1).all() and np.isnan(dm).all() and np.isnan(da).all() and np.isnan(an.objective).all() and (it == 0).all()
    for i in touch:
        lav(jg).updatePmu_(an, int(i) + 1, status=1)
    again = solve(jg, an, mag, ang)
    assert all(np.array_equal(a, b) for a, b in zip(again, first))
    an.close()


def test_power_current_and_suspects(jg):
    """70 noisy lanes on case14test with branch 1 out of service: the device's branch and bus quantities against numpy on the device's own voltages, exact
    zeros on the branches out of service, and the suspect tables against numpy on the device's own residuals"""
    case = "case14test"
    t0, vm, va = grid(case)[:3]
    t = dict(t0)
    t["br_status"] = np.array(t0["br_status"]).copy()
    t["br_status"][0] = 0
    pmus = P.pmu_table(t, vm, va)                                   # (the readings need not fit the changed grid: they are noisy anyway)
    T, Pn = 70, pmus.kind.size
    rng = np.random.default_rng(9)
    mag = pmus.magnitude[None, :] + 1e-2 * rng.standard_normal((T, Pn))
    ang = pmus.angle[None, :] + 1e-2 * rng.standard_normal((T, Pn))
    for s in range(0, T, 3):
        d = rng.choice(Pn, 1 + s % 3, replace=False)
        mag[s, d] *= 1.5
        ang[s, d] += 0.5
    an = handle(jg, case, T, pmus=pmus, t=t)
    lav(jg).setReadings_(an, mag, ang)
    lav(jg).stateEstimation_(an, power=True, current=True)
    assert (an.status == 0).all()
    V = an.voltage.magnitude * np.exp(1j * an.voltage.angle)
    f = P.flows(t, V)
    scale = max(np.abs(f.from_).max(), np.abs(f.to).max())
    pw, cu = an.power, an.current
    dev = lambda ns, a, b: ns.__dict__[a] + 1j * ns.__dict__[b]
    worst_flow = 0.0
    for name, got, ref in (("from", dev(pw.from_, "active", "reactive"), f.from_), ("to", dev(pw.to, "active", "reactive"), f.to),
                           ("series", dev(pw.series, "active", "reactive"), f.series), ("charging", dev(pw.charging, "active", "reactive"), f.charging),
                           ("injection", dev(pw.injection, "active", "reactive"), f.injection),
                           ("from current", cu.from_.magnitude * np.exp(1j * cu.from_.angle), np.where(f.on, f.fromCurrent, 0.0)),
                           ("to current", cu.to.magnitude * np.exp(1j * cu.to.angle), np.where(f.on, f.toCurrent, 0.0)),
                           ("series current", cu.series.magnitude * np.exp(1j * cu.series.angle), np.where(f.on, f.seriesCurrent, 0.0))):
        e = np.abs(got - ref).max() / scale
        print("flows:", name, "largest deviation relative to the largest flow", e)
        worst_flow = max(worst_flow, e)
    print("flows: largest", worst_flow)
    gone = np.flatnonzero(~f.on)
    assert gone.size == 3 and 0 in gone
    for ns in (pw.from_, pw.to, pw.series, pw.charging):
        assert (ns.active[:, gone] == 0.0).all() and (ns.reactive[:, gone] == 0.0).all()
    for ns in (cu.from_, cu.to, cu.series):
        assert (ns.magnitude[:, gone] == 0.0).all() and (ns.angle[:, gone] == 0.0).all()
    I = np.conj(f.injection / V)
    assert np.abs(cu.injection.magnitude - np.abs(I)).max() <= 1e-12 * np.abs(I).max()
    sh = np.abs(V) ** 2 * np.conj(np.asarray(t["bus_gs"]) + 1j * np.asarray(t["bus_bs"]))
    assert np.abs(dev(pw.shunt, "active", "reactive") - sh).max() <= 1e-14 * max(1.0, np.abs(sh).max())
    sup = f.injection + (np.asarray(t["bus_pd"], dtype=np.float64) + 1j * np.asarray(t["bus_qd"], dtype=np.float64))[None, :]      # acAnalysis.jl:240-241
    assert np.abs(dev(pw.supply, "active", "reactive") - sup).max() <= FLOW_TOL * scale and np.abs(sup).max() > 0.1
    assert np.array_equal(pw.supply.active, pw.injection.active + an.system.bus.demand.active[None, :]) and not hasattr(pw, "generator")
    assert not np.signbit(pw.charging.reactive[:, gone]).any() and not np.signbit(pw.from_.reactive[:, gone]).any()
    assert worst_flow <= FLOW_TOL
    # suspects
    thr = 0.02
    lav(jg).suspect_(an, thr)
    on = np.ones(2 * Pn, dtype=bool)
    rho = P.rho(an.residual, on)
    assert np.abs(an.rho - rho).max() <= 4 * ULP * rho.max()
    assert np.array_equal(an.suspectCount, (rho > thr).sum(axis=1)) and np.array_equal(an.worst, rho.argmax(axis=1))
    assert all(np.array_equal(an.suspect[s], np.flatnonzero(rho[s] > thr)) for s in range(T))
    assert an.suspectCount.max() >= 3 and an.suspectCount.min() <= 1
    an.close()


def test_coefficient_equals_the_wls_models(jg):
    """the LAV model's H is pmuStateEstimation(monitoring).coefficient as scipy.sparse reads it: same pattern, values within 1e-12 relative"""
    import scipy.sparse as sp
    for case in CASES:
        t, vm, va, pmus = grid(case)[:4]
        mon = monitoring_of(jg, t, pmus)
        wls = jg.pmuStateEstimation(mon)
        lavm = jg.pmuLavModel(mon)
        mats = []
        for c in (wls.coefficient, lavm.coefficient):
            A = sp.csc_matrix((np.asarray(c.nzval, dtype=np.float64).reshape(-1), c.rowval - 1, c.colptr - 1), shape=(2 * pmus.kind.size, 2 * vm.size))
            A.eliminate_zeros()
            A.sort_indices()
            mats.append(A)
        assert np.array_equal(mats[0].indptr, mats[1].indptr) and np.array_equal(mats[0].indices, mats[1].indices)
        assert np.abs(mats[0].data - mats[1].data).max() <= 1e-12 * np.abs(mats[0].data).max()
        wls.close()


def test_initial_point(jg):
    """a start from the power-flow state with exact readings finishes within 3 iterations; a start from a DC analysis keeps the magnitudes"""
    case = "case14test"
    t, vm, va, pmus = grid(case)[:4]
    an = handle(jg, case, 1)
    lav(jg).setInitialPoint_(an, NS(voltage=NS(magnitude=vm, angle=va)))
    dm, da, st, it = solve(jg, an, pmus.magnitude[None, :], pmus.angle[None, :])
    assert st[0] == 0 and it[0] <= 3 and np.abs(dm[0] - vm).max() <= KNOWN_TOL and np.abs(da[0] - va).max() <= KNOWN_TOL
    dc = jg.dcPowerFlow(an.system)
    jg.dcpowerflow.solve_(dc)
    before = np.array(an.voltage.magnitude)
    lav(jg).setInitialPoint_(an, dc)
    assert np.array_equal(an.voltage.magnitude, before) and np.array_equal(an.voltage.angle, dc.voltage.angle)
    dm, da, st, it = solve(jg, an, pmus.magnitude[None, :], pmus.angle[None, :])
    assert st[0] == 0 and np.abs(dm[0] - vm).max() <= KNOWN_TOL and np.abs(da[0] - va).max() <= KNOWN_TOL
    pf = jg.newtonRaphson(jg.powerSystem(t))                        # a solved AC analysis gives magnitude and angle
    jg.powerFlow_(pf)
    lav(jg).setInitialPoint_(an, pf)
    assert np.array_equal(an.voltage.magnitude, pf.voltage.magnitude) and np.array_equal(an.voltage.angle, pf.voltage.angle)
    dm, da, st, it = solve(jg, an, pmus.magnitude[None, :], pmus.angle[None, :])
    assert st[0] == 0 and it[0] <= 3 and np.abs(dm[0] - vm).max() <= KNOWN_TOL
    pf.close()
    pf4 = jg.newtonRaphson(jg.powerSystem(t), batch=4)              # a batched source gives lane s its own lane
    jg.powerFlow_(pf4)
    an4 = handle(jg, case, 4)
    lav(jg).setInitialPoint_(an4, pf4)
    assert np.array_equal(an4.voltage.magnitude, pf4.voltage.magnitude)
    mag4, ang4 = mixed_readings(case, 4)
    got = solve(jg, an4, mag4, ang4)
    assert (got[2] == 0).all() and got[3][0] <= 3
    with pytest.raises(ValueError):
        lav(jg).setInitialPoint_(an, pf4)                           # four lanes into a batch of one
    pf4.close()
    an4.close()
    lav(jg).setInitialPoint_(an)                                    # the system's bus voltages
    assert np.array_equal(an.voltage.magnitude, np.asarray(an.system.bus.voltage.magnitude, dtype=np.float64))
    assert solve(jg, an, pmus.magnitude[None, :], pmus.angle[None, :])[2][0] == 0
    dc.close()
    an.close()


def test_weighted(jg):
    """weighted=True with unequal variances per device and channel: the estimate, the objective and the residual are those of the rows scaled by
    1 / sigma of the stored readings' rectangular variances (restated here from the polar variances), rho stays in per unit"""
    case = "case14test"
    t, vm, va, pmus, H, _, on = grid(case)
    Pn = pmus.kind.size
    rng = np.random.default_rng(21)
    var_m, var_a = 10.0 ** rng.uniform(-6.0, -4.0, Pn), 10.0 ** rng.uniform(-6.0, -4.0, Pn)
    mon = jg.measurement(jg.powerSystem(t))
    for i in range(Pn):
        where = {0: "bus", 1: "from_", 2: "to"}[int(pmus.kind[i])]
        jg.addPmu_(mon, **{where: int(pmus.index[i])}, magnitude=float(pmus.magnitude[i]), angle=float(pmus.angle[i]), varianceMagnitude=float(var_m[i]),
                   varianceAngle=float(var_a[i]))
    s_, c_ = np.sin(pmus.angle), np.cos(pmus.angle)                 # variancePmu of the stored readings (equations.jl:576-600), uncorrelated
    vre, vim = var_m * c_ ** 2 + var_a * (pmus.magnitude * s_) ** 2, var_m * s_ ** 2 + var_a * (pmus.magnitude * c_) ** 2
    scale = 1.0 / np.sqrt(np.stack([vre, vim], axis=1).reshape(-1))
    assert scale.min() >= 50.0 and np.abs(scale[0::2] / scale[1::2] - 1.0).max() > 0.5
    mag, ang = mixed_readings(case, 4)
    an = jg.pmuLavStateEstimation(mon, batch=4, weighted=True)
    dm, da, st, it = solve(jg, an, mag, ang)
    assert (st == 0).all()
    lav(jg).suspect_(an, 0.05)
    w = dict(voltage=0.0, objective=0.0, residual=0.0, rho=0.0)
    Hs = H * scale[:, None]
    for s in range(4):
        z = P.pmulav_rows(t, pmus, mag[s], ang[s])[1]
        ref = P.pmulav_ipm(Hs, z * scale, on, tolerance=TOL)
        rm, ra = P.polar(ref.x)
        assert ref.status == 0 and it[s] == ref.iterations, s
        r = an.residual[s]
        w["voltage"] = max(w["voltage"], np.abs(dm[s] - rm).max(), np.abs(da[s] - ra).max())
        w["objective"] = max(w["objective"], abs(an.objective[s] - ref.objective) / (1.0 + ref.objective))
        w["residual"] = max(w["residual"], np.abs(r - ref.residual).max() / np.abs(z * scale).max())
        w["rho"] = max(w["rho"], np.abs(an.rho[s] - P.rho(z - H @ ref.x, on)).max())
        assert abs(np.abs(r).sum() - an.objective[s]) <= 1e-12 * (1.0 + an.objective[s])                # the objective is that of the scaled rows
        assert np.abs(an.rho[s] - np.hypot(r[0::2] / scale[0::2], r[1::2] / scale[1::2])).max() <= 4 * ULP * max(an.rho[s].max(), 1.0)
        assert np.array_equal(an.suspect[s], np.flatnonzero(an.rho[s] > 0.05)) and an.suspectCount[s] == an.suspect[s].size
    print("weighted: largest", w)
    plain = handle(jg, case, 4)
    assert not np.array_equal(solve(jg, plain, mag, ang)[0][2], dm[2])                                  # the weights do move the estimate
    plain.close()
    an.close()
    for k in w:
        assert w[k] <= WEIGHTED_TOL[k], (k, w[k])
