"""The lane-valued factor's schedule and the robust estimators' references on the (grid, measurement set) pairs of tests/dc_lane_grids.py, without a GPU.

Four things are held here, so that device tests on these pairs compare the device with something sound:
the pairs TOGETHER reach every class of LANE_COVERAGE (asserted per class and printed, so that a change of the ordering that drops one is named); the
schedule of every pair's gain pattern is race-free and solves H'QH (the numpy replay with "final" flags against a dense solve); the restatements
dclav_reference.lav_ipm and dchuber_reference.huber_ipm are usable as references on every lane the device is compared on (status 0, LAV against
linprog, Huber's certificate, no verdict near its bound); and numpy's f64 solve of H'QH, the reference's reference, is not the limit of the factor
test's bound cond(G) x 2^-52 (a dense solve in extended precision)."""
import numpy as np
import pytest

import dc_grids as G
import dc_lane_grids as D
import dchuber_reference as U
import dclav_reference as L
from test_dc_grids_cpu import REPLAY_TOL
from test_dchuber_host import CERTIFICATE_TOL
from test_dclav_host import OBJECTIVE_TOL

ALL = D.PAIRS + D.EDGE_PAIRS
IDS = [f"{n}/{D.label(k)}" for n, k in ALL]


def test_the_pairs_reach_every_class(jg):
    """Coverage is asserted, not assumed.  If a change of the ordering drops a class, this names it: add a pair or a family that reaches it (choose it
    with dc_lane_grids.lane_levels on the CPU); do not delete the assertion."""
    reached = {}
    for name, kind in ALL + [("one bus", "flows")]:
        su = D.setup(name, kind, jg)
        for c in D.lane_classes(su.levels(jg), su.n, su.m):
            reached.setdefault(c, []).append(f"{name}/{D.label(kind)}")
    for c in D.LANE_COVERAGE:
        print(f"{c}: {', '.join(reached.get(c, [])) or 'NOT REACHED'}")
    missing = [c for c in D.LANE_COVERAGE if c not in reached]
    assert not missing, missing
    assert 12 <= len(D.PAIRS) <= 16
    # the classes of the sweep kernels come from PAIRS alone (the factor tests run on these)
    swept = set()
    for name, kind in D.PAIRS:
        su = D.setup(name, kind, jg)
        swept |= D.lane_classes(su.levels(jg), su.n, su.m)
    assert not [c for c in G.COVERAGE + D.LANE_COVERAGE[len(G.COVERAGE):len(G.COVERAGE) + 10] if c not in swept]


def test_the_sets_are_what_they_are_called(jg):
    for name, kind in ALL:
        su = D.setup(name, kind, jg)
        on = int((np.asarray(su.t["br_status"]) == 1).sum())
        nb = np.asarray(su.t["br_from"]).size
        if kind == "full":
            assert su.m == 2 * su.n + 2 * nb
        elif kind == "flows":
            assert su.m == on + 1
        elif kind == "tree":
            assert su.m == su.n and int(su.on.sum()) - 1 == su.n - 1          # n - 1 flow meters and the slack's PMU: just determined
            assert np.linalg.matrix_rank(su.H) == su.n - 1
        else:
            assert su.m == kind[1]
        assert np.linalg.matrix_rank(su.H) == su.n - 1, "a bus is not observed"
        assert np.abs(su.z - su.H @ (su.th - su.va)).max() <= 1e-12              # exact readings of the DC power flow
    su = D.setup("star 71, leaf slack", "full", jg)
    assert su.pattern[1].size == 71 * 71                               # the full set on a star: the complete gain matrix


def test_lane_levels_is_sweep_levels_on_the_nodal_pattern(jg):
    """the generalisation changes nothing: on the nodal matrix's own pattern lane_levels gives what dc_grids.sweep_levels gives"""
    for name in ("ring 17", "mesh 8x8"):
        t = G.family(name, jg)
        s = jg.powerSystem({k: np.array(v) for k, v in t.items()})
        jg.dcModel_(s)
        B = s.model.dc.nodalMatrix
        a, b = D.lane_levels((B.colptr - 1, B.rowval - 1), jg), G.sweep_levels(t, jg)
        for key in b:
            assert np.array_equal(a[key], b[key]) if isinstance(b[key], np.ndarray) else a[key] == b[key], key
        assert a["factor"].sum() == a["entries"]


@pytest.mark.parametrize("name,kind", D.PAIRS, ids=IDS[:len(D.PAIRS)])
def test_the_schedule_replays_without_a_race_and_solves_the_gain(jg, name, kind):
    su = D.setup(name, kind, jg)
    _, rhs = D.factor_inputs(su, 1, seed=5)
    q = np.random.default_rng(5).uniform(1.0, 2.0, su.m)             # a weight of its own per row, no decades: REPLAY_TOL is the bound of a well-conditioned matrix
    x = D.replay_gain(su, q, rhs[0], jg)                             # raises ScheduleError on a term that reads a value that is not final
    ref = np.linalg.solve(D.gain(su.H, q, su.slack), rhs[0])
    dev = float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))
    print(name, D.label(kind), "replay against numpy's solve", dev, "condition", np.linalg.cond(D.gain(su.H, q, su.slack)))
    assert dev <= REPLAY_TOL


@pytest.mark.parametrize("name,kind", ALL, ids=IDS)
def test_the_restatements_are_usable_as_references(jg, name, kind):
    """conditions on the INPUTS: if a seed fails one, change the seed or the noise (dc_lane_grids.LANE_SEEDS), not the bound"""
    su = D.setup(name, kind, jg)
    for s, (z, ref, margins) in enumerate(D.lav_refs(su)):
        lp = L.lav_linprog(su.H, z, su.on, su.slack)
        print(name, D.label(kind), "LAV", s, "status", ref.status, "iterations", ref.iterations, "objective - linprog's", ref.objective - lp.objective,
              "last margin", margins[-1])
        assert ref.status == 0 and ref.iterations <= 50, s
        assert abs(ref.objective - lp.objective) <= OBJECTIVE_TOL, s
        assert D.fair(margins), (s, margins)
        if kind == "tree":
            # a just-determined set fits every reading but the slack's PMU, whose row is empty (the slack's angle is fixed)
            assert not su.H[-1].any() and abs(lp.objective - abs(z[-1])) <= OBJECTIVE_TOL
    for s, (z, ref) in enumerate(D.huber_refs(su)):
        c = U.huber_certificate(su.Hs, z / su.sigma * su.on, ref.theta, D.THRESHOLD)
        print(name, D.label(kind), "Huber", s, "status", ref.status, "iterations", ref.iterations, "certificate", c, "last margin", ref.margin)
        assert ref.status == 0 and ref.iterations <= 50, s
        assert D.fair(ref.margins), (s, ref.margins)
        assert c <= CERTIFICATE_TOL, s
    # the exact lanes: the power-flow angles, nothing to pay
    assert D.lav_refs(su)[0][1].objective <= OBJECTIVE_TOL and D.huber_refs(su)[0][1].objective <= 1e-12


ONE_BUS_READINGS = (0.0, 0.3, -2.0)


def test_the_restatements_are_usable_on_the_one_bus_grid(jg):
    """the slack alone: H has only the slack's zeroed column, hnorm = 0 and the dual test is 0 <= 0 on the device and in both restatements"""
    su = D.setup("one bus", "flows", jg)
    assert su.n == 1 and su.m == 1 and not su.H.any() and np.abs(su.H).sum(axis=0).max() == 0.0
    for z in ONE_BUS_READINGS:
        ref = L.lav_ipm(su.H, np.array([z]), su.on, su.slack, tolerance=D.TOL)
        print("one bus LAV", z, "status", ref.status, "iterations", ref.iterations, "margins", ref.margins)
        assert ref.status == 0 and ref.objective == abs(z) and ref.theta[0] == 0.0 and D.fair(ref.margins)
        ref = U.huber_ipm(su.Hs, np.array([z]), D.THRESHOLD, su.on, su.slack, tolerance=D.TOL)
        print("one bus Huber", z, "status", ref.status, "iterations", ref.iterations, "margins", ref.margins)
        assert ref.status == 0 and ref.theta[0] == 0.0 and D.fair(ref.margins)
        assert abs(ref.objective - U.huber_loss(np.array([z]), D.THRESHOLD)) <= 1e-12 * (1.0 + ref.objective)


@pytest.mark.parametrize("name,kind", [p for p in D.PAIRS if p[0] != "pegaseShaped 160"], ids=[i for i in IDS[:len(D.PAIRS)] if "160" not in i])
def test_the_reference_of_the_linear_solve_is_not_the_limit(jg, name, kind):
    """numpy's f64 solve of H'QH meets cond(G) x 2^-52, the bound the device is held to, against plain Gaussian elimination in numpy.longdouble, on the
    Q and the lanes of the factor test (twelve decades on every pair: none had to be reduced)"""
    su = D.setup(name, kind, jg)
    assert su.n <= 100
    q, rhs = D.factor_inputs(su, 65)
    worst = 0.0
    for s in D.FACTOR_LANES:
        Gm = D.gain(su.H, q[s], su.slack)
        ref = D.dense_longdouble(Gm, rhs[s])
        x = np.linalg.solve(Gm, rhs[s])
        err, bound = float(np.abs(x - ref).max() / np.abs(ref).max()), np.linalg.cond(Gm) * 2.0 ** -52
        worst = max(worst, err / bound)
        print(name, D.label(kind), s, "numpy against extended precision", err, "bound", bound)
        assert err <= bound, (s, err, bound)
    print(name, D.label(kind), "largest error / bound", worst)


def test_the_lane_that_breaks_is_traced(jg):
    """Readings of +-1e308 on two rows of case14test are finite (jg_dclav_set_readings takes them) but H'z overflows: the trace of the start in the
    device's operations gives NaN in every angle (the slack's included: its pattern entries hold 0, and 0 x NaN is NaN), so every residual is NaN,
    the start's mean residual is NaN and fmax leaves the floor: u = v = 1e-8 and Q = 5e7 on every row.  The FIRST gain is therefore finite and
    well-posed (no bad pivot at iteration 0, the step is applied); its right-hand side is NaN, so u, v, y and the angles are NaN afterwards, Q of
    iteration 1 is NaN, that factorisation sets the lane's flag, and the verdict of iteration 2 finds it: status 3 with iterations = 1 is what
    tests/test_dcrobust_grids_gpu.py asserts on the device"""
    import test_dclav_gpu as LG
    t, th, ms, H, z, on, slack, va = LG.grid("case14test")
    zz = LG.mixed_readings("case14test", 4)[1][2].copy()
    for row, value in D.BREAK_ROWS:
        zz[row] = value
    assert np.isfinite(zz).all()
    tr = D.lav_break_trace(t, ms, zz, jg)
    print("angles", tr["theta"], "objective", tr["objective"], "s", tr["s"], "Q", tr["q"].min(), tr["q"].max())
    assert np.isnan(tr["theta"]).all() and np.isnan(tr["r0"]).all() and np.isnan(tr["objective"])
    assert tr["s"] == L.START_FLOOR and (tr["q"] == 1.0 / (2.0 * L.START_FLOOR)).all() and not tr["zero_pivot_states"]
    Gm = D.gain(H, tr["q"], slack)
    assert np.isfinite(Gm).all() and np.linalg.cond(Gm) < 1e12      # iteration 0 factorises without a bad pivot
    # and the trace is the restatement's start on readings that do not overflow
    ok = LG.mixed_readings("case14test", 4)[1][2]
    tr = D.lav_break_trace(t, ms, ok, jg)
    ref = L.lav_ipm(H, ok, on, slack, iteration=0)
    assert np.abs(tr["theta"] - ref.theta).max() <= 1e-12 and np.abs(tr["r0"] - ref.residual).max() <= 1e-12
    # Huber (rows scaled by 1 / sigma; +-1e307 unscaled, so that the scaled readings stay finite): the same NaN start.  hub_clip(NaN, k / 2) is
    # fmin(fmax(NaN, -k / 2), k / 2) = -k / 2, the mean of |r1| is NaN and leaves the floor: u = v = 1e-8, y = -k / 2, Q = 1 / (1 + u / (1.5 k) + v / (0.5 k))
    # is finite on every row, the first gain factorises, and the same two iterations follow
    import test_dchuber_gpu as HG
    sigma = HG.grid("case14test")[7]
    zh = HG.unscaled("case14test", 4)[1][2].copy()
    for row, value in D.BREAK_ROWS:
        zh[row] = value / 10.0
    zs = zh * (1.0 / sigma)
    assert np.isfinite(zs).all() and np.abs(zs).max() >= 1e308
    tr = D.lav_break_trace(t, ms, zs, jg, scale=1.0 / sigma)
    assert np.isnan(tr["theta"]).all() and np.isnan(tr["r0"]).all()
    k, e = D.THRESHOLD, U.START_FLOOR
    assert np.isfinite(1.0 / (1.0 + e / (1.5 * k) + e / (0.5 * k)))
