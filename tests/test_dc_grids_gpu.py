"""The shared DC factor and its sweeps (csrc/jg_dc_sweep.hip) on the device, on the degenerate and seeded grids of tests/dc_grids.py: the families that
tests/test_dc_grids_cpu.py shows to reach every wave split of k_dc_chain, the hand-over to k_dc_sweep at 16 / 17 rows, wide levels of every residue
mod 4, list lengths of every residue mod DC_T, empty lists, a 70-term list, one- and two-bus systems, and the lane-group lists.

Tolerance of every lane-by-lane comparison: |got - ref| <= 1e-9 * max(1, max |ref|) against dc_reference.solve, which rebuilds and refactorises per
outage (tests/test_dc_gpu.py: TOL); the screens and the state estimation keep the bounds and the guards of their own reference modules.  Every worst
deviation is printed before it is asserted.  dc_reference.solve itself lies this close to a dense solve in numpy.longdouble (scaled the same way;
tests/test_dc_grids_cpu.py asserts 1e-11): one bus 0, two buses 2.9e-19, path 40 1.4e-14, star 33 6.2e-18, star 71 1.7e-15, complete 12 1.8e-18,
ring 17 1.2e-16, mesh 8x8 3.2e-16, binary tree 63 9.2e-15, two cliques 2.8e-17, comb 16 x 2 6.0e-15, pegaseShaped 72 3.7e-16."""
import numpy as np
import pytest

import dc_generator_reference as X
import dc_grids as G
import dc_pair_reference as P
import dc_reference as R
import dc_series_reference as S
import dcse_reference as E
from test_dc_gpu import TOL, check_lanes

pytestmark = pytest.mark.gpu

WITH_A_BRANCH = [k for k in G.FAMILIES if k != "one bus"]


def grid(jg, name):
    t = G.family(name, jg)
    return t, jg.powerSystem({k: np.array(v) for k, v in t.items()})


def worst(a, ref):
    return R.worst(a, ref) if np.size(ref) else 0.0


@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_single_solve(jg, name):
    t, s = grid(jg, name)
    an = jg.dcPowerFlow(s)
    jg.solve_(an)
    jg.power_(an)
    rth, rfr = R.solve(t)
    assert an.voltage.angle.shape == rth.shape and an.power.from_.active.shape == rfr.shape
    a, f = worst(an.voltage.angle, rth), worst(an.power.from_.active, rfr)
    d, lv = an.dims(), G.sweep_levels(t, jg)
    print(name, "angle", a, "flow", f, d)
    assert an.status == 0 and a <= TOL and f <= TOL
    # build_sweep's levels and launches are what the analysis predicts (dc_grids.launches restates the rule)
    assert d["forwardLevels"] == len(lv["forward"]) and d["backwardLevels"] == len(lv["backward"])
    assert d["sweepLaunches"] == len(lv["forwardLaunches"]) + len(lv["backwardLaunches"]) and d["sweepTerms"] == lv["terms"]
    if name == "one bus":                                            # the slack alone: its angle, no flow
        assert np.array_equal(an.voltage.angle, t["bus_va"]) and an.power.from_.active.size == 0 and d["branches"] == 0
    pw = R.power(t, rth)
    for key in ("injection", "supply", "generator"):
        assert worst(getattr(an.power, key).active, pw[key]) <= TOL, key
    an.close()


@pytest.mark.parametrize("name", WITH_A_BRANCH)
def test_n_minus_1_and_the_same_scenarios_in_other_lanes(jg, name):
    t, s = grid(jg, name)
    labels = np.r_[0, np.flatnonzero(s.branch.layout.status == 1) + 1]
    an = jg.contingencyAnalysis(s, labels, method="dc")
    is_bridge = jg.bridges(s)
    want = {i for i, lab in enumerate(labels) if lab and is_bridge[lab - 1]}
    got = {int(i) for i in np.flatnonzero(np.asarray(an.status) == 3)}
    assert got == want, (sorted(got), sorted(want))                 # status 3 exactly on the bridges
    assert set(np.unique(an.status)) <= {0, 3}
    if name in ("path 40", "star 33, hub slack", "star 71, leaf slack", "binary tree 63", "comb 16 x 2"):      # a tree: every branch but the parallel ones
        f, to = s.branch.layout.from_, s.branch.layout.to
        for i in set(range(1, labels.size)) - want:
            k = labels[i] - 1
            assert any(l != k and {f[l], to[l]} == {f[k], to[k]} for l in labels[1:] - 1), k
    if name == "two cliques":
        assert len(want) == 1
    print(name, "lanes", labels.size, "bridges", len(want))
    check_lanes(jg, t, an, labels, skip=want)
    th, fr = np.atleast_2d(an.voltage.angle).copy(), np.atleast_2d(an.power.from_.active).copy()
    st = np.atleast_1d(an.status).copy()
    an.close()
    for batch in (1, 63, 64, 65, 130):                               # a scenario must not depend on its lane or its lane group
        cyc = np.resize(labels, batch)
        b = jg.contingencyAnalysis(s, cyc, method="dc")
        jg.power_(b)
        first = np.arange(batch) % labels.size
        assert np.array_equal(np.atleast_1d(b.status), st[first]), batch
        assert np.array_equal(np.atleast_2d(b.voltage.angle), th[first], equal_nan=True), batch
        assert np.array_equal(np.atleast_2d(b.power.from_.active), fr[first], equal_nan=True), batch
        b.close()


def _at(s, ok, buses):
    """label of the first branch of `ok` (0-based indices) with an end at the first bus of `buses` (0-based, in order of preference) that has one"""
    for bus in buses:
        hit = [k for k in ok if s.branch.layout.from_[k] == bus + 1 or s.branch.layout.to[k] == bus + 1]
        if hit:
            return int(hit[0]) + 1, int(bus)
    raise AssertionError("no such branch")


@pytest.mark.parametrize("name", ["ring 17", "mesh 8x8", "pegaseShaped 160"])
def test_outages_at_the_ends_of_the_elimination_order(jg, name):
    """MODE 1 forms e_from - e_to from the lanes' outage buses: the slack's component is dropped, the first and the last pivot are the rows without a
    term below / above them"""
    t, s = grid(jg, name)
    perm = G.sweep_levels(t, jg)["perm"]
    lay = s.branch.layout
    ok = np.flatnonzero((lay.status == 1) & ~jg.bridges(s))
    pairs = {}
    for k in ok:
        pairs.setdefault(tuple(sorted((int(lay.from_[k]), int(lay.to[k])))), []).append(int(k))
    twins = [v for v in pairs.values() if len(v) >= 2]
    assert twins
    # (where the first or the last pivot is a leaf, its one branch is a bridge: the nearest pivot in the order that has a branch on a cycle)
    (at_slack, _), (at_last, last), (at_first, first) = _at(s, ok, [int(s.bus.layout.slack) - 1]), _at(s, ok, perm[::-1]), _at(s, ok, perm)
    labels = [at_slack, at_last, at_first, twins[0][0] + 1, twins[0][1] + 1, 0]
    an = jg.contingencyAnalysis(s, labels, method="dc")
    assert np.all(np.asarray(an.status) == 0)
    where = {int(b): i for i, b in enumerate(perm)}
    print(name, "labels", labels, "pivots of their buses: first", where[first], "last", where[last], "of", perm.size, "slack bus", int(s.bus.layout.slack))
    assert where[last] == perm.size - 1 and (where[first] == 0 or name == "pegaseShaped 160")
    check_lanes(jg, t, an, labels)
    an.close()


def test_lane_group_lists(jg):
    """Sweeps with right-hand sides of their own run over the lane groups that need them only: blockIdx.y goes through glist (groups 1 and 3 of 4 here)
    and glist2 (group 2 alone: the one lane with two outages)"""
    t, s = grid(jg, "pegaseShaped 160")
    rng = np.random.default_rng(160)
    ok = np.flatnonzero((s.branch.layout.status == 1) & ~jg.bridges(s)) + 1
    base_comp = P.base_components(t)
    k2, l2 = next((int(a), int(b)) for a in ok[5:] for b in ok[40:] if a != b and not P.islands(t, int(a) - 1, int(b) - 1, base_comp))
    labels = [0] * 200
    labels[70], labels[195], labels[130] = int(ok[3]), int(ok[17]), (k2, l2)
    base = s.bus.supply.active - s.bus.demand.active
    own = {lane: base * (1.0 + 0.1 * rng.standard_normal(base.size)) for lane in list(range(64, 128)) + list(range(192, 200))}

    def run(with_injections):
        an = jg.dcPowerFlow(s, batch=200)
        jg.setOutages_(an, labels)
        if with_injections:
            jg.setInjection_(an, np.array([own[i] for i in range(64, 128)]), scenario0=64)
            jg.setInjection_(an, np.array([own[i] for i in range(192, 200)]), scenario0=192)
        jg.solve_(an)
        jg.power_(an)
        return an
    a, b = run(True), run(False)
    assert a.dims()["ld"] == 256 and np.all(np.asarray(a.status) == 0) and np.all(np.asarray(b.status) == 0)
    single = [0 if isinstance(x, tuple) else x for x in labels]
    check_lanes(jg, t, a, single, injection=[own.get(i) for i in range(200)], skip=set(range(200)) - set(own))
    rest = np.array([i for i in range(200) if i not in own])
    assert np.array_equal(a.voltage.angle[rest], b.voltage.angle[rest]) and np.array_equal(a.power.from_.active[rest], b.power.from_.active[rest])
    assert not np.array_equal(a.voltage.angle[70], b.voltage.angle[70])
    check_lanes(jg, t, b, single, skip={130})
    rth, rfr = P.pair_solve(t, k2 - 1, l2 - 1)
    pa, pf = R.worst(b.voltage.angle[130], rth), R.worst(b.power.from_.active[130], rfr)
    print("lane 130, branches", (k2, l2), "angle", pa, "flow", pf)
    assert pa <= TOL and pf <= TOL
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["mesh 8x8", "binary tree 63"])
def test_a_lane_recovers_from_a_non_finite_injection(jg, name):
    """The padding of a term list multiplies the factor value 0 with the scratch's ZERO row (column n).  Any live row in its place goes unnoticed while
    the scratch holds finite numbers (0 x finite = 0); so a lane first leaves Inf and NaN in every row of its scratch -- an injection of Inf -- and
    is then solved again with finite injections: the answer must be the reference's, and the neighbouring lanes never see any of it"""
    t, s = grid(jg, name)
    k = int(np.flatnonzero((s.branch.layout.status == 1) & ~jg.bridges(s))[0]) + 1
    labels = [0, k, 0]
    base = s.bus.supply.active - s.bus.demand.active
    slack = int(s.bus.layout.slack) - 1
    bad, good = base.copy(), base * 1.05
    bad[(slack + 1) % base.size or 1] = np.inf                       # (not column 0, which marks a lane without injections of its own, and not the slack)
    an = jg.dcPowerFlow(s, batch=3)
    jg.setOutages_(an, labels)
    jg.setInjection_(an, np.array([bad]), scenario0=1)
    jg.solve_(an)
    rest = np.arange(base.size) != slack
    assert not np.isfinite(an.voltage.angle[1][rest]).any() and np.isfinite(an.voltage.angle[[0, 2]]).all()
    jg.setInjection_(an, np.array([good]), scenario0=1)
    jg.solve_(an)
    assert np.all(np.asarray(an.status) == 0)
    check_lanes(jg, t, an, labels, injection=[None, good, None])
    an.close()


@pytest.mark.parametrize("name", ["mesh 8x8", "pegaseShaped 72"])
def test_the_pair_screen_on_the_same_factor(jg, name):
    t, s = grid(jg, name)
    rating = P.rating_of(t)
    res = jg.dcPairScreen(s, rating=rating, dense=True)
    cand = res.candidates - 1
    nk = cand.size
    assert np.array_equal(res.candidates, jg.pairCandidates(s)) and res.totals["pairs"] == nk * (nk - 1) // 2
    Phi, f0, _ = P.sensitivities(t, cand)
    base = P.base_components(t)
    worst_dev, isl, rebuilt = 0.0, set(), 0
    for i in range(nk):
        for j in range(i + 1, nk):
            k, l = int(cand[i]), int(cand[j])
            if P.islands(t, k, l, base):                             # the graph oracle, not any linear algebra
                assert np.isnan(res.loading[i, j]), (k, l)
                isl.add((k + 1, l + 1))
                continue
            routes = [P.pair_flows(Phi, f0, cand, i, j)[0]]
            if (i * nk + j) % 23 == 0:                               # the rebuild route on a sample of the pairs, the restated formulas on all
                routes.append(P.pair_solve(t, k, l)[1])
                rebuilt += 1
            for fr in routes:
                assert fr is not None, (k, l)
                w, b, load = P.loading(fr, rating)
                scale = max(1.0, w)
                dev = abs(res.loading[i, j] - w) / scale
                assert dev <= TOL, (k, l, res.loading[i, j], w)
                gb = int(res.branch[i, j])
                assert gb == b or (gb >= 1 and abs(load[gb - 1] - w) <= TOL * scale), (k, l, gb, b)     # ties go to the lowest index
                worst_dev = max(worst_dev, dev)
    print(name, "pairs", res.totals["pairs"], "islanding", len(isl), "rebuilt", rebuilt, "worst scaled deviation of the worst loading", worst_dev)
    assert {tuple(int(x) for x in r) for r in res.islanding} == isl and rebuilt > 50


@pytest.mark.parametrize("name", ["mesh 8x8", "pegaseShaped 72"])
def test_the_series_screen_on_the_same_factor(jg, name):
    t, s = grid(jg, name)
    rating = P.rating_of(t)
    prof = S.profiles(t, 3)
    res = jg.dcSeriesScreen(s, prof, rating=rating, dense=True)
    cand = res.candidates - 1
    assert res.loading.shape == (cand.size, 3) and not np.isin(cand, S.bridges(t)).any() and res.islanding.size == 0
    worst_dev = 0.0
    for i, k in enumerate(cand):
        for tt in range(3):
            _, fr = S.rebuild(t, int(k), prof[tt])
            w, b, load = P.loading(fr, rating)
            scale = max(1.0, w)
            dev = abs(res.loading[i, tt] - w) / scale
            assert dev <= TOL, (k, tt, res.loading[i, tt], w)
            gb = int(res.branch[i, tt])
            assert gb == b or (gb >= 1 and abs(load[gb - 1] - w) <= TOL * scale), (k, tt, gb, b)
            near = int((np.abs(load - 1.0) <= TOL * scale).sum())
            assert abs(int(res.count[i, tt]) - int((load > 1.0).sum())) <= near, (k, tt)
            worst_dev = max(worst_dev, dev)
    print(name, "cases", cand.size * 3, "worst scaled deviation of the worst loading", worst_dev)


@pytest.mark.parametrize("name", ["mesh 8x8", "pegaseShaped 72"])
def test_the_generator_screen_on_the_same_factor(jg, name):
    t, s = grid(jg, name)
    rating = P.rating_of(t)
    thr = 0.9
    res = jg.dcGeneratorScreen(s, rating=rating, threshold=thr, pickup="slack", dense=True)
    assert np.array_equal(res.generators - 1, X.candidates(t))
    e = X.expect(t, rating, res.generators - 1, res.candidates - 1, thr, "slack")
    got_load = np.vstack([res.base[:, 0][None, :], res.loading])
    got_branch = np.vstack([res.base[:, 1][None, :], res.branch]).astype(np.int64)
    got_count = np.vstack([res.base[:, 2][None, :], res.count]).astype(np.int64)
    dev = float((np.abs(got_load - e["load"]) / np.maximum(1.0, e["load"])).max())
    print(name, "cases", e["load"].size, "worst scaled deviation", dev, "excluded by the guards", X.excluded_share(e))
    assert dev <= X.TOL
    assert np.array_equal(got_branch[~e["tie"]], e["branch"][~e["tie"]])
    assert np.array_equal(got_count[~e["near"]], e["count"][~e["near"]])
    assert X.excluded_share(e) <= 0.02


@pytest.mark.parametrize("name", ["binary tree 63", "mesh 8x8"])
def test_state_estimation_on_a_gain_matrix_of_the_same_shapes(jg, name):
    """the gain matrix of DC state estimation goes through the same build_sweep (keep = true) and the same kernels: exact meters of the DC solution on
    every in-service branch and every bus give the solution back; noisy lanes give what the rebuilt normal equations give"""
    from test_dcse_gpu import TOL as SE_TOL
    from test_dcse_host import monitoring_of
    t, _ = grid(jg, name)
    th, _ = R.solve(t)
    pw = R.power(t, th)
    n = t["bus_type"].size
    on = np.flatnonzero(np.asarray(t["br_status"]) == 1)
    ms = E.meters(np.r_[np.zeros(n), np.ones(on.size)], np.r_[np.arange(1, n + 1), on + 1], np.r_[pw["injection"], pw["from_"][on]], np.full(n + on.size, 1e-2))
    an = jg.dcStateEstimation(monitoring_of(jg, t, ms), batch=65)
    jg.setNoise_(an, np.random.default_rng(65))
    jg.setReadings_(an, an.method.mean[None, :], 0)                  # lane 0: the exact readings
    jg.stateEstimation_(an)
    assert np.all(an.status == 0) and an.dims()["ld"] == 128
    rb = E.Rebuilt(t, ms)
    known = R.worst(an.voltage.angle[0], th)
    devs = [R.worst(an.voltage.angle[k], rb.solve(an.readings[k])) for k in range(65)]
    print(name, "known answer", known, "worst lane against the rebuilt normal equations", max(devs), an.dims())
    assert known <= SE_TOL and max(devs) <= SE_TOL
    assert R.worst(an.voltage.angle[64], an.voltage.angle[0]) > 1e-6     # (the noise is there: the lanes differ)
    an.close()
