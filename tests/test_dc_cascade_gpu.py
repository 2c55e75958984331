"""The DC cascading-outage screen (dcCascadeScreen, csrc/jg_dc_cascade.hip) on the device, against route (a) of tests/dc_cascade_reference.py: every
stage of every cascade rebuilt and refactorised, islanding from the graph oracle (connected components), never the compensation.

A cascade makes discrete decisions, so the trip sequences are compared exactly -- away from ties: a cascade whose margin by route (a) (the smallest
|loading - trip| over every stage and monitored branch; for rule "worst" also the gap between the two largest loadings of a stage that trips) is below
1e-6 is ambiguous and left out of the comparison of sequences; at most 5 % of the cascades of a test may be, and every test asserts it (measured: none,
the smallest margin is 2.9e-5).  Tolerance of every comparison of numbers: |got - ref| <= 1e-9 * max(1, max |ref|), the measure and the bound of
tests/test_dc_group_gpu.py.  Every set a cascade passes through has, by the k x k formula on the host, a smallest pivot below 1e-12 or above 1e-6: no
case sits near DC_SINGULAR = 1e-9, and the tests assert it.  Ratings: dc_cascade_reference.ratings.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_cascade_reference as K
import dc_grids as G
import dc_group_reference as Q
import dc_reference as R
from conftest import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
_GRID, _REF = {}, {}


def grid(name):
    """per grid, computed once and left unchanged: the table, the dense sensitivities of route (b), the components of the whole graph, the ratings"""
    if name not in _GRID:
        t = G.family(name) if name in G.FAMILIES else load_case(name)
        Phi, f0 = Q.dense_sensitivities(t)
        _GRID[name] = (t, Phi, f0, Q.base_components(t), K.ratings(t))
    return _GRID[name]


def ref_of(name, S0, rule, trip=1.0, most=8, monitored=None):
    """route (a) for one cascade, computed once per (grid, event, rule, trip, most, monitored)"""
    key = (name, tuple(S0), rule, trip, most, None if monitored is None else tuple(int(m) for m in monitored))
    if key not in _REF:
        t, _, _, base, rating = grid(name)
        mon = K.default_monitored(t, rating) if monitored is None else np.asarray(monitored)
        _REF[key] = K.cascade_rebuild(t, S0, rating, mon, trip, rule, most, base)
    return _REF[key]


def labels_of(events):
    return [tuple(int(s) + 1 for s in S) for S in events]


def singles(name):
    return [(k,) for k in K.in_service(grid(name)[0])]


def screen(jg, name, events, rule, trip=1.0, most=8, monitored=None, **kw):
    t, _, _, _, rating = grid(name)
    mon = None if monitored is None else np.asarray(monitored) + 1
    return jg.dcCascadeScreen(jg.powerSystem(t), labels_of(events), monitored=mon, rating=rating, trip=trip, rule=rule, most=most, dense=True, **kw)


def check(name, events, res, rule, trip=1.0, most=8, monitored=None):
    """every cascade of a dense screen against route (a); returns (the references, worst scaled deviation, ambiguous cascades)"""
    t, Phi, f0, base, rating = grid(name)
    mon = res.monitored - 1
    C = len(events)
    assert res.events == labels_of(events) and res.flows.shape == (C, mon.size) and res.tripped.shape == (C, most)
    assert (res.rule, res.most, res.trip) == (rule, most, trip)
    inv = np.where(rating[mon] > 0, 1.0 / np.where(rating[mon] > 0, rating[mon], 1.0), 0.0)
    refs, dev, ambiguous, pivots = [], 0.0, 0, []
    for c, S0 in enumerate(events):
        ref = ref_of(name, S0, rule, trip, most, monitored)
        refs.append(ref)
        pivots += [Q.group_flows(Phi, f0, S)[1] for S in ref.sets]
        size = int(res.size[c])
        final = [int(x) - 1 for x in res.tripped[c, :size]]
        # the layout of a cascade's own record, whatever the reference says
        assert np.all(res.tripped[c, size:] == 0) and np.all(res.stage[c, size:] == -1) and np.all(np.isnan(res.loading[c, size:])), c
        k0 = len(S0)
        assert final[:k0] == list(S0) and np.all(res.stage[c, :k0] == 0) and np.all(np.isnan(res.loading[c, :k0])), c
        assert np.all(np.diff(res.stage[c, :size]) >= 0) and res.stages[c] == (res.stage[c, size - 1] if size else 0), c
        for s in range(1, int(res.stages[c]) + 1):                # ascending by branch within a stage
            assert np.all(np.diff(res.tripped[c, :size][res.stage[c, :size] == s]) > 0), (c, s)
        assert set(final[k0:]) <= set(mon.tolist()), c
        # what the device's own final flows imply
        got = res.flows[c]
        if res.status[c] == 3:
            assert Q.islands(t, final, base), (c, final)         # the graph oracle
            assert np.all(np.isnan(got)) and np.isnan(res.worst[c]) and res.worstBranch[c] == 0 and res.pending[c] == 0, c
        else:
            assert not Q.islands(t, final, base), (c, final)
            dl = np.abs(got) * inv
            assert all(got[np.searchsorted(mon, s)] == 0.0 for s in final if s in set(mon.tolist())), c
            assert res.worst[c] == dl.max() and res.worstBranch[c] == (int(mon[int(np.argmax(dl))]) + 1 if dl.max() > 0 else 0), c
            if res.status[c] == 0:
                assert res.worst[c] <= trip and res.pending[c] == 0, c
            else:
                assert res.status[c] == K.TRUNCATED and res.worst[c] > trip and res.pending[c] == int((dl > trip).sum()) > 0, c
                assert size + (res.pending[c] if rule == "all" else 1) > most, c
        if ref.margin < K.AMBIGUOUS:
            ambiguous += 1
            continue
        want = (ref.status, ref.stages, len(ref.tripped), ref.tripped, ref.stage, ref.pending)
        have = (int(res.status[c]), int(res.stages[c]), size, final, [int(x) for x in res.stage[c, :size]], int(res.pending[c]))
        assert have == want, (c, S0, have, want)
        ld = np.array(ref.loading[k0:])
        if ld.size:
            d = float(np.abs(res.loading[c, k0:size] - ld).max() / max(1.0, ld.max()))
            assert d <= TOL, (c, d)
            dev = max(dev, d)
        if ref.flows is not None:
            d = R.worst(got, ref.flows[mon])
            assert d <= TOL, (c, S0, d)
            scale = max(1.0, ref.worst)
            assert abs(res.worst[c] - ref.worst) <= TOL * scale, c
            dev = max(dev, d, abs(res.worst[c] - ref.worst) / scale)
    pivots = np.array(pivots)
    print(name, rule, "cascades", C, "shares", K.shares(refs), "ambiguous", ambiguous, "smallest margin", min(r.margin for r in refs),
          "deepest", max(r.stages for r in refs), "pivots: largest below the gap", pivots[pivots < 1e-9].max(initial=0.0), "smallest above",
          pivots[pivots >= 1e-9].min(initial=np.inf), "worst scaled deviation", dev)
    assert np.all((pivots < 1e-12) | (pivots > 1e-6))
    assert ambiguous <= 0.05 * C
    st = np.array([r.status for r in refs])
    if not ambiguous:
        assert res.totals == dict(cascades=C, stable=int((st == 0).sum()), islanding=int((st == 3).sum()), truncated=int((st == K.TRUNCATED).sum()),
                                  trips=int(sum(len(r.tripped) - len(S0) for r, S0 in zip(refs, events))))
    assert res.totals["trips"] == int((res.stage > 0).sum()) and res.totals["stable"] + res.totals["islanding"] + res.totals["truncated"] == C
    return refs, dev, ambiguous


SHARES = {("case14test", "worst"): (3, 15, 0), ("case14test", "all"): (3, 15, 0), ("case30test", "worst"): (16, 26, 0), ("case30test", "all"): (15, 26, 1),
          ("mesh 8x8", "worst"): (58, 33, 23), ("mesh 8x8", "all"): (58, 13, 43), ("pegaseShaped 160", "worst"): (117, 127, 26),
          ("pegaseShaped 160", "all"): (115, 102, 53)}


@pytest.mark.parametrize("rule", ["all", "worst"])
@pytest.mark.parametrize("name", ["case14test", "case30test", "mesh 8x8", "pegaseShaped 160"])
def test_every_single_outage_cascades_as_the_rebuild_route_says(jg, name, rule):
    events = singles(name)
    res = screen(jg, name, events, rule)
    refs, dev, ambiguous = check(name, events, res, rule)
    t = grid(name)[0]
    assert np.array_equal(res.candidates, np.unique(np.r_[res.monitored, [s + 1 for S in events for s in S]]))
    assert R.worst(res.base, R.solve(t)[1][res.monitored - 1]) <= TOL and res.buildMs > 0 and res.screenMs > 0
    assert ambiguous == 0 and K.shares(refs) == SHARES[name, rule]
    if name != "case14test":
        assert max(r.stages for r in refs) >= (7 if rule == "worst" else 2) and max(len(r.tripped) for r in refs) == 8


def repeated(events, count):
    return (events * (count // len(events) + 1))[:count]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_cascade_counts_around_the_lane_width(jg, count):
    name = "case30test"
    events = repeated(singles(name), count)
    for rule in ("all", "worst"):
        check(name, events, screen(jg, name, events, rule), rule)


FIELDS = ("status", "stages", "size", "tripped", "stage", "loading", "worst", "worstBranch", "pending", "base", "flows", "candidates", "monitored")


def same(a, b):
    for field in FIELDS:
        assert np.array_equal(getattr(a, field), getattr(b, field), equal_nan=True), field
    assert a.totals == b.totals


@pytest.mark.parametrize("rule", ["all", "worst"])
def test_rows_per_call_do_not_change_a_bit_and_a_second_call_gives_the_same(jg, rule):
    name = "mesh 8x8"
    events = repeated(singles(name), 130)
    one = screen(jg, name, events, rule)
    check(name, events, one, rule)
    for rows in (1, 64, 65):
        same(screen(jg, name, events, rule, rows=rows), one)
    same(screen(jg, name, events, rule), one)


def test_one_lane_runs_seven_stages_while_the_other_63_stop_at_stage_zero(jg):
    """the barrier / uniform-loop case: every thread of the workgroup reaches every barrier of the seven stages one lane needs"""
    name, rule = "case30test", "worst"
    refs = {S: ref_of(name, S, rule) for S in singles(name)}
    deep = next(S for S, r in refs.items() if r.stages == 7)
    still = [S for S, r in refs.items() if r.stages == 0]
    assert len(still) >= 2
    events = repeated(still, 64)
    events[17] = deep
    res = screen(jg, name, events, rule)
    check(name, events, res, rule)
    print("deep", deep, refs[deep].tripped, "stages of the workgroup", res.stages.tolist())
    assert res.stages[17] == 7 and res.size[17] == 8 and np.all(np.delete(res.stages, 17) == 0)
    alone = screen(jg, name, [deep], rule)
    for field in FIELDS[:9]:
        assert np.array_equal(getattr(alone, field)[0], getattr(res, field)[17], equal_nan=True), field
    assert np.array_equal(alone.flows[0], res.flows[17], equal_nan=True)


@pytest.mark.parametrize("most", [2, 4, 8])
def test_the_bound_on_outages_selects_the_instance_and_truncates(jg, most):
    name = "mesh 8x8"
    events = singles(name)
    for rule in ("all", "worst"):
        res = screen(jg, name, events, rule, most=most)
        refs, _, _ = check(name, events, res, rule, most=most)
        assert K.shares(refs)[2] > 0 and np.all(res.size <= most) and int(res.size.max()) == most


def test_initiating_events_of_one_to_eight_members(jg):
    name = "pegaseShaped 160"
    t = grid(name)[0]
    events = Q.seeded_groups(t, 29, [1, 2, 3, 4, 5, 8, 8, 5, 4, 3, 2, 1] * 3, whole=True)
    for rule in ("all", "worst"):
        res = screen(jg, name, events, rule)
        refs, _, _ = check(name, events, res, rule)
        print(rule, "sizes", [len(S) for S in events], "status", res.status.tolist(), "final size", res.size.tolist())
        assert any(len(S) == 8 and r.status != 3 for S, r in zip(events, refs)) and any(len(S) == 5 and r.stages > 0 for S, r in zip(events, refs))
    for most, sizes in ((2, [1, 2, 2, 1]), (4, [3, 4, 1, 4, 2]), (5, [5, 4, 5, 1])):
        events = Q.seeded_groups(t, 31 + most, sizes * 4, whole=True)
        check(name, events, screen(jg, name, events, "all", most=most), "all", most=most)


@pytest.mark.parametrize("rule", ["all", "worst"])
def test_a_full_event_that_is_stable_one_that_is_overloaded_and_a_cascade_that_ends_full_and_stable(jg, rule):
    name = "mesh 8x8"
    refs = {S: ref_of(name, S, rule) for S in singles(name)}
    # a cascade that ends stable with s >= 2 branches out: with most = s it ends with exactly `most` out and stable
    S, r = next((S, r) for S, r in refs.items() if r.status == 0 and len(r.tripped) >= 2)
    s = len(r.tripped)
    res = screen(jg, name, [S], rule, most=s)
    check(name, [S], res, rule, most=s)
    assert res.status[0] == 0 and res.size[0] == s == res.most and res.stages[0] == r.stages > 0
    # its final set as the initiating event: `most` members, stable, no trip
    full = tuple(r.tripped)
    res = screen(jg, name, [full], rule, most=s)
    check(name, [full], res, rule, most=s)
    assert res.status[0] == 0 and res.stages[0] == 0 and res.size[0] == s and np.all(res.stage[0] == 0)
    # a truncated cascade's set as the initiating event with most = its size: overloaded, status 5 at stage 0
    r = next(r for r in refs.values() if r.status == K.TRUNCATED and len(r.tripped) >= 2)     # (rule "worst" truncates only at 8)
    over, s = tuple(r.tripped), len(r.tripped)
    res = screen(jg, name, [over], rule, most=s)
    check(name, [over], res, rule, most=s)
    print(rule, "full and stable", full, "overloaded", over, "pending", res.pending[0], "worst", res.worst[0])
    assert res.status[0] == K.TRUNCATED and res.stages[0] == 0 and res.size[0] == s and res.pending[0] >= 1 and res.worst[0] > 1.0


def test_rule_all_appends_in_order_across_the_waves_and_truncates_inside_one(jg):
    """wave w walks the rows [w q, (w + 1) q) of Phi, q = rows / 4 rounded up; with every monitored branch a candidate the rows are the candidates"""
    name, rule = "mesh 8x8", "all"
    events = singles(name)
    crossed = packed = 0
    for most in (8, 3):
        res = screen(jg, name, events, rule, most=most)
        check(name, events, res, rule, most=most)
        rows = res.candidates.size
        per = (rows + 3) // 4
        quarter = lambda labels: np.searchsorted(res.candidates, labels) // per
        for c in range(len(events)):
            for s in range(1, int(res.stages[c]) + 1):
                crossed += len(set(quarter(res.tripped[c][res.stage[c] == s]).tolist())) > 1
            if res.status[c] == K.TRUNCATED:
                dl = np.abs(res.flows[c]) / grid(name)[4][res.monitored - 1]
                counts = np.bincount(quarter(res.monitored[dl > res.trip]), minlength=4)
                packed += counts.max() > most - res.size[c]
    print("stages whose trips lie in more than one wave's quarter", crossed, "truncations with one quarter holding more than most - |S|", packed)
    assert crossed > 0 and packed > 0


def test_only_monitored_branches_trip(jg):
    name = "mesh 8x8"
    t, _, _, _, rating = grid(name)
    events = singles(name)
    mon = K.default_monitored(t, rating)[::2]
    for rule in ("all", "worst"):
        res = screen(jg, name, events, rule, monitored=mon)
        refs, _, _ = check(name, events, res, rule, monitored=mon)
        assert np.array_equal(res.monitored, mon + 1) and res.totals["trips"] > 0
        assert set(res.tripped[res.stage > 0].tolist()) <= set((mon + 1).tolist())
        assert set(res.candidates.tolist()) == set((mon + 1).tolist()) | {s + 1 for S in events for s in S}
        assert K.shares(refs) != SHARES[name, rule]              # (the unmonitored half would have tripped)


@pytest.mark.parametrize("trip", [0.8, 1.5])
def test_trip_levels(jg, trip):
    name = "mesh 8x8"
    events = singles(name)
    for rule in ("all", "worst"):
        res = screen(jg, name, events, rule, trip=trip)
        refs, _, _ = check(name, events, res, rule, trip=trip)
        assert res.totals["trips"] > 0 and K.shares(refs) != SHARES[name, rule]


def test_an_initiating_bridge_gives_status_three_at_stage_zero(jg):
    name = "case14test"
    t = grid(name)[0]
    bridges = [int(k) for k in np.flatnonzero(jg.bridges(jg.powerSystem(t)))]
    assert bridges
    events = [(k,) for k in bridges] + [(bridges[0], next(k for k in K.in_service(t) if k not in bridges))]
    res = screen(jg, name, events, "all")
    check(name, events, res, "all")
    assert np.all(res.status == 3) and np.all(res.stages == 0) and np.all(np.isnan(res.worst)) and res.size.tolist() == [len(S) for S in events]


def test_a_stable_cascade_ends_where_the_group_screen_puts_its_final_set(jg):
    name = "mesh 8x8"
    t, _, _, _, rating = grid(name)
    events = singles(name)
    s = jg.powerSystem(t)
    for rule in ("all", "worst"):
        res = screen(jg, name, events, rule)
        stable = np.flatnonzero(res.status == 0)
        groups = [tuple(int(x) for x in res.tripped[c, :res.size[c]]) for c in stable]
        grp = jg.dcGroupScreen(s, groups, monitored=res.monitored, rating=rating, dense=True)
        dev = max(R.worst(res.flows[c], grp.flows[g]) for g, c in enumerate(stable))
        print(rule, "stable cascades", stable.size, "largest final set", max(len(g) for g in groups), "worst scaled deviation from dcGroupScreen", dev)
        assert stable.size > 20 and max(len(g) for g in groups) >= 2 and np.all(grp.status == 0) and dev <= TOL
        assert np.all(grp.count == 0) and np.all(np.abs(grp.worst - res.worst[stable]) <= TOL * np.maximum(1.0, grp.worst))


def test_on_a_live_analysis_on_a_system_and_through_the_handle(jg):
    name = "case30test"
    t, _, _, _, rating = grid(name)
    events = singles(name)
    s = jg.powerSystem(t)
    own = jg.dcCascadeScreen(s, labels_of(events), rating=rating, rule="worst", dense=True)
    check(name, events, own, "worst")
    an = jg.dcPowerFlow(s)
    pair = jg.dcPairScreen(an, rating=rating)
    live = jg.dcCascadeScreen(an, labels_of(events), rating=rating, rule="worst", dense=True)
    same(live, own)
    L = jg._lib.lib()
    dims = np.zeros(6, dtype=np.int64)
    with pytest.raises(jg._lib.JGridError) as e:                  # the screen released what it held on the caller's handle
        jg._lib.check(L.jg_dc_cascade_get_dims(an._h, dims))
    assert e.value.code == 4
    again = jg.dcPairScreen(an, rating=rating)
    assert np.array_equal(again.records, pair.records) and again.totals == pair.totals
    # the handle's own calls: a refused build names the event; a build, the kernel timer before and after a run, release; destroy behind a build
    info = np.zeros(8)
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_cascade_build(an._h, 2, np.array([0, 1, 3], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64), 0, None, 0, info))
    assert e.value.code == 1 and "event 1" in str(e.value)
    lab = labels_of(events)
    off = np.arange(len(lab) + 1, dtype=np.int64)
    mem = np.array([x for g in lab for x in g], dtype=np.int64)
    mon = np.ascontiguousarray(own.monitored)
    jg._lib.check(L.jg_dc_cascade_build(an._h, len(lab), off, mem, mon.size, mon.ctypes.data_as(jg._lib.VP), 0, info))
    jg._lib.check(L.jg_dc_cascade_get_dims(an._h, dims))
    assert dims.tolist() == [len(lab), 64, own.candidates.size, own.candidates.size, mon.size, 1]
    ms = np.zeros(3)
    with pytest.raises(jg._lib.JGridError) as e:                  # no block has been run yet
        jg._lib.check(L.jg_dc_cascade_time_kernel(an._h, 0, 0, len(lab), 3, ms))
    assert e.value.code == 4
    st = np.zeros(len(lab), dtype=np.int32)
    with pytest.raises(jg._lib.JGridError) as e:
        jg._lib.check(L.jg_dc_cascade_run(an._h, 0, len(lab), 1.0, 1, 9, st.ctypes.data_as(jg._lib.VP), *([None] * 10)))
    assert e.value.code == 1
    jg._lib.check(L.jg_dc_cascade_run(an._h, 0, len(lab), 1.0, 1, 8, st.ctypes.data_as(jg._lib.VP), *([None] * 10)))
    assert np.array_equal(st, own.status)
    for kernel in (0, 1):
        jg._lib.check(L.jg_dc_cascade_time_kernel(an._h, kernel, 0, len(lab), 3, ms))
        assert np.all(ms > 0)
    jg._lib.check(L.jg_dc_cascade_release(an._h))
    jg._lib.check(L.jg_dc_cascade_release(an._h))                 # nothing held: still fine
    jg._lib.check(L.jg_dc_cascade_build(an._h, len(lab), off, mem, mon.size, mon.ctypes.data_as(jg._lib.VP), 0, info))
    an.close()                                                    # jg_dc_destroy frees what the build holds


def test_sensitivities_that_do_not_fit_the_budget_are_refused_with_the_sizes(jg):
    name = "case30test"
    t, _, _, _, rating = grid(name)
    with pytest.raises(ValueError) as e:
        jg.dcCascadeScreen(jg.powerSystem(t), labels_of(singles(name)), rating=rating, budget=4096)
    print(e.value)
    assert "bytes" in str(e.value) and "budget is 4096 bytes" in str(e.value)
