"""The DC generator-outage screen (dcGeneratorScreen, csrc/jg_dc_generator.hip) on the device, against the rebuild route of
tests/dc_generator_reference.py: per case the injections are moved by the pickup rule, the branch goes out of service, and the model is rebuilt and
refactorised -- never the sensitivities the kernels use.

Tolerance of every comparison: |got - ref| <= 1e-9 * max(1, |ref worst loading|), the bound of the sibling screens.  The worst branch is compared where
the two largest loadings of a case differ by more than that, counts and record lists where no loading lies within it of the threshold; the share of the
cases those two guards take out is asserted to stay within 2 % (tests/test_dc_generator_host.py holds the restatement alone to the same).  Every figure
is printed before it is asserted."""
import numpy as np
import pytest

import dc_generator_reference as X
import dc_pair_reference as P
import dc_reference as R
import dc_series_reference as S
import dc_series_shed_reference as H
from conftest import load_case
from test_dc_generator_host import X_THRESHOLD, default_candidates, grid

pytestmark = pytest.mark.gpu

TOL = X.TOL
NAMES = ("violating", "bridges", "worst", "worstGenerator", "violatingGenerator", "base", "loading", "branch", "count", "lost", "shortfall", "slackActive")


def same(a, b, names=NAMES):
    return all(np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True) for n in names) and a.totals == b.totals and a.overflow == b.overflow


def compare(res, e, thr, what):
    """the dense result, the G-1 table, the records and the summaries of `res` (rows from candidate 0) against the expectation `e`; returns the worst scaled deviation"""
    got_load = np.vstack([res.base[:, 0][None, :], res.loading])
    got_branch = np.vstack([res.base[:, 1][None, :], res.branch]).astype(np.int64)
    got_count = np.vstack([res.base[:, 2][None, :], res.count]).astype(np.int64)
    scale = np.maximum(1.0, e["load"])
    dev = float((np.abs(got_load - e["load"]) / scale).max())
    share = X.excluded_share(e)
    print(what, "cases", e["load"].size, "violating", res.totals["violating"], "worst scaled deviation", dev, "excluded by the guards", share)
    assert dev <= TOL, (what, dev)
    assert share <= 0.02, (what, share)
    assert np.array_equal(got_branch[~e["tie"]], e["branch"][~e["tie"]]), what
    assert np.array_equal(got_count[~e["near"]], e["count"][~e["near"]]), what
    assert res.totals["cases"] == e["load"].size and not res.overflow
    want = X.records(e, res.candidates, thr)
    lab = np.r_[0, res.candidates]
    ok = lambda rec: np.array([not e["near"][int(np.flatnonzero(lab == r[0])[0]), int(r[1])] for r in rec], dtype=bool)
    got, want = res.violating[ok(res.violating)] if res.violating.size else res.violating, want[ok(want)] if want.size else want
    assert got.shape == want.shape and np.array_equal(got[:, [0, 1, 4]], want[:, [0, 1, 4]]), what
    assert (np.abs(got[:, 3] - want[:, 3]) <= TOL * np.maximum(1.0, want[:, 3])).all(), what
    tie = np.array([e["tie"][int(np.flatnonzero(lab == r[0])[0]), int(r[1])] for r in want], dtype=bool)
    assert np.array_equal(got[~tie, 2], want[~tie, 2]), what
    if not e["near"].any():
        assert res.totals["violating"] == want.shape[0]
    # the summaries are what the dense result implies, bit for bit
    assert np.array_equal(res.worst, res.loading.max(axis=1)) and np.array_equal(res.worstGenerator, got_load.max(axis=0))
    assert np.array_equal(res.violatingGenerator, (res.loading > thr).sum(axis=0))
    return dev


_RUN = {}


def run(jg, case, pickup):
    """one screen of a test grid with every default generator x every default candidate, and its expectation: computed once"""
    if (case, pickup) not in _RUN:
        t = grid(case)
        s = jg.powerSystem(t)
        rating = P.rating_of(t)
        thr = X_THRESHOLD[case]
        res = jg.dcGeneratorScreen(s, rating=rating, threshold=thr, pickup=pickup, dense=True, share=True, flows=True)
        e = X.expect(t, rating, res.generators - 1, res.candidates - 1, thr, pickup)
        _RUN[case, pickup] = dict(t=t, s=s, rating=rating, thr=thr, res=res, e=e)
    return _RUN[case, pickup]


@pytest.mark.parametrize("pickup", ["slack", "participation"])
@pytest.mark.parametrize("case", ["case14test", "case30test"])
def test_every_case_against_the_rebuild_route(jg, case, pickup):
    r = run(jg, case, pickup)
    t, res, e = r["t"], r["res"], r["e"]
    assert np.array_equal(res.generators, X.candidates(t) + 1) and np.array_equal(res.candidates, default_candidates(t) + 1) and res.bridges.size == 0
    compare(res, e, r["thr"], f"{case} {pickup}")
    bus, _, pg = X._gen(t)
    assert np.array_equal(res.lost, pg[res.generators - 1])
    fdev = float(np.abs(res.flow - e["flow0"][res.flowRows - 1]).max())
    sdev = float(np.abs(res.slackActive - e["slack"]).max())
    print(case, pickup, "G-1 flows worst deviation", fdev, "slackActive", sdev, "shortfall", res.shortfall)
    assert fdev <= TOL and sdev <= TOL and np.abs(res.shortfall - e["shortfall"]).max() <= 1e-14
    if pickup == "slack":
        assert not res.shortfall.any() and res.pickupShare.take.nnz == 0
        zero = np.flatnonzero((pg[res.generators - 1] == 0) | (bus[res.generators - 1] == R.slack_of(t)))      # nothing moves: the column is the base case
        assert zero.size and all(np.array_equal(res.loading[:, j], res.loading[:, zero[0]]) for j in zero)


def test_participation_with_caps_and_with_a_shortfall(jg):
    """case14test: units cap and the rest is re-shared, nothing is short; case30test: the loss of the large unit exhausts every headroom"""
    a, b = run(jg, "case14test", "participation"), run(jg, "case30test", "participation")
    for r, short in ((a, False), (b, True)):
        sh, t = r["res"].pickupShare, r["t"]
        room = np.maximum(X.pmax_of(t) - np.asarray(t["gen_pg"]), 0.0)
        take = sh.take.toarray()
        capped = (take >= room[:, None]) & (take > 0)
        print("participation: capped units per outage", capped.sum(axis=0), "shortfall", sh.shortfall)
        assert (take <= room[:, None] + 1e-15).all() and capped.any()
        assert np.abs(take.sum(axis=0) + sh.shortfall - sh.lost).max() <= 1e-14
        j = int(np.argmax(capped.sum(axis=0)))
        free = (take[:, j] > 0) & ~capped[:, j]
        assert (sh.shortfall > 0).any() == short
        if short:
            js = int(np.argmax(sh.shortfall))
            on = np.asarray(t["gen_status"]) == 1
            on[sh.generators[js] - 1] = False
            assert np.array_equal(take[on, js], room[on]) and abs(r["res"].slackActive[js] - r["e"]["slack"][js]) <= TOL
        else:
            assert free.sum() > 1 and np.ptp(take[free, j] / X.pmax_of(t)[free]) <= 1e-12      # the re-split follows the weights


def test_slack_pickup_equals_the_series_screen_fed_hand_made_injection_rows(jg):
    for case in ("case14test", "case30test"):
        r = run(jg, case, "slack")
        t, s, res = r["t"], r["s"], r["res"]
        bus, _, pg = X._gen(t)
        own = R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64)
        rows = np.tile(own, (res.generators.size, 1))
        for j, g in enumerate(res.generators - 1):
            rows[j, bus[g]] -= pg[g]
        ser = jg.dcSeriesScreen(s, rows, candidates=res.candidates, rating=r["rating"], threshold=r["thr"], dense=True)
        dev = float((np.abs(res.loading - ser.loading) / np.maximum(1.0, ser.loading)).max())
        bdev = float((np.abs(res.base[:, 0] - ser.base[:, 0]) / np.maximum(1.0, ser.base[:, 0])).max())
        print(case, "generator screen against the series screen on the same cases: worst scaled deviation", dev, "G-1 rows", bdev)
        assert dev <= 1e-12 and bdev <= 1e-12
        assert np.array_equal(res.branch, ser.branch) and np.array_equal(res.base[:, 1], ser.base[:, 1])


_EDGE = {}


def edge(jg):
    """case118 with 80 units added: two on one bus with different outputs, one with no output, one beside the slack's own; 7 candidates (no multiple of
    the tile of 4); G = 130 is the full run the smaller ones are columns of"""
    if not _EDGE:
        t0 = load_case("case118")
        rng = np.random.default_rng(9)
        slack = R.slack_of(t0) + 1
        buses = np.r_[[5, 5, 17, slack], rng.choice(np.setdiff1d(np.arange(1, 119), [slack]), 76, replace=True)]
        pg = np.r_[[0.4, 0.9, 0.0, 0.2], 0.1 + rng.random(76)]
        t = X.with_generators(t0, buses, pg, pmax=pg + 0.05 + 0.5 * rng.random(80))
        s = jg.powerSystem(t)
        rating = 25.0 * P.rating_of(t)                            # (the added units load the grid some 29 times the seeded ratings)
        gens = jg.generatorCandidates(s)[:130]
        new = t0["gen_bus"].size
        assert gens.size == 130 and {new + 1, new + 2, new + 3, new + 4} <= set(gens.tolist())
        cand = np.sort(rng.choice(default_candidates(t) + 1, 7, replace=False))
        thr = 1.16                                               # splits the cases: their worst loadings lie between 1.02 and 1.30
        out = {}
        for pickup in ("slack", "participation"):
            out[pickup] = jg.dcGeneratorScreen(s, generators=gens, candidates=cand, rating=rating, threshold=thr, pickup=pickup, dense=True)
        _EDGE.update(t=t, s=s, rating=rating, gens=gens, cand=cand, thr=thr, res=out, new=new)
    return _EDGE


@pytest.mark.parametrize("pickup", ["slack", "participation"])
def test_lane_and_tile_edges_against_the_rebuild_route(jg, pickup):
    h = edge(jg)
    res = h["res"][pickup]
    e = X.expect(h["t"], h["rating"], h["gens"] - 1, h["cand"] - 1, h["thr"], pickup)
    compare(res, e, h["thr"], f"case118 + 80 units, G = 130, 7 candidates, {pickup}")
    col = {int(g): j for j, g in enumerate(h["gens"])}
    a, b, z = col[h["new"] + 1], col[h["new"] + 2], col[h["new"] + 3]
    assert not np.array_equal(res.loading[:, a], res.loading[:, b])                          # one bus column, two outputs
    if pickup == "slack":
        none = jg.dcSeriesScreen(h["s"], (R.supply(h["t"]) - h["t"]["bus_pd"])[None, :], candidates=h["cand"], rating=h["rating"], threshold=h["thr"], dense=True)
        dev = float(np.abs(res.loading[:, z] - none.loading[:, 0]).max())
        print("a unit without output against the base case:", dev)
        assert dev <= 1e-12 and res.lost[z] == 0.0


@pytest.mark.parametrize("pickup", ["slack", "participation"])
def test_fewer_generators_are_columns_of_the_full_run(jg, pickup):
    h = edge(jg)
    full = h["res"][pickup]
    for G in (1, 63, 64, 65):
        part = jg.dcGeneratorScreen(h["s"], generators=h["gens"][:G], candidates=h["cand"], rating=h["rating"], threshold=h["thr"], pickup=pickup, dense=True)
        for name in ("loading", "branch", "count"):
            assert np.array_equal(getattr(part, name), getattr(full, name)[:, :G]), (G, name)
        assert np.array_equal(part.base, full.base[:G]) and np.array_equal(part.violating, full.violating[full.violating[:, 1] < G]), G
        assert part.totals["cases"] == 8 * G and np.array_equal(part.worstGenerator, full.worstGenerator[:G])


def test_blocks_rows_and_capacity(jg):
    h = edge(jg)
    ref = h["res"]["participation"]
    kw = dict(generators=h["gens"], candidates=h["cand"], rating=h["rating"], threshold=h["thr"], pickup="participation", dense=True)
    nv = ref.totals["violating"]
    print("edge grid: cases", ref.totals["cases"], "violating", nv, "of them G-1", int((ref.violating[:, 0] == 0).sum()))
    assert 20 < nv < ref.totals["cases"] and (ref.violating[:, 0] == 0).any() and (ref.violating[:, 0] > 0).any()
    order = np.lexsort((ref.violating[:, 1], ref.violating[:, 0]))
    assert np.array_equal(order, np.arange(nv))                                              # sorted by (k, g), the G-1 row first
    for block in (1, 3):
        assert same(jg.dcGeneratorScreen(h["s"], block=block, **kw), ref), block
    parts = [jg.dcGeneratorScreen(h["s"], rows=(a, b), block=2, **kw) for a, b in ((0, 1), (1, 4), (4, 7))]
    assert np.array_equal(np.vstack([p.violating for p in parts]), ref.violating) and sum(p.totals["cases"] for p in parts) == ref.totals["cases"]
    assert np.array_equal(np.vstack([p.loading for p in parts]), ref.loading) and all(np.array_equal(p.base, ref.base) for p in parts)
    assert np.array_equal(np.max([p.worstGenerator for p in parts], axis=0), ref.worstGenerator)
    assert np.array_equal(np.sum([p.violatingGenerator for p in parts], axis=0), ref.violatingGenerator)
    for cap in (0, 5, nv - 1):
        for block in (None, 3):
            cut = jg.dcGeneratorScreen(h["s"], capacity=cap, block=block, **kw)
            assert cut.totals == ref.totals and cut.overflow and cut.violating.shape == (cap, 5), (cap, block)
            assert np.array_equal(cut.violating, ref.violating[:cap]) and np.array_equal(cut.worst, ref.worst), (cap, block)


def test_shed_mode_with_a_unit_behind_a_bridge(jg):
    """case14test with a generator on a new bus hung on bus 9 by one branch: the feeder is a bridge, and behind it sits the lost unit"""
    t = X.with_feeder(grid("case14test"), 9, 0.35)
    t["gen_pmax"] = np.r_[grid("case14test")["gen_pmax"], 0.6]
    s = jg.powerSystem(t)
    rating = np.r_[P.rating_of(load_case("case14test")), 0.45]
    thr = X_THRESHOLD["case14test"]
    feeder, unit = t["br_from"].size, t["gen_bus"].size                                      # labels
    br = H.bridges(t)
    assert feeder - 1 in br
    for pickup in ("slack", "participation"):
        res = jg.dcGeneratorScreen(s, rating=rating, threshold=thr, pickup=pickup, dense=True, islands="shed")
        assert np.array_equal(res.candidates, jg.shedCandidates(s)) and np.array_equal(res.shed, np.array(sorted(br)) + 1) and res.bridges.size == 0
        e = X.expect(t, rating, res.generators - 1, res.candidates - 1, thr, pickup, shed=True)
        compare(res, e, thr, f"case14test + feeder, shed, {pickup}")
        i, j = int(np.flatnonzero(res.candidates == feeder)[0]), int(np.flatnonzero(res.generators == unit)[0])
        js = int(np.flatnonzero(res.shed == feeder)[0])
        assert res.shedBuses[js] == 1 and res.shedM[js] == 9 and res.shedFlow.shape == (res.shed.size, res.generators.size)
        assert abs(res.shedDemand[js] - 0.02) <= 1e-15
        if pickup == "slack":
            # the lost unit leaves with the bridge anyway: the case equals the shed case of a column where nothing moves
            inj = (R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64))[None, :]
            none = jg.dcSeriesScreen(s, inj, candidates=res.candidates, rating=rating, threshold=thr, dense=True, islands="shed")
            dev = abs(res.loading[i, j] - none.loading[i, 0])
            print("shed: the feeder out with the unit behind it lost, against the shed case without the outage:", dev, "flow that left", res.shedFlow[js, j])
            assert dev <= 1e-12 and res.branch[i, j] == none.branch[i, 0] and abs(res.shedFlow[js, j] - (0.02 - 0.0)) <= 1e-12
    skip = jg.dcGeneratorScreen(s, candidates=res.candidates, rating=rating, threshold=thr, dense=True)
    isb = np.isin(res.candidates, res.shed)
    assert np.array_equal(skip.bridges, res.candidates[isb]) and np.isnan(skip.loading[isb]).all() and skip.shed is None


def test_errors_leave_the_handle_usable(jg):
    r = run(jg, "case14test", "slack")
    t, s, rating, thr = r["t"], r["s"], r["rating"], r["thr"]
    ng = t["gen_bus"].size
    off = int(np.flatnonzero(np.asarray(t["gen_status"]) == 0)[0]) + 1
    t1 = dict(t)
    t1["gen_status"] = np.where((np.asarray(t["gen_bus"]) == R.slack_of(t) + 1) & (np.arange(ng) > 0), 0, t["gen_status"]).astype(np.int8)
    an, an1 = jg.dcPowerFlow(s), jg.dcPowerFlow(jg.powerSystem(t1))
    first = jg.dcGeneratorScreen(an, rating=rating, threshold=thr, dense=True)
    assert same(first, r["res"])
    with pytest.raises(ValueError, match="last in-service unit of the slack bus"):
        jg.dcGeneratorScreen(an1, generators=[1], rating=rating)
    for bad, exc in (([off], ValueError), ([ng + 1], IndexError), ([0], IndexError)):
        with pytest.raises(exc):
            jg.dcGeneratorScreen(an, generators=bad, rating=rating)
    for bad in (np.ones(ng + 1), -np.ones(ng)):
        with pytest.raises(ValueError):
            jg.dcGeneratorScreen(an, rating=rating, pickup="participation", participation=bad)
    L = jg._lib.lib()
    one = np.ones(1, dtype=np.int64)
    z2 = np.zeros(2, dtype=np.int64)
    for args in ((1, one, 0, None, 1, 1, np.array([99], dtype=np.int64), z2, one * 0, np.ones(1)),             # a bus out of range
                 (1, one, 0, None, 1, 1, one, np.array([0, 1], dtype=np.int64), one * 3, np.ones(1)),         # an entry that names no generator bus
                 (1, one, 0, None, 0, 0, one, z2, one * 0, np.ones(1))):                                     # no generator
        assert L.jg_dc_generator_build(an._h, *args, 0, np.zeros(16)) == 1 and b"jg_dc_generator_build" in L.jg_last_error()
    assert L.jg_dc_generator_screen(an._h, 0, 1, 1.0, 0, None, None, np.zeros(5, dtype=np.int64), None, None, None, None, None, None, None) == 4
    again = jg.dcGeneratorScreen(an, rating=rating, threshold=thr, dense=True)              # the analysis still works afterwards
    assert same(again, first)
    rest = jg.dcGeneratorScreen(an1, rating=rating, threshold=thr)                           # and so does the one whose slack unit was refused
    assert 1 not in rest.generators
    an.close()
    an1.close()
