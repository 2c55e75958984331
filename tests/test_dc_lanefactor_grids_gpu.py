"""The lane-valued factor and its sweeps (csrc/jg_dc_lanefactor.hip) alone on the device, through DcLavStateEstimation.factor_solve, on the (grid,
measurement set) pairs of tests/dc_lane_grids.py: the pairs that tests/test_dc_lane_grids_cpu.py shows to reach every wave split of k_lf_chain, the
hand-over to k_lf_sweep at 16 / 17 rows, wide levels of every residue mod 4, the launch sequence chain, wide, chain, list lengths of every residue mod
DC_T, empty lists, the 70-term lists of the complete gain matrix of a star, factorisation levels of every width mod 4, entries without update terms,
fill entries and n of every residue mod 4.

Bounds.  A lane against plain Gaussian elimination in numpy.longdouble of that lane's H'QH: relative error <= cond(G) x 2^-52, the bound of a
backward-stable solve (test_the_lane_valued_factor_alone of tests/test_dclav_gpu.py); tests/test_dc_lane_grids_cpu.py shows that numpy's own f64 solve
meets it on the same inputs.  Everything else is bitwise (np.array_equal)."""
import numpy as np
import pytest

import dc_grids as G
import dc_lane_grids as D
from test_dcse_host import monitoring_of

pytestmark = pytest.mark.gpu

IDS = [f"{n}/{D.label(k)}" for n, k in D.PAIRS]


def handle(jg, su, batch):
    return jg.dcLavStateEstimation(monitoring_of(jg, su.t, su.ms), batch=batch)


@pytest.mark.parametrize("name,kind", D.PAIRS, ids=IDS)
def test_every_pair_against_extended_precision(jg, name, kind):
    su = D.setup(name, kind, jg)
    T = 65
    an = handle(jg, su, T)
    d, lv = an.dims(), su.levels(jg)
    print(name, D.label(kind), d)
    # the pattern, the levels and the launches are what the analysis of the restated pattern predicts
    assert d["ld"] == 128 and d["n"] == su.n and d["m"] == su.m and d["gainEntries"] == su.pattern[1].size and d["entries"] == lv["entries"]
    assert d["factorLevels"] == len(lv["factor"]) - 1
    assert d["forwardLevels"] == len(lv["forward"]) and d["backwardLevels"] == len(lv["backward"])
    assert d["sweepLaunches"] == len(G.launches(lv["forward"])) + len(G.launches(lv["backward"]))
    q, rhs = D.factor_inputs(su, T)
    x, bad = an.factor_solve(q, rhs)
    assert not bad.any()
    worst = 0.0
    for s in D.FACTOR_LANES:
        Gm = D.gain(su.H, q[s], su.slack)
        ref = D.dense_longdouble(Gm, rhs[s])
        err, bound = float(np.abs(x[s] - ref).max() / np.abs(ref).max()), np.linalg.cond(Gm) * 2.0 ** -52
        worst = max(worst, err / bound)
        print(name, D.label(kind), s, "error", err, "bound", bound)
        assert err <= bound, (s, err, bound)
    print(name, D.label(kind), "largest error / bound", worst)
    # every lane the same Q and right-hand side: every lane is bitwise lane 0 (a wave split that mixes lanes through the LDS would not be)
    x1, bad1 = an.factor_solve(np.tile(q[1], (T, 1)), np.tile(rhs[1], (T, 1)))
    assert not bad1.any() and (x1 == x1[0]).all() and np.array_equal(x1[0], x[1])
    an.close()


def _pivot_buses(su, jg):
    """the buses of the first pivot, the last pivot and the hub (the bus most rows touch) or a middle pivot, the slack left out"""
    perm = [int(b) for b in su.levels(jg)["perm"] if b != su.slack]
    hub = int(np.argmax((su.H != 0.0).sum(axis=0)))
    mid = hub if hub not in (perm[0], perm[-1]) else perm[len(perm) // 2]
    return perm[0], perm[-1], mid


@pytest.mark.parametrize("name,kind", [("path 40", "flows"), ("star 71, leaf slack", "full"), ("mesh 8x8", "full")], ids=["path 40/flows", "star 71/full", "mesh 8x8/full"])
def test_a_bad_pivot_stays_in_its_lane(jg, name, kind):
    """a lane whose weights leave a state unobserved (a zero pivot: its NaN and Inf run through every later level, the pad terms' 0 x dinv[0] included)
    reports its own flag; every other lane is bitwise what it is without the zeroing"""
    su = D.setup(name, kind, jg)
    T = 65
    an = handle(jg, su, T)
    q, rhs = D.factor_inputs(su, T)
    x0, bad0 = an.factor_solve(q, rhs)
    assert not bad0.any()
    for lane, bus in zip((0, 63, 64), _pivot_buses(su, jg)):
        q2 = q.copy()
        q2[lane, su.H[:, bus] != 0.0] = 0.0
        x, bad = an.factor_solve(q2, rhs)
        rest = np.arange(T) != lane
        print(name, D.label(kind), "lane", lane, "bus", bus, "flags", np.flatnonzero(bad))
        assert bad[lane] == 1 and bad.sum() == 1
        assert np.array_equal(x[rest], x0[rest])
    x, bad = an.factor_solve(q, rhs)                                 # and the lane recovers
    assert not bad.any() and np.array_equal(x, x0)
    an.close()


@pytest.mark.parametrize("name,kind", [("path 40", "flows"), ("star 71, leaf slack", "full")], ids=["path 40/flows", "star 71/full"])
def test_the_same_scenarios_in_other_lanes(jg, name, kind):
    """a lane's result does not depend on its lane index or its lane group: five (Q, rhs) scenarios cycled through batches of 1, 63, 64, 65 and 130"""
    su = D.setup(name, kind, jg)
    q, rhs = D.factor_inputs(su, 5, seed=23)
    first = None
    for batch in (1, 63, 64, 65, 130):
        pick = np.arange(batch) % 5
        an = handle(jg, su, batch)
        x, bad = an.factor_solve(q[pick], rhs[pick])
        an.close()
        assert not bad.any()
        if first is None:
            one = handle(jg, su, 5)
            first, _ = one.factor_solve(q, rhs)
            one.close()
        assert np.array_equal(x, first[pick]), batch
