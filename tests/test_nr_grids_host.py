"""Newton-Raphson and Gauss-Newton on the grids of tests/nr_grids.py, host side: what makes the device comparisons of tests/test_nr_grids_gpu.py and
tests/test_gn_grids_gpu.py mean something.  Nothing here needs a GPU; every figure is printed (`pytest -s`).

  * every class of nr_grids.COVERAGE is reached by some family (the table family -> classes is printed);
  * the oracle alone, on every family and every lane of nr_grids.labels: a lane that is no bridge converges and stops clear of the tolerance on both
    sides (MARGIN = 1e-3, the rule of tests/test_wide_batches_gpu.py), so that an iteration count can be compared exactly.  At 1e-8 two lanes of "ring 12
    with twins" (0 and 15) stop at 0.9996e-8 and miss the margin; at nr_grids.TOLERANCE = 1e-9 every lane holds it (closest: a factor 1.23 on either
    side; at 1e-10 the closest check before the last is a factor 1.06 above).  No lane is left out;
  * the oracle's first increment against a dense solve of its own Jacobian in numpy.longdouble (Gaussian elimination with partial pivoting): measured
    1.9e-14 on "path 40 AC", 1.3e-14 on "star 71, hub last", 1.2e-14 on "comb 16 x 2 AC", below 6e-15 elsewhere; asserted <= 1e-12, three orders
    below the 1e-9 increment bar of the device tests;
  * what the oracle makes of the bridge lanes, printed; nothing is asserted on it beyond status != 0.  Seen: status 3 at iteration 0 for leaf bridges on
    the stars and pegaseShaped 60, status 3 at iteration 3 .. 6 on the paths and the cliques, status 1 at the limit on "star 40", the tree and the comb;
  * Gauss-Newton: the contribution list of the hub row of "star 71, hub last" (875 measurement rows) against the 147 tests/test_methods_grids_gpu.py
    reaches, and per family the oracle's increment() against increment_orthogonal() at the start point -- the yardstick nr_grids.GN_DEV_REF records.
"""
import numpy as np
import pytest

import methods_reference as R
import nr_grids as N


def test_every_class_of_the_coverage_list_is_reached():
    reach = {}
    for name in N.NAMES:
        c = N.classes(N.family(name))
        assert c <= set(N.COVERAGE), c - set(N.COVERAGE)
        print(f"{name}: n = {N.family(name)['bus_type'].size}; " + "; ".join(k for k in N.COVERAGE if k in c))
        for k in c:
            reach.setdefault(k, []).append(name)
    for k in N.COVERAGE:
        print(f"  {k} <- {reach.get(k, [])}")
    assert not [k for k in N.COVERAGE if k not in reach]
    assert len(N.COVERAGE) == len(set(N.COVERAGE)) == 30
    # what single families are there for
    assert "row of 64 or more entries" in N.classes(N.family("star 71, hub last")) and "long row, diagonal last" in N.classes(N.family("star 71, hub last"))
    assert "long row, diagonal first" in N.classes(N.family("star 40, hub first PV"))
    assert {"no PQ bus", "no PV bus", "n = 1"} <= N.classes(N.family("one bus"))


def test_one_tolerance_for_the_whole_file():
    assert N.TOLERANCE in (1e-9, 1e-10) and N.ITERATION == 20 and N.MARGIN == 1e-3
    miss = [(name, lab) for name in N.NAMES for lab in N.labels(name) if lab not in N.bridge(name) and not N.margins_hold(N.run(name, lab, 1e-8), 1e-8)]
    print("lanes that miss the margin at 1e-8:", miss)
    assert miss == [("ring 12 with twins", 0), ("ring 12 with twins", 15)]              # why the tolerance is not the default


@pytest.mark.parametrize("name", N.NAMES)
def test_the_oracle_stops_clear_of_the_tolerance_on_every_lane_that_is_no_bridge(name):
    lab = N.labels(name)
    assert lab[0] == 0 and 0 not in N.bridge(name)
    runs = {k: N.run(name, k) for k in lab}
    for k in lab:
        r = runs[k]
        if k in N.bridge(name):
            print(f"[{name}] bridge lane, label {k}: status {r.status} at iteration {r.iteration}")
            assert r.status != 0
        else:
            assert r.status == 0, (name, k, r.status)
            assert N.margins_hold(r), (name, k, r.history[-2:].tolist())
            assert np.all(np.isfinite(r.vm)) and np.all(np.isfinite(r.va))
    print(f"[{name}] labels {lab}: status {[runs[k].status for k in lab]}, iterations {[runs[k].iteration for k in lab]}")
    if name == "one bus":
        assert runs[0].iteration == 0 and N.first(name, 0).dim == 0


@pytest.mark.parametrize("name", N.NAMES)
def test_the_oracle_increment_against_a_dense_solve_in_extended_precision(name):
    """J x = f, J from jcolptr / jrowval and the oracle's own values: the oracle is not the limit of the 1e-9 increment bar of the device tests"""
    worst = 0.0
    for k in N.labels(name):
        if k in N.bridge(name):
            continue
        f = N.first(name, k)
        if f.dim == 0:
            continue
        x = N.dense_longdouble(f.dim, f.jcolptr, f.jrowval, f.J, f.f)
        worst = max(worst, float(np.abs(f.inc.astype(np.longdouble) - x).max() / max(np.longdouble(1.0), np.abs(x).max())))
    print(f"[{name}] oracle increment against the extended-precision dense solve: {worst:.2e}")
    assert worst <= 1e-12


def test_dimensions_follow_the_bus_types():
    for name in N.NAMES:
        t = N.family(name)
        n, npq = t["bus_type"].size, int(np.sum(t["bus_type"] == 1))
        assert N.first(name, 0).dim == n - 1 + npq
    assert N.first("one bus", 0).dim == 0 and N.first("two buses, PV", 0).dim == 1
    assert N.first("all PV ring 9", 0).dim == 8 and N.first("star 17 all PV", 0).dim == 16


@pytest.mark.parametrize("name", N.GN_FAMILIES)
def test_gauss_newton_yardstick_of_the_family(oracle, name):
    """increment() (the normal equations, sparse LU) against increment_orthogonal() (dense QR) at the start point, relative to max|orthogonal|: what the
    two reference solvers differ by on this family.  nr_grids.GN_DEV_REF holds these figures; the device bounds are built from them"""
    t, s, vm, va = N.gn_grid(name)
    tab = N.gn_table(name)
    gn = oracle.OracleGN(s, tab)
    contrib = R.contributions_per_bus(gn.hcolptr, gn.hrowval, s.n)
    gn.increment()
    lu = gn.vectors()["increment"].copy()
    orth = gn.increment_orthogonal()
    dev = float(np.abs(lu - orth).max() / np.abs(orth).max())
    print(f"[{name}] {gn.m} measurement rows; longest contribution list {int(contrib.max())} (bus {int(contrib.argmax()) + 1}); increment() against "
          f"increment_orthogonal() {dev:.2e} (recorded {N.GN_DEV_REF[name]:.1e}); max|increment| {np.abs(orth).max():.3f}")
    assert N.GN_DEV_REF[name] / 4.0 <= dev <= 2.0 * N.GN_DEV_REF[name]      # the recorded figure is the measured one (another LAPACK moves it a little)
    assert N.lu_bound(name) == 1e-9 and 1e-13 <= N.orthogonal_bound(name) <= 2e-10
    if name == "star 71, hub last":
        assert int(contrib.argmax()) == 70 and contrib.max() > 147          # the hub row: 875 rows, six times tests/test_methods_grids_gpu.py's longest
    assert gn.state_estimation(40, N.GN_TOLERANCE) == 0                     # the known answer of the device test: exact readings give the power flow back
    v = gn.vectors()
    assert max(np.abs(v["magnitude"] - vm).max(), np.abs(v["angle"] - va).max()) <= 1e-11
