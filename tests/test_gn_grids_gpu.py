"""Batched Gauss-Newton (csrc/jg_gn.hip: the row kernels, k_gn_gain, the correction pass of the Orthogonal tag; csrc/jg_engine.hip on the gain pattern)
on seven of the degenerate AC grids of tests/nr_grids.py: two buses, a grid without a PQ bus, one without a PV bus, a clique of 24, the two long stars
and the 8 x 8 mesh.  Voltmeters, ammeters, wattmeters, varmeters and PMUs sit at every place and read the oracle's converged power flow exactly
(methods_reference.all_families); both sides start from the seeded voltages nr_grids.gn_grid writes into the table (at the flat point a plain branch
carries no current and an ammeter row has no derivative).

The gain matrix has the two-hop pattern of the grid: on a star it is COMPLETE -- 71 block rows in one front on "star 71, hub last", whose hub row
collects 875 measurement rows (tests/test_methods_grids_gpu.py reaches 147); on "complete 24 AC" every bus row collects 281.

Bounds.  tests/test_nr_grids_host.py measures per family what the oracle's two solvers differ by at the start point, max|increment() -
increment_orthogonal()| / max|.| (nr_grids.GN_DEV_REF: 1.4e-14 on the ring ... 2.1e-12 on star 71, 9.9e-12 on the clique).  First increment under LU
against increment(): 10 x that, floored at the 1e-9 bar of the NR increment (nr_grids.lu_bound: the floor everywhere).  First increment under
Orthogonal against increment_orthogonal(): 10 x that, never looser than 1e-6 (nr_grids.orthogonal_bound, the rule of methods_reference.increment_bound:
1.4e-13 ... 9.9e-11).  Known answer: every lane within 1e-9 of the power flow (the bar of tests/test_random_grids_gpu.py::test_wls_known_answer).

Worst values measured on one MI355X (`pytest -s` prints every family; DESIGN.md 3.6.1 has the table):
    H and residual vs the oracle ......... 4.03e-16 / 5.35e-15 ("complete 24 AC")
    LU increment vs increment() .......... 2.95e-12 ("complete 24 AC"), 5.80e-13 ("star 71, hub last"), <= 1.2e-13 elsewhere (bound 1e-9)
    Orthogonal increment vs dense QR ..... 1.80e-15 ("mesh 8x8 AC"; bounds 1.4e-13 ... 9.9e-11)
    known answer, 65 lanes ............... 8.73e-13 ("two buses, PQ", 3 iterations: the oracle's own run ends 8.7e-13 from the power flow there), 4.44e-16 elsewhere
    the dense fronts ..................... "star 71, hub last": 5 041 = 71 x 71 gain and factor blocks, 71 factorisation launches; "star 40": 1 600 blocks, 9 launches;
                                           "complete 24 AC": 576 blocks, 7 launches

What these tests can and cannot see.  A contribution dropped from a long bus row of H'WH or H'Wr (the hub's 875) changes the gain or the right-hand
side by one measurement's weight, 1e4 ... 1e8 against sums of that size: the first increment moves by far more than 1e-9, and the known answer no longer
returns the power flow.  A lane of the second lane group reading the first group's operands is seen by the bitwise comparison of lanes 0, 63 and 64
only through a difference, so a fault that gives every lane lane 0's answer passes there -- it is the NR file's per-lane outages that see such a fault.
"""
import numpy as np
import pytest

import nr_grids as N
from test_se_gpu import _mirror, _system_like

pytestmark = pytest.mark.gpu


def _analysis(jg, name, tag="LU", batch=1):
    t, s, vm, va = N.gn_grid(name)
    sysm = _system_like(jg, t, s)
    return jg.gaussNewton(_mirror(jg, sysm, N.gn_table(name)), getattr(jg, tag), batch=batch)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", N.GN_FAMILIES)
def test_first_increment_under_lu(jg, oracle, name):
    t, s, vm, va = N.gn_grid(name)
    gn = oracle.OracleGN(s, N.gn_table(name))
    an = _analysis(jg, name)
    J = an.jacobian
    assert np.array_equal(J.colptr, gn.hcolptr) and np.array_equal(J.rowval, gn.hrowval) and an.dims["m"] == gn.m
    mo = gn.increment()
    v = gn.vectors()
    mx = jg.incrementSE_(an)
    dj = float(np.abs(an.jacobian.nzval - v["jacobian"]).max() / np.abs(v["jacobian"]).max())
    dr = float(np.abs(an.residual - v["residual"]).max() / max(1.0, np.abs(v["residual"]).max()))
    err = _rel(an.increment, v["increment"])
    d = an.dims
    print(f"\n[{name}] {gn.m} rows, {s.n} buses: gain blocks {d['gain_blocks']}, factor blocks {d['lu_blocks']}, factorisation launches {d['factor_launches']}, "
          f"backward launches {d['backward_launches']}; H {dj:.2e}, residual {dr:.2e}, LU increment vs the oracle's {err:.2e} (bound {N.lu_bound(name):.1e})")
    assert dj <= 1e-12 and dr <= 1e-12                               # the bars of tests/test_se_gpu.py
    assert err <= N.lu_bound(name)
    assert abs(mx - mo) <= N.lu_bound(name) * mo
    assert an.increment[s.slack - 1] == 0.0
    if name == "star 71, hub last":                                  # two-hop fill on a star: every pair of buses shares the hub
        assert d["lu_blocks"] >= 71 * 72 // 2
    an.close()


@pytest.mark.parametrize("name", N.GN_FAMILIES)
def test_first_increment_under_the_orthogonal_tag(jg, oracle, name):
    t, s, vm, va = N.gn_grid(name)
    gn = oracle.OracleGN(s, N.gn_table(name))
    ref = gn.increment_orthogonal()
    an = _analysis(jg, name, "Orthogonal")
    mx = jg.incrementSE_(an)
    err = _rel(an.increment, ref)
    print(f"\n[{name}] Orthogonal increment vs the dense QR {err:.2e} (bound {N.orthogonal_bound(name):.1e})")
    assert err <= N.orthogonal_bound(name)
    assert abs(mx - np.abs(ref).max()) <= N.orthogonal_bound(name) * np.abs(ref).max()
    assert an.increment[s.slack - 1] == 0.0
    an.close()


@pytest.mark.parametrize("name", N.GN_FAMILIES)
def test_exact_readings_give_the_power_flow_back_in_every_lane(jg, oracle, name):
    """batch 65 (two lane groups), noise-free readings, stateEstimation_ at 1e-11: every lane returns the power-flow state within 1e-9; lanes 0, 63 and 64
    are equal bit for bit; residualTest_ detects nothing"""
    t, s, vm, va = N.gn_grid(name)
    an = _analysis(jg, name, batch=65)
    jg.stateEstimation_(an, iteration=40, tolerance=N.GN_TOLERANCE)
    st, it = np.array(an.status), np.array(an.method.iteration)
    dv = float(np.abs(an.voltage.magnitude - vm[None, :]).max())
    da = float(np.abs(an.voltage.angle - va[None, :]).max())
    print(f"\n[{name}] 65 lanes: max |dV| {dv:.2e}, |dtheta| {da:.2e} from the power flow; iterations {np.bincount(it).tolist()}")
    assert np.all(st == 0)
    assert dv <= 1e-9 and da <= 1e-9
    for b in (63, 64):
        assert np.array_equal(an.voltage.magnitude[b], an.voltage.magnitude[0]) and np.array_equal(an.voltage.angle[b], an.voltage.angle[0]) and it[b] == it[0]
    out = jg.residualTest_(an)
    assert not np.any(out.detect)
    an.close()
