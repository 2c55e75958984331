"""Gauss-Seidel power flow, host side: the numpy restatement (tests/gs_reference.py) is pinned to the reference's own MATPOWER vectors and iteration
counts (tests/golden/results_gs_*.npz, tools/make_gs_fixtures.py), and the outage patch the device applies to the TRANSPOSED Ybus values equals the
matrix of a system rebuilt without the branch."""
import os

import numpy as np
import pytest

import gs_reference as R
from conftest import GOLDEN, load_case


def gs_golden(case):
    with np.load(os.path.join(GOLDEN, f"results_gs_{case}.npz")) as z:
        return {k: z[k] for k in z.files}


def ac_system(case):
    import juliagrid.jl_amd as jg
    s = jg.powerSystem(load_case(case))
    jg.acModel_(s)
    return s


@pytest.mark.parametrize("case, limit, count", [("case14test", 300, 281), ("case30test", 900, 761)])
def test_the_restatement_reproduces_the_reference_vectors_and_counts(case, limit, count):
    """test/powerFlow/analysis.jl:145-171: gaussSeidel, powerFlow!(iteration = 300 / 900) against MATPOWER's voltages; the counts are MATPOWER's too"""
    gold = gs_golden(case)
    g = R.problem(ac_system(case))
    yt, v, P, Q = R.lanes(g, 1)
    out = R.run(g, yt, v, P, Q, limit, 1e-8)
    print(case, int(out.iteration[0]), int(out.status[0]), float(out.stop[0][0]), float(out.stop[1][0]), float(out.before[0]))
    assert int(gold["iteration"][0]) == count                    # what the fixture holds
    assert out.iteration[0] == count and out.status[0] == 0
    assert R.isapprox(np.abs(v[0]), gold["voltageMagnitude"])
    assert R.isapprox(np.angle(v[0]), gold["voltageAngle"])
    assert R.margins_hold(out, 1e-8)


@pytest.mark.parametrize("case", ["case14test", "case30test"])
def test_the_patch_on_the_transposed_values_equals_a_rebuilt_system(case):
    """every in-service branch: the 4 positions + deltas of transposedOutageTable, applied on the host to nodalMatrixTranspose.nzval, give the values of a
    system rebuilt with updateBranch_(status = 0).  1e-15 absolute: one subtraction per entry."""
    from juliagrid.jl_amd.gaussseidel import transposedOutageTable
    s = ac_system(case)
    ptr, dy = transposedOutageTable(s)
    base = np.array(s.model.ac.nodalMatrixTranspose.nzval)
    live = np.flatnonzero(s.branch.layout.status == 1) + 1
    assert live.size >= 18
    rebuilt = R.lane_values(s, live)
    worst = 0.0
    for row, k in zip(rebuilt, live):
        got = base.copy()
        np.add.at(got, ptr[k - 1] - 1, dy[k - 1])
        assert not np.array_equal(row, base)                      # the rebuilt system does differ from the base
        worst = max(worst, float(np.abs(got - row).max()))
    print(case, "worst |patched - rebuilt|", worst)
    assert worst <= 1e-15


def test_gaussSeidel_is_exported_and_lists_the_buses_by_type():
    import juliagrid.jl_amd as jg
    assert "gaussSeidel" in jg.__all__ and callable(jg.gaussSeidel)
    s = ac_system("case14test")
    with pytest.raises(TypeError):                                # not offered on this type, and said so before anything reaches the device
        jg.power_(object.__new__(jg.GaussSeidelPowerFlow))
    if jg._lib.device_count() < 1:
        pytest.skip("creating the analysis needs a HIP device")
    an = jg.gaussSeidel(s, batch=2)
    typ = s.bus.layout.type
    assert np.array_equal(an.method.pq, np.flatnonzero(typ == 1) + 1) and np.array_equal(an.method.pv, np.flatnonzero(typ == 2) + 1)
    assert an.method.iteration == 0 and an.method.voltage.shape == (2, 14)
    assert an.method.signature.type == s.model.revision.type and an.method.signature.topology == s.model.revision.topology
