"""DC power flow, host side: the numpy / scipy restatement (tests/dc_reference.py) is pinned to the reference's own vectors
(tests/golden/results_dc_*.npz, tools/make_dc_fixtures.py), and dcModel_ equals the restatement's matrix element for element."""
import os

import numpy as np
import pytest

import dc_reference as R
from conftest import GOLDEN, load_case


def dc_golden(case):
    with np.load(os.path.join(GOLDEN, f"results_dc_{case}.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", ["case14test", "case30test"])
def test_the_restatement_reproduces_the_reference_vectors(case):
    t, g = load_case(case), dc_golden(case)
    th, fr = R.solve(t)
    pw = R.power(t, th)
    for name, got in (("voltage", th), ("from", fr), ("from", pw["from_"]), ("injection", pw["injection"]), ("supply", pw["supply"]), ("generator", pw["generator"])):
        print(case, name, float(np.linalg.norm(got - g[name])), float(np.linalg.norm(g[name])))
        assert got.shape == g[name].shape, name
        assert R.isapprox(got, g[name]), name                    # the reference's own criterion (isapprox default)


@pytest.mark.parametrize("case", ["case14", "case14test", "case118", "case300", "case_ACTIVSg10k"])
def test_dcModel_equals_the_restatement_element_for_element(case):
    import juliagrid.jl_amd as jg
    t = load_case(case)
    s = jg.powerSystem(t)
    jg.dcModel_(s)
    (colptr, rowval, nzval), y, psh = R.model(t)
    B = s.model.dc.nodalMatrix
    assert np.array_equal(B.colptr, colptr) and np.array_equal(B.rowval, rowval)
    assert np.array_equal(B.nzval, nzval)                         # same insertion order, same sums: bit for bit, stored zeros included
    assert np.array_equal(s.model.dc.admittance, y) and np.array_equal(s.model.dc.shiftPower, psh)
    off = np.flatnonzero(np.asarray(t["br_status"]) != 1)
    for k in off:                                                 # an out-of-service branch keeps its two stored entries
        assert B.has(int(t["br_from"][k]), int(t["br_to"][k])) and B.has(int(t["br_to"][k]), int(t["br_from"][k]))


def test_an_outage_of_the_restatement_rebuilds_the_matrix():
    """the check must not share the library's shortcut: model(t, out=k) has branch k as stored zeros and the solution differs from the base"""
    t = load_case("case14")
    (_, _, v0), y0, _ = R.model(t)
    (_, _, v1), y1, _ = R.model(t, out=3)
    assert y0[3] != 0.0 and y1[3] == 0.0 and v0.shape == v1.shape and not np.array_equal(v0, v1)
    th0, _ = R.solve(t)
    th1, f1 = R.solve(t, out=3)
    assert np.abs(th0 - th1).max() > 1e-4 and f1[3] == 0.0


def test_the_two_assemblies_of_the_restatement_agree():
    import scipy.sparse as sp
    t = load_case("case300")
    (colptr, rowval, nzval), y, psh = R.model(t, out=7)
    B, y2, psh2 = R.assemble(t, out=7)
    A = sp.csc_matrix((nzval, rowval - 1, colptr - 1), shape=B.shape)
    assert abs(A - B).max() <= 1e-12 * abs(B).max() and np.array_equal(y, y2) and np.allclose(psh, psh2, rtol=0, atol=1e-13)


def test_arguments_without_a_meaning_for_the_method_are_refused():
    """checked before anything touches the device"""
    import juliagrid.jl_amd as jg
    s = jg.powerSystem(load_case("case14"))
    for kw in (dict(reactiveLimit=2), dict(start=(np.ones(14), np.zeros(14))), dict(iteration=5), dict(tolerance=1e-6)):
        with pytest.raises(ValueError):
            jg.contingencyAnalysis(s, [1, 2], method="dc", **kw)
    with pytest.raises(ValueError):
        jg.contingencyAnalysis(s, [1, 2], method="nr", rating=np.ones(s.branch.number))
