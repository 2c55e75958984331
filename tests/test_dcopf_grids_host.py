"""The dressed grids of tests/dcopf_grids.py without a device: modelRows and the library's K against the dense restatement on every grid, the conditions
the set has to meet (so that a choice of grids or seeds that reaches less fails here, not silently on the GPU), and the polish: a second reference
that shares no iteration with the restatement.

Per grid (rho = 0.1, not adapted, tolerance 1e-9): variables n, rows m, the restatement's iterations, classes of the sweep kernels the factor of K
reaches, active rows (flow, capability at its upper limit, piecewise, angle):
  two buses              6   10   550  chain                        0 1 1 0
  path 40               46   68  1575  chain                        0 1 1 1
  star 71, leaf slack   77  111  2600  chain, list of 64 or more    1 0 1 0
  star 33, hub slack    39   58  1475  chain                        1 1 1 0
  binary tree 63        69  100   800  chain, wide forward          0 1 1 1
  two cliques           23   55   950  chain                        0 2 1 0
  mesh 8x8              70  122   950  chain                        0 1 2 0
  ring 17               23   36  3550  chain                        1 1 1 0
  case118              191  305  2825  chain, wide forward          3 16 23 0
No grid of the set has a backward level of K above 16 rows: that class is left out (dcopf_grids.K_COVERAGE).
The polished point passes the certificate at 1e-16 .. 1e-13 relative; the restatement lies 1e-11 .. 4e-6 from it (dcopf_grids.MEASURED).
"""
import importlib

import numpy as np
import pytest

import dcopf_grids as Q
import dcopf_reference as R

jg = importlib.import_module("juliagrid.jl_amd")
opf = importlib.import_module("juliagrid.jl_amd.dcoptimalpowerflow")

NAMES = list(Q.GRIDS)


@pytest.mark.parametrize("name", NAMES)
def test_model_rows_equal_the_restatement(name):
    s, md = Q.grid(name)
    pm = opf.modelRows(s)
    assert (pm.n, pm.m) == (md.n, md.m)
    assert np.array_equal(opf.denseRows(pm), md.A)
    assert np.array_equal(pm.l, md.l) and np.array_equal(pm.u, md.u)
    assert np.array_equal(pm.P, md.P) and np.array_equal(pm.q, md.q) and pm.constant == md.constant
    assert list(pm.kind) == list(md.kind) and np.array_equal(pm.equality == 1, md.eq)


@pytest.mark.parametrize("name", NAMES)
def test_the_dressing_is_what_it_says(name):
    s, md = Q.grid(name)
    d, gen = s.dressing, s.generator
    assert gen.layout.bus[d.twin - 1] == gen.layout.bus[d.twin_of - 1] and d.twin != d.twin_of          # two units at one bus
    on = np.flatnonzero(gen.layout.status == 1)
    assert np.all(gen.capability.minActive[on] == 0.0) and np.all(np.isfinite(gen.capability.maxActive[on]))
    total, demand = gen.capability.maxActive[on].sum(), s.bus.demand.active.sum()
    assert 1.7 * demand <= total <= 2.5 * demand
    assert sum(1 for k in on if gen.cost.active.model[k] == 1 and len(gen.cost.active.piecewise[k + 1]) == 4) == len(on) // 3 == len(md.hv)
    assert (md.kind == "flow").sum() == d.rated.size and (md.kind == "angle").sum() == d.angled.size
    assert d.angled.size >= 1 or s.branch.number == d.rated.size           # (the two-bus grid's one branch is rated)
    assert (md.kind == "piecewise").sum() == 3 * len(md.hv)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("rho", (0.1, 7.0))
def test_K_from_the_term_lists(name, rho):
    s, md = Q.grid(name)
    pm = opf.modelRows(s)
    K, c, E = opf.hostModel(pm, rho, 1e-6)
    assert c == 1.0 / max(md.P.max(), np.abs(md.q).max())
    assert np.allclose(E, 1.0 / np.sqrt((md.A ** 2).sum(axis=1)), rtol=1e-15, atol=0)
    A = md.A * E[:, None]
    dense = np.diag(c * md.P + 1e-6) + A.T @ (np.where(md.eq, 1e3 * rho, rho)[:, None] * A)
    assert np.abs(K - dense).max() <= 1e-12 * np.abs(dense).max()
    assert np.array_equal(K != 0, (A.T @ A != 0) | np.eye(pm.n, dtype=bool))
    ptr, idx = Q.k_pattern(md)                                          # the pattern the sweep classes are worked out on is this one
    P = np.zeros((md.n, md.n), dtype=bool)
    P[np.repeat(np.arange(md.n), np.diff(ptr)), idx] = True
    assert np.array_equal(P, K != 0)


def test_the_restatement_solves_every_grid():
    for name in NAMES:
        md, r = Q.solved(name)
        lv = Q.k_levels(md)
        print(f"{name}: n {md.n}, m {md.m}, iterations {r.iterations}, K sweep classes {sorted(Q.k_classes(lv))}, active rows {Q.active_kinds(md, r.y)}")
        assert r.status == 0 and r.iterations <= 6000, (name, r.status, r.iterations)


def test_the_residual_pass_gets_a_second_block_and_an_early_return():
    md = Q.grid(Q.LARGEST)[1]
    n, m = md.n, md.m
    assert all(Q.grid(name)[1].n <= n for name in NAMES)
    assert n > 128 and m > 128 and n % 32 != 0 and m % 32 != 0
    assert ((n + 31) // 32) % 4 != 0 or ((m + 31) // 32) % 4 != 0


def test_active_constraints():
    full, angle = [], []
    for name in NAMES:
        md, r = Q.solved(name)
        a = Q.active_kinds(md, r.y)
        if a["flow"] and a["capability upper"] and a["piecewise"]:
            full.append(name)
        if a["angle"]:
            angle.append(name)
    print("a flow row, a capability row at its upper limit and a piecewise row active:", full, "; an angle row active:", angle)
    assert len(full) >= 2 and len(angle) >= 1


def test_the_factor_of_K_reaches_the_sweep_classes():
    reached = {}
    for name in NAMES:
        got = Q.k_classes(Q.k_levels(Q.grid(name)[1]))
        print(f"{name}: {sorted(got)}")
        for c in got:
            reached.setdefault(c, []).append(name)
    missing = [c for c in Q.K_COVERAGE if c not in reached]
    assert not missing, missing
    assert max(int(Q.k_levels(Q.grid(name)[1])["backward"].max()) for name in NAMES) <= 16, "a wide backward level is reached now: add it to K_COVERAGE"


@pytest.mark.parametrize("name", NAMES)
def test_polish(name):
    """One dense solve on the restatement's active set is a KKT point: a degenerate set fails here, and its grid is re-seeded"""
    s, _ = Q.grid(name)
    md, r = Q.solved(name)
    p = Q.polished(name)
    th, gp, h = R.parts(md, s, p.x)
    cert = R.kkt(md, md.l, md.u, th, gp, h, R.duals(md, s, p.y))
    price = np.abs(p.y[md.kind == "balance"]).max()
    dist = Q.distance(md, r.x, r.y, p.x, p.y)
    print(name, "polished certificate", cert, "active rows", p.rows.size, "restatement's distance (angles, outputs, prices)", dist)
    assert cert[0] <= 1e-9 * np.abs(md.A @ p.x).max() and cert[1] <= 1e-9 * price
    assert np.all(p.y[p.upper & ~md.eq] >= 0.0) and np.all(p.y[p.lower] <= 0.0)          # the multipliers of the set keep their signs
    assert cert[2] <= 1e-9 * price * max(1.0, np.abs(md.A @ p.x).max())
    assert np.all(dist <= 2 * np.array(Q.MEASURED[name]["polish"][:3]))                   # MEASURED is not below what a CPU gives (x 2: other BLAS)
