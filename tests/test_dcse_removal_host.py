"""The inputs of tests/test_dcse_removal_gpu.py, checked on the host against the restatement (tests/dcse_reference.py) alone, so that a failure on the
device is the library's and not the inputs'.

A cluster is four meters round one bus b of the full set (dcse_reference.full_set: n injections, from / to of every branch, n bus PMUs): the
injection wattmeter of b, the from-wattmeter of b's first branch, the PMU at b and the injection wattmeter at that branch's other end.  Their rows of H
share columns, so Omega_SS = W_S^-1 - H_S G^-1 H_S' has large off-diagonal terms: the arithmetic of the compensation that exists only for two or more
removed rows (the off-diagonal part of L in Omega_SS = L D L') decides the answer.  Checked here for every cluster the device tests use:

  * every prefix of the cluster leaves the grid observable (the restatement's rebuilt gain is not singular);
  * every kept in-service row keeps w_i Omega'_ii >= 1e-3 (the relative error of a normalised residual grows like 1 / (w_i Omega'_ii));
  * the dense compensation formula Omega'_ii = Omega_ii - q' Omega_SS^-1 q, q = h_i U, U = G^-1 H_S', equals the variances of the rebuilt set;
  * the same formula with Omega_SS replaced by its diagonal moves some kept row's sqrt(Omega') by more than 1e-3 relative (measured: >= 9.8e-3 on
    case118, >= 3.4e-2 on case14test, >= 1.9e-2 on case30test), six decades above the device tests' bound, so they cannot pass a kernel that drops
    the coupling.

The twice-metered leaf of case14: a leaf bus seen by the from- and the to-wattmeter of its branch and by nothing else.  Either may leave; the second
one to leave is critical, and its pivot of L D L' goes to 0 by cancellation (d = Omega_kk - sum L^2 D), not at the first step."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
from conftest import load_case
from test_dcse_gpu import at_zero
from test_dcse_host import bad_data_set, case14_moved_slack

CONDITION = 1e-3                                                     # w_i Omega'_ii of every kept in-service row, at least
DISCRIMINATION = 1e-3                                                # relative move of some kept sqrt(Omega') without the coupling, more than
# the same for the first two or three rows of a cluster, where nothing was measured beforehand: 1000 x the device tests' bound of 1.122e-9 on a
# normalised residual (which is |r| / sqrt(Omega')), so a kernel without the coupling still misses that bound by three decades
PREFIX_DISCRIMINATION = 1e-6
# the grids whose clusters tests/test_dcse_removal_gpu.py removes (it takes them from gpu_clusters below and nowhere else)
GPU_GRIDS = ["case118", "case118kept", "case118outage", "case118pmu11", "case30test", "case14moved"]


def grid(name):
    """the table of a grid of GPU_GRIDS.  case118: the slack's angle at 0 (tests/test_dcse_gpu.py: at_zero); case118kept: as stored, 0.52 rad"""
    if name == "case14moved":
        return case14_moved_slack()
    t = load_case("case118" if name.startswith("case118") else name)
    return at_zero(t) if name.startswith("case118") and name != "case118kept" else t


def ends(t):
    return np.asarray(t["br_from"]).astype(np.int64), np.asarray(t["br_to"]).astype(np.int64), np.asarray(t["br_status"]).astype(np.int64)


def eligible_buses(t):
    """1-based: every bus but the slack with three or more in-service branch ends"""
    f, to, st = ends(t)
    n = t["bus_type"].size
    deg = np.bincount(np.r_[f[st == 1], to[st == 1]], minlength=n + 1)
    return [b for b in range(1, n + 1) if deg[b] >= 3 and b - 1 != R.slack_of(t)]


def coupled_cluster(t, b):
    """0-based rows of the full set round bus b (1-based): its injection wattmeter, the from-wattmeter of its first in-service branch, its PMU, the
    injection wattmeter at that branch's other end"""
    f, to, st = ends(t)
    n, nb = t["bus_type"].size, f.size
    k = int(np.flatnonzero(((f == b) | (to == b)) & (st == 1))[0])
    other = int(to[k] if f[k] == b else f[k])
    return [b - 1, n + 2 * k, n + 2 * nb + b - 1, other - 1]


def outage_rows(t):
    """the out-of-service rows of "case118outage" (0-based): three wattmeters -- the to-wattmeter of the first cluster's branch (a row at the cluster's
    bus, not in the cluster), an injection and a from-wattmeter elsewhere -- and one PMU"""
    n, nb = t["bus_type"].size, ends(t)[0].size
    first = coupled_cluster(t, eligible_buses(t)[0])
    return [first[1] + 1, 40, n + 2 * 100, n + 2 * nb + 28]


def measurement_set(name, t):
    """(power-flow angles, measurement set) of a grid of GPU_GRIDS: the full set of the bad-data tests; case118outage with outage_rows out of service;
    case118pmu11 with the variance of PMU 11 at 1e-4"""
    th, ms = bad_data_set(t)
    if name == "case118outage":
        nw = ms.w_index.size
        for r in outage_rows(t):
            if r < nw:
                ms.w_status[r] = 0
            else:
                ms.p_status[r - nw] = 0
    if name == "case118pmu11":
        ms.p_variance[10] = 1e-4
    return th, ms


def gpu_clusters(name, t):
    """the clusters the device tests remove on this grid: one per eligible bus, in bus order"""
    dead = set(outage_rows(t)) if name == "case118outage" else set()
    out = [coupled_cluster(t, b) for b in eligible_buses(t)]
    assert not any(dead & set(c) for c in out)
    return out


def dense_of(base):
    """(G^-1, H) of a Rebuilt, dense, computed once"""
    if not hasattr(base, "dense"):
        base.dense = (np.linalg.inv(base.G.toarray()), base.H.toarray())
    return base.dense


def dense_compensation(base, rows, coupled=True):
    """Omega'_ii = Omega_ii - q' Omega_SS^-1 q for every row, dense and on the FULL set's gain `base` (a Rebuilt without removed rows): q = h_i U,
    U = G^-1 H_S'.  coupled = False: Omega_SS replaced by its diagonal"""
    Gi, H = dense_of(base)
    U = Gi @ H[rows].T
    omega = 1.0 / base.w - np.einsum("ij,jk,ik->i", H, Gi, H)
    oss = np.diag(1.0 / base.w[rows]) - H[rows] @ U
    if not coupled:
        oss = np.diag(np.diag(oss))
    Q = H @ U
    return omega - np.einsum("ik,ik->i", Q, np.linalg.solve(oss, Q.T).T)


def kept(rb):
    return np.flatnonzero(rb.status == 1.0)


def ldl_pivots(base, rows):
    """w_k d_k of Omega_SS = L D L', one row per removal in the order given, in exact (dense, double) arithmetic on the full set's gain"""
    Gi, H = dense_of(base)
    H = H[rows]
    oss = np.diag(1.0 / base.w[rows]) - H @ Gi @ H.T
    k = len(rows)
    L, D = np.eye(k), np.zeros(k)
    for a in range(k):
        for b in range(a):
            L[a, b] = (oss[a, b] - sum(L[a, c] * D[c] * L[b, c] for c in range(b))) / D[b]
        D[a] = oss[a, a] - sum(L[a, c] ** 2 * D[c] for c in range(a))
    return D * base.w[rows]


def twice_metered_leaf(t):
    """(angles, measurement set, leaf, neighbour) of case14: row 0 the from- and row 1 the to-wattmeter of the leaf's branch, rows 2.. injections at
    every bus but the leaf and its neighbour, then PMUs everywhere but at the leaf"""
    th, _ = R.solve(t)
    f, to, _ = ends(t)
    n = t["bus_type"].size
    deg = np.bincount(np.r_[f, to], minlength=n + 1)
    leaf = int(np.flatnonzero(deg[1:] == 1)[0]) + 1
    k = int(np.flatnonzero((f == leaf) | (to == leaf))[0])
    neighbour = int(to[k] if f[k] == leaf else f[k])
    fr = R.power(t, th)["from_"][k]
    inj = R.power(t, th)["injection"]
    buses = [b for b in range(1, n + 1) if b not in (leaf, neighbour)]
    seen = [b for b in range(1, n + 1) if b != leaf]
    ms = S.meters([1, 2] + [0] * len(buses), [k + 1, k + 1] + buses, [fr, -fr] + [inj[b - 1] for b in buses], [1e-2] * (2 + len(buses)), None,
                  seen, None, [th[b - 1] for b in seen], [1e-5] * len(seen))
    return th, ms, leaf, neighbour


@pytest.mark.parametrize("case", ["case14test", "case30test", "case118"])
def test_every_cluster_is_observable_conditioned_and_compensated(case):
    t = load_case(case)
    th, ms = bad_data_set(t)
    base = S.Rebuilt(t, ms)
    lowest, worst = np.inf, 0.0
    for b in eligible_buses(t):
        rows = coupled_cluster(t, b)
        assert len(set(rows)) == 4, (b, rows)
        for k in range(1, 5):
            rb = S.Rebuilt(t, ms, rows[:k])
            assert not rb.singular, (b, rows[:k])
            var, keep = rb.variances(), kept(rb)
            share = (rb.w * var)[keep]
            assert share.min() >= CONDITION, (b, rows[:k], float(share.min()))
            got = dense_compensation(base, rows[:k])
            np.testing.assert_allclose(got[keep], var[keep], rtol=1e-7, atol=0.0, err_msg=str((b, rows[:k])))
            lowest = min(lowest, float(share.min()))
            worst = max(worst, float(np.abs(got[keep] / var[keep] - 1.0).max()))
    print(case, "clusters", len(eligible_buses(t)), "lowest w Omega'", lowest, "worst relative deviation of the dense formula", worst)


def discrimination(base, rb, rows):
    keep = kept(rb)
    right = np.sqrt(np.abs(rb.variances()[keep]))
    wrong = np.sqrt(np.abs(dense_compensation(base, rows, coupled=False)[keep]))
    return float(np.abs(wrong / right - 1.0).max())


@pytest.mark.parametrize("name", GPU_GRIDS)
def test_dropping_the_coupling_would_show_on_every_cluster_of_the_device_tests(name):
    """for every cluster of gpu_clusters(name), the whole cluster and its first two rows (the device tests stop there too): non-singular, conditioned,
    and a compensation without the off-diagonal terms of Omega_SS is off by more than 1e-3 on some kept row (two rows: PREFIX_DISCRIMINATION)"""
    t = grid(name)
    th, ms = measurement_set(name, t)
    base = S.Rebuilt(t, ms)
    clusters = gpu_clusters(name, t)
    assert len(clusters) >= 3
    seen = {2: [], 4: []}
    for rows in clusters:
        for k in (2, 4):
            rb = S.Rebuilt(t, ms, rows[:k])
            assert not rb.singular, (name, rows[:k])
            assert (rb.w * rb.variances())[kept(rb)].min() >= CONDITION, (name, rows[:k])
            seen[k].append(discrimination(base, rb, rows[:k]))
            assert seen[k][-1] > (DISCRIMINATION if k == 4 else PREFIX_DISCRIMINATION), (name, rows[:k], seen[k][-1])
    for k in (2, 4):
        print(name, "clusters", len(clusters), "rows", k, "least move", min(seen[k]), "median", float(np.median(seen[k])))


def test_three_rows_of_a_cluster_are_coupled_as_well():
    """the mixed-count test holds lanes with three rows: case118, every cluster"""
    t = grid("case118")
    th, ms = measurement_set("case118", t)
    base = S.Rebuilt(t, ms)
    moves = [discrimination(base, S.Rebuilt(t, ms, rows[:3]), rows[:3]) for rows in gpu_clusters("case118", t)]
    print("three rows: least move", min(moves), "median", float(np.median(moves)))
    assert min(moves) > PREFIX_DISCRIMINATION


def test_the_out_of_service_rows_sit_where_the_device_test_needs_them():
    t = grid("case118outage")
    th, ms = measurement_set("case118outage", t)
    dead = outage_rows(t)
    first = coupled_cluster(t, eligible_buses(t)[0])
    nw = ms.w_index.size
    assert sum(r < nw for r in dead) == 3 and sum(r >= nw for r in dead) == 1
    assert dead[0] not in first and dead[0] == first[1] + 1          # the to-wattmeter of the cluster's own branch
    rb = S.Rebuilt(t, ms)
    assert not rb.singular and np.all(rb.status[dead] == 0.0) and int(rb.status.sum()) == rb.status.size - 4


def test_the_twice_metered_leaf_turns_critical_at_the_second_of_its_two_meters():
    t = load_case("case14")
    th, ms, leaf, neighbour = twice_metered_leaf(t)
    base = S.Rebuilt(t, ms)
    for rows in ([], [0], [1], [4, 0]):
        assert not S.Rebuilt(t, ms, rows).singular, rows
    for rows in ([0, 1], [0, 4, 1], [4, 0, 1]):
        assert S.Rebuilt(t, ms, rows).singular, rows
        piv = ldl_pivots(base, rows)
        print(rows, piv)
        assert abs(piv[-1]) <= 1e-12 and np.all(piv[:-1] >= 1e-2), (rows, piv)
    for rows in ([0], [1], [4, 0], [4]):
        piv = ldl_pivots(base, rows)
        print(rows, piv)
        assert np.all(piv >= 1e-2), (rows, piv)
