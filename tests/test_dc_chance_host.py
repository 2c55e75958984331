"""The DC probabilistic N-1 screen, host side (no device): the screen's formula restated in numpy on a dense Phi against the rebuild-and-refactorise
route of tests/dc_chance_reference.py, the reason for the direct sum of squares on a series-connected pair, a Monte-Carlo over the rebuild route,
injectionFactors, and the argument checks of dcChanceScreen that run before the device is touched.

Tolerance: max |got - ref| <= 1e-9 * max(1, max |ref|), TOL and the measure of tests/test_dc_pair_gpu.py.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_chance_reference as Q
import dc_grids as G
import dc_pair_reference as P
import dc_reference as R

TOL = 1e-9


@pytest.mark.parametrize("name", ["case14test", "case30test", "case118"])
def test_the_formula_on_a_dense_phi_agrees_with_the_rebuild_route(name):
    g = Q.grid(name)
    t, cand = g["t"], g["cand"]
    Phi, f0, _ = P.sensitivities(t, cand)
    assert R.worst(f0, g["base"][0]) <= TOL
    S0 = g["base"][1]
    br = set(int(b) for b in Q.bridges(t))
    worst = 0.0
    for i, k in enumerate(cand):
        got = Q.formula(Phi, f0, S0, cand, i)
        if g["mom"][i] is None:
            assert k in br and got is None, k
            continue
        mu, S = g["mom"][i]
        sigma = np.sqrt((S ** 2).sum(axis=1))
        dev = max(R.worst(got[0], mu), R.worst(got[1], sigma))
        assert dev <= TOL, (k, dev)
        assert mu[k] == 0.0 and sigma[k] == 0.0                   # the rebuild route: an outaged branch carries nothing, with certainty
        worst = max(worst, dev)
    print(name, "candidates", len(cand), "bridges", sum(m is None for m in g["mom"]), "worst scaled deviation of the formula from the rebuild route", worst)
    assert 0 < sum(m is None for m in g["mom"]) < len(cand)
    assert g["L"][0, R.slack_of(t)] != 0.0                        # a factor with a slack entry was part of it


@pytest.mark.parametrize("name", Q.GRIDS)
def test_few_reference_records_lie_near_the_probability_the_device_tests_use(name):
    """what tests/test_dc_chance_gpu.py leaves out of its comparison of record sets is at most 1 % of the reference records, for the seeds it uses"""
    g = Q.grid(name)
    on = np.flatnonzero(np.asarray(g["t"]["br_status"]) == 1)
    for r in (8, 32):
        rec, near = Q.records_of(Q.cut(g["mom"], r), g["cand"], g["rating"], on, Q.PROBABILITY)
        print(name, "r", r, "reference records", len(rec), "within", Q.NEAR, "of the threshold", near)
        assert len(rec) >= 5 and near <= 0.01 * len(rec)
        assert rec == sorted(rec, key=lambda x: (x[0], x[1]))


def series_pair(t):
    """(k, m, b): the two in-service branches at a bus b of degree 2 that is not the slack, neither of them a bridge"""
    f, to, on = np.asarray(t["br_from"]) - 1, np.asarray(t["br_to"]) - 1, np.asarray(t["br_status"]) == 1
    br = set(int(x) for x in Q.bridges(t))
    for b in range(t["bus_type"].size):
        at = np.flatnonzero(on & ((f == b) | (to == b)))
        if b != R.slack_of(t) and at.size == 2 and not (set(at.tolist()) & br):
            return int(at[0]), int(at[1]), b
    raise AssertionError("no series pair")


def test_a_series_pair_is_certain_by_the_direct_sum_and_not_by_the_expanded_form():
    """Branches k and m meet at a bus of degree 2 that no factor touches: they carry the same uncertain flow, and with k out m carries the bus's own
    certain injection.  The ring family has such pairs that are no bridges (on the path and comb families every series branch is a bridge: status 3).
    scale: the base-case sigma of m, the size of what cancels.  The direct sum of the squared combined sensitivities gives sigma <= 1e-12 x scale; the
    variance expanded over a Gram matrix gives more than 1e-9 x scale -- the reason csrc/jg_dc_chance.hpp and DESIGN.md 3.18 give for the direct sum."""
    t = G.family("ring 17")
    k, m, b = series_pair(t)
    L = Q.factors(t, 32, Q.SEED)
    L[:, b] = 0.0
    assert np.abs(L).sum(axis=0)[[x for x in range(L.shape[1]) if x != R.slack_of(t)]].max() > 0
    cand = [k, m]
    Phi, f0, _ = P.sensitivities(t, cand)
    S0 = Q.rebuild(t, None, Q.own_injection(t), L)[1]
    scale = float(np.sqrt((S0[m] ** 2).sum()))
    ref = Q.rebuild(t, k, Q.own_injection(t), L)
    ref_sigma = float(np.sqrt((ref[1][m] ** 2).sum()))
    direct = float(Q.formula(Phi, f0, S0, cand, 0)[1][m])
    wide = float(np.sqrt(abs(Q.expanded(Phi, S0, cand, 0)[m])))
    print("ring 17: k", k + 1, "m", m + 1, "bus", b + 1, "base sigma of m (scale)", scale, "rebuild route", ref_sigma, "direct sum", direct, "expanded form", wide)
    assert scale > 1e-3
    assert ref_sigma <= 1e-12 * scale and direct <= 1e-12 * scale
    assert wide > 1e-9 * scale


def test_a_monte_carlo_over_the_rebuild_route_agrees_with_the_probability():
    """200 000 seeded samples of p0 + L' xi on case14test, solved on the rebuilt and refactorised matrix per candidate: the frequency of |flow| > rating on
    the five (k, m) whose P is nearest 0.5 lies within 4 binomial standard errors of P."""
    g = Q.grid("case14test")
    t, cand, rating = g["t"], g["cand"], g["rating"]
    r, T = 8, 200_000
    mom = Q.cut(g["mom"], r)
    cases = []
    for i, k in enumerate(cand):
        if mom[i] is None:
            continue
        p = Q.probability(mom[i][0], np.sqrt((mom[i][1] ** 2).sum(axis=1)), rating)
        cases += [(abs(p[m] - 0.5), k, m, float(p[m])) for m in np.flatnonzero(rating > 0) if m != k]
    cases.sort()
    xi = np.random.default_rng(99).standard_normal((T, r))
    inj = g["p0"][None, :] + xi @ g["L"][:r]
    for _, k, m, p in cases[:5]:
        freq = float((np.abs(Q.sample_flows(t, k, inj)[:, m]) > rating[m]).mean())
        se = np.sqrt(p * (1.0 - p) / T)
        print("outage", k + 1, "branch", m + 1, "P", p, "frequency", freq, "deviation in standard errors", abs(freq - p) / se)
        assert 0.05 < p < 0.95 and abs(freq - p) <= 4.0 * se


def test_injection_factors_reproduce_the_covariance_and_refuse_what_they_cannot_factor():
    import juliagrid.jl_amd as jg
    t = Q.grid("case30test")["t"]
    s = jg.powerSystem(t)
    n = t["bus_type"].size
    buses = [3, 7, 8, 21, 30]
    std = np.array([0.1, 0.2, 0.05, 0.3, 0.15])
    for rho in (0.0, 0.4, -0.2, 1.0, -0.25):
        L = jg.injectionFactors(s, buses, std, correlation=rho)
        assert L.shape == (5, n)
        C = np.zeros((n, n))
        idx = np.array(buses) - 1
        C[np.ix_(idx, idx)] = np.outer(std, std) * np.where(np.eye(5) > 0, 1.0, rho)
        dev = float(np.abs(L.T @ L - C).max())
        print("correlation", rho, "max |L' L - C|", dev)
        assert dev <= 1e-14
    one = jg.injectionFactors(s, [5], 0.2)
    assert one.shape == (1, n) and one[0, 4] == 0.2 and np.count_nonzero(one) == 1
    with pytest.raises(ValueError, match="32 at the most"):
        jg.injectionFactors(jg.powerSystem(Q.grid("case118")["t"]), list(range(1, 34)), 0.1)
    for rho in (-0.3, 1.5):
        with pytest.raises(ValueError, match="indefinite"):
            jg.injectionFactors(s, buses, std, correlation=rho)


def test_bad_arguments_are_refused_on_the_host_and_the_names_are_exported():
    import juliagrid.jl_amd as jg
    assert {"dcChanceScreen", "injectionFactors", "DC_CHANCE_MAX"} <= set(jg.__all__) and jg.DC_CHANCE_MAX == 32
    g = Q.grid("case14test")
    s = jg.powerSystem(g["t"])
    n = g["t"]["bus_type"].size
    for kw, text in ((dict(factors=np.zeros((33, n))), "33 factors, 1 to 32"), (dict(factors=np.zeros((0, n))), "0 factors, 1 to 32"),
                     (dict(factors=np.zeros((2, n + 1))), "[r, buses]"), (dict(factors=g["L"][:2], islands="shed"), "no shed mode"),
                     (dict(factors=g["L"][:2], probability=0.0), "0 < probability <= 1"), (dict(factors=g["L"][:2], injection=np.zeros(n + 1)), "injection must be")):
        with pytest.raises(ValueError) as e:
            jg.dcChanceScreen(s, rating=g["rating"], **kw)
        print(e.value)
        assert text in str(e.value)
