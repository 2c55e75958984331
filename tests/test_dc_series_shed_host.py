"""Bridge candidates of the DC series and transfer screens on the slack's island (islands="shed"), host side (no device): the numpy restatement of the
algebra (tests/dc_series_shed_reference.py: z = B^-1 e_m on the unsplit grid, f_l = F0[l] + Z[l,k] s_k F0[k], 0 on what left) against the rebuild route
dc_island_reference.solve(t, out=k, injection=p), which rebuilds the model of the slack's component alone and never uses that identity.  Z, s_k and the
mask come from a search of the graph, not from the library's table.

Tolerance: |got - ref| <= 1e-9 * max(1, worst reference loading), the project's DC one.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import dc_island_reference as I
import dc_pair_reference as P
import dc_series_reference as S
import dc_series_shed_reference as H
import dc_transfer_reference as X
from conftest import load_case

TOL = 1e-9


def grid(name):
    return I.hand_grid()[0] if name == "hand_grid" else load_case(name)


def restatement_against_rebuild(t, br, prof, dirs):
    """every bridge of `br` x every profile (flows) and x every direction (sensitivities); returns the worst scaled deviations"""
    rating = P.rating_of(t)
    F0 = S.base_flows(t, prof)
    P0 = X.own_injection(t)
    f0 = R_solve(t, P0)
    G = np.stack([R_solve(t, P0 + d) - f0 for d in dirs], axis=1) if len(dirs) else np.zeros((f0.size, 0))
    z, y = H.unit_columns(t, [sp[1] for sp in br.values()])
    wf = wg = 0.0
    for k, sp in br.items():
        fr = H.shed_flows(t, k, sp, z[sp[1]], y, F0)
        keep = None
        for tt in range(prof.shape[0]):
            _, ref, keep = I.solve(t, out=k, injection=prof[tt])
            assert np.array_equal(keep, ~sp[0]), k                # the search of the restatement and the component of the rebuild route agree
            w, b, load = P.loading(ref, rating)
            gw, gb, gload = P.loading(fr[:, tt], rating)
            scale = max(1.0, w)
            dev = max(abs(gw - w), float(np.abs(gload - load).max())) / scale
            assert dev <= TOL, (k, tt, gw, w, dev)
            assert gb == b or abs(load[gb - 1] - w) <= TOL * scale, (k, tt, gb, b)
            assert np.all(fr[H._gone(t, sp[0], k), tt] == 0.0) and np.all(ref[H._gone(t, sp[0], k)] == 0.0)
            wf = max(wf, dev)
        if len(dirs):
            g = H.shed_sensitivity(t, k, sp, z[sp[1]], y, G)
            _, r0, _ = I.solve(t, out=k, injection=P0)
            for tt, d in enumerate(dirs):                         # the flows are affine in the injection: the difference is the sensitivity
                _, r1, _ = I.solve(t, out=k, injection=P0 + d)
                dev = float(np.abs(g[:, tt] - (r1 - r0)).max()) / max(1.0, float(np.abs(r1).max()), float(np.abs(r0).max()))
                assert dev <= TOL, (k, tt, dev)
                wg = max(wg, dev)
    return wf, wg


def R_solve(t, inj):
    return S.rebuild(t, None, inj)[1]


@pytest.mark.parametrize("case", ["hand_grid", "case14test", "case300"])
def test_the_restatement_agrees_with_the_rebuild_route_on_every_bridge(case):
    t = grid(case)
    br = H.bridges(t)
    oracle = S.bridges(t)                                         # components counted with the branch deleted
    assert sorted(br) == [int(k) for k in oracle] and len(br) > 0
    wf, wg = restatement_against_rebuild(t, br, S.profiles(t, 3), X.directions(t, 2))
    print(case, "bridges", len(br), "x 3 profiles: worst scaled deviation of the loadings", wf, "; x 2 directions: of the sensitivities", wg)


@pytest.mark.parametrize("case", ["hand_grid", "case14test", "case300", "case_ACTIVSg10k"])
def test_a_branch_other_than_the_bridge_with_one_end_in_what_leaves_has_both_ends_there(case):
    t = grid(case)
    br = H.bridges(t)
    bad = [k for k, sp in br.items() if not H.one_side(t, sp[0], k)]
    sizes = [int(sp[0].sum()) for sp in br.values()]
    print(case, "bridges", len(br), "largest side that leaves", max(sizes), "buses; bridges whose side is cut by another branch", len(bad))
    assert len(br) > 0 and not bad
    slack = I.R.slack_of(t)
    assert all(not sp[0][slack] and not sp[0][sp[1]] for sp in br.values())


def test_the_restatement_alone_passes_on_the_sample_of_the_large_grid():
    """the 32 seeded bridges x 8 profiles tests/test_dc_series_shed_gpu.py screens on the 10k-bus grid"""
    t = load_case("case_ACTIVSg10k")
    pick, br = H.sample(t)
    assert len(pick) == 32
    wf, _ = restatement_against_rebuild(t, pick, S.profiles(t, 8), [])
    print("case_ACTIVSg10k: bridges", len(br), "sample 32 x 8 profiles: worst scaled deviation of the loadings", wf)


def test_arguments_are_refused_before_the_device_is_touched():
    import juliagrid.jl_amd as jg
    t = load_case("case14test")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    prof = S.profiles(t, 2)
    for call in (lambda: jg.dcSeriesScreen(s, prof, rating=rating, islands="nonsense"),
                 lambda: jg.dcTransferScreen(s, X.directions(t, 1), rating=rating, islands="nonsense"),
                 lambda: jg.dcSeriesScreen(s, prof, rating=rating, demand=np.zeros_like(prof)),              # demand goes with islands="shed"
                 lambda: jg.dcSeriesScreen(s, prof, rating=rating, islands="shed", demand=np.zeros((3, 14)))):
        with pytest.raises(ValueError):
            call()
    every = jg.shedCandidates(s)
    assert np.array_equal(every, S.in_service(t) + 1) and every.size > jg.pairCandidates(s).size
