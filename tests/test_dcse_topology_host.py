"""The branch status tests (dcTopologyScreen) on the CPU: the two routes of tests/dcse_topology_reference.py agree with each other before either is used
as the oracle, the known answers of a flipped branch status hold, and the inputs of tests/test_dcse_topology_gpu.py are pinned: on every set a critical
branch sits at or below 1e-9 and every testable one at or above 1e-3 in D / (m' W m) -- three decades on either side of DCSE_SINGULAR = 1e-6, as
csrc/jg_dcse.hpp documents for single rows.  A set that fails this is to be changed, not the bounds.  No library compute here."""
import numpy as np
import pytest

import dc_reference as R
import dcse_reference as S
import dcse_topology_reference as T
from conftest import load_case

TOL = 1e-9
NAMES = list(T.FIXTURES)
_LANES = {}


def scaled(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0


def lanes_of(name):
    """(fixture, Z, roles, statistics of the restatement, threshold) of a set, computed once and shared; callers do not change them.  The threshold is
    half the smallest |t| of a planted branch, so that the records are the planted errors and what they drag along, never the noise"""
    if name not in _LANES:
        fx = T.fixture(name, load_case)
        Z, roles = T.lanes(fx)
        st = fx.dense.statistics(Z, fx.sc)
        pos = {int(k): q for q, k in enumerate(fx.cand)}
        planted = [abs(st.t[pos[k], l]) for l, (kind, k) in enumerate(roles) if kind in ("open", "close")]
        _LANES[name] = (fx, Z, roles, st, float(f"{0.5 * min(planted):.3g}"))
    return _LANES[name]


@pytest.mark.parametrize("name", NAMES)
def test_three_decades_on_either_side_of_the_threshold(name):
    fx = T.fixture(name, load_case)
    G = S.gain(fx.t, fx.ms).toarray()
    assert np.linalg.matrix_rank(G) == G.shape[0]
    sc = fx.sc
    ratio = sc.D / np.where(sc.norm > 0.0, sc.norm, 1.0)
    crit, ok = np.abs(ratio[sc.status == 1]), ratio[sc.status == 0]
    print(name, "rows", fx.status.size, "candidates", sc.cand.size, "status counts", np.bincount(sc.status, minlength=3), "critical <=",
          crit.max() if crit.size else None, "testable >=", ok.min())
    assert ok.size and ok.min() >= 1e-3 and (not crit.size or crit.max() <= 1e-9)
    assert int((fx.status == 0).sum()) >= 1 and int((np.asarray(fx.t["br_status"]) == 0).sum()) >= 1


def test_the_shapes_the_kernels_can_go_wrong_at():
    f14, f118, peg, mesh, comb = (T.fixture(n, load_case) for n in ("case14", "case118", "pegase777", "mesh", "comb"))
    assert f14.cand.size == 20 and f14.batch == 5 and T.fixture("case14 slack", load_case).batch == 1
    assert T.fixture("case14 slack", load_case).dense.va != 0.0 and f14.dense.va == 0.0
    assert f118.cand.size == 186 and f118.batch == 70 and f118.sc.status.max() == 0
    assert peg.cand.size == 1300 and peg.cand.size % 512 == 276 and peg.batch == 3 and np.any(peg.sc.status == 2)
    assert mesh.dense.va != 0.0 and np.count_nonzero(mesh.t["br_shift"]) >= 1          # a mix-up of the two residuals would show here
    for fx in (f14, comb):
        assert np.any(fx.sc.status == 1)                                               # critical branches: leaves without a PMU
    # parallel circuits that only injection meters see share a column; with a flow meter of their own they do not
    M = peg.dense.M
    ends = [tuple(sorted(p)) for p in zip(peg.t["br_from"].tolist(), peg.t["br_to"].tolist())]
    first = {}
    same = differ = 0
    for k, p in enumerate(ends):
        if p in first:
            j = first[p]
            sg = 1.0 if peg.t["br_from"][j] == peg.t["br_from"][k] else -1.0
            if np.any(M[:, k]):
                same += np.array_equal(M[:, k], sg * M[:, j])
                differ += not np.array_equal(M[:, k], sg * M[:, j])
        first.setdefault(p, k)
    assert same >= 1 and differ >= 1, (same, differ)


def test_the_columns_at_their_edges():
    """a bus with two injection meters (both counted), a meter out of service (0), a twin with and without a flow meter, a branch nobody sees, a
    candidate out of service in the model"""
    t = dict(load_case("case14"))
    t["br_from"], t["br_to"] = np.r_[t["br_from"], t["br_from"][0]], np.r_[t["br_to"], t["br_to"][0]]      # a twin of branch 1
    for k in ("br_status", "br_r", "br_x", "br_g", "br_b", "br_tap", "br_shift"):
        t[k] = np.r_[t[k], t[k][0]]
    t["br_status"] = np.asarray(t["br_status"]).copy()
    t["br_status"][2] = 0
    f, to = int(t["br_from"][0]), int(t["br_to"][0])
    th, _ = R.solve(t)
    full = S.full_set(t, th)
    n = t["bus_type"].size
    ms = S.meters(np.r_[full.w_kind[:n], 0, 1, 2, 1], np.r_[full.w_index[:n], f, 1, 1, 3], np.r_[full.w_mean[:n], full.w_mean[f - 1], 0.0, 0.0, 0.0],
                  np.full(n + 4, 1e-2), np.r_[np.ones(n + 2), 0, 1], full.p_index, None, full.p_angle, full.p_variance)
    M = T.columns(t, ms)
    twin = M.shape[1] - 1
    assert M[f - 1, 0] == 1.0 and M[n, 0] == 1.0 and M[to - 1, 0] == -1.0                 # two injection meters at from(1), both counted
    assert M[n + 1, 0] == 1.0 and M[n + 2, 0] == 0.0                                       # its from-end meter; the to-end meter is out of service
    assert M[n + 1, twin] == 0.0 and np.array_equal(np.delete(M[:, twin], n + 1), np.delete(M[:, 0], n + 1))     # unequal only by the flow meter
    assert M[n + 3, 2] == 1.0 and np.count_nonzero(M[:, 2]) >= 3                           # out of service in the model: its meters still count
    assert not np.any(M[n + 4:])                                                           # PMUs
    ms.w_status[:n] = 0
    M = T.columns(t, ms)
    assert np.count_nonzero(M[:, 5]) == 0                                                  # seen by nothing: status 2
    D = T.Dense(t, S.meters(ms.w_kind, ms.w_index, ms.w_mean, ms.w_variance, ms.w_status, full.p_index, None, full.p_angle, full.p_variance))
    assert D.screen(np.array([5])).status[0] == 2


@pytest.mark.parametrize("name", NAMES)
def test_the_two_routes_agree(name):
    """formulas on a dense inverse of the gain against least squares on the widened matrix: phi, the drop of the objective = t^2, the corrected angles"""
    fx, Z, roles, st, _ = lanes_of(name)
    pos = {int(k): q for q, k in enumerate(fx.cand)}
    ok = np.flatnonzero(fx.sc.status == 0)
    sample = sorted(set(ok[np.linspace(0, ok.size - 1, min(ok.size, 12)).astype(int)].tolist()) | {pos[k] for kind, k in roles if kind in ("open", "close")})
    worst = dict(phi=0.0, drop=0.0, angle=0.0)
    for l in range(min(fx.batch, 5)):
        for q in sample:
            phi, th, drop = fx.dense.augmented(Z[l], int(fx.cand[q]))
            worst["phi"] = max(worst["phi"], scaled(st.phi[q, l], phi))
            worst["drop"] = max(worst["drop"], scaled(st.t[q, l] ** 2, drop))
            worst["angle"] = max(worst["angle"], scaled(fx.dense.corrected(st, fx.sc, q, l), th))
    print(name, "candidates compared", len(sample), "worst scaled deviations", worst)
    assert max(worst.values()) <= TOL


@pytest.mark.parametrize("name", ["case14", "case14 slack", "mesh"])
def test_known_answers_of_a_flipped_status(name):
    """noise-free readings of the grid with branch k open while the model holds it closed: r = -S m_k f_k, so phi^ = -f_k with f_k the model's flow on k
    at the corrected estimate, t^2 is the whole objective and the corrected angles are the true ones.  The mirror, k modelled open and really closed:
    phi^ = + the true flow"""
    fx = T.fixture(name, load_case)
    pos = {int(k): q for q, k in enumerate(fx.cand)}
    y = R.admittance(fx.t)
    f, to = np.asarray(fx.t["br_from"]).astype(int) - 1, np.asarray(fx.t["br_to"]).astype(int) - 1
    sh = np.asarray(fx.t["br_shift"], dtype=np.float64)
    for k in T.plantable(fx, True, 2):
        z, truth, _ = T.readings(fx, k)
        st = fx.dense.statistics(z, fx.sc)
        q = pos[k]
        th = fx.dense.corrected(st, fx.sc, q, 0)
        fk = y[k] * (th[f[k]] - th[to[k]] - sh[k])
        assert abs(fk) > 1e-3
        assert scaled(st.phi[q, 0], -fk) <= TOL and scaled(st.t[q, 0] ** 2, st.objective[0]) <= TOL and scaled(th, truth) <= TOL
        assert scaled(fx.dense.augmented(z, k)[0], -fk) <= TOL
    for k in T.plantable(fx, False, 1):
        z, truth, flow = T.readings(fx, k)
        st = fx.dense.statistics(z, fx.sc)
        q = pos[k]
        assert abs(flow[k]) > 1e-3
        assert scaled(st.phi[q, 0], flow[k]) <= TOL and scaled(st.t[q, 0] ** 2, st.objective[0]) <= TOL
        assert scaled(fx.dense.corrected(st, fx.sc, q, 0), truth) <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_the_lanes_of_the_gpu_test(name):
    """the planted branch is the restatement's best in its lane or ties with it, stands well clear of the noise, and nothing sits on the threshold"""
    fx, Z, roles, st, thr = lanes_of(name)
    pos = {int(k): q for q, k in enumerate(fx.cand)}
    a = np.abs(np.where(np.isnan(st.t), 0.0, st.t))
    kinds = [kind for kind, _ in roles]
    assert kinds.count("open") + kinds.count("close") >= 1 and (fx.batch < 3 or ("meter" in kinds and "clean" in kinds))
    for l, (kind, k) in enumerate(roles):
        if kind in ("open", "close"):
            assert a[pos[k], l] >= a[:, l].max() * (1.0 - 1e-9), (l, kind, k)
        if kind == "clean":
            assert a[:, l].max() < thr / 5.0
    assert np.abs(a - thr).min() > 1e-6 * thr
    order = np.sort(a, axis=0)
    clear = order[-1] - order[-2] > 1e-6 * order[-1]                  # where the GPU test compares `best`: at most 5 % of the lanes are left out, no planted one
    assert (~clear).sum() <= 0.05 * fx.batch and all(clear[l] for l, (kind, _) in enumerate(roles) if kind in ("open", "close"))
    print(name, "threshold", thr, "records", int((a[:, :fx.batch] >= thr).sum()), "roles", roles[:5])


def test_the_restatement_never_uses_the_block_scheme():
    src = open(T.__file__).read().split('"""', 2)[2]
    assert "splu" not in src and "OMEGA_LD" not in src and "linalg.inv" in src and "lstsq" in src
