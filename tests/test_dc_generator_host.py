"""The host side of the DC generator-outage screen (juliagrid.jl_amd/dcgenerator.py) and its numpy restatement (tests/dc_generator_reference.py), without
a device: the restatement's G-1 flows against a plain DC solve of the host model with the unit's status set to 0; the capped re-sharing; the default
generator list; the column sums of A; the argument checks that are refused before the device is touched; and the share of the test grids' cases the two
guards of the device comparison take out (it must stay within 2 %)."""
import numpy as np
import pytest
import scipy.sparse.linalg as sla

import dc_generator_reference as X
import dc_pair_reference as P
import dc_reference as R
from conftest import load_case


def host_model_flows(jg, s):
    """from-end flows of a plain DC solve of the host model `s` as it stands (dcPowerFlow.jl:63-101, dcAnalysis.jl:41-48)"""
    from juliagrid.jl_amd.dcpowerflow import _base_rhs
    if s.model.dc.nodalMatrix is None:
        jg.dcModel_(s)
    n, slack = s.bus.number, s.bus.layout.slack - 1
    keep = np.r_[0:slack, slack + 1:n]
    B = s.model.dc.nodalMatrix.toscipy().tocsc()
    th = np.zeros(n)
    th[keep] = sla.splu(B[keep][:, keep].tocsc()).solve(_base_rhs(s)[keep])
    th += s.bus.voltage.angle[slack]
    f, to = s.branch.layout.from_ - 1, s.branch.layout.to - 1
    return s.model.dc.admittance * (th[f] - th[to] - s.branch.parameter.shiftAngle)


@pytest.mark.parametrize("case", ["case14test", "case30test"])
def test_g1_flows_of_the_restatement_equal_a_plain_solve_with_the_unit_out(jg, case):
    t = load_case(case)
    worst = 0.0
    for g in X.candidates(t):
        s = jg.powerSystem(t)
        jg.updateGeneratorSystem_(s, int(g) + 1, status=0)
        want = host_model_flows(jg, s)
        got = X.flows(t, X.change(t, int(g))[0])
        worst = max(worst, float(np.abs(got - want).max()))
    print(case, "G-1 flows: restatement against the host model with status = 0, worst deviation", worst)
    assert worst <= 1e-12


def test_capped_resharing():
    rng = np.random.default_rng(5)
    for trial in range(200):
        m = int(rng.integers(1, 9))
        w = rng.random(m) * (rng.random(m) > 0.2)
        room = rng.random(m) * (rng.random(m) > 0.2)
        lost = float(rng.random() * 2.5 * max(room.sum(), 0.1))
        from juliagrid.jl_amd.dcgenerator import shareLoss
        take, short = shareLoss(lost, w, room)
        want, wshort = X.share_loss(lost, list(w), list(room))
        assert abs(take.sum() + short - lost) <= 8 * np.finfo(float).eps * max(1.0, lost), (trial, take, short, lost)       # conserves Pg to rounding
        assert (take <= room).all() and (take >= 0).all() and (take[w == 0] == 0).all() and short >= 0                         # never beyond a headroom
        assert np.allclose(take, want, rtol=0, atol=1e-14) and abs(short - wshort) <= 1e-14
        if lost >= room[w > 0].sum():                                                                                          # all headroom exhausted
            assert np.array_equal(take[w > 0], room[w > 0]) and abs(short - (lost - room[w > 0].sum())) <= 1e-14
        else:
            assert short == 0.0
        free = (w > 0) & (take < room)
        if free.sum() > 1 and short == 0.0:                                                                                    # the uncapped share by the weights
            r = take[free] / w[free]
            assert np.ptp(r) <= 1e-12 * max(1.0, r.max())
    take, short = shareLoss(-0.7, np.array([1.0, 3.0]), np.array([0.0, 0.1]))      # a unit that absorbed power: shared by the weights, no cap bites
    assert np.allclose(take, [-0.175, -0.525]) and short == 0.0
    take, short = shareLoss(1.0, np.zeros(3), np.ones(3))                         # nobody takes part
    assert not take.any() and short == 1.0


def test_default_generators_leave_out_the_slacks_last_unit_and_units_out_of_service(jg):
    for case in ("case14test", "case30test", "case118"):
        t = load_case(case)
        s = jg.powerSystem(t)
        assert np.array_equal(jg.generatorCandidates(s), X.candidates(t) + 1), case
    t = load_case("case118")                                          # ONE unit on the slack bus
    s = jg.powerSystem(t)
    slack = s.bus.layout.slack
    at = np.flatnonzero((s.generator.layout.bus == slack) & (s.generator.layout.status == 1)) + 1
    assert at.size == 1 and at[0] not in jg.generatorCandidates(s) and jg.generatorCandidates(s).size == int((s.generator.layout.status == 1).sum()) - 1
    t2 = X.with_generators(t, [slack], [0.3])                         # a second one: both may go (one at a time)
    s2 = jg.powerSystem(t2)
    assert at[0] in jg.generatorCandidates(s2) and t2["gen_bus"].size in jg.generatorCandidates(s2)
    off = int(np.flatnonzero(np.asarray(load_case("case14test")["gen_status"]) == 0)[0]) + 1
    assert off not in jg.generatorCandidates(jg.powerSystem(load_case("case14test")))


@pytest.mark.parametrize("pickup", ["slack", "participation"])
def test_column_sums_of_the_injection_changes(jg, pickup):
    t = dict(load_case("case30test"))
    pg = np.asarray(t["gen_pg"], dtype=np.float64)
    t["gen_pmax"] = pg + np.linspace(0.0, 0.4, pg.size)               # little headroom: units cap, and the large unit leaves a shortfall
    s = jg.powerSystem(t)
    sh = jg.pickupShare(s, pickup=pickup)
    A = sh.A.toarray()
    slack = R.slack_of(t)
    assert sh.buses.size == A.shape[0] and slack + 1 not in sh.buses and np.array_equal(sh.generators, X.candidates(t) + 1)
    assert np.abs(A.sum(axis=0) + sh.shortfall + sh.slackShare).max() <= 1e-14 * max(1.0, np.abs(sh.lost).max())
    for j, g in enumerate(sh.generators - 1):
        d, take, short = X.change(t, int(g), pickup)
        full = np.zeros(t["bus_type"].size)
        full[sh.buses - 1] = A[:, j]
        d_rest = d.copy()
        d_rest[slack] = 0.0
        assert np.abs(full - d_rest).max() <= 1e-14 and abs(short - sh.shortfall[j]) <= 1e-14
        assert abs(d[slack] - sh.slackShare[j]) <= 1e-14 if pickup == "participation" else sh.slackShare[j] == (0.0 if t["gen_bus"][g] - 1 == slack else pg[g])
        assert np.abs(sh.take.toarray()[:, j] - take).max() <= 1e-14
    if pickup == "participation":
        assert (sh.shortfall > 0).any() and (sh.shortfall == 0).any()
    else:
        assert not sh.shortfall.any() and sh.take.nnz == 0 and (np.count_nonzero(A, axis=0) <= 1).all()


def test_slack_generation_of_the_host_routine(jg):
    from juliagrid.jl_amd.dcgenerator import _slack_generation
    for case in ("case14test", "case30test"):
        t = load_case(case)
        s = jg.powerSystem(t)
        jg.dcModel_(s)
        assert abs(_slack_generation(s) - X.slack_generation(t, np.zeros(t["bus_type"].size))) <= 1e-12


def test_bad_arguments_are_refused_before_the_device(jg):
    t = load_case("case14test")
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    ng = t["gen_bus"].size
    slack = R.slack_of(t) + 1
    off = int(np.flatnonzero(np.asarray(t["gen_status"]) == 0)[0]) + 1
    t1 = dict(t)
    t1["gen_status"] = np.where((np.asarray(t["gen_bus"]) == slack) & (np.arange(ng) > 0), 0, t["gen_status"]).astype(np.int8)      # one unit left on the slack bus
    s1 = jg.powerSystem(t1)
    with pytest.raises(ValueError, match="generator 1 is the last in-service unit of the slack bus"):
        jg.dcGeneratorScreen(s1, generators=[1, 4], rating=rating)
    with pytest.raises(ValueError, match=f"generator {off} is out of service"):
        jg.dcGeneratorScreen(s, generators=[off], rating=rating)
    for bad in ([0], [ng + 1]):
        with pytest.raises(IndexError):
            jg.dcGeneratorScreen(s, generators=bad, rating=rating)
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s, generators=[], rating=rating)
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s, rating=rating, pickup="nobody")
    for bad in (np.ones(ng - 1), -np.ones(ng), np.full(ng, np.nan)):
        with pytest.raises(ValueError):
            jg.dcGeneratorScreen(s, rating=rating, pickup="participation", participation=bad)
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s, rating=rating, participation=np.ones(ng))          # participation without the pickup that reads it
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s)                                                     # no rating
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s, rating=rating, islands="nonsense")
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s, rating=rating, threshold=-1.0)
    with pytest.raises(IndexError):
        jg.dcGeneratorScreen(s, rating=rating, candidates=[1, 99])
    with pytest.raises(ValueError):
        jg.dcGeneratorScreen(s, rating=rating, candidates=[1, 2], rows=(2, 1))


def test_the_guards_take_out_at_most_two_percent_of_the_restatements_cases():
    """the ratings and thresholds of tests/test_dc_generator_gpu.py, on the restatement alone"""
    for case, thr in (("case14test", X_THRESHOLD["case14test"]), ("case30test", X_THRESHOLD["case30test"])):
        t = grid(case)
        e = X.expect(t, P.rating_of(t), X.candidates(t), default_candidates(t), thr, "participation")
        share = X.excluded_share(e)
        viol = int((e["load"] > thr).sum())
        print(case, "cases", e["load"].size, "violating", viol, "excluded by the guards", share)
        assert share <= 0.02 and 0 < viol < e["load"].size


X_THRESHOLD = {"case14test": 1.7, "case30test": 0.76}           # near the upper quartile of the cases' worst loadings


def grid(case):
    """the test grids with headroom that makes units cap: maxActive = output + a few hundredths to tenths"""
    t = dict(load_case(case))
    pg = np.asarray(t["gen_pg"], dtype=np.float64)
    t["gen_pmax"] = pg + 0.02 + 0.3 * np.random.default_rng(2).random(pg.size)
    return t


def default_candidates(t):
    """0-based in-service branches that are neither bridges nor self-loops (pairCandidates)"""
    import dc_series_reference as S
    f, to = np.asarray(t["br_from"]), np.asarray(t["br_to"])
    br = set(int(k) for k in S.bridges(t))
    return np.array([k for k in S.in_service(t) if k not in br and f[k] != to[k]], dtype=np.int64)
