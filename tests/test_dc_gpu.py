"""DC power flow and the batched DC N-1 screen on the device against the numpy / scipy restatement (tests/dc_reference.py), which REBUILDS and
refactorises the matrix for every outage -- the library never does (one shared factor + a rank-1 correction per lane, csrc/jg_dc.hpp).

Tolerance of every lane-by-lane comparison: max |got - ref| <= 1e-9 * max(1, max |ref|), the tolerance the project holds its linear step to; two
correct f64 routes differ by <= 1.2e-12 on these grids.  Goldens: the reference's own criterion (isapprox default)."""
import ctypes as C
import os

import numpy as np
import pytest

import dc_reference as R
from conftest import GOLDEN, load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9


def dc_golden(case):
    with np.load(os.path.join(GOLDEN, f"results_dc_{case}.npz")) as z:
        return {k: z[k] for k in z.files}


def check_lanes(jg, t, an, labels, injection=None, skip=()):
    """every lane of a solved batch against a rebuilt-and-refactorised solve: angles and flows; returns the worst scaled differences"""
    jg.power_(an)
    th = np.atleast_2d(an.voltage.angle)
    fr = np.atleast_2d(an.power.from_.active)
    cache, wa, wf = {}, 0.0, 0.0
    for s, lab in enumerate(labels):
        if s in skip:
            continue
        inj = None if injection is None or injection[s] is None else injection[s]
        key = (int(lab), s if inj is not None else -1)
        if key not in cache:
            cache[key] = R.solve(t, out=int(lab) - 1 if lab else None, injection=inj)
        rth, rfr = cache[key]
        assert rth is not None, (s, lab)
        a, f = R.worst(th[s], rth), R.worst(fr[s], rfr)
        assert a <= TOL and f <= TOL, (s, int(lab), a, f)
        wa, wf = max(wa, a), max(wf, f)
    print("worst angle", wa, "worst flow", wf, "lanes", len(labels) - len(skip))
    return wa, wf


@pytest.mark.parametrize("case", ["case14test", "case30test"])
@pytest.mark.parametrize("batch", [1, 64, 100])
def test_goldens_on_the_device(jg, case, batch):
    t, g = load_case(case), dc_golden(case)
    an = jg.dcPowerFlow(jg.powerSystem(t), batch=batch)
    jg.powerFlow_(an, power=True)
    for s in range(batch):
        lane = (lambda a: np.atleast_2d(a)[s])
        for name, got in (("voltage", an.voltage.angle), ("from", an.power.from_.active), ("injection", an.power.injection.active),
                          ("supply", an.power.supply.active), ("generator", an.power.generator.active)):
            assert R.isapprox(lane(got), g[name]), (s, name)
        assert np.array_equal(lane(an.power.to.active), -lane(an.power.from_.active))
    assert np.all(np.asarray(an.status) == 0)
    an.close()


@pytest.mark.parametrize("case", ["case118", "case300", "case1354pegase", "case_ACTIVSg10k", "case9241synth"])
def test_single_solve_against_the_restatement(jg, case):
    t = load_case(case)
    an = jg.dcPowerFlow(jg.powerSystem(t))
    jg.solve_(an)
    jg.power_(an)
    rth, rfr = R.solve(t)
    a, f = R.worst(an.voltage.angle, rth), R.worst(an.power.from_.active, rfr)
    print(case, "angle", a, "flow", f, an.dims())
    assert an.status == 0 and a <= TOL and f <= TOL
    pw = R.power(t, rth)
    for name in ("injection", "supply", "generator"):
        assert R.worst(getattr(an.power, name).active, pw[name]) <= TOL, name
    an.close()


@pytest.mark.parametrize("case", ["case14", "case118", "case300"])
def test_n_minus_1_over_every_in_service_branch(jg, case):
    t = load_case(case)
    s = jg.powerSystem(t)
    labels = np.flatnonzero(s.branch.layout.status == 1) + 1
    an = jg.contingencyAnalysis(s, labels, method="dc")
    is_bridge = jg.bridges(s)
    want = {i for i, lab in enumerate(labels) if is_bridge[lab - 1]}
    got = {int(i) for i in np.flatnonzero(np.asarray(an.status) == 3)}
    assert got == want, (sorted(got), sorted(want))              # status 3 exactly on the bridges: the only lanes left out below
    assert set(np.unique(an.status)) <= {0, 3}
    if case == "case118":
        assert len(want) == 9 and labels.size == 186
    check_lanes(jg, t, an, labels, skip=want)
    an.close()


@pytest.mark.parametrize("case,lanes", [("case1354pegase", 512), ("case_ACTIVSg10k", 512), ("case_ACTIVSg10k", 640)])
def test_n_minus_1_over_an_outage_list(jg, case, lanes):
    t = load_case(case)
    s = jg.powerSystem(t)
    labels = jg.outageList(s, lanes)
    an = jg.contingencyAnalysis(s, labels, method="dc")
    assert np.all(np.asarray(an.status) == 0)                     # outageList leaves the bridges out: no lane is skipped
    check_lanes(jg, t, an, labels)
    an.close()


def _screen(jg, case, labels):
    t = load_case(case)
    s = jg.powerSystem(t)
    an = jg.contingencyAnalysis(s, labels, method="dc")
    return t, s, an


def test_outage_of_a_branch_with_a_shift_angle(jg):
    for case, count in (("case14test", 2), ("case1354pegase", 6), ("case_ACTIVSg10k", 5)):
        t = load_case(case)
        k = np.flatnonzero((t["br_shift"] != 0) & (t["br_status"] == 1))
        assert k.size == count
        s = jg.powerSystem(t)
        ok = k[~jg.bridges(s)[k]]
        assert ok.size
        t, s, an = _screen(jg, case, list(ok + 1) + [0])
        assert np.all(np.asarray(an.status) == 0)
        check_lanes(jg, t, an, list(ok + 1) + [0])
        an.close()


def test_outage_of_a_branch_at_the_slack_bus(jg):
    for case in ("case14", "case118", "case1354pegase"):             # (the one branch at the slack of case300 and of case_ACTIVSg10k is a bridge)
        t = load_case(case)
        s = jg.powerSystem(t)
        at = np.flatnonzero(((s.branch.layout.from_ == s.bus.layout.slack) | (s.branch.layout.to == s.bus.layout.slack)) & (s.branch.layout.status == 1)
                            & ~jg.bridges(s))
        assert at.size
        labels = list(at + 1)
        an = jg.contingencyAnalysis(s, labels, method="dc")
        assert np.all(np.asarray(an.status) == 0)
        check_lanes(jg, t, an, labels)
        an.close()


def test_outage_of_one_of_two_parallel_branches(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    pair = {}
    for k in range(s.branch.number):
        if s.branch.layout.status[k] == 1:
            pair.setdefault(tuple(sorted((int(s.branch.layout.from_[k]), int(s.branch.layout.to[k])))), []).append(k)
    par = [v for v in pair.values() if len(v) == 2]
    assert len(par) == 7
    labels = [v[0] + 1 for v in par] + [v[1] + 1 for v in par]
    an = jg.contingencyAnalysis(s, labels, method="dc")
    assert np.all(np.asarray(an.status) == 0)
    check_lanes(jg, t, an, labels)
    an.close()


def test_outage_of_a_branch_that_is_already_out_of_service(jg):
    t = load_case("case14test")
    off = np.flatnonzero(t["br_status"] != 1)
    assert off.size == 2
    s = jg.powerSystem(t)
    an = jg.contingencyAnalysis(s, [0] + list(off + 1), method="dc")
    assert np.all(np.asarray(an.status) == 0)
    assert np.array_equal(an.voltage.angle[1], an.voltage.angle[0]) and np.array_equal(an.voltage.angle[2], an.voltage.angle[0])   # a no-op
    check_lanes(jg, t, an, [0] + list(off + 1))
    an.close()


def test_lanes_without_an_outage_mixed_in(jg):
    t = load_case("case300")
    s = jg.powerSystem(t)
    labels = jg.outageList(s, 70)
    labels[::3] = 0
    an = jg.contingencyAnalysis(s, labels, method="dc")
    single = jg.dcPowerFlow(s)
    jg.solve_(single)
    for i in np.flatnonzero(labels == 0):
        assert np.array_equal(an.voltage.angle[i], single.voltage.angle)
    check_lanes(jg, t, an, labels)
    an.close()
    single.close()


def test_a_slack_angle_that_is_not_zero(jg):
    for case, angle in (("case118", 0.5236), ("case_ACTIVSg10k", -0.8623)):
        t = load_case(case)
        assert abs(t["bus_va"][R.slack_of(t)] - angle) < 1e-4
        s = jg.powerSystem(t)
        labels = jg.outageList(s, 8)
        an = jg.contingencyAnalysis(s, labels, method="dc")
        assert np.all(an.voltage.angle[:, s.bus.layout.slack - 1] == t["bus_va"][R.slack_of(t)])
        check_lanes(jg, t, an, labels)
        an.close()


def test_per_scenario_injections_with_and_without_an_outage(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    rng = np.random.default_rng(7)
    labels = jg.outageList(s, 130)
    labels[5] = 0
    labels[70] = 0
    an = jg.dcPowerFlow(s, batch=130)
    jg.setOutages_(an, labels)
    base = s.bus.supply.active - s.bus.demand.active
    own = {3: None, 5: None, 69: None, 70: None, 71: None}           # lanes 3, 69, 71 also lose a branch; lane group 1 (64 .. 127) and 0 pay the second sweep pair, group 2 does not
    for lane in own:
        own[lane] = base * (1.0 + 0.1 * rng.standard_normal(base.size))
    jg.setInjection_(an, np.array([own[3]]), scenario0=3)
    jg.setInjection_(an, np.array([own[5]]), scenario0=5)
    jg.setInjection_(an, np.array([own[69], own[70], own[71]]), scenario0=69)
    jg.solve_(an)
    assert np.all(np.asarray(an.status) == 0)
    check_lanes(jg, t, an, labels, injection=[own.get(i) for i in range(130)])
    pw = R.power(t, R.solve(t, out=int(labels[69]) - 1, injection=own[69])[0], out=int(labels[69]) - 1, injection=own[69])
    for name in ("injection", "supply", "generator"):
        assert R.worst(getattr(an.power, name).active[69], pw[name]) <= TOL, name
    an.close()


def test_screen_summary_against_the_restatement(jg):
    t = load_case("case300")
    s = jg.powerSystem(t)
    labels = jg.outageList(s, 100)
    rating = 0.5 + np.random.default_rng(3).random(s.branch.number)
    rating[::7] = 0.0                                              # not rated
    an = jg.contingencyAnalysis(s, labels, method="dc", rating=rating)
    assert an.screen.shape == (100, 5)
    for i, lab in enumerate(labels):
        _, fr = R.solve(t, out=int(lab) - 1)
        m = np.abs(fr)
        load = np.where(rating > 0, m / np.where(rating > 0, rating, 1.0), 0.0)
        assert int(an.screen[i, 1]) == int(np.argmax(load)) + 1 and int(an.screen[i, 3]) == int(np.argmax(m)) + 1, i
        assert abs(an.screen[i, 0] - load.max()) <= TOL * max(1.0, load.max()) and abs(an.screen[i, 2] - m.max()) <= TOL * max(1.0, m.max()), i
        assert an.screen[i, 4] == 0
    an.close()


def test_a_planted_tie_goes_to_the_lowest_branch(jg):
    """two identical parallel branches carry bitwise the same flow: with equal ratings the summary must name the first of them.  The tie is planted by
    rating every other branch out of the comparison; the largest flow, which runs over all branches, gets a small grid of its own."""
    t = load_case("case118")
    f, to = t["br_from"], t["br_to"]
    pairs = [(a, b) for a in range(f.size) for b in range(a + 1, f.size)
             if f[a] == f[b] and to[a] == to[b] and t["br_x"][a] == t["br_x"][b] and t["br_tap"][a] == t["br_tap"][b] and t["br_shift"][a] == t["br_shift"][b]]
    if not pairs:                                                  # no identical pair in the case: make one (the second branch becomes a copy of the first)
        a, b = next((a, b) for a in range(f.size) for b in range(a + 1, f.size) if f[a] == f[b] and to[a] == to[b])
        for key in ("br_x", "br_tap", "br_shift", "br_r", "br_b", "br_status"):
            t[key][b] = t[key][a]
        pairs = [(a, b)]
    a, b = pairs[0]
    s = jg.powerSystem(t)
    rating = np.zeros(s.branch.number)
    rating[a] = rating[b] = 1.0
    an = jg.contingencyAnalysis(s, [0, 0, 0], method="dc", rating=rating)
    jg.power_(an)
    fr = an.power.from_.active
    assert fr[0, a] == fr[0, b] and fr[0, a] != 0.0                # the tie is real, bit for bit
    assert np.all(an.screen[:, 1] == a + 1) and np.all(an.screen[:, 0] == abs(fr[0, a]))
    an.close()
    # largest flow as well: a three-bus grid whose two identical parallel branches 1-2 carry the largest flow (0.55 each against 0.1 on 2-3)
    z = lambda *v: np.array(v, dtype=np.float64)
    t3 = dict(base_power=np.array([1e8]), bus_type=np.array([3, 1, 1], dtype=np.int8), bus_pd=z(0, 1.0, 0.1), bus_qd=z(0, 0, 0), bus_gs=z(0, 0, 0), bus_bs=z(0, 0, 0),
              bus_vm=z(1, 1, 1), bus_va=z(0, 0, 0), br_from=np.array([2, 1, 1]), br_to=np.array([3, 2, 2]), br_status=np.array([1, 1, 1], dtype=np.int8),
              br_r=z(0, 0, 0), br_x=z(0.1, 0.1, 0.1), br_g=z(0, 0, 0), br_b=z(0, 0, 0), br_tap=z(1, 1, 1), br_shift=z(0, 0, 0),
              gen_bus=np.array([1]), gen_status=np.array([1], dtype=np.int8), gen_pg=z(1.1), gen_qg=z(0), gen_vg=z(1), gen_qmax=z(1), gen_qmin=z(-1))
    s3 = jg.powerSystem(t3)
    an3 = jg.contingencyAnalysis(s3, [0, 0], method="dc", rating=np.ones(3))
    jg.power_(an3)
    fr3 = an3.power.from_.active[0]
    assert fr3[1] == fr3[2] and abs(fr3[1]) > abs(fr3[0]) > 0 and abs(fr3[1] - 0.55) < 1e-12
    assert np.all(an3.screen[:, 3] == 2) and np.all(an3.screen[:, 1] == 2) and np.all(an3.screen[:, 2] == abs(fr3[1]))
    an3.close()


def test_a_bridge_lane_leaves_the_other_lanes_bitwise_alone(jg):
    t = load_case("case118")
    s = jg.powerSystem(t)
    bridge = int(np.flatnonzero(jg.bridges(s))[0]) + 1
    labels = jg.outageList(s, 100)
    with_bridge = labels.copy()
    with_bridge[50] = bridge
    without = labels.copy()
    without[50] = 0
    a = jg.contingencyAnalysis(s, with_bridge, method="dc")
    b = jg.contingencyAnalysis(s, without, method="dc")
    assert a.status[50] == 3 and np.all(np.isnan(a.voltage.angle[50])) and np.all(np.delete(np.asarray(a.status), 50) == 0) and np.all(np.asarray(b.status) == 0)
    keep = np.arange(100) != 50
    assert np.array_equal(a.voltage.angle[keep], b.voltage.angle[keep])
    jg.power_(a)
    jg.power_(b)
    assert np.array_equal(a.power.from_.active[keep], b.power.from_.active[keep])
    a.close()
    b.close()


def test_packed_record_through_a_one_rank_allgather(jg):
    import torch
    t = load_case("case118")
    s = jg.powerSystem(t)
    labels = jg.outageList(s, 70, seed=3)
    labels[9] = int(np.flatnonzero(jg.bridges(s))[0]) + 1
    an = jg.contingencyAnalysis(s, labels, method="dc", rating=np.ones(s.branch.number))
    n = s.bus.number
    packed = torch.zeros((70, n + 1), dtype=torch.float64, device="cuda")
    screen = torch.zeros((70, 5), dtype=torch.float64, device="cuda")
    torch.cuda.current_stream().synchronize()                     # the fill runs on torch's stream, the library writes on its own: finish it first
    an.pack_results_device(packed.data_ptr())
    an.screen_device(screen.data_ptr(), rating=np.ones(s.branch.number))
    comm = jg._lib.Comm(0, 1, jg._lib.Comm.unique_id(), device=0)
    out = torch.full((70, n + 1), -1.0, dtype=torch.float64, device="cuda")
    out5 = torch.full((70, 5), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.current_stream().synchronize()
    comm.allgather_device(packed.data_ptr(), out.data_ptr(), packed.numel())
    comm.allgather_device(screen.data_ptr(), out5.data_ptr(), screen.numel())
    torch.cuda.current_stream().synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, n], np.asarray(an.status, dtype=np.float64)) and got[9, n] == 3
    assert np.array_equal(got[:, :n], an.voltage.angle, equal_nan=True)
    assert np.array_equal(out5.cpu().numpy(), an.screen, equal_nan=True)
    comm.close()
    an.close()


def test_one_solve_through_the_plain_c_abi(jg):
    """ctypes calls with raw pointers only: what a C driver does (include/jgrid.h)"""
    t = load_case("case14")
    (colptr, rowval, nzval), y, psh = R.model(t)
    n, nb = t["bus_type"].size, t["br_from"].size
    L = C.CDLL(jg._lib.LIB_PATH)
    L.jg_last_error.restype = C.c_char_p
    i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    L.jg_dc_create.argtypes = [i64, C.c_int64, i64, i64, f64, C.c_int64, C.c_double, C.c_int64, C.c_int]
    L.jg_dc_set_rhs.argtypes = [C.c_int64, f64]
    L.jg_dc_set_branches.argtypes = [C.c_int64, C.c_int64, i64, i64, f64, f64]
    L.jg_dc_solve.argtypes = [C.c_int64]
    L.jg_dc_get_angle.argtypes = [C.c_int64, f64, C.POINTER(C.c_int32)]
    L.jg_dc_get_flows.argtypes = [C.c_int64, f64]
    L.jg_dc_destroy.argtypes = [C.c_int64]
    L.jg_dc_destroy.restype = None
    arr = lambda a, ct: (ct * len(a))(*a)
    h = C.c_int64(0)
    slack = R.slack_of(t)
    rc = L.jg_dc_create(C.byref(h), n, arr(colptr.tolist(), C.c_int64), arr(rowval.tolist(), C.c_int64), arr(nzval.tolist(), C.c_double), slack + 1,
                        float(t["bus_va"][slack]), 1, 0)
    assert rc == 0 and h.value != 0, L.jg_last_error()
    rhs = R.rhs_of(t, psh)
    assert L.jg_dc_set_rhs(h, arr(rhs.tolist(), C.c_double)) == 0
    assert L.jg_dc_set_branches(h, nb, arr([int(x) for x in t["br_from"]], C.c_int64), arr([int(x) for x in t["br_to"]], C.c_int64),
                                arr(y.tolist(), C.c_double), arr([float(x) for x in t["br_shift"]], C.c_double)) == 0
    assert L.jg_dc_solve(h) == 0, L.jg_last_error()
    th, st, fr = (C.c_double * n)(), (C.c_int32 * 1)(), (C.c_double * nb)()
    assert L.jg_dc_get_angle(h, th, st) == 0 and L.jg_dc_get_flows(h, fr) == 0
    rth, rfr = R.solve(t)
    assert st[0] == 0 and R.worst(np.array(th[:]), rth) <= TOL and R.worst(np.array(fr[:]), rfr) <= TOL
    L.jg_dc_destroy(h)
    assert L.jg_dc_solve(C.c_int64(0)) == 1                         # a null token is a bad argument, not a crash


def test_a_dc_and_a_dcse_handle_take_turns_in_one_process(jg):
    """The factorisation and sweep kernels and their launchers are ONE compiled unit (csrc/jg_dc_sweep.hip) that both kinds of handle call.  A DC handle
    (batch 70: ld 128, the second lane group partial) and a DC state-estimation handle (batch 3) take turns call by call -- DC rhs and outages, DCSE
    readings, DC solve, DCSE solve, DC screen, DCSE residual test with one removal, DC solve again (and the DCSE solve that applies the removal) -- and
    every angle, status, screen record and estimate is bit for bit that of equal handles run alone, one after the other.  It fails if the unit keeps any
    state of its own: a static table, a cached argument block, a shared stream."""
    from test_dcse_host import bad_data_set, monitoring_of
    D, E = jg.dcpowerflow, jg.dcstateestimation
    t = load_case("case14")
    s = jg.powerSystem(t)
    labels = np.resize(np.flatnonzero(s.branch.layout.status == 1) + 1, 70)      # every branch in turn, the bridge 7-8 among them (status 3)
    labels[::9] = 0
    rating = 0.5 + np.random.default_rng(5).random(s.branch.number)
    mon = monitoring_of(jg, t, bad_data_set(t)[1])

    def run(taking_turns):
        dc, se = jg.dcPowerFlow(s, batch=70), jg.dcStateEstimation(mon, batch=3)
        assert dc.dims()["ld"] == 128 and se.dims()["ld"] == 64
        z = se.readings.copy()
        z[2] *= 1.0 + 1e-4 * np.sin(np.arange(z.shape[1]))         # lane 0 exact, lane 2 slightly off: neither reaches the threshold
        z[1, 1] += 50.0                                            # lane 1: one gross error
        out = {}

        def dc_set():
            D.setOutages_(dc, labels)
            dc._rhs = np.ascontiguousarray(D._base_rhs(s), dtype=np.float64)
            jg._lib.check(jg._lib.lib().jg_dc_set_rhs(dc._h, dc._rhs))

        def se_set():
            E.setReadings_(se, z)
            E._sync(se)

        def dc_solve(key):
            D.solve_(dc)
            out[key], out[key + " status"] = dc.voltage.angle.copy(), np.array(dc.status)

        def se_solve(key):
            E.solve_(se)
            out[key], out[key + " status"], out[key + " objective"] = se.voltage.angle.copy(), np.array(se.status), np.array(se.objective)

        def dc_screen():
            out["screen"] = D.screenSummary_(dc, rating)

        def se_test():
            r = E.residualTest_(se, threshold=3.0)
            out["maximum"], out["index"] = r.maxNormalizedResidual.copy(), r.index.copy()
            out["removed"] = np.array([len(rows) for rows in E.removed(se).rows])

        dc_steps = [dc_set, lambda: dc_solve("angle"), dc_screen, lambda: dc_solve("angle again")]
        se_steps = [se_set, lambda: se_solve("estimate"), se_test, lambda: se_solve("reduced estimate")]
        steps = [f for pair in zip(dc_steps, se_steps) for f in pair] if taking_turns else dc_steps + se_steps
        for f in steps:
            f()
        dc.close()
        se.close()
        return out

    a, b = run(True), run(False)
    assert sorted(a) == sorted(b) and len(a) == 14
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.array_equal(a["removed"], [0, 1, 0]) and np.all(a["estimate status"] == 0) and np.all(a["reduced estimate status"] == 0)
    assert set(np.unique(a["angle status"])) == {0, 3} and np.array_equal(a["angle"], a["angle again"], equal_nan=True)
    assert not np.array_equal(a["estimate"][1], a["reduced estimate"][1]) and np.all(np.isfinite(a["screen"][a["angle status"] == 0]))
