"""reactiveLimit! per scenario of a batched Newton-Raphson analysis (jgrid.h: jg_nr_set_bus_type, jg_nr_reactive_limit, jg_nr_adjust_angle):
per-lane bus types in the batched assembly, the limit kernels of csrc/jg_qlim.hip, the slack hand-over in the reference's loop order, status 5,
against the MATPOWER goldens of test/powerFlow/limits.jl and the oracle's restatement of the reference sequence per scenario."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_case, load_golden

pytestmark = pytest.mark.gpu


def _oracle_sequence(oracle, t, typ=None, vm0=None, va0=None):
    """newtonRaphson -> powerFlow! -> reactiveLimit! -> newtonRaphson -> powerFlow! on the oracle (one scenario).  A scenario without a violation
    keeps its converged state (what the batch does: the next run confirms it in 0 iterations)."""
    osys = oracle.OracleSystem(t)
    if typ is not None:
        osys.type = np.ascontiguousarray(typ, dtype=np.int8).copy()
        osys.slack = int(np.flatnonzero(osys.type == 3)[0]) + 1
    o = oracle.OracleNR(osys)
    if vm0 is not None:
        o.set_voltage(vm0, va0)
    st0 = o.power_flow()
    it0 = o.iteration
    vm, va = o.voltage()
    try:
        violate = oracle.reactive_limit(osys, o.type, vm, va)
    except RuntimeError:
        return dict(dead=True, it0=it0, st0=st0)
    if not np.any(violate):
        return dict(dead=False, it0=it0, st0=st0, violate=violate, it1=0, st1=st0, vm=vm, va=va, slack=o.slack, type=o.type.copy())
    o2 = oracle.OracleNR(osys)
    st1 = o2.power_flow()
    vm2, va2 = o2.voltage()
    return dict(dead=False, it0=it0, st0=st0, violate=violate, it1=o2.iteration, st1=st1, vm=vm2, va=va2, slack=o2.slack, type=o2.type.copy())


@pytest.mark.parametrize("name", ["case14test", "case30test"])
def test_batch_reactive_limits_hit_the_goldens(jg, oracle, name):
    """test/powerFlow/limits.jl:4-42 in every lane of a batch of 70 identical scenarios (two lane groups): powerFlow! -> reactiveLimit! ->
    powerFlow! -> adjustAngle!(original slack)."""
    g = load_golden(name)
    t = load_case(name)
    system = jg.powerSystem(t)
    slack0 = system.bus.layout.slack
    an = jg.newtonRaphson(system, batch=70)
    jg.powerFlow_(an)
    it0 = an.method.iteration.copy()
    violate = jg.reactiveLimit_(an)
    jg.powerFlow_(an)
    it1 = an.method.iteration.copy()
    jg.adjustAngle_(an, slack0)
    ref = _oracle_sequence(oracle, t)
    assert np.any(ref["violate"] != 0)
    assert violate.shape == (70, system.generator.number)
    assert np.array_equal(violate, np.broadcast_to(ref["violate"], violate.shape))
    assert np.all(an.status == 0)
    assert np.all(it0 + it1 == int(g["reactiveLimit_newtonRaphson_iteration"][0]))
    vm, va = an.voltage.magnitude, an.voltage.angle
    assert np.abs(vm - g["reactiveLimit_newtonRaphson_voltageMagnitude"][None, :]).max() <= 1e-8
    assert np.abs(va - g["reactiveLimit_newtonRaphson_voltageAngle"][None, :]).max() <= 1e-8
    assert np.array_equal(vm, np.broadcast_to(vm[0], vm.shape)) and np.array_equal(va, np.broadcast_to(va[0], va.shape))
    typ, slack = jg.busType(an)
    assert np.all(slack == ref["slack"]) and np.array_equal(typ, np.broadcast_to(ref["type"], typ.shape))
    assert system.bus.layout.slack == slack0                     # the system is not touched


def _n1(jg, oracle, name, batch, check_every=1):
    t = load_case(name)
    system = jg.powerSystem(t)
    base = jg.newtonRaphson(jg.powerSystem(t))
    jg.powerFlow_(base)
    vm0, va0 = base.voltage.magnitude.copy(), base.voltage.angle.copy()
    labels = [int(x) for x in jg.outageList(system, batch, seed=17)]
    an = jg.contingencyAnalysis(system, labels)
    jg.setInitialPoint_(an, base)
    jg.powerFlow_(an)
    it0, st0 = an.method.iteration.copy(), an.status.copy()
    violate = jg.reactiveLimit_(an)
    jg.powerFlow_(an)
    it1, st1 = an.method.iteration.copy(), an.status.copy()
    typ, slack = jg.busType(an)
    assert np.any(violate != 0) and len({v.tobytes() for v in violate}) > 1      # lanes violate, and not all alike
    # the lanes with new types finished at different iterations of the second solve: the compaction moved lanes that carry their types
    assert len(set(it1[np.any(violate != 0, axis=1)].tolist())) > 1
    checked = 0
    for s in range(0, batch, check_every):
        tt = dict(t)
        tt["br_status"] = np.array(t["br_status"]).copy()
        tt["br_status"][labels[s] - 1] = 0
        ref = _oracle_sequence(oracle, tt, vm0=vm0, va0=va0)
        assert (it0[s], st0[s]) == (ref["it0"], ref["st0"]), s
        if ref["dead"]:
            assert st1[s] == 5, s
            continue
        assert np.array_equal(violate[s], ref["violate"]), s
        assert (it1[s], st1[s], slack[s]) == (ref["it1"], ref["st1"], ref["slack"]), s
        if st1[s] == 0:
            assert np.abs(an.voltage.magnitude[s] - ref["vm"]).max() <= 1e-8, s
            assert np.abs(an.voltage.angle[s] - ref["va"]).max() <= 1e-8, s
        checked += 1
    assert checked >= min(batch, 12)


def test_n1_reactive_limits_per_lane_case1951rte(jg, oracle):
    _n1(jg, oracle, "case1951rte", 512)


def test_n1_reactive_limits_per_lane_case_activsg10k(jg, oracle):
    _n1(jg, oracle, "case_ACTIVSg10k", 512, check_every=4)


def test_slack_hand_over_twice_and_no_slack_left(jg, oracle):
    """Tightened limits in a copy of case14test: the slack's generator violates (hand-over to bus 2), the generator of bus 2 violates later in the
    same loop (hand-over again).  Lanes whose other generator buses are already PQ lose their slack: status 5 there only."""
    t = dict(load_case("case14test"))
    gb = np.asarray(t["gen_bus"]).astype(int)
    qmin, qmax = np.array(t["gen_qmin"], dtype=float), np.array(t["gen_qmax"], dtype=float)
    system0 = jg.powerSystem(t)
    slack_bus = system0.bus.layout.slack
    first_pv = int(np.flatnonzero(system0.bus.layout.type == 2)[0]) + 1
    for b, band in ((slack_bus, 1e-4), (first_pv, 0.3)):               # every generator of the two buses (several, one with infinite limits)
        for k in np.flatnonzero(gb == b):
            qmin[k], qmax[k] = -band, band
    t["gen_qmin"], t["gen_qmax"] = qmin, qmax
    system = jg.powerSystem(t)
    batch = 20                                                         # one lane group of a handful of scenarios: the wide assembly variant
    an = jg.newtonRaphson(system, batch=batch)
    typ0 = system.bus.layout.type.copy()
    lone = typ0.copy()
    lone[lone == 2] = 1                                                # only the slack is a generator bus
    dead_lanes = [3, 17]
    jg.setBusType_(an, lone, dead_lanes)
    vs, ts = an.voltage.magnitude[3].copy(), an.voltage.angle[3].copy()
    jg.powerFlow_(an)
    it0 = an.method.iteration.copy()
    violate = jg.reactiveLimit_(an)
    jg.powerFlow_(an)
    it1, st1 = an.method.iteration.copy(), an.status.copy()
    typ, slack = jg.busType(an)
    ref = _oracle_sequence(oracle, t)
    assert not ref["dead"]
    assert np.any(ref["violate"][gb == slack_bus] != 0) and np.any(ref["violate"][gb == first_pv] != 0)
    assert ref["slack"] not in (slack_bus, first_pv)                  # handed over twice
    refd = _oracle_sequence(oracle, t, typ=lone, vm0=vs, va0=ts)
    assert refd["dead"]
    for s in range(batch):
        if s in dead_lanes:
            assert st1[s] == 5 and it0[s] == refd["it0"] and np.array_equal(typ[s], lone), s
            continue
        assert np.array_equal(violate[s], ref["violate"]), s
        assert (it0[s], it1[s], st1[s], slack[s]) == (ref["it0"], ref["it1"], ref["st1"], ref["slack"]), s
        assert np.abs(an.voltage.magnitude[s] - ref["vm"]).max() <= 1e-8
        assert np.abs(an.voltage.angle[s] - ref["va"]).max() <= 1e-8
    # the dead lanes come back with their create-time types
    jg.setBusType_(an, None, dead_lanes)
    jg.powerFlow_(an)
    assert np.all(an.status[dead_lanes] != 5)


def test_set_bus_type_matches_the_oracle_and_resets_bitwise(jg, oracle):
    t = load_case("case30test")
    system = jg.powerSystem(t)
    batch = 70
    an = jg.newtonRaphson(system, batch=batch)
    plain = jg.newtonRaphson(jg.powerSystem(t), batch=batch)
    vm0, va0 = an.voltage.magnitude.copy(), an.voltage.angle.copy()
    typ0 = system.bus.layout.type.copy()
    pv = np.flatnonzero(typ0 == 2)
    k = int(pv[1])
    tp = typ0.copy()
    tp[k] = 1                                                          # PV -> PQ with a given Q injection
    lanes = list(range(60, 70))
    jg.setBusType_(an, tp, lanes)
    bus = system.bus
    P = np.broadcast_to(bus.supply.active - bus.demand.active, (batch, bus.number)).copy()
    Q = np.broadcast_to(bus.supply.reactive - bus.demand.reactive, (batch, bus.number)).copy()
    Q[lanes, k] = 0.25
    jg.setInjection_(an, P, Q)
    jg.powerFlow_(an)
    jg.powerFlow_(plain)
    osys = oracle.OracleSystem(t)
    osys.type = tp.astype(np.int8)
    o = oracle.OracleNR(osys)
    qs = osys.qs.copy()
    qs[k] = 0.25 + osys.qd[k]
    o.set_power(osys.ps, qs, osys.pd, osys.qd)
    o.set_voltage(vm0[0], va0[0])
    assert o.power_flow() == 0
    vm, va = o.voltage()
    typ, slack = jg.busType(an)
    for s in lanes:
        assert np.array_equal(typ[s], tp)
        assert an.method.iteration[s] == o.iteration and an.status[s] == 0
        assert np.abs(an.voltage.magnitude[s] - vm).max() <= 1e-8 and np.abs(an.voltage.angle[s] - va).max() <= 1e-8
        # a masked variable's increment is exactly 0: PV magnitudes and the slack's angle stay bitwise at their start values
        assert np.array_equal(an.voltage.magnitude[s][tp != 1], vm0[s][tp != 1])
        assert np.array_equal(an.voltage.angle[s][tp == 3], va0[s][tp == 3])
    others = [s for s in range(batch) if s not in lanes]
    assert np.array_equal(an.voltage.magnitude[others], plain.voltage.magnitude[others])
    assert np.array_equal(an.voltage.angle[others], plain.voltage.angle[others])
    # back to the create-time types: bitwise what a handle that never had overrides computes
    jg.setBusType_(an, None)
    jg.setInjection_(an)
    jg.setInitialPoint_(an)
    jg.powerFlow_(an)
    assert np.array_equal(an.voltage.magnitude, plain.voltage.magnitude) and np.array_equal(an.voltage.angle, plain.voltage.angle)
    assert np.array_equal(an.method.iteration, plain.method.iteration)
    assert an.jacobian is not None                                     # the reference-layout getters work again


def test_adjust_angle_on_the_device_matches_the_host(jg):
    t = load_case("case14test")
    system = jg.powerSystem(t)
    an = jg.newtonRaphson(system, batch=70)
    jg.powerFlow_(an)
    jg.adjustAngle_(an, 4)
    host = an.voltage.angle.copy()
    jg._lib.check(jg._lib.lib().jg_nr_adjust_angle(an._h, 4, float(system.bus.voltage.angle[3])))
    an._pull_voltage()
    assert np.array_equal(an.voltage.angle, host)


def test_refusals_and_the_shared_base_factor(jg):
    t = load_case("case30test")
    system = jg.powerSystem(t)
    L = jg._lib.lib()
    an = jg.newtonRaphson(system, batch=70)
    n = system.bus.number
    two = system.bus.layout.type.copy()
    two[np.flatnonzero(two == 2)[0]] = 3
    with pytest.raises(jg._lib.JGridError, match="exactly one slack") as e:
        jg.setBusType_(an, two, [0])
    assert e.value.code == 1
    one = jg.newtonRaphson(jg.powerSystem(t))
    with pytest.raises(jg._lib.JGridError, match="one scenario") as e:
        jg.setBusType_(one, system.bus.layout.type, [0])
    assert e.value.code == 1
    fast = jg.fastNewtonRaphsonBX(jg.powerSystem(t), batch=4)
    assert L.jg_nr_set_bus_type(fast._h, 0, 1, system.bus.layout.type.astype(np.int8).ctypes.data) == 1
    assert b"fast" in L.jg_last_error()
    # a base-case start: the first run takes the shared factor, a run after reactiveLimit_ refactorises
    jg.powerFlow_(one)
    base = jg.BaseCase(one)
    base.attach(an)
    jg.startFromBase_(an)
    jg.powerFlow_(an)
    c0 = jg.firstIterationCounts(an)
    assert c0[0] == 1
    jg.reactiveLimit_(an)
    assert L.jg_nr_set_refine(an._h, 1) == 1 and b"bus types" in L.jg_last_error()
    m = np.zeros(70 * an.dims["dimJ"])
    assert L.jg_nr_get_mismatch(an._h, m) == 1
    assert L.jg_nr_get_jacobian(an._h, np.zeros(70 * an.dims["nnzJ"])) == 1
    pool = jg.newtonRaphson(jg.powerSystem(t), batch=64)
    home = np.zeros(64, dtype=np.int32)
    cnt = C.c_int32(0)
    assert L.jg_nr_move_lanes(pool._h, 0, an._h, home, C.byref(cnt)) == 1
    jg.startFromBase_(an)
    jg.powerFlow_(an)
    c1 = jg.firstIterationCounts(an)
    assert c1 == (c0[0], c0[1] + 1)                                   # refactorised
    assert np.all(an.status == 0)


def _tightened_case14(bands):
    t = dict(load_case("case14test"))
    gb = np.asarray(t["gen_bus"]).astype(int)
    qmin, qmax = np.array(t["gen_qmin"], dtype=float), np.array(t["gen_qmax"], dtype=float)
    for b, band in bands:
        for k in np.flatnonzero(gb == b):
            qmin[k], qmax[k] = -band, band
    t["gen_qmin"], t["gen_qmax"] = qmin, qmax
    return t


def test_rounds_after_a_slack_hand_over_match_the_oracle(jg, oracle):
    """Three rounds of reactiveLimit! + powerFlow!: round 1 hands the slack from bus 1 to bus 2, round 2 from bus 2 to bus 6 -- bus 1, now PQ, keeps
    the P its generators took as the slack in round 1 (gen.output.active, acPowerFlow.jl:1097) -- and round 3 finds no violation: the lanes stay at
    their converged state (0 iterations)."""
    t = _tightened_case14(((1, 1e-4), (2, 0.5)))
    batch = 70
    an = jg.newtonRaphson(jg.powerSystem(t), batch=batch)
    jg.powerFlow_(an)
    osys = oracle.OracleSystem(t)
    o = oracle.OracleNR(osys)
    assert o.power_flow() == 0
    assert np.all(an.method.iteration == o.iteration)
    total = np.array(an.method.iteration, dtype=np.int64)
    slacks = []
    for r in range(3):
        vm, va = o.voltage()
        ref = oracle.reactive_limit(osys, o.type, vm, va)
        violate = jg.reactiveLimit_(an)
        assert np.array_equal(violate, np.broadcast_to(ref, violate.shape)), r
        vm_before, va_before = an.voltage.magnitude.copy(), an.voltage.angle.copy()
        jg.powerFlow_(an)
        assert np.all(an.status == 0), r
        if not np.any(ref):
            assert np.all(an.method.iteration == 0), r
            assert np.array_equal(an.voltage.magnitude, vm_before) and np.array_equal(an.voltage.angle, va_before)
            break
        o = oracle.OracleNR(osys)
        assert o.power_flow() == 0
        assert np.all(an.method.iteration == o.iteration), r
        total += an.method.iteration
        vm, va = o.voltage()
        assert np.abs(an.voltage.magnitude - vm[None, :]).max() <= 1e-8 and np.abs(an.voltage.angle - va[None, :]).max() <= 1e-8, r
        typ, slack = jg.busType(an)
        assert np.all(slack == osys.slack), r
        slacks.append(osys.slack)
    else:
        raise AssertionError("the third round was expected to find no violation")
    assert slacks == [2, 6]
    # the same rounds in one call: iterations summed per scenario
    an2 = jg.newtonRaphson(jg.powerSystem(t), batch=batch)
    jg.powerFlowLimits_(an2, 3)
    assert np.array_equal(an2.method.iteration, total)
    assert np.array_equal(an2.voltage.magnitude, an.voltage.magnitude) and np.array_equal(an2.voltage.angle, an.voltage.angle)


def test_power_refuses_lane_types(jg):
    t = load_case("case14test")
    an = jg.newtonRaphson(jg.powerSystem(t), batch=4)
    jg.powerFlow_(an)
    jg.reactiveLimit_(an)
    with pytest.raises(ValueError, match="bus types of their own"):
        jg.power_(an)
    jg.setBusType_(an, None)
    jg.power_(an)                                                      # create-time types again: allowed


def test_pipeline_with_reactive_limits_matches_one_handle(jg):
    """ContingencyPipeline(reactive_limit=1, pool=0): every batch bitwise what one handle gives for powerFlow! -> reactiveLimit! -> powerFlow!
    (iterations summed); a handle reused for the next job starts from the create-time types and injections again."""
    t = load_case("case1951rte")
    system = jg.powerSystem(t)
    base = jg.newtonRaphson(jg.powerSystem(t))
    jg.powerFlow_(base)
    vm0, va0 = base.voltage.magnitude.copy(), base.voltage.angle.copy()
    batch = 128
    labels = [int(x) for x in jg.outageList(system, 3 * batch, seed=23)]
    jobs = [labels[i * batch:(i + 1) * batch] for i in range(3)]
    pipe = jg.ContingencyPipeline(system, batch, inflight=2, start=(vm0, va0), reactive_limit=1, shared_first=False)
    got = {}

    def on_done(j, an):
        an._pull_voltage()
        got[j] = (an.voltage.magnitude.copy(), an.voltage.angle.copy())

    res = pipe.run(jobs, on_done=on_done)
    pipe.close()
    for j, job in enumerate(jobs):
        an = jg.contingencyAnalysis(system, job)
        jg._lib.check(jg._lib.lib().jg_nr_set_shared(an._h, 1))       # what the pipeline's handles run with (same bits, a performance hint)
        jg.setInitialPoint_(an, base)
        jg.powerFlow_(an)
        it = an.method.iteration.copy()
        jg.reactiveLimit_(an)
        jg.powerFlow_(an)
        it = it + an.method.iteration
        assert np.array_equal(res[j][0], it) and np.array_equal(res[j][1], an.status), j
        assert np.array_equal(got[j][0], an.voltage.magnitude) and np.array_equal(got[j][1], an.voltage.angle), j
        an2 = jg.contingencyAnalysis(system, job, reactiveLimit=1, start=(vm0, va0))
        assert np.array_equal(an2.method.iteration, it) and np.array_equal(an2.voltage.magnitude, an.voltage.magnitude), j
        an.close()
        an2.close()
    with pytest.raises(ValueError, match="pool"):
        jg.ContingencyPipeline(system, batch, inflight=1, pool=64, reactive_limit=1)
