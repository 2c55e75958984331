"""Sweep-only factorisation on the device (Engine::sweep_only, jg_symbolic.hpp: top_dead): a batched Newton-Raphson handle whose factor is read by the
Jordan sweep alone leaves the entries nothing of that path reads unstored.  Every stored value that something reads keeps its bits, so

  * the refactorising iteration gives what the oracle gives (V, theta 1e-8, equal iteration counts and status, last increment 1e-9 -- the tolerances of
    tests/test_nr_gpu.py and tests/test_comp_gpu.py) and, bit for bit, what the same handle gives with the flag off (JG_SWEEP_ONLY=0),
  * a compensated start takes the same first step (1e-9 against the oracle's, tests/test_comp_gpu.py),
  * the paths that need the full factor (selected inverse / bad data, the orthogonal Gauss-Newton method) never see the flag.

Shapes: 70 lanes = two lane groups with a padded last one, 260 = five (the plan class of 256 lanes and more: factorisation tasks below the top); an N-1 batch
started at the base-case solution finishes its scenarios at different iterations, so lanes are compacted between iterations."""
import numpy as np
import pytest

from conftest import load_case

pytestmark = pytest.mark.gpu


def _labels(jg, s, batch):
    ok = [int(x) for x in jg.outageList(s, batch - 2, seed=11)]
    return [0] + ok[:batch - 2] + [ok[0]]                           # the base case (converged at the start), outages, a duplicate


def _oracle_run(oracle, jg, osys, s, label, start):
    o = oracle.OracleNR(osys)
    if label:
        ptr, dy = jg.outagePatch(s, label)
        for p, d in zip(ptr, dy):
            o.add_ybus(p - 1, d)
    o.set_voltage(*start)
    rc = o.power_flow()
    _, _, inc = o.vectors()
    vm, va = o.voltage()
    return rc, o.iteration, np.array(vm), np.array(va), np.array(inc)


@pytest.fixture(scope="module")
def solved(jg, oracle):
    """per grid: tables, system, base-case solution, oracle system, and the oracle's N-1 runs by label (computed once, shared, never changed)"""
    out = {}
    for name in ("case30test", "case1354pegase"):
        t = load_case(name)
        s = jg.powerSystem(t)
        single = jg.newtonRaphson(s)
        jg.powerFlow_(single)
        assert single.status == 0
        start = (single.voltage.magnitude.copy(), single.voltage.angle.copy())
        single.close()
        out[name] = dict(t=t, s=s, start=start, osys=oracle.OracleSystem(t), runs={})
    return out


def _run_refactorising(jg, s, labels, start, iteration=None):
    an = jg.contingencyAnalysis(s, labels)
    jg.setFirstIteration_(an, False)
    jg.powerflow._push_voltage(an, *start)
    jg.powerFlow_(an) if iteration is None else jg.powerFlow_(an, iteration=iteration)
    res = dict(vm=an.voltage.magnitude.copy(), va=an.voltage.angle.copy(), it=np.array(an.method.iteration).copy(), status=np.array(an.status).copy(),
               inc=np.array(an.increment).copy(), counts=jg.firstIterationCounts(an))
    an.close()
    return res


@pytest.mark.parametrize("name,batch", [("case30test", 70), ("case30test", 260), ("case1354pegase", 70), ("case1354pegase", 260)])
def test_refactorising_path_matches_the_oracle_and_the_full_factor_bitwise(jg, oracle, solved, monkeypatch, name, batch):
    d = solved[name]
    s, start, osys = d["s"], d["start"], d["osys"]
    labels = _labels(jg, s, batch)
    monkeypatch.delenv("JG_SWEEP_ONLY", raising=False)
    on = _run_refactorising(jg, s, labels, start)
    monkeypatch.setenv("JG_SWEEP_ONLY", "0")
    off = _run_refactorising(jg, s, labels, start)
    assert on["counts"] == (0, 1) and off["counts"] == (0, 1)
    for k in ("vm", "va", "it", "status", "inc"):
        assert np.array_equal(on[k], off[k]), k
    good = on["status"] == 0
    assert good.sum() >= batch - 3
    its = set(int(v) for v in on["it"][good])
    print(f"[{name} x {batch}] iterations of the converged lanes: {sorted(its)}")
    assert len(its) >= 2                                            # lanes finish at different iterations: the increment of a finished lane is an earlier sweep's
    worst_v, worst_inc = 0.0, 0.0
    for sc in range(batch):
        lab = labels[sc]
        if lab not in d["runs"]:
            d["runs"][lab] = _oracle_run(oracle, jg, osys, s, lab, start)
        rc, it, vm, va, inc = d["runs"][lab]
        assert (rc == 0) == bool(good[sc]), (sc, lab)
        if rc != 0:
            continue
        assert it == on["it"][sc], (sc, lab)
        worst_v = max(worst_v, np.abs(on["vm"][sc] - vm).max(), np.abs(on["va"][sc] - va).max())
        if it == 0:
            continue                                               # converged at the start: no step was taken
        scale = max(1e-3, np.abs(inc).max())
        worst_inc = max(worst_inc, np.abs(on["inc"][sc] - inc).max() / scale)
    print(f"[{name} x {batch}] worst |dV|, |dtheta| {worst_v:.2e}; worst relative error of the last increment {worst_inc:.2e}")
    assert worst_v <= 1e-8
    assert worst_inc <= 1e-9


def test_compensated_start_takes_the_oracles_first_step(jg, oracle, solved):
    d = solved["case1354pegase"]
    s, start, osys, batch = d["s"], d["start"], d["osys"], 130
    single = jg.newtonRaphson(s)
    jg.powerFlow_(single)
    start0 = (single.voltage.magnitude.copy(), single.voltage.angle.copy())
    base = jg.BaseCase(single)
    labels = _labels(jg, s, batch)
    an = jg.contingencyAnalysis(s, labels)
    base.attach(an)
    jg.startFromBase_(an)
    jg.powerFlow_(an, iteration=1)
    assert jg.firstIterationCounts(an) == (1, 0)
    inc_c = np.array(an.increment)
    worst = 0.0
    for sc in range(batch):
        if not labels[sc]:
            continue
        o = oracle.OracleNR(osys)
        ptr, dy = jg.outagePatch(s, labels[sc])
        for p, dlt in zip(ptr, dy):
            o.add_ybus(p - 1, dlt)
        o.set_voltage(*start0)
        o.mismatch()
        o.solve()
        _, _, inc = o.vectors()
        scale = max(1e-3, np.abs(inc).max())
        worst = max(worst, np.abs(inc_c[sc] - inc).max() / scale)
    print(f"[compensated start case1354pegase x {batch}] first increment against the oracle's, worst relative error {worst:.2e}")
    assert worst <= 1e-9
    # ... and the iterations behind it run the sweep-only factorisation: the whole flow ends where the refactorising one ends
    jg.startFromBase_(an)
    jg.powerFlow_(an)
    ref = _run_refactorising(jg, s, labels, start0)
    good = np.array(an.status) == 0
    assert np.array_equal(np.array(an.status), ref["status"]) and np.array_equal(np.array(an.method.iteration)[good], ref["it"][good])
    assert np.abs(an.voltage.magnitude[good] - ref["vm"][good]).max() <= 1e-10 and np.abs(an.voltage.angle[good] - ref["va"][good]).max() <= 1e-10
    an.close(); base.close(); single.close()


def _se_case14(jg, method):
    s = jg.powerSystem(load_case("case14test"))
    pf = jg.newtonRaphson(s)
    jg.powerFlow_(pf, tolerance=1e-10)
    mon = jg.measurement(s)
    jg.addVoltmeter_(mon, pf)
    jg.addWattmeter_(mon, pf)
    jg.addVarmeter_(mon, pf)
    jg.addPmu_(mon, pf, minMagnitude=1e-6)
    mon.wattmeter.active.mean[3] += 0.5                                  # one gross error for the residual test to find
    an = jg.gaussNewton(mon, method)
    jg.stateEstimation_(an, iteration=50, tolerance=1e-10)
    out = dict(vm=an.voltage.magnitude.copy(), va=an.voltage.angle.copy(), it=int(an.method.iteration), status=int(an.status))
    if method is jg.LU:
        r = jg.residualTest_(an)
        out.update(detect=bool(r.detect), mx=float(r.maxNormalizedResidual), index=int(r.index))
    an.close(); pf.close()
    return out


@pytest.mark.parametrize("method", ["LU", "Orthogonal"])
def test_full_factor_paths_do_not_see_the_flag(jg, monkeypatch, method):
    """selected inverse + bad data (LU) and the orthogonal method (jg_gn_set_method(h, 1): forward() on the factor) with the switch on and off: same bits"""
    m = getattr(jg, method)
    monkeypatch.delenv("JG_SWEEP_ONLY", raising=False)
    on = _se_case14(jg, m)
    monkeypatch.setenv("JG_SWEEP_ONLY", "0")
    off = _se_case14(jg, m)
    assert on["status"] == 0 and on["it"] == off["it"]
    assert np.array_equal(on["vm"], off["vm"]) and np.array_equal(on["va"], off["va"])
    if method == "LU":
        assert on["detect"] and (on["mx"], on["index"]) == (off["mx"], off["index"])
