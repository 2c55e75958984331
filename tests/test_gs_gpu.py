"""Gauss-Seidel power flow on the device (csrc/jg_gs.hip), one scenario per lane, against the reference's MATPOWER vectors and the numpy restatement
(tests/gs_reference.py, itself pinned to those vectors in tests/test_gs_host.py).

Bounds.  Voltages of a converged lane: 1e-10 against the restatement -- the iteration contracts by about 0.94 / 0.976 per sweep on the 14 / 30 bus cases,
so rounding of 1e-15 per sweep (the device's plain complex division against numpy's scaled one included) settles near 1e-15 / (1 - rho) < 1e-13.  Single
steps: 1e-12.  Iteration counts are compared on EVERY lane; that they can be is asserted first, on the CPU: the restatement's mismatch of a converging
lane lies at least 1e-6 (relative) below the tolerance at its last check and at least 1e-6 above it at the check before (gs_reference.margins_hold).

Measured on an MI355X, worst |dV| against the restatement: see DESIGN.md section 3.15.
"""
import functools

import numpy as np
import pytest

import gs_reference as R
from conftest import load_case, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-8
# case118: four branches that are no bridges, spread over the grid; the restatement converges on each with the margin (checked when this was written:
# 2111 sweeps for the base case, 2036, 1907, 1998 and 2049 for these)
CASE118_OUTAGES = (10, 109, 127, 163)


def ac_system(jg, case):
    s = jg.powerSystem(load_case(case))
    jg.acModel_(s)
    return s


@functools.lru_cache(maxsize=None)
def restated(case, labels, scale, limit):
    """the restatement's run of one lane per (label, demand scale) -- computed once, shared by the tests, never changed"""
    import juliagrid.jl_amd as jg
    s = ac_system(jg, case)
    g = R.problem(s)
    bus = s.bus
    P = np.stack([bus.supply.active - f * bus.demand.active for f in scale])
    Q = np.stack([bus.supply.reactive - f * bus.demand.reactive for f in scale])
    yt, v, P, Q = R.lanes(g, len(labels), R.lane_values(s, labels), P, Q)
    out = R.run(g, yt, v, P, Q, limit, TOL)
    for a in (v, out.iteration, out.status, out.before, *out.stop):
        a.flags.writeable = False
    return out, v


def compare_lanes(an, out, v, pick):
    """status and iteration count on every lane, voltages on the converged ones; returns the worst voltage deviation"""
    it, st = np.atleast_1d(an.method.iteration), np.atleast_1d(an.status)
    assert np.array_equal(st, out.status[pick]), (st, out.status[pick])
    assert np.array_equal(it, out.iteration[pick]), (it, out.iteration[pick])
    ok = st == 0
    dev = float(np.abs(np.atleast_2d(an.method.voltage)[ok] - v[pick][ok]).max())
    assert dev <= 1e-10, dev
    return dev


@pytest.mark.parametrize("case, limit, count", [("case14test", 300, 281), ("case30test", 900, 761)])
def test_goldens_on_the_device(jg, case, limit, count):
    gold = load_golden(f"gs_{case}")
    s = ac_system(jg, case)
    an = jg.gaussSeidel(s)
    assert np.array_equal(an.method.pq, np.flatnonzero(s.bus.layout.type == 1) + 1) and np.array_equal(an.method.pv, np.flatnonzero(s.bus.layout.type == 2) + 1)
    jg.powerFlow_(an, iteration=limit)
    assert an.method.iteration == count == int(gold["iteration"][0]) and an.status == 0
    assert R.isapprox(an.voltage.magnitude, gold["voltageMagnitude"]) and R.isapprox(an.voltage.angle, gold["voltageAngle"])
    out, v = restated(case, (0,), (1.0,), limit)
    dev = compare_lanes(an, out, v, np.array([0]))
    print(f"{case}: worst |dV| device - restatement {dev:.3e}")
    assert np.allclose(an.voltage.magnitude, np.abs(an.method.voltage), rtol=0, atol=1e-15)
    p, q = an.mismatch
    assert max(p, q) < TOL and abs(p - out.stop[0][0]) < 1e-12 and abs(q - out.stop[1][0]) < 1e-12


def test_single_steps_follow_the_restatement_and_the_loop_repeats_them_bit_for_bit(jg):
    labels = (1, 7, 13)
    s = ac_system(jg, "case14test")
    an = jg.gaussSeidel(s, batch=3)
    jg.setOutages_(an, labels)
    g = R.problem(s)
    yt, v, P, Q = R.lanes(g, 3, R.lane_values(s, labels))
    assert np.abs(np.asarray(an.method.voltage) - v).max() <= 1e-15
    for step in range(5):
        p, q = jg.mismatch_(an)
        rp, rq = R.mismatch(g, yt, v, P, Q)
        assert np.abs(p - rp).max() <= 1e-12 and np.abs(q - rq).max() <= 1e-12, step
        jg.solve_(an)
        R.sweep(g, yt, v, P, Q)
        assert np.abs(an.method.voltage.real - v.real).max() <= 1e-12 and np.abs(an.method.voltage.imag - v.imag).max() <= 1e-12, step
    assert an.method.iteration == 5
    whole = jg.gaussSeidel(s, batch=3)
    jg.setOutages_(whole, labels)
    jg.powerFlow_(whole, iteration=5, tolerance=0.0)
    assert list(whole.method.iteration) == [5, 5, 5] and list(whole.status) == [1, 1, 1]
    assert np.array_equal(whole.method.voltage, an.method.voltage)                      # bitwise
    assert np.array_equal(np.stack(whole.mismatch), np.stack(jg.mismatch_(an)))


CASE14_COUNTS = {1: 923, 2: 454, 4: 465, 5: 366, 7: 525, 8: 343, 9: 336, 10: 541, 12: 272, 13: 274, 15: 232, 17: 270, 19: 275, 20: 284, 0: 281, 3: 281, 18: 281}


@pytest.mark.parametrize("batch", [21, 64, 65, 130])
def test_divergent_lanes_and_a_partial_last_wave(jg, batch):
    """lane b loses branch b mod 21: lanes of one wave converge after 232 .. 923 sweeps, two stagnate to the limit, two turn non-finite at once"""
    out, v = restated("case14test", tuple(range(21)), (1.0,) * 21, 1500)
    assert R.margins_hold(out, TOL)                               # FIRST: no count hangs on a rounding
    for k in range(21):                                           # what the restatement gives, as the issue recorded it
        want = (0, CASE14_COUNTS[k]) if k in CASE14_COUNTS else (1, 1500) if k in (6, 16) else (3, None)
        assert out.status[k] == want[0] and (want[1] is None or out.iteration[k] == want[1]), (k, out.status[k], out.iteration[k])
    pick = np.arange(batch) % 21
    an = jg.gaussSeidel(ac_system(jg, "case14test"), batch=batch)
    jg.setOutages_(an, pick)
    jg.powerFlow_(an, iteration=1500, tolerance=TOL)
    dev = compare_lanes(an, out, v, pick)
    print(f"batch {batch}: worst |dV| device - restatement {dev:.3e}")
    for b in range(21, batch):                                    # the same outage in another lane / another wave: the same bits
        if an.status[b] != 3:
            assert np.array_equal(an.method.voltage[b], an.method.voltage[b % 21]), b


def test_injections_of_their_own_per_lane(jg):
    scale = (0.9, 1.0, 1.1)
    out, v = restated("case30test", (0, 0, 0), scale, 2000)
    assert R.margins_hold(out, TOL) and np.all(out.status == 0) and len(set(out.iteration)) == 3
    s = ac_system(jg, "case30test")
    an = jg.gaussSeidel(s, batch=3)
    bus = s.bus
    jg.setInjection_(an, np.stack([bus.supply.active - f * bus.demand.active for f in scale]), np.stack([bus.supply.reactive - f * bus.demand.reactive for f in scale]))
    jg.powerFlow_(an, iteration=2000, tolerance=TOL)
    print("case30test, demand x", scale, "sweeps", list(an.method.iteration), "worst |dV|", compare_lanes(an, out, v, np.arange(3)))


def test_hand_off_to_newton_raphson_and_back(jg):
    s = ac_system(jg, "case118")
    flat = jg.newtonRaphson(s, batch=2)
    jg.powerFlow_(flat)
    assert list(flat.status) == [0, 0]
    gs = jg.gaussSeidel(s, batch=2)
    jg.powerFlow_(gs, iteration=5)
    assert list(gs.method.iteration) == [5, 5] and list(gs.status) == [1, 1]
    nr = jg.newtonRaphson(s, batch=2)
    jg.setInitialPoint_(nr, gs)
    assert np.array_equal(nr.voltage.magnitude, gs.voltage.magnitude) and np.array_equal(nr.voltage.angle, gs.voltage.angle)
    jg.powerFlow_(nr)
    assert list(nr.status) == [0, 0]
    assert np.abs(nr.voltage.magnitude - flat.voltage.magnitude).max() < 1e-8 and np.abs(nr.voltage.angle - flat.voltage.angle).max() < 1e-8
    jg.setInitialPoint_(gs, nr)
    p, q = jg.mismatch_(gs)
    print("Gauss-Seidel mismatch at the Newton-Raphson solution", p, q)
    assert p.max() < 1e-8 and q.max() < 1e-8


def test_a_grid_that_needs_thousands_of_sweeps(jg):
    labels = (0,) + CASE118_OUTAGES
    out, v = restated("case118", labels, (1.0,) * 5, 3000)
    assert np.all(out.status == 0) and out.iteration[0] == 2111 and R.margins_hold(out, TOL)
    pick = np.arange(65) % 5
    an = jg.gaussSeidel(ac_system(jg, "case118"), batch=65)
    jg.setOutages_(an, np.array(labels)[pick])
    jg.powerFlow_(an, iteration=3000, tolerance=TOL)
    dev = compare_lanes(an, out, v, pick)
    print("case118 sweeps", list(out.iteration), f"worst |dV| device - restatement {dev:.3e}")
    assert np.array_equal(an.method.voltage[64], an.method.voltage[4])


def test_edits_of_a_live_analysis(jg):
    s = ac_system(jg, "case14test")
    an = jg.gaussSeidel(s, batch=2)
    jg.setOutages_(an, [0, 9])
    g = R.problem(s)
    yt, v, P, Q = R.lanes(g, 2, R.lane_values(s, [0, 9]))
    for _ in range(3):
        jg.solve_(an)
        R.sweep(g, yt, v, P, Q)
    # updateGenerator!(...; magnitude): the set-point of the sweeps to come, and the bus takes it at its present angle (generator.jl:425-430)
    k = int(g.pv[0])
    gen = s.bus.supply.generator[k + 1][0]
    jg.updateGenerator_(an, gen, magnitude=1.02)
    g.vg[0] = 1.02
    v[:, k] = 1.02 * np.exp(1j * np.angle(v[:, k]))
    assert np.abs(an.method.voltage - v).max() <= 1e-12 and np.abs(an.voltage.magnitude[:, k] - 1.02).max() <= 1e-15
    jg.solve_(an)
    R.sweep(g, yt, v, P, Q)
    assert np.abs(an.method.voltage - v).max() <= 1e-12
    # updateBus!(...; active): the demand of every scenario, and the bus starts again from the system's voltage (bus.jl:350-362)
    i = int(g.pq[2])
    label = next(l for l, idx in s.bus.label.items() if idx == i + 1)
    jg.updateBus_(an, label, active=float(s.bus.demand.active[i]) + 0.05)
    P[:, i] = s.bus.supply.active[i] - s.bus.demand.active[i]
    v[:, i] = s.bus.voltage.magnitude[i] * np.exp(1j * s.bus.voltage.angle[i])
    before = v.copy()
    jg.solve_(an)
    R.sweep(g, yt, v, P, Q)
    assert np.abs(v - before).max() > 1e-4 and np.abs(an.method.voltage - v).max() <= 1e-12
    assert an.method.iteration == 5
    # all zeros after outages: the base lane again, bit for bit
    base = jg.gaussSeidel(s, batch=2)
    jg.setOutages_(an, [0, 0])
    jg.setInitialPoint_(an)
    jg.powerFlow_(an, iteration=7, tolerance=0.0)
    jg.powerFlow_(base, iteration=7, tolerance=0.0)
    assert np.array_equal(an.method.voltage, base.method.voltage) and np.array_equal(an.method.voltage[0], an.method.voltage[1])
    with pytest.raises(TypeError):
        jg.power_(an)
    # a bus type change under the analysis
    jg.updateBusSystem_(s, label, type=2)
    with pytest.raises(RuntimeError, match="cannot be reused"):
        jg.solve_(an)
    with pytest.raises(RuntimeError, match="cannot be reused"):
        jg.powerFlow_(an)
