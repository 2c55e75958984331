"""The host I/O that the Newton-Raphson and the Gauss-Newton handle share (csrc/jg_lanes.hip): rows go up and come down through ONE staging buffer and two
transpose kernels, result records are packed by the same kernel, and the state of all that is per handle.  Every value that passes is copied, never computed,
so every comparison here is bitwise.  Shapes: 14 buses (less than one 64 x 64 tile) and 118 (two row tiles, the second ragged); batches 1, 3, 64 and 70 --
70 pads to 128 lanes, so lanes 70..127 are padding and the last lane tile is ragged on the way down."""
import numpy as np
import pytest

from conftest import load_case
from test_oracle_se import se_case14
from test_se_gpu import _all_families, _mirror, _system_like

pytestmark = pytest.mark.gpu

BATCHES = [1, 3, 64, 70]
SHAPES = [(name, b) for name in ("case14", "case118") for b in BATCHES]
_CACHE = {}


def _system(jg, name):
    return jg.powerSystem(load_case(name))


def _monitoring(jg, oracle, name):
    """The measurement sets of tests/test_se_gpu.py: every family on the modified IEEE 14 system (correlated PMUs), every device the product can synthesise
    from a power flow on case118.  Built once."""
    if name not in _CACHE:
        if name == "case14":
            t, osys, vm, va = se_case14(oracle)
            _CACHE[name] = _mirror(jg, _system_like(jg, t, osys), _all_families(oracle, osys, vm, va, dict(correlated=True)))
        else:
            s = _system(jg, name)
            pf = jg.newtonRaphson(s)
            jg.powerFlow_(pf, tolerance=1e-10)
            assert pf.status == 0
            mon = jg.measurement(s)
            jg.addVoltmeter_(mon, pf)
            jg.addAmmeter_(mon, pf, minMagnitude=1e-6)
            jg.addWattmeter_(mon, pf)
            jg.addVarmeter_(mon, pf)
            jg.addPmu_(mon, pf, minMagnitude=1e-6)
            _CACHE[name] = mon
    return _CACHE[name]


def _voltage(an):
    """(magnitude, angle) as the device holds them, [batch, n]"""
    an._pull_voltage()
    return np.array(np.atleast_2d(an.voltage.magnitude)), np.array(np.atleast_2d(an.voltage.angle))


def _device_buffer(torch, shape):
    t = torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.current_stream().synchronize()                     # the fill runs on torch's stream, the library writes on its own: finish it first
    return t


@pytest.mark.parametrize("name,batch", SHAPES)
def test_nr_voltage_round_trip(jg, name, batch):
    an = jg.newtonRaphson(_system(jg, name), batch=batch)
    n = an.system.bus.number
    rng = np.random.default_rng(100 + batch)
    vm, va = rng.uniform(0.9, 1.1, (batch, n)), rng.uniform(-0.5, 0.5, (batch, n))
    jg.powerflow._push_voltage(an, vm, va)
    gm, ga = _voltage(an)
    assert np.array_equal(gm, vm) and np.array_equal(ga, va)
    jg.powerflow._push_voltage(an, vm[0], va[0])                  # ONE [n] vector (stride 0): every scenario gets it
    gm, ga = _voltage(an)
    assert gm.shape == (batch, n)
    assert np.array_equal(gm, np.broadcast_to(vm[0], (batch, n))) and np.array_equal(ga, np.broadcast_to(va[0], (batch, n)))


@pytest.mark.parametrize("name,batch", SHAPES)
def test_nr_voltage_with_a_pitch_of_the_callers(jg, name, batch):
    an = jg.newtonRaphson(_system(jg, name), batch=batch)
    n = an.system.bus.number
    rng = np.random.default_rng(200 + batch)
    wide_m, wide_a = rng.uniform(0.9, 1.1, (batch, n + 3)), rng.uniform(-0.5, 0.5, (batch, n + 3))
    jg.powerflow._push_voltage(an, wide_m[:, :n], wide_a[:, :n])                                   # contiguous: the staged way
    cm, ca = _voltage(an)
    jg.powerflow._push_voltage(an, np.zeros(n), np.zeros(n))
    jg._lib.check(jg._lib.lib().jg_nr_set_voltage(an._h, wide_m.reshape(-1), wide_a.reshape(-1), n + 3))
    gm, ga = _voltage(an)
    assert np.array_equal(gm, cm) and np.array_equal(ga, ca)
    assert np.array_equal(gm, wide_m[:, :n]) and np.array_equal(ga, wide_a[:, :n])


@pytest.mark.parametrize("name,batch", SHAPES)
def test_gn_voltage_with_a_pitch_of_the_callers(jg, oracle, name, batch):
    an = jg.gaussNewton(_monitoring(jg, oracle, name), batch=batch)
    n = an.system.bus.number
    rng = np.random.default_rng(300 + batch)
    wide_m, wide_a = rng.uniform(0.9, 1.1, (batch, n + 3)), rng.uniform(-0.5, 0.5, (batch, n + 3))
    an.setVoltage(wide_m[:, :n], wide_a[:, :n])
    cm, ca = _voltage(an)
    an.setVoltage(np.zeros(n), np.zeros(n))
    jg._lib.check(jg._lib.lib().jg_gn_set_voltage(an._h, wide_m.reshape(-1), wide_a.reshape(-1), n + 3))
    gm, ga = _voltage(an)
    assert np.array_equal(gm, cm) and np.array_equal(ga, ca)
    assert np.array_equal(gm, wide_m[:, :n]) and np.array_equal(ga, wide_a[:, :n])


def _nr_started(jg, s, batch, seed):
    """A batch whose scenarios start from points of their own, further from the flat start the higher the lane: states, iteration counts and records differ by lane."""
    an = jg.newtonRaphson(s, batch=batch)
    n = s.bus.number
    rng = np.random.default_rng(seed)
    amp = np.linspace(0.0, 1.0, batch)[:, None]
    vm0, va0 = np.atleast_2d(an.voltage.magnitude)[:1], np.atleast_2d(an.voltage.angle)[:1]
    jg.powerflow._push_voltage(an, vm0 * (1.0 + 0.04 * amp * rng.uniform(-1, 1, (batch, n))), va0 + 0.15 * amp * rng.uniform(-1, 1, (batch, n)))
    return an


def test_nr_records(jg):
    import torch
    s = _system(jg, "case118")
    B, n = 70, s.bus.number
    an = _nr_started(jg, s, B, 7)
    jg.powerFlow_(an)
    vm, va = _voltage(an)
    assert len(np.unique(vm, axis=0)) > 1                         # the lanes do hold different states
    dm, da = _device_buffer(torch, (B, n)), _device_buffer(torch, (B, n))
    an.voltage_device(dm.data_ptr(), da.data_ptr())
    assert np.array_equal(dm.cpu().numpy(), vm, equal_nan=True) and np.array_equal(da.cpu().numpy(), va, equal_nan=True)
    rec = _device_buffer(torch, (B, 2 * n + 2))
    an.pack_results_device(rec.data_ptr())
    rec = rec.cpu().numpy()
    assert np.array_equal(rec[:, :n], vm, equal_nan=True) and np.array_equal(rec[:, n:2 * n], va, equal_nan=True)
    assert np.array_equal(rec[:, 2 * n], an.method.iteration.astype(np.float64)) and np.array_equal(rec[:, 2 * n + 1], an.status.astype(np.float64))


def _noisy_measurement(jg, an, seed):
    """Per-scenario readings: [batch, m] means and weights (and the pair terms of correlated PMUs) that differ by lane."""
    jg.setNoise_(an, np.random.default_rng(seed), scale=0.1)
    return tuple(np.array(np.atleast_2d(x)) for x in (an.method.mean, an.method._wdiag, an.method._woff))


@pytest.mark.parametrize("name,batch", SHAPES)
def test_gn_round_trip_and_staging_growth(jg, oracle, name, batch):
    an = jg.gaussNewton(_monitoring(jg, oracle, name), batch=batch)
    n, m, nc = an.system.bus.number, an.dims["m"], int(an.method._corr.size)
    assert m > n
    rng = np.random.default_rng(400 + batch)
    vm, va = rng.uniform(0.9, 1.1, (batch, n)), rng.uniform(-0.5, 0.5, (batch, n))
    an.setVoltage(vm, va)                                         # n rows per scenario in the staging buffer ...
    mean, wd, wo = _noisy_measurement(jg, an, 500 + batch)        # ... then m > n rows: it grows
    assert mean.shape == (batch, m) and (batch == 1 or len(np.unique(mean, axis=0)) > 1)
    gmean, gwd, gwo = jg.measurementDevice(an)
    assert np.array_equal(gmean, mean) and np.array_equal(gwd, wd)
    assert nc == 0 or np.array_equal(gwo, wo.reshape(batch, nc))
    gm, ga = _voltage(an)
    assert np.array_equal(gm, vm) and np.array_equal(ga, va)     # what went up before the buffer grew is still what the device holds


def _gn_run(jg, an, seed):
    _noisy_measurement(jg, an, seed)
    jg.stateEstimation_(an)
    vm, va = _voltage(an)
    return vm, va, np.atleast_1d(an.method.iteration).copy(), np.atleast_1d(an.status).copy(), np.atleast_1d(an.objectiveDevice()).copy()


@pytest.mark.parametrize("name", ["case14", "case118"])
def test_gn_records(jg, oracle, name):
    import torch
    B = 70
    an = jg.gaussNewton(_monitoring(jg, oracle, name), batch=B)
    n = an.system.bus.number
    vm, va, it, st, obj = _gn_run(jg, an, 11)
    assert len(np.unique(vm, axis=0)) > 1
    rec = _device_buffer(torch, (B, 2 * n + 3))
    an.pack_results_device(rec.data_ptr())
    rec = rec.cpu().numpy()
    assert np.array_equal(rec[:, :n], vm, equal_nan=True) and np.array_equal(rec[:, n:2 * n], va, equal_nan=True)
    assert np.array_equal(rec[:, 2 * n], it.astype(np.float64)) and np.array_equal(rec[:, 2 * n + 1], st.astype(np.float64))
    assert np.array_equal(rec[:, 2 * n + 2], obj, equal_nan=True)


def test_two_handles_take_turns(jg, oracle):
    """What the handles share is code, not state: an NR and a GN handle that alternate puts, runs and gets in one process give what each gives alone."""
    s, mon, B = _system(jg, "case118"), _monitoring(jg, oracle, "case118"), 70
    nr = _nr_started(jg, s, B, 21)
    jg.powerFlow_(nr)
    nr_alone = _voltage(nr) + (nr.method.iteration.copy(), nr.status.copy())
    gn_alone = _gn_run(jg, jg.gaussNewton(mon, batch=B), 22)
    nr = _nr_started(jg, s, B, 21)                                # put (NR)
    gn = jg.gaussNewton(mon, batch=B)
    _noisy_measurement(jg, gn, 22)                                # put (GN)
    jg.powerFlow_(nr, fetch=False)                                # run (NR)
    jg.stateEstimation_(gn, fetch=False)                          # run (GN)
    nr_turns = _voltage(nr) + (nr.method.iteration.copy(), nr.status.copy())      # get (NR)
    gn_turns = _voltage(gn) + (gn.method.iteration.copy(), gn.status.copy(), np.atleast_1d(gn.objectiveDevice()).copy())   # get (GN)
    gm, ga = _voltage(nr)                                      # ... and once more after the other handle's downloads
    assert np.array_equal(gm, nr_turns[0], equal_nan=True) and np.array_equal(ga, nr_turns[1], equal_nan=True)
    for a, b in zip(nr_alone + gn_alone, nr_turns + gn_turns):
        assert np.array_equal(a, b, equal_nan=True)
