"""Gauss-Seidel AC power flow, one scenario per lane (the reference's gaussSeidel and what it dispatches on AcPowerFlow{GaussSeidel}).

  gaussSeidel(system)                    src/powerFlow/acPowerFlow.jl:563-619      gaussSeidel(system, batch=1)
  mismatch!(analysis)                    acPowerFlow.jl:732-764                    mismatch_(analysis)
  solve!(analysis)                       acPowerFlow.jl:985-1041                   solve_(analysis)
  powerFlow!(analysis; ...)              acPowerFlow.jl:1389-1433                  powerFlow_(analysis, iteration, tolerance): ONE launch for the batch
  setInitialPoint!(analysis[, source])   acPowerFlow.jl:1226-1295                  setInitialPoint_
  updateBus! / updateGenerator!          bus.jl:350-362, generator.jl:410-431      updateBus_ / updateGenerator_
  updateBranch!(analysis; ...)           branch.jl:453-475                         updateBranch_ (the analysis reads the system's nodal matrix)

The functions are reached through powerflow.py, which dispatches on the analysis type.  A sweep is sequential over the buses of a scenario, so a lane
of the device runs the reference's update sequence unchanged (csrc/jg_gs.hpp); `batch` scenarios of one grid differ by a branch outage
(setOutages_) and / or by their injections (setInjection_).  power_ / current_ / reactiveLimit_ are not offered on this type: hand the state to a
Newton-Raphson analysis with setInitialPoint_(nr, gs).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from .system import (PowerSystem, acModel_, updateBus_ as _update_bus_system, updateGenerator_ as _update_generator_system)


def _reim(z):
    out = np.empty(2 * z.size, dtype=np.float64)
    out[0::2], out[1::2] = z.real, z.imag
    return out


def _setpoint(system: PowerSystem) -> np.ndarray:
    """generator.voltage.magnitude of the first in-service generator of every bus that has one (acPowerFlow.jl:1032-1033), 0 elsewhere"""
    g = np.zeros(system.bus.number)
    for i, gens in system.bus.supply.generator.items():
        g[i - 1] = system.generator.voltage.magnitude[gens[0] - 1]
    return g


class GaussSeidelPowerFlow:
    """AcPowerFlow{GaussSeidel} (src/definition/analysis.jl:211-258): voltage.{magnitude, angle}, method.{voltage, pq, pv, iteration, signature}."""

    def __init__(self, system: PowerSystem, batch: int, device: int):
        self.system, self.batch, self._device = system, int(batch), int(device)
        self._h = 0
        self.voltage = NS(magnitude=None, angle=None)
        self.method = NS(voltage=None, pq=None, pv=None, iteration=0, signature=None)
        self.status = None
        n = system.bus.number
        self._outage_labels = np.zeros(self.batch, dtype=np.int64)     # branch out of service per scenario (0 = none)
        self._P, self._Q = np.zeros((self.batch, n)), np.zeros((self.batch, n))   # what the device holds (kept for a rebuild)
        self._create()

    def _create(self):
        """jg_gs_create from the system's CURRENT nodal matrix and bus types"""
        system = self.system
        ac, rev, typ = system.model.ac, system.model.revision, system.bus.layout.type
        Y, YT = ac.nodalMatrix, ac.nodalMatrixTranspose
        h = C.c_int64(0)
        _lib.check(_lib.lib().jg_gs_create(C.byref(h), system.bus.number, Y.colptr, Y.rowval, _reim(YT.nzval), np.ascontiguousarray(typ, dtype=np.int8),
                                           int(system.bus.layout.slack), _setpoint(system), self.batch, self._device))
        self._h = h.value
        self.method.pq = np.flatnonzero(typ == 1).astype(np.int64) + 1                  # acPowerFlow.jl:575-584
        self.method.pv = np.flatnonzero(typ == 2).astype(np.int64) + 1
        self.method.signature = NS(topology=rev.topology, type=rev.type, acPattern=rev.acPattern)

    def close(self):
        if getattr(self, "_h", 0):
            _lib.lib().jg_gs_destroy(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def _pull_voltage(self):
        vm, va, re, im = (np.zeros((self.batch, self.system.bus.number)) for _ in range(4))
        _lib.check(_lib.lib().jg_gs_get_voltage(self._h, vm.ctypes.data, va.ctypes.data, re.ctypes.data, im.ctypes.data))
        self.voltage.magnitude, self.voltage.angle = self._shape(vm), self._shape(va)
        self.method.voltage = self._shape(re + 1j * im)

    @property
    def mismatch(self):
        """(stopP, stopQ) of the last mismatch_ / the last check of powerFlow_"""
        p, q = np.zeros(self.batch), np.zeros(self.batch)
        _lib.check(_lib.lib().jg_gs_get_mismatch(self._h, p, q))
        return (float(p[0]), float(q[0])) if self.batch == 1 else (p, q)

    def time_kernel(self, kernel: int, sweeps: int = 1, reps: int = 10) -> np.ndarray:
        """milliseconds of `reps` runs (HIP events): 0 powerFlow_'s launch with `sweeps` as the limit and tolerance 0, 1 the mismatch, 2 one sweep"""
        ms = np.zeros(int(reps))
        _lib.check(_lib.lib().jg_gs_time_kernel(self._h, int(kernel), int(sweeps), int(reps), ms))
        return ms


def gaussSeidel(system: PowerSystem, batch: int = 1, device: int = 0) -> GaussSeidelPowerFlow:
    """gaussSeidel(system) (acPowerFlow.jl:563-619).  Mutates bus types / slack like the reference."""
    from .powerflow import initializeACPowerFlow
    if system.bus.layout.slack == 0:
        raise RuntimeError("The slack bus is missing.")
    if system.model.ac.nodalMatrix is None:
        acModel_(system)
    vm, va = initializeACPowerFlow(system)
    an = GaussSeidelPowerFlow(system, batch, device)
    setInjection_(an)
    _push_voltage(an, vm, va)
    return an


def _push_voltage(an: GaussSeidelPowerFlow, vm, va):
    vm, va = np.ascontiguousarray(vm, dtype=np.float64), np.ascontiguousarray(va, dtype=np.float64)
    n = an.system.bus.number
    if vm.shape != va.shape or vm.shape not in ((n,), (an.batch, n)):
        raise ValueError("voltage: [n] or [batch, n]")
    _lib.check(_lib.lib().jg_gs_set_voltage(an._h, vm.reshape(-1), va.reshape(-1), 0 if vm.ndim == 1 else n))
    an._pull_voltage()


def setInjection_(an: GaussSeidelPowerFlow, active=None, reactive=None, scenario0: int = 0):
    """supply - demand per scenario: [n] for every lane, or [count, n] for lanes scenario0 .. scenario0 + count - 1; default: the system's own"""
    bus = an.system.bus
    p = np.asarray(bus.supply.active - bus.demand.active if active is None else active, dtype=np.float64)
    q = np.asarray(bus.supply.reactive - bus.demand.reactive if reactive is None else reactive, dtype=np.float64)
    if p.ndim == 1 and q.ndim == 1:
        if scenario0:
            raise ValueError("setInjection_: scenario0 goes with [count, n] injections")
        p, q = np.broadcast_to(p, (an.batch, bus.number)), np.broadcast_to(q, (an.batch, bus.number))
    elif p.ndim != q.ndim:
        k = max(p.shape[0] if p.ndim == 2 else 0, q.shape[0] if q.ndim == 2 else 0)
        p, q = np.broadcast_to(p, (k, bus.number)), np.broadcast_to(q, (k, bus.number))
    if p.shape != q.shape or p.shape[1] != bus.number or scenario0 < 0 or scenario0 + p.shape[0] > an.batch:
        raise ValueError("setInjection_: [n] or [count, n] with scenario0 + count <= batch")
    p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
    _lib.check(_lib.lib().jg_gs_set_injection(an._h, int(scenario0), p.shape[0], p.reshape(-1), q.reshape(-1), bus.number))
    an._P[scenario0:scenario0 + p.shape[0]], an._Q[scenario0:scenario0 + p.shape[0]] = p, q


def transposedOutageTable(system: PowerSystem):
    """outagePatchTable for a walk of nodalMatrixTranspose.nzval: the position of Ybus entry (row, col) there is the position of (col, row) in
    nodalMatrix, so the (i, j) and (j, i) pointers change places; the deltas stay."""
    from .powerflow import outagePatchTable
    ptr, dy = outagePatchTable(system)
    return ptr[:, [0, 1, 3, 2]], dy


def setOutages_(an: GaussSeidelPowerFlow, labels, scenario0: int = 0):
    """scenario scenario0 + s = base grid with branch labels[s] out of service (0 / None = base grid)"""
    lab = np.array([int(x) if x else 0 for x in labels], dtype=np.int64)
    if lab.size == 0:
        return
    if lab.min() < 0 or lab.max() > an.system.branch.number:
        raise IndexError("setOutages_: branch label out of range")
    on = lab > 0
    ptr, dy = np.zeros((lab.size, 4), dtype=np.int64), np.zeros((lab.size, 4), dtype=np.complex128)
    if on.any():                                                  # (a grid without a branch has no table to index)
        tptr, tdy = transposedOutageTable(an.system)
        ptr[on], dy[on] = tptr[lab[on] - 1], tdy[lab[on] - 1]
    _lib.check(_lib.lib().jg_gs_set_outages(an._h, int(scenario0), lab.size, np.ascontiguousarray(ptr.reshape(-1)), _reim(np.ascontiguousarray(dy.reshape(-1)))))
    an._outage_labels[scenario0:scenario0 + lab.size] = lab


def _upload_ybus(an: GaussSeidelPowerFlow):
    """New values of the system's nodal matrix on the pattern the handle has; the lanes' outages are edits of THOSE values, so they follow"""
    if an.system.model.revision.acPattern != an.method.signature.acPattern:
        return                                                    # new pattern: the next mismatch_ / solve_ / powerFlow_ rebuilds the handle
    _lib.check(_lib.lib().jg_gs_set_ybus(an._h, _reim(an.system.model.ac.nodalMatrixTranspose.nzval)))
    if np.any(an._outage_labels):
        setOutages_(an, an._outage_labels)


def _rebuild(an: GaussSeidelPowerFlow):
    """The Ybus pattern changed under a live analysis (addBranch_ between two buses that had no entry): a new handle, and the state moves over --
    voltages, injections, outages.  The reference goes on here: its solve! reads the system's nodal matrix, _addBranch! (branch.jl:190-192) only checks
    the bus types and syncTopology! takes the new topology revision, so method.voltage stays what it was.  The voltages therefore move as re / im, bit
    for bit, not through magnitude and angle."""
    an._pull_voltage()
    v = np.atleast_2d(an.method.voltage)
    an.close()
    an._create()
    _lib.check(_lib.lib().jg_gs_set_injection(an._h, 0, an.batch, an._P.reshape(-1), an._Q.reshape(-1), an.system.bus.number))
    _lib.check(_lib.lib().jg_gs_set_voltage_rect(an._h, np.ascontiguousarray(v.real).reshape(-1), np.ascontiguousarray(v.imag).reshape(-1), an.system.bus.number))
    an._pull_voltage()
    if np.any(an._outage_labels):
        setOutages_(an, an._outage_labels)


def _check_signature(an: GaussSeidelPowerFlow):
    rev, sig = an.system.model.revision, an.method.signature
    if rev.topology != sig.topology or rev.type != sig.type:     # acPowerFlow.jl:993-995
        raise RuntimeError("The power flow model cannot be reused due to required bus type conversion.")
    if rev.acPattern != sig.acPattern:
        _rebuild(an)


def mismatch_(an: GaussSeidelPowerFlow):
    """mismatch!(analysis) -> (stopP, stopQ); arrays of length batch when batch > 1"""
    if an.system.model.revision.acPattern != an.method.signature.acPattern:
        _rebuild(an)
    p, q = np.zeros(an.batch), np.zeros(an.batch)
    _lib.check(_lib.lib().jg_gs_mismatch(an._h, p, q))
    return (float(p[0]), float(q[0])) if an.batch == 1 else (p, q)


def solve_(an: GaussSeidelPowerFlow):
    """solve!(analysis): one sweep of every scenario"""
    _check_signature(an)
    _lib.check(_lib.lib().jg_gs_solve(an._h))
    an.method.iteration += 1
    an._pull_voltage()


def powerFlow_(an: GaussSeidelPowerFlow, iteration: int = 20, tolerance: float = 1e-8, fetch: bool = True):
    """powerFlow!(analysis; iteration, tolerance): method.iteration and status per scenario (0 converged, 1 iteration limit, 3 a mismatch that is not
    finite: an outage left a bus without admittance)"""
    _check_signature(an)
    it, st = np.zeros(an.batch, dtype=np.int32), np.zeros(an.batch, dtype=np.int32)
    _lib.check(_lib.lib().jg_gs_run(an._h, int(iteration), float(tolerance), it, st))
    an.method.iteration = int(it[0]) if an.batch == 1 else it
    an.status = int(st[0]) if an.batch == 1 else st
    if fetch:
        an._pull_voltage()


def setInitialPoint_(an: GaussSeidelPowerFlow, source=None):
    """setInitialPoint!(analysis) / setInitialPoint!(target, source) (acPowerFlow.jl:1226-1295)"""
    if source is not None:
        return _push_voltage(an, source.voltage.magnitude, source.voltage.angle)
    bus = an.system.bus
    vm = bus.voltage.magnitude.copy()
    for i, gens in bus.supply.generator.items():
        if bus.layout.type[i - 1] != 1:
            vm[i - 1] = an.system.generator.voltage.magnitude[gens[0] - 1]
    _push_voltage(an, vm, bus.voltage.angle.copy())


def _set_bus_voltage(an: GaussSeidelPowerFlow, i: int, magnitude, angle):
    """method.voltage[i] = magnitude * cis(angle) in every scenario (i 0-based); the other buses keep their bits"""
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(magnitude, dtype=np.float64), (an.batch,)))
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), (an.batch,)))
    _lib.check(_lib.lib().jg_gs_set_bus_voltage(an._h, i + 1, m, a))
    an._pull_voltage()


def updateBus_(an: GaussSeidelPowerFlow, label: int, **kwargs):
    """updateBus!(analysis; label, ...) (bus.jl:343-362): demand -> injections of every scenario, shunt -> nodal matrix diagonal, and the bus starts again
    from the system's voltage (its magnitude on a demand bus, its angle on every bus), as _updateBus! sets method.voltage[idx]"""
    _update_bus_system(an.system, label, **kwargs)
    if an.system.model.revision.type != an.method.signature.type:          # errorTypeConversion
        raise RuntimeError("The power flow model cannot be reused due to required bus type conversion.")
    bus = an.system.bus
    i = bus.label[int(label)] - 1
    if "conductance" in kwargs or "susceptance" in kwargs:
        _upload_ybus(an)
    if "active" in kwargs or "reactive" in kwargs:
        setInjection_(an)
    an._pull_voltage()
    now = np.atleast_2d(an.voltage.magnitude)[:, i]
    _set_bus_voltage(an, i, bus.voltage.magnitude[i] if bus.layout.type[i] == 1 else now, bus.voltage.angle[i])


def updateGenerator_(an: GaussSeidelPowerFlow, label: int, **kwargs):
    """updateGenerator!(analysis; label, status, active, reactive, magnitude) (generator.jl:382-431): supply -> injections of every scenario; a generator
    or slack bus takes the magnitude of its first in-service generator at its present angle"""
    sysm = an.system
    k = int(label) - 1
    if 0 <= k < sysm.generator.number and kwargs.get("status") == 0 and sysm.generator.layout.status[k] == 1:
        b = int(sysm.generator.layout.bus[k])
        if sysm.bus.layout.type[b - 1] in (2, 3) and sysm.bus.supply.generator.get(b, []) == [k + 1]:
            raise RuntimeError("The power flow model cannot be reused due to required bus type conversion.")
    _update_generator_system(sysm, label, **kwargs)
    if sysm.model.revision.type != an.method.signature.type:
        raise RuntimeError("The power flow model cannot be reused due to required bus type conversion.")
    setInjection_(an)
    i = int(sysm.generator.layout.bus[k]) - 1
    if sysm.bus.layout.type[i] in (2, 3):
        g = _setpoint(sysm)
        _lib.check(_lib.lib().jg_gs_set_setpoint(an._h, g))
        an._pull_voltage()
        _set_bus_voltage(an, i, g[i], np.atleast_2d(an.voltage.angle)[:, i])
