"""Batched DC least-absolute-value state estimation (the reference's dcLavStateEstimation / solve! / power!).

  dcLavStateEstimation(monitoring, optimizer)   src/stateEstimation/dcStateEstimation.jl:201-313, src/backend/expressions.jl:381-421
  solve!(analysis)                              :436-480 (the reference hands the LP to a JuMP optimizer)
  power!(analysis)                              src/postprocessing/dcAnalysis.jl:106-131, 353-374
  setInitialPoint!(analysis[, source])          the angles of a DcStateEstimation, a DcPowerFlow or another LAV analysis
  updateWattmeter! / updatePmu!                 src/measurement/powermeter.jl:704-757, pmu.jl:877-899 (status and mean)

The rows are those of the DC WLS model (dcstateestimation._dc_rows / _dc_values): every wattmeter in stored order, then every PMU at a bus; the slack's
angle is fixed; a row with status 0 leaves the model.  The objective is unweighted, as in the reference: min sum_i |z_i - h_i theta|.  `weighted=True`
scales row i by 1 / sigma_i on the host (the common form in the literature): the device sees a scaled H and z, nothing else changes, and `residual`,
`objective` and `dual` are those of the scaled rows.

All numerics run in libjgrid_hip.so (csrc/jg_dclav.hip): per lane a primal-dual interior-point method (Mehrotra's predictor-corrector), whose gain
matrix H' Q H has a diagonal Q of its own in every lane and iteration and is factorised per lane on ONE symbolic analysis (csrc/jg_dc_lanefactor.hip).
A batched analysis keeps `batch` realisations of ONE measurement set; arrays are [batch, ...] (1-D for batch 1).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from . import stateestimation as _se
from .dcstateestimation import _dc_rows, _dc_values, _to_csc
from .measurement import Measurement
from .system import dcModel_


def dcLavModel(monitoring: Measurement):
    """the LAV model on the host, no device: coefficient (CscMatrix in the reference's layout, [number, buses]), mean, index (PMU -> row), number,
    inservice -- the rows of dcWlsModel without its precision."""
    sysm = monitoring.system
    if sysm.bus.layout.slack == 0:
        raise RuntimeError("The slack bus is missing.")
    if sysm.model.dc.nodalMatrix is None:
        dcModel_(sysm)
    ptr, col, val, devs, index = _dc_rows(monitoring)
    status, _, mean, _ = _dc_values(monitoring, devs)
    coefficient = _to_csc(sysm.bus.number, ptr, col, val, status)[0]
    return NS(coefficient=coefficient, mean=mean, index=index, number=len(devs), inservice=int(status.sum()))


class DcLavStateEstimation:
    """DcStateEstimation{LAV} (src/definition/analysis.jl) with a batch: voltage.angle, power.{injection, supply, from_, to, generator},
    method.{coefficient, mean, index, number, inservice}; objective, iterations, status, residual, dual and gap per lane after solve_."""

    def __init__(self, monitoring: Measurement, batch: int, iteration: int, tolerance: float, weighted: bool, device: int):
        self.monitoring, self.system = monitoring, monitoring.system
        sysm = self.system
        self.batch, self.device, self.iteration, self.tolerance, self.weighted = int(batch), int(device), int(iteration), float(tolerance), bool(weighted)
        if sysm.bus.layout.slack == 0:
            raise RuntimeError("The slack bus is missing.")
        if sysm.model.dc.nodalMatrix is None:
            dcModel_(sysm)
        n = sysm.bus.number
        self._ptr, self._col, self._val, self._devs, index = _dc_rows(monitoring)
        status, _, mean, sigma = _dc_values(monitoring, self._devs)
        coefficient, self._order, self._row = _to_csc(n, self._ptr, self._col, self._val, status)
        self.method = NS(coefficient=coefficient, mean=mean, index=index, number=len(self._devs), inservice=int(status.sum()))
        self._status = status
        self._scale = 1.0 / sigma if self.weighted else np.ones(mean.size)          # what a row of H and its reading are multiplied by on the way to the device
        self._h = 0
        h = C.c_int64(0)
        slack = int(sysm.bus.layout.slack)
        val = np.ascontiguousarray(self._val * np.repeat(self._scale, np.diff(self._ptr)))
        _lib.check(_lib.lib().jg_dclav_create(C.byref(h), n, self.method.number, self._ptr, self._col, val, np.ascontiguousarray(status, dtype=np.int32), slack,
                                              float(sysm.bus.voltage.angle[slack - 1]), self.batch, self.device))
        self._h = h.value
        br = sysm.branch
        _lib.check(_lib.lib().jg_dclav_set_branches(self._h, br.number, np.ascontiguousarray(br.layout.from_, dtype=np.int64),
                                                    np.ascontiguousarray(br.layout.to, dtype=np.int64), np.ascontiguousarray(sysm.model.dc.admittance),
                                                    np.ascontiguousarray(br.parameter.shiftAngle, dtype=np.float64)))
        self.readings = np.tile(mean, (self.batch, 1))                      # [batch, m] the mean of every lane, unscaled
        self._readings_dirty, self._status_dirty = True, False
        self.voltage = NS(angle=self._shape(np.tile(np.asarray(sysm.bus.voltage.angle, dtype=np.float64), (self.batch, 1))))
        self.power = NS(injection=NS(active=None), supply=NS(active=None), generator=NS(active=None), from_=NS(active=None), to=NS(active=None))
        self.status = 0 if self.batch == 1 else np.zeros(self.batch, dtype=np.int32)
        self.objective = self.iterations = self.residual = self.dual = self.gap = None

    coefficient = property(lambda self: self.method.coefficient)
    mean = property(lambda self: self.method.mean)

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def close(self):
        if getattr(self, "_h", 0):
            _lib.lib().jg_dclav_destroy(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        d = np.zeros(14, dtype=np.int64)
        _lib.check(_lib.lib().jg_dclav_dims(self._h, d))
        return dict(zip(("n", "m", "batch", "ld", "gainEntries", "entries", "factorLevels", "forwardLevels", "backwardLevels", "sweepLaunches", "bytesPerLane",
                         "inservice", "factorizations", "lastIterations"), map(int, d)))

    def time_kernel(self, kernel: int, reps: int = 20) -> np.ndarray:
        """milliseconds of `reps` runs (HIP events), every lane running: 0 a whole iteration but its update, 1 the assembly, 2 the factorisation, 3 one
        sweep pair, 4 the row, column and step passes"""
        ms = np.zeros(int(reps))
        _lib.check(_lib.lib().jg_dclav_time_kernel(self._h, int(kernel), int(reps), ms))
        return ms

    def factor_solve(self, q, rhs):
        """the lane-valued factor alone: q [batch, m] the lanes' weights, rhs [batch, buses] -> (H' Q H)^-1 rhs [batch, buses] (the slack's row and
        column the identity) and the lanes' bad-pivot flags.  The analysis needs a new solve_ afterwards."""
        q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float64)
        rhs = np.ascontiguousarray(np.atleast_2d(rhs), dtype=np.float64)
        if q.shape != (self.batch, self.method.number) or rhs.shape != (self.batch, self.system.bus.number):
            raise ValueError("factor_solve: q must be [batch, rows], rhs [batch, buses]")
        x, bad = np.zeros_like(rhs), np.zeros(self.batch, dtype=np.int32)
        _lib.check(_lib.lib().jg_dclav_factor_solve(self._h, q.reshape(-1), rhs.reshape(-1), x.reshape(-1), bad))
        return x, bad

    def _refresh_row(self, family: str, i: int):
        """the analysis follows its Measurement container for ONE device: a changed status re-runs the start of the next solve_ on the changed row set
        (nothing symbolic), a changed reading moves the mean of every lane"""
        key = ("w" if family == "wattmeter" else "p", i)
        if key not in self._devs:
            return                                                          # a PMU at a branch has no row
        r = self._devs.index(key)
        status, _, mean, _ = _dc_values(self.monitoring, self._devs)
        se = self.method
        if status[r] != self._status[r]:
            self._status_dirty = True
        self._status[r], se.mean[r] = status[r], mean[r]
        se.inservice = int(self._status.sum())
        se.coefficient.nzval[:] = (self._val * self._status[self._row])[self._order]
        self.readings[:, r] = mean[r]
        self._readings_dirty = True


def dcLavStateEstimation(monitoring: Measurement, batch: int = 1, iteration: int = 50, tolerance: float = 1e-8, weighted: bool = False,
                         device: int = 0) -> DcLavStateEstimation:
    """dcLavStateEstimation(monitoring, optimizer) without an optimizer: the LAV model of the DC framework for `batch` realisations, its gain pattern
    analysed once on the device.  iteration, tolerance: the limits of solve_; weighted: rows scaled by 1 / sigma (the reference's model is unweighted)."""
    if int(iteration) < 0 or not float(tolerance) > 0.0:
        raise ValueError("dcLavStateEstimation: iteration must not be negative, tolerance positive")
    return DcLavStateEstimation(monitoring, batch, iteration, tolerance, weighted, device)


def _sync(an: DcLavStateEstimation):
    L = _lib.lib()
    if an._status_dirty:
        _lib.check(L.jg_dclav_set_status(an._h, np.ascontiguousarray(an._status, dtype=np.int32)))
        an._status_dirty = False
    if an._readings_dirty:
        _lib.check(L.jg_dclav_set_readings(an._h, 0, an.batch, np.ascontiguousarray(an.readings * an._scale[None, :]).reshape(-1)))
        an._readings_dirty = False


def solve_(an: DcLavStateEstimation):
    """solve!(analysis) for every lane.  analysis.status: 0 solved, 5 the iteration limit (the angles are the last iterate), 1 the in-service rows do
    not observe the grid (every lane, NaN), 3 a zero or non-finite pivot in a later iteration of that lane (frozen at its last iterate).  Every call
    starts anew from the start rule (or from setInitialPoint_, once): interior-point iterations are not warm-started, so a second solve_ after
    setReadings_ equals a fresh analysis."""
    _sync(an)
    L = _lib.lib()
    _lib.check(L.jg_dclav_solve(an._h, an.iteration, an.tolerance))
    n, m, T = an.system.bus.number, an.method.number, an.batch
    th, st, obj, it = np.zeros((T, n)), np.zeros(T, dtype=np.int32), np.zeros(T), np.zeros(T, dtype=np.int32)
    _lib.check(L.jg_dclav_get_angle(an._h, th.ctypes.data_as(_lib.VP), st.ctypes.data_as(_lib.VP), obj.ctypes.data_as(_lib.VP), it.ctypes.data_as(_lib.VP)))
    r, y, gap = np.zeros((T, m)), np.zeros((T, m)), np.zeros(T)
    _lib.check(L.jg_dclav_get_residual(an._h, r.reshape(-1)))
    _lib.check(L.jg_dclav_get_dual(an._h, y.ctypes.data_as(_lib.VP), gap.ctypes.data_as(_lib.VP)))
    an.voltage.angle = an._shape(th)
    an.residual, an.dual = an._shape(r), an._shape(y)
    if T == 1:
        an.status, an.objective, an.iterations, an.gap = int(st[0]), float(obj[0]), int(it[0]), float(gap[0])
    else:
        an.status, an.objective, an.iterations, an.gap = st, obj, it, gap


def stateEstimation_(an: DcLavStateEstimation, power: bool = False):
    """stateEstimation!(analysis; power)."""
    solve_(an)
    if power:
        power_(an)


def setReadings_(an: DcLavStateEstimation, values, scenario0: int = 0):
    """the mean of lanes scenario0 .. : values [count, m] in row order, as the WLS analysis takes them (the constants of meanPi / meanPij / meanθi already
    taken out, as in analysis.method.mean; unscaled also for a weighted analysis)."""
    v = np.atleast_2d(np.asarray(values, dtype=np.float64))
    if v.shape[1] != an.method.number or scenario0 < 0 or scenario0 + v.shape[0] > an.batch:
        raise ValueError("setReadings_: values must be [count, rows] with scenario0 + count <= batch")
    an.readings[scenario0:scenario0 + v.shape[0]] = v * an._status[None, :]
    an._readings_dirty = True


def setInitialPoint_(an: DcLavStateEstimation, other=None):
    """setInitialPoint!(analysis[, source]): the NEXT solve_ starts from these angles instead of the unit-weight least-squares estimate -- those of
    `other` (a DcStateEstimation, a DcPowerFlow or another LAV analysis; one lane is given to every lane), or the bus angles of the power system."""
    n = an.system.bus.number
    src = np.asarray(an.system.bus.voltage.angle if other is None else other.voltage.angle, dtype=np.float64)
    src = np.atleast_2d(src)
    if src.shape[1] != n or src.shape[0] not in (1, an.batch):
        raise ValueError("setInitialPoint_: the source holds angles of another grid or another batch")
    th = np.ascontiguousarray(np.broadcast_to(src, (an.batch, n)))
    _lib.check(_lib.lib().jg_dclav_set_initial(an._h, th.reshape(-1)))


def updateWattmeter_(an: DcLavStateEstimation, label, active=None, status=None):
    """updateWattmeter!(analysis; label, active, status): the container and the analysis' row follow."""
    _se.updateWattmeter_(an.monitoring, label, active=active, status=status)
    an._refresh_row("wattmeter", int(label) - 1)


def updatePmu_(an: DcLavStateEstimation, label, angle=None, statusAngle=None):
    """updatePmu!(analysis; label, angle, statusAngle): the container and the analysis' row follow."""
    _se.updatePmu_(an.monitoring, label, angle=angle, statusAngle=statusAngle)
    an._refresh_row("pmu", int(label) - 1)


def power_(an: DcLavStateEstimation):
    """power!(analysis) for every lane, as dcstateestimation.power_: branch flows on the device (the DC flow kernel); injection = B theta + shiftPower +
    shunt conductance and supply = injection + demand on the host; generator by the rule of the DC power flow."""
    _power(an, _lib.lib().jg_dclav_get_flows)


def _power(an, get_flows):
    """power_ of an analysis whose handle delivers its branch flows through `get_flows` (dchuberstateestimation shares it)"""
    sysm = an.system
    bus, gen, br, dc = sysm.bus, sysm.generator, sysm.branch, sysm.model.dc
    fr = np.zeros((an.batch, br.number))
    _lib.check(get_flows(an._h, fr.reshape(-1)))
    th = np.atleast_2d(an.voltage.angle)
    B = dc.nodalMatrix
    col_of = np.repeat(np.arange(bus.number), np.diff(B.colptr))
    inj = np.zeros((an.batch, bus.number))
    for b in range(an.batch):
        np.add.at(inj[b], B.rowval - 1, B.nzval * th[b, col_of])
    inj += (dc.shiftPower + bus.shunt.conductance)[None, :]
    sup = inj + bus.demand.active[None, :]
    slack = bus.layout.slack - 1
    gp = np.zeros((an.batch, gen.number))
    on = gen.layout.status == 1
    gp[:, on] = gen.output.active[on]
    lst = bus.supply.generator.get(slack + 1, [])
    if lst and gen.layout.status[lst[0] - 1] == 1:
        gp[:, lst[0] - 1] = inj[:, slack] + bus.demand.active[slack] - sum(gen.output.active[j - 1] for j in lst[1:])
    pw = an.power
    pw.injection, pw.supply, pw.generator = NS(active=an._shape(inj)), NS(active=an._shape(sup)), NS(active=an._shape(gp))
    pw.from_, pw.to = NS(active=an._shape(fr)), NS(active=an._shape(-fr))
