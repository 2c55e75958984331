"""Batched DC Huber and Schweppe-Huber state estimation: the M-estimator between WLS with bad-data removal (dcstateestimation) and LAV
(dclavstateestimation).  The reference has neither; the rows, the containers and the update functions are those of its DC estimators:

  solve!(analysis) / stateEstimation!           for every lane
  power!(analysis)                              src/postprocessing/dcAnalysis.jl:106-131, 353-374
  updateWattmeter! / updatePmu!                 src/measurement/powermeter.jl:704-757, pmu.jl:877-899 (status and mean)

The rows are those of the DC WLS model (dcstateestimation._dc_rows / _dc_values): every wattmeter in stored order, then every PMU at a bus; the slack's
angle is fixed; a row with status 0 leaves the model.  Row i is scaled by 1 / sigma_i on the host, so the device sees H~, z~ and unit weights, and a
bound kappa_i = threshold x omega_i per row, shared by the lanes:

    min sum_i rho_kappa_i(z~_i - h~_i theta),   rho_k(r) = r^2 / 2 for |r| <= k,  k |r| - k^2 / 2 beyond

omega = 1 is Huber's estimator; omega_i in (0, 1] are Schweppe's leverage weights, which lower the bound of a row the estimate leans on.

All numerics run in libjgrid_hip.so (csrc/jg_dchuber.hip): the problem is a QP of the shape of the LAV LP and goes through the same primal-dual
interior-point method per lane (Mehrotra's predictor-corrector), on the same lane-valued factor of H~' Q H~ (csrc/jg_dc_lanefactor.hip).  A batched
analysis keeps `batch` realisations of ONE measurement set; arrays are [batch, ...] (1-D for batch 1).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from . import stateestimation as _se
from .dclavstateestimation import _power
from .dcstateestimation import _dc_rows, _dc_values, _to_csc
from .measurement import Measurement
from .system import dcModel_


class DcHuberStateEstimation:
    """voltage.angle, power.{injection, supply, from_, to, generator}, method.{coefficient, mean, index, number, inservice}; objective (the Huber loss of
    the scaled residuals), iterations, status, residual (unscaled), weight, suspect, dual and gap per lane after solve_; threshold, omega, kappa [m]."""

    def __init__(self, monitoring: Measurement, batch: int, threshold: float, leverage, floor: float, iteration: int, tolerance: float, device: int):
        self.monitoring, self.system = monitoring, monitoring.system
        sysm = self.system
        self.batch, self.device, self.iteration, self.tolerance, self.floor = int(batch), int(device), int(iteration), float(tolerance), float(floor)
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
        self._sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        self._scale = 1.0 / self._sigma                                      # what a row of H and its reading are multiplied by on the way to the device
        self.threshold, self.leverage = float(threshold), leverage
        self.omega = self._omega_of(leverage)
        self.kappa = self.threshold * self.omega
        self._h = 0
        h = C.c_int64(0)
        slack = int(sysm.bus.layout.slack)
        val = np.ascontiguousarray(self._val * np.repeat(self._scale, np.diff(self._ptr)))
        _lib.check(_lib.lib().jg_dchuber_create(C.byref(h), n, self.method.number, self._ptr, self._col, val, np.ascontiguousarray(status, dtype=np.int32),
                                                np.ascontiguousarray(self.kappa), self._sigma, slack, float(sysm.bus.voltage.angle[slack - 1]), self.batch,
                                                self.device))
        self._h = h.value
        br = sysm.branch
        _lib.check(_lib.lib().jg_dchuber_set_branches(self._h, br.number, np.ascontiguousarray(br.layout.from_, dtype=np.int64),
                                                      np.ascontiguousarray(br.layout.to, dtype=np.int64), np.ascontiguousarray(sysm.model.dc.admittance),
                                                      np.ascontiguousarray(br.parameter.shiftAngle, dtype=np.float64)))
        self.readings = np.tile(mean, (self.batch, 1))                      # [batch, m] the mean of every lane, unscaled
        self._readings_dirty, self._status_dirty, self._bounds_dirty = True, False, False
        self.voltage = NS(angle=self._shape(np.tile(np.asarray(sysm.bus.voltage.angle, dtype=np.float64), (self.batch, 1))))
        self.power = NS(injection=NS(active=None), supply=NS(active=None), generator=NS(active=None), from_=NS(active=None), to=NS(active=None))
        self.status = 0 if self.batch == 1 else np.zeros(self.batch, dtype=np.int32)
        self.objective = self.iterations = self.residual = self.weight = self.suspect = self.dual = self.gap = None

    coefficient = property(lambda self: self.method.coefficient)
    mean = property(lambda self: self.method.mean)

    def _omega_of(self, leverage):
        """omega [m] in [floor, 1]: None -> 1; an array [m] as given; "schweppe" -> sqrt(Omega_ii / sigma_i^2) from the residual variances of the WLS path
        (dcCriticalScreen on the same monitoring).  The floor keeps kappa > 0: a critical row has Omega = 0 and a zero residual whatever its bound."""
        m = self._sigma.size
        if leverage is None:
            return np.ones(m)
        if isinstance(leverage, str):
            if leverage != "schweppe":
                raise ValueError(f"dcHuberStateEstimation: leverage is None, an array [rows] or \"schweppe\", not {leverage!r}")
            from .dccritical import dcCriticalScreen
            with np.errstate(invalid="ignore"):
                om = np.sqrt(np.maximum(dcCriticalScreen(self.monitoring).variance / self._sigma ** 2, 0.0))
            om = np.nan_to_num(om, nan=1.0, posinf=1.0)
        else:
            om = np.array(leverage, dtype=np.float64)
            if om.shape != (m,) or not np.isfinite(om).all():
                raise ValueError("dcHuberStateEstimation: leverage must be [rows] and finite")
        return np.clip(om, self.floor, 1.0)

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def close(self):
        if getattr(self, "_h", 0):
            _lib.lib().jg_dchuber_destroy(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        d = np.zeros(14, dtype=np.int64)
        _lib.check(_lib.lib().jg_dchuber_dims(self._h, d))
        return dict(zip(("n", "m", "batch", "ld", "gainEntries", "entries", "factorLevels", "forwardLevels", "backwardLevels", "sweepLaunches", "bytesPerLane",
                         "inservice", "factorizations", "lastIterations"), map(int, d)))

    def time_kernel(self, kernel: int, reps: int = 20) -> np.ndarray:
        """milliseconds of `reps` runs (HIP events), every lane running: 0 a whole iteration but its update, 1 the assembly, 2 the factorisation, 3 one
        sweep pair, 4 the row, column and step passes"""
        ms = np.zeros(int(reps))
        _lib.check(_lib.lib().jg_dchuber_time_kernel(self._h, int(kernel), int(reps), ms))
        return ms

    def _refresh_row(self, family: str, i: int):
        """the analysis follows its Measurement container for ONE device: a changed status re-runs the start of the next solve_ on the changed row set
        (nothing symbolic; Schweppe's weights follow the new set), a changed reading moves the mean of every lane"""
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


def dcHuberStateEstimation(monitoring: Measurement, batch: int = 1, threshold: float = 1.345, leverage=None, floor: float = 1e-3, iteration: int = 50,
                           tolerance: float = 1e-8, device: int = 0) -> DcHuberStateEstimation:
    """The Huber model of the DC framework for `batch` realisations, its gain pattern analysed once on the device.  threshold: c, in standard
    deviations; leverage: None (omega = 1, Huber), an array [rows] of omega, or "schweppe" (omega_i = sqrt(Omega_ii / sigma_i^2)); omega is clipped to
    [floor, 1]; iteration, tolerance: the limits of solve_."""
    if int(iteration) < 0 or not float(tolerance) > 0.0:
        raise ValueError("dcHuberStateEstimation: iteration must not be negative, tolerance positive")
    if not float(threshold) > 0.0 or not 0.0 < float(floor) <= 1.0:
        raise ValueError("dcHuberStateEstimation: threshold must be positive, floor in (0, 1]")
    return DcHuberStateEstimation(monitoring, batch, threshold, leverage, floor, iteration, tolerance, device)


def _sync(an: DcHuberStateEstimation):
    L = _lib.lib()
    if an._status_dirty:
        _lib.check(L.jg_dchuber_set_status(an._h, np.ascontiguousarray(an._status, dtype=np.int32)))
        an._status_dirty = False
        if isinstance(an.leverage, str):
            an.omega = an._omega_of(an.leverage)
            an.kappa = an.threshold * an.omega
            an._bounds_dirty = True
    if an._bounds_dirty:
        _lib.check(L.jg_dchuber_set_bounds(an._h, np.ascontiguousarray(an.kappa)))
        an._bounds_dirty = False
    if an._readings_dirty:
        _lib.check(L.jg_dchuber_set_readings(an._h, 0, an.batch, np.ascontiguousarray(an.readings * an._scale[None, :]).reshape(-1)))
        an._readings_dirty = False


def solve_(an: DcHuberStateEstimation):
    """Every lane.  analysis.status: 0 solved, 5 the iteration limit (the angles are the last iterate), 1 the in-service rows do not observe the grid
    (every lane, NaN), 3 a zero or non-finite pivot in a later iteration of that lane (frozen at its last iterate).  Every call starts anew from the
    start rule: interior-point iterations are not warm-started, so a second solve_ after setReadings_ or setThreshold_ equals a fresh analysis."""
    _sync(an)
    L = _lib.lib()
    _lib.check(L.jg_dchuber_solve(an._h, an.iteration, an.tolerance))
    n, m, T = an.system.bus.number, an.method.number, an.batch
    th, st, obj, it = np.zeros((T, n)), np.zeros(T, dtype=np.int32), np.zeros(T), np.zeros(T, dtype=np.int32)
    _lib.check(L.jg_dchuber_get_angle(an._h, th.ctypes.data_as(_lib.VP), st.ctypes.data_as(_lib.VP), obj.ctypes.data_as(_lib.VP), it.ctypes.data_as(_lib.VP)))
    r, w, y, gap = np.zeros((T, m)), np.zeros((T, m)), np.zeros((T, m)), np.zeros(T)
    _lib.check(L.jg_dchuber_get_residual(an._h, r.reshape(-1)))
    _lib.check(L.jg_dchuber_get_weight(an._h, w.reshape(-1)))
    _lib.check(L.jg_dchuber_get_dual(an._h, y.ctypes.data_as(_lib.VP), gap.ctypes.data_as(_lib.VP)))
    suspect = (w < 1.0).sum(axis=1).astype(np.int64)
    an.voltage.angle = an._shape(th)
    an.residual, an.weight, an.dual = an._shape(r), an._shape(w), an._shape(y)
    if T == 1:
        an.status, an.objective, an.iterations, an.gap, an.suspect = int(st[0]), float(obj[0]), int(it[0]), float(gap[0]), int(suspect[0])
    else:
        an.status, an.objective, an.iterations, an.gap, an.suspect = st, obj, it, gap, suspect


def stateEstimation_(an: DcHuberStateEstimation, power: bool = False):
    """stateEstimation!(analysis; power)."""
    solve_(an)
    if power:
        power_(an)


def setReadings_(an: DcHuberStateEstimation, values, scenario0: int = 0):
    """the mean of lanes scenario0 .. : values [count, m] in row order, unscaled, as the WLS analysis takes them (the constants of meanPi / meanPij /
    meanθi already taken out, as in analysis.method.mean)."""
    v = np.atleast_2d(np.asarray(values, dtype=np.float64))
    if v.shape[1] != an.method.number or scenario0 < 0 or scenario0 + v.shape[0] > an.batch:
        raise ValueError("setReadings_: values must be [count, rows] with scenario0 + count <= batch")
    an.readings[scenario0:scenario0 + v.shape[0]] = v * an._status[None, :]
    an._readings_dirty = True


def setThreshold_(an: DcHuberStateEstimation, threshold=None, leverage="unchanged"):
    """a new threshold c and / or new leverage weights (None, an array [rows], "schweppe"): kappa = c omega goes to the device, the next solve_ starts anew."""
    if threshold is not None:
        if not float(threshold) > 0.0:
            raise ValueError("setThreshold_: threshold must be positive")
        an.threshold = float(threshold)
    if not (isinstance(leverage, str) and leverage == "unchanged"):
        an.omega = an._omega_of(leverage)
        an.leverage = leverage
    an.kappa = an.threshold * an.omega
    an._bounds_dirty = True


def updateWattmeter_(an: DcHuberStateEstimation, label, active=None, status=None):
    """updateWattmeter!(analysis; label, active, status): the container and the analysis' row follow."""
    _se.updateWattmeter_(an.monitoring, label, active=active, status=status)
    an._refresh_row("wattmeter", int(label) - 1)


def updatePmu_(an: DcHuberStateEstimation, label, angle=None, statusAngle=None):
    """updatePmu!(analysis; label, angle, statusAngle): the container and the analysis' row follow."""
    _se.updatePmu_(an.monitoring, label, angle=angle, statusAngle=statusAngle)
    an._refresh_row("pmu", int(label) - 1)


def power_(an: DcHuberStateEstimation):
    """power!(analysis) for every lane, as dclavstateestimation.power_: branch flows on the device, the rest on the host."""
    _power(an, _lib.lib().jg_dchuber_get_flows)
