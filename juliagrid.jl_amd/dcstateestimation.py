"""DC state estimation with batched bad-data removal (the reference's dcStateEstimation / solve! / power! / residualTest! / chiTest).

  dcStateEstimation(monitoring[, T])   src/stateEstimation/dcStateEstimation.jl:42-151 (dcStateEstimationWls restated row for row)
  solve!(analysis)                     :342-434
  power!(analysis)                     src/postprocessing/dcAnalysis.jl:106-131, 353-374
  residualTest!(analysis; threshold)   src/stateEstimation/badData.jl:48-117
  chiTest(analysis; confidence)        :963-977
  updateWattmeter! / updatePmu!        src/measurement/powermeter.jl:704-757, pmu.jl:877-899

All numerics run in libjgrid_hip.so (csrc/jg_dcse.hip): the gain matrix is assembled and factorised ONCE per measurement set on the device, every
realisation of a batch is one right-hand side on that factor, and a lane that removes bad measurements is compensated on it (csrc/jg_dcse.hpp) where
the reference refactorises.  A batched analysis keeps `batch` realisations of ONE measurement set; arrays are [batch, ...] (1-D for batch 1).  The model
(coefficient, mean, precision) is built here on the host.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from .measurement import Measurement
from .stateestimation import WlsMethod, LU
from .system import CscMatrix, dcModel_


def _dc_rows(monitoring: Measurement):
    """Rows of se.coefficient in the reference's order: every wattmeter as stored, then every PMU at a bus (dcStateEstimation.jl:75-94).  Per row: its
    columns (1-based, ascending) and values with status 1; the device (family, 0-based index) behind it; the PMU -> row map se.index (1-based)."""
    sysm = monitoring.system
    dc, br = sysm.model.dc, sysm.branch
    B = dc.nodalMatrix
    w, p = monitoring.wattmeter, monitoring.pmu
    ptr, cols, vals, devs = [0], [], [], []
    for i in range(w.number):
        k = int(w.layout.index[i]) - 1
        if w.layout.bus[i]:                                             # column k of the nodal matrix (:108-113)
            lo, hi = B.colptr[k] - 1, B.colptr[k + 1] - 1
            cols.append(B.rowval[lo:hi])
            vals.append(np.asarray(B.nzval[lo:hi], dtype=np.float64))
        else:                                                           # +-admittance on the two ends (:115-128)
            a = dc.admittance[k] if w.layout.from_[i] else -dc.admittance[k]
            f, t = int(br.layout.from_[k]), int(br.layout.to[k])
            if f == t:
                raise ValueError(f"wattmeter {i + 1}: branch {k + 1} connects a bus to itself")
            pair = ((f, a), (t, -a)) if f < t else ((t, -a), (f, a))
            cols.append(np.array([pair[0][0], pair[1][0]], dtype=np.int64))
            vals.append(np.array([pair[0][1], pair[1][1]]))
        ptr.append(ptr[-1] + cols[-1].size)
        devs.append(("w", i))
    index = {}
    for i in range(p.number):
        if not p.layout.bus[i]:
            continue                                                    # branch PMUs are skipped (:88-94)
        index[i + 1] = len(devs) + 1
        cols.append(np.array([int(p.layout.index[i])], dtype=np.int64))
        vals.append(np.array([1.0]))
        ptr.append(ptr[-1] + 1)
        devs.append(("p", i))
    if not devs:
        raise ValueError("the measurement set holds no wattmeter and no PMU at a bus")
    return np.array(ptr, dtype=np.int64), np.concatenate(cols).astype(np.int64), np.concatenate(vals), devs, index


def _dc_values(monitoring: Measurement, devs, readings=None):
    """status, precision, and mean = status * (reading + offset) per row: meanPi / meanPij / meanθi (src/backend/equations.jl:121, 178, 461) take the shift
    power and the shunt conductance, the shift angle, and the slack's angle out of the readings.  readings: [.., m] raw readings instead of the
    container's."""
    sysm = monitoring.system
    dc, br, bus = sysm.model.dc, sysm.branch, sysm.bus
    w, p = monitoring.wattmeter, monitoring.pmu
    m = len(devs)
    status, var, z, off = np.zeros(m, dtype=np.int32), np.zeros(m), np.zeros(m), np.zeros(m)
    va_slack = float(bus.voltage.angle[bus.layout.slack - 1])
    for r, (fam, i) in enumerate(devs):
        if fam == "w":
            k = int(w.layout.index[i]) - 1
            status[r], var[r], z[r] = w.active.status[i], w.active.variance[i], w.active.mean[i]
            if w.layout.bus[i]:
                off[r] = -dc.shiftPower[k] - bus.shunt.conductance[k]
            else:
                off[r] = br.parameter.shiftAngle[k] * (dc.admittance[k] if w.layout.from_[i] else -dc.admittance[k])
        else:
            status[r], var[r], z[r], off[r] = p.angle.status[i], p.angle.variance[i], p.angle.mean[i], -va_slack
    if readings is not None:
        z = np.asarray(readings, dtype=np.float64)
    return status, 1.0 / var, status * (z + off), np.sqrt(var)


def _to_csc(n, ptr, col, val, status):
    """sparse(row, col, val): columns ascending, rows ascending inside a column, out-of-service rows as stored zeros"""
    m = ptr.size - 1
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
    order = np.lexsort((row, col))
    colptr = np.r_[1, 1 + np.cumsum(np.bincount(col - 1, minlength=n))].astype(np.int64)
    return CscMatrix(n, colptr, row[order] + 1, (val * status[row])[order]), order, row


def dcWlsModel(monitoring: Measurement):
    """dcStateEstimationWls (dcStateEstimation.jl:68-151) on the host, no device: coefficient (CscMatrix in the reference's layout, [number, buses]), mean,
    precision (the diagonal), index (PMU -> row), number, inservice."""
    sysm = monitoring.system
    if sysm.bus.layout.slack == 0:
        raise RuntimeError("The slack bus is missing.")
    if sysm.model.dc.nodalMatrix is None:
        dcModel_(sysm)
    ptr, col, val, devs, index = _dc_rows(monitoring)
    status, precision, mean, _ = _dc_values(monitoring, devs)
    coefficient = _to_csc(sysm.bus.number, ptr, col, val, status)[0]
    return NS(coefficient=coefficient, mean=mean, precision=precision, index=index, number=len(devs), inservice=int(status.sum()))


class DcStateEstimation:
    """DcStateEstimation{WLS{T}} (src/definition/analysis.jl:580-601): voltage.angle, power.{injection, supply, from_, to, generator},
    method.{coefficient, mean, precision, index, number, inservice, factorization}; also as analysis.coefficient / .mean / .precision."""

    def __init__(self, monitoring: Measurement, method, batch: int, device: int):
        if not (isinstance(method, type) and issubclass(method, WlsMethod)):
            raise TypeError("dcStateEstimation(monitoring, T): T must be one of LU, KLU, QR, LDLt, LL, Orthogonal, PetersWilkinson")
        self.monitoring, self.system = monitoring, monitoring.system
        sysm = self.system
        self.batch, self.device = int(batch), int(device)
        if sysm.bus.layout.slack == 0:
            raise RuntimeError("The slack bus is missing.")                 # checkSlackBus (:76)
        if sysm.model.dc.nodalMatrix is None:
            dcModel_(sysm)                                                  # model!(system, dc) (:77)
        n = sysm.bus.number
        self._ptr, self._col, self._val, self._devs, index = _dc_rows(monitoring)
        status, precision, mean, _ = _dc_values(monitoring, self._devs)
        coefficient, self._order, self._row = _to_csc(n, self._ptr, self._col, self._val, status)
        self.method = NS(coefficient=coefficient, mean=mean, precision=precision, index=index, number=len(self._devs), inservice=int(status.sum()),
                         factorization=method, signature={"run": False})
        self._status = status
        self._h = 0
        h = C.c_int64(0)
        slack = int(sysm.bus.layout.slack)
        _lib.check(_lib.lib().jg_dcse_create(C.byref(h), n, self.method.number, self._ptr, self._col, np.ascontiguousarray(self._val), np.ascontiguousarray(precision),
                                             np.ascontiguousarray(status, dtype=np.int32), slack, float(sysm.bus.voltage.angle[slack - 1]), self.batch, self.device))
        self._h = h.value
        br = sysm.branch
        _lib.check(_lib.lib().jg_dcse_set_branches(self._h, br.number, np.ascontiguousarray(br.layout.from_, dtype=np.int64),
                                                   np.ascontiguousarray(br.layout.to, dtype=np.int64), np.ascontiguousarray(sysm.model.dc.admittance),
                                                   np.ascontiguousarray(br.parameter.shiftAngle, dtype=np.float64)))
        self.readings = np.tile(mean, (self.batch, 1))                      # [batch, m] se.mean of every lane
        self._readings_dirty = True
        self.voltage = NS(angle=self._shape(np.tile(np.asarray(sysm.bus.voltage.angle, dtype=np.float64), (self.batch, 1))))
        self.power = NS(injection=NS(active=None), supply=NS(active=None), generator=NS(active=None), from_=NS(active=None), to=NS(active=None))
        self.status = 0 if self.batch == 1 else np.zeros(self.batch, dtype=np.int32)
        self.objective = None

    coefficient = property(lambda self: self.method.coefficient)
    mean = property(lambda self: self.method.mean)
    precision = property(lambda self: self.method.precision)

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def close(self):
        if getattr(self, "_h", 0):
            _lib.lib().jg_dcse_destroy(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        d = np.zeros(14, dtype=np.int64)
        _lib.check(_lib.lib().jg_dcse_dims(self._h, d))
        return dict(zip(("n", "m", "batch", "ld", "gainEntries", "entries", "factorLevels", "forwardLevels", "backwardLevels", "sweepLaunches", "sweepTerms",
                         "refactorizations", "omegaRuns", "maxRemoved"), map(int, d)))

    def time_kernel(self, kernel: int, reps: int = 20) -> np.ndarray:
        """milliseconds of `reps` runs (HIP events): 0 the chain of a batch, 1 the right-hand side, 2 the sweep pair, 3 the residual pass, 4 the normalised
        residual pass, 5 the Omega diagonal + that pass"""
        ms = np.zeros(int(reps))
        _lib.check(_lib.lib().jg_dcse_time_kernel(self._h, int(kernel), int(reps), ms))
        return ms

    def _refresh_row(self, family: str, i: int):
        """the analysis follows its Measurement container for ONE device (_updateWattmeter! / _updatePmu!): a changed status or variance asks for a
        re-assembly and a numeric refactorisation at the next solve (signature[:run]); a changed reading only moves se.mean -- of every lane"""
        key = ("w" if family == "wattmeter" else "p", i)
        if key not in self._devs:
            return                                                          # a PMU at a branch has no row
        r = self._devs.index(key)
        status, precision, mean, _ = _dc_values(self.monitoring, self._devs)
        se = self.method
        if status[r] != self._status[r] or precision[r] != se.precision[r]:
            se.signature["run"] = True
        self._status[r], se.precision[r], se.mean[r] = status[r], precision[r], mean[r]
        se.inservice = int(self._status.sum())
        se.coefficient.nzval[:] = (self._val * self._status[self._row])[self._order]
        self.readings[:, r] = mean[r]
        self._readings_dirty = True


def dcStateEstimation(monitoring: Measurement, method=LU, batch: int = 1, device: int = 0, **unknown) -> DcStateEstimation:
    """dcStateEstimation(monitoring[, T]): the WLS model of the DC framework, its gain matrix assembled and factorised once on the device.
    T: LU (default) | KLU | QR | LDLt | LL are the normal equations; Orthogonal | PetersWilkinson add one correction step on the same factor."""
    for name in unknown:
        raise ValueError(f"dcStateEstimation: `{name}` means nothing for a DC analysis (no iteration, no tolerance, no start: the model is linear)")
    return DcStateEstimation(monitoring, method, batch, device)


def _sync(an: DcStateEstimation):
    L = _lib.lib()
    if an.method.signature["run"]:
        an.method.signature["run"] = False
        _lib.check(L.jg_dcse_set_weights(an._h, np.ascontiguousarray(an.method.precision), np.ascontiguousarray(an._status, dtype=np.int32)))
    if an._readings_dirty:
        _lib.check(L.jg_dcse_set_readings(an._h, 0, an.batch, np.ascontiguousarray(an.readings).reshape(-1)))
        an._readings_dirty = False


def solve_(an: DcStateEstimation):
    """solve!(analysis::DcStateEstimation) for every lane; analysis.status: 0, 1 where a removed measurement was critical, 2 where a lane removed more
    rows than the device keeps (angles NaN in both)."""
    _sync(an)
    L = _lib.lib()
    _lib.check(L.jg_dcse_solve(an._h, int(an.method.factorization.code)))
    th, st, obj = np.zeros((an.batch, an.system.bus.number)), np.zeros(an.batch, dtype=np.int32), np.zeros(an.batch)
    _lib.check(L.jg_dcse_get_angle(an._h, th.ctypes.data_as(_lib.VP), st.ctypes.data_as(_lib.VP), obj.ctypes.data_as(_lib.VP)))
    an.voltage.angle = an._shape(th)
    an.status = int(st[0]) if an.batch == 1 else st
    an.objective = float(obj[0]) if an.batch == 1 else obj


def stateEstimation_(an: DcStateEstimation, power: bool = False, **unknown):
    """stateEstimation!(analysis::DcStateEstimation; power)."""
    for name in unknown:
        raise ValueError(f"stateEstimation_: `{name}` means nothing for a DC analysis (nothing is iterated)")
    solve_(an)
    if power:
        power_(an)


def setReadings_(an: DcStateEstimation, values, scenario0: int = 0):
    """se.mean of lanes scenario0 .. : values [count, m] in row order (the constants of meanPi / meanPij / meanθi already taken out, as in
    analysis.method.mean)."""
    v = np.atleast_2d(np.asarray(values, dtype=np.float64))
    if v.shape[1] != an.method.number or scenario0 < 0 or scenario0 + v.shape[0] > an.batch:
        raise ValueError("setReadings_: values must be [count, rows] with scenario0 + count <= batch")
    an.readings[scenario0:scenario0 + v.shape[0]] = v * an._status[None, :]
    an._readings_dirty = True


def setNoise_(an: DcStateEstimation, rng, scale: float = 1.0):
    """Monte-Carlo realisations drawn on the host: lane b reads z + scale * sigma * N(0, 1) on every meter (what `noise = true` does in add*!)."""
    _, _, mean, sigma = _dc_values(an.monitoring, an._devs)
    an.readings = mean[None, :] + an._status[None, :] * scale * sigma[None, :] * rng.standard_normal((an.batch, mean.size))
    an._readings_dirty = True


def _label(an: DcStateEstimation, row1: int) -> str:
    if row1 == 0:
        return ""
    fam, i = an._devs[row1 - 1]
    return f"{'Wattmeter' if fam == 'w' else 'PMU'} {i + 1}"


def residualTest_(an: DcStateEstimation, threshold: float = 3.0, labels: bool = False):
    """residualTest!(analysis; threshold) for every lane.  batch 1 follows the reference: the meter's status becomes 0 in the monitoring, its row and
    se.mean[i] are zeroed, the next solve_ re-assembles and refactorises.  A lane of a batch drops the row by compensation on the shared factor instead
    (removed(analysis)); fields are per-lane arrays, `label` on request."""
    mx, idx = np.zeros(an.batch), np.zeros(an.batch, dtype=np.int32)
    _lib.check(_lib.lib().jg_dcse_residual_test(an._h, float(threshold), 0 if an.batch == 1 else 1, mx, idx))
    with np.errstate(invalid="ignore"):
        detect = mx > threshold
    if an.batch > 1:
        return NS(detect=detect, maxNormalizedResidual=mx, index=idx, label=[_label(an, int(i)) for i in idx] if labels else None)
    i = int(idx[0])
    if detect[0] and i:
        fam, k = an._devs[i - 1]
        (an.monitoring.wattmeter.active if fam == "w" else an.monitoring.pmu.angle).status[k] = 0
        an._refresh_row("wattmeter" if fam == "w" else "pmu", k)
    return NS(detect=bool(detect[0]), maxNormalizedResidual=float(mx[0]), label=_label(an, i), index=i)


def removeMeasurement_(an: DcStateEstimation, rows):
    """lane b of a batch drops row rows[b] of se.mean (1-based, 0: none) by compensation, whatever its residual; the next solve_ applies it"""
    r = np.ascontiguousarray(rows, dtype=np.int32)
    if an.batch == 1 or r.shape != (an.batch,):
        raise ValueError("removeMeasurement_: one row per lane of a batched analysis (batch 1: updateWattmeter_ / updatePmu_ with status = 0)")
    _lib.check(_lib.lib().jg_dcse_remove_rows(an._h, r))


def removed(an: DcStateEstimation):
    """per lane the rows (1-based) it has removed, and the lane's status"""
    kmax = an.dims()["maxRemoved"]
    rows, cnt = np.zeros((an.batch, kmax), dtype=np.int32), np.zeros(an.batch, dtype=np.int32)
    _lib.check(_lib.lib().jg_dcse_get_removed(an._h, rows.reshape(-1), cnt))
    return NS(rows=[rows[b, :cnt[b]].copy() for b in range(an.batch)], status=np.atleast_1d(an.status).copy())


def normalizedResidual(an: DcStateEstimation):
    """all normalised residuals of the current estimate [batch, m] (the reference keeps only the largest)"""
    r = np.zeros((an.batch, an.method.number))
    _lib.check(_lib.lib().jg_dcse_get_normalized_residual(an._h, r.reshape(-1)))
    return an._shape(r)


def chiTest(an: DcStateEstimation, confidence: float = 0.95):
    """chiTest(analysis; confidence): the objective of the last solve against the chi-square quantile with df = inservice - bus.number + 1 (:974)."""
    from scipy.stats import chi2
    if an.objective is None:
        raise RuntimeError("chiTest: solve the analysis first")
    gone = np.array([r.size for r in removed(an).rows]) if an.batch > 1 else 0
    df = an.method.inservice - gone - an.system.bus.number + 1
    thr = chi2.ppf(confidence, df)
    if an.batch == 1:
        return NS(detect=bool(an.objective >= thr), threshold=float(thr), objective=float(an.objective))
    with np.errstate(invalid="ignore"):
        return NS(detect=an.objective >= thr, threshold=np.broadcast_to(thr, an.objective.shape).copy(), objective=an.objective)


def power_(an: DcStateEstimation):
    """power!(analysis::DcStateEstimation) for every lane: branch flows on the device (the DC flow kernel); injection = B theta + shiftPower + shunt
    conductance and supply = injection + demand on the host.  generator (the reference leaves it empty for an estimate) is filled by the rule of the DC
    power flow: outputs as given, the first in-service generator at the slack bus takes what the slack's estimated injection asks for."""
    sysm = an.system
    bus, gen, br, dc = sysm.bus, sysm.generator, sysm.branch, sysm.model.dc
    fr = np.zeros((an.batch, br.number))
    _lib.check(_lib.lib().jg_dcse_get_flows(an._h, fr.reshape(-1)))
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
