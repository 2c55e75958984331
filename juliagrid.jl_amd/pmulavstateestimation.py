"""Batched PMU least-absolute-value state estimation (the reference's pmuLavStateEstimation / solve! / power! / current!).

  pmuLavStateEstimation(monitoring, optimizer)   src/stateEstimation/pmuStateEstimation.jl:223-338
  solve!(analysis)                               :474-512 (the reference hands the LP to a JuMP optimizer)
  setInitialPoint!(analysis[, source])           :514-550: the system's bus voltages, an AC analysis (magnitude and angle), a DC analysis (angles)
  power! / current!(analysis)                    src/postprocessing/acAnalysis.jl:221-262 (power! of a state estimation), 672-704
  updatePmu!(analysis; ...)                      src/measurement/pmu.jl:877-899

The model is linear in the rectangular bus voltages: states re(1 .. n) then im(1 .. n), two rows per PMU in device order (real part, imaginary part),
the coefficient matrix of pmuStateEstimation (stateestimation._pmu_layout gives the rows, pmuCoefficient below their values).  Readings are polar,
`magnitude` and `angle` per PMU, and become z_re = magnitude cos(angle), z_im = magnitude sin(angle) on the device.  A PMU is in the model only if its
magnitude status AND its angle status are 1; otherwise both rows leave.  No state is fixed.  The objective is unweighted, as in the reference:
min sum |z - H x|.  `weighted=True` scales the rows of PMU i by 1 / sigma_re,i and 1 / sigma_im,i, the square roots of the diagonal of the rectangular
precision the WLS model computes for the STORED readings: the scale is constant across lanes, whatever a lane's own readings are; `residual`,
`objective` and `dual` are then those of the scaled rows, `rho` of suspect_ stays in per unit.

All numerics run in libjgrid_hip.so (csrc/jg_pmulav.hip on the interior-point iteration of csrc/jg_dclav.hip, here without a fixed state).  A batched
analysis keeps `batch` realisations of ONE PMU set; arrays are [batch, ...] (1-D for batch 1).

status per lane: 0 solved, 5 the iteration limit, 1 a state that no in-service row touches (every lane, NaN voltages), 3 a bad pivot in a later iteration
of that lane.  Status 1 is an exact zero pivot of the unit-weight start, as in the DC module: it is guaranteed only where a state has no in-service row
touching it.  A rank deficiency that leaves small non-zero pivots ends as 3 or 5; there is no rank test.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from . import stateestimation as _se
from .dcstateestimation import _to_csc
from .measurement import Measurement
from .powerflow import _branch_table, _ns2
from .system import acModel_


def pmuCoefficient(monitoring: Measurement):
    """the rows of the linear PMU model as CSR over the 2 n rectangular states: (rowptr 0-based, col 1-based ascending, val), two rows per PMU in the
    order of stateestimation._pmu_layout -- a bus PMU reads its bus, a branch PMU the pi-model's current I = y_a V_from + y_b V_to of its end"""
    sysm = monitoring.system
    if sysm.model.ac.nodalMatrix is None:
        acModel_(sysm)
    ac, n = sysm.model.ac, sysm.bus.number
    code, index = _se._pmu_layout(monitoring)[:2]
    f, t = sysm.branch.layout.from_, sysm.branch.layout.to
    ptr, col, val = [0], [], []
    for r in range(code.size):
        k, c = int(index[r]) - 1, int(code[r])
        if c in (22, 23):
            col.append(k + 1 + (n if c == 23 else 0)); val.append(1.0)
        else:
            ya, yb = (ac.nodalFromFrom[k], ac.nodalFromTo[k]) if c in (24, 25) else (ac.nodalToFrom[k], ac.nodalToTo[k])
            i, j = int(f[k]), int(t[k])
            if c in (24, 26):                                      # Re I = Re y Re V - Im y Im V
                ent = [(i, ya.real), (j, yb.real), (n + i, -ya.imag), (n + j, -yb.imag)]
            else:                                                   # Im I = Im y Re V + Re y Im V
                ent = [(i, ya.imag), (j, yb.imag), (n + i, ya.real), (n + j, yb.real)]
            for cc, v in sorted(ent):
                col.append(cc); val.append(float(v))
        ptr.append(len(col))
    return np.array(ptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=np.float64)


def _pmu_status(monitoring: Measurement):
    p = monitoring.pmu
    return (np.array(p.magnitude.status, dtype=np.int32) * np.array(p.angle.status, dtype=np.int32)).astype(np.int32)


def pmuLavModel(monitoring: Measurement):
    """the LAV model on the host, no device: coefficient (CscMatrix in the reference's layout, [2 pmus, 2 buses]), mean (rectangular, 0 on rows outside the
    model), number (rows), inservice (rows) -- the rows of the WLS model without its precision."""
    if monitoring.pmu.number == 0:
        raise ValueError("the measurement set holds no PMU")
    ptr, col, val = pmuCoefficient(monitoring)
    st = np.repeat(_pmu_status(monitoring), 2)
    p = monitoring.pmu
    mag, ang = np.array(p.magnitude.mean, dtype=np.float64), np.array(p.angle.mean, dtype=np.float64)
    mean = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1).reshape(-1) * st
    coefficient = _to_csc(2 * monitoring.system.bus.number, ptr, col, val, st)[0]
    return NS(coefficient=coefficient, mean=mean, number=int(st.size), inservice=int(st.sum()))


class PmuLavStateEstimation:
    """PmuStateEstimation{LAV} (src/definition/analysis.jl) with a batch: voltage.{magnitude, angle}, method.{coefficient, mean, number, inservice};
    objective, iterations, status, residual, dual and gap per lane after solve_; power.{injection, supply, shunt, from_, to, series, charging} and
    current.{injection, from_, to, series} after power_ / current_; rho, suspect, suspectCount,
    worst after suspect_."""

    def __init__(self, monitoring: Measurement, batch: int, iteration: int, tolerance: float, weighted: bool, device: int):
        self.monitoring, self.system = monitoring, monitoring.system
        sysm = self.system
        self.batch, self.device, self.iteration, self.tolerance, self.weighted = int(batch), int(device), int(iteration), float(tolerance), bool(weighted)
        model = pmuLavModel(monitoring)
        self._ptr, self._col, self._val = pmuCoefficient(monitoring)
        n, npmu = sysm.bus.number, monitoring.pmu.number
        self._status = _pmu_status(monitoring)
        self.method = model
        self._order, self._row = _to_csc(2 * n, self._ptr, self._col, self._val, np.repeat(self._status, 2))[1:]
        if self.weighted:
            _, _, _, _, devs, dev_row = _se._pmu_layout(monitoring)
            wdiag = _se._pmu_values(monitoring, devs, dev_row, 2 * npmu, *_se._pmu_readings(monitoring))[1]
            self._scale = np.sqrt(wdiag)
        else:
            self._scale = np.ones(2 * npmu)
        self._h = 0
        h = C.c_int64(0)
        L = _lib.lib()
        val = np.ascontiguousarray(self._val * np.repeat(self._scale, np.diff(self._ptr)))
        _lib.check(L.jg_pmulav_create(C.byref(h), n, npmu, self._ptr, self._col, val, np.ascontiguousarray(self._status), self.batch, self.device))
        self._h = h.value
        if self.weighted:
            _lib.check(L.jg_pmulav_set_scale(self._h, np.ascontiguousarray(self._scale)))
        self._branches_on_device = False
        p = monitoring.pmu
        self.magnitude = np.tile(np.array(p.magnitude.mean, dtype=np.float64), (self.batch, 1))     # [batch, pmus] the polar readings of every lane
        self.angle = np.tile(np.array(p.angle.mean, dtype=np.float64), (self.batch, 1))
        self._readings_dirty, self._status_dirty = True, False
        self.voltage = NS(magnitude=self._shape(np.tile(np.asarray(sysm.bus.voltage.magnitude, dtype=np.float64), (self.batch, 1))),
                          angle=self._shape(np.tile(np.asarray(sysm.bus.voltage.angle, dtype=np.float64), (self.batch, 1))))
        self.power = NS(injection=None, supply=None, shunt=None, from_=None, to=None, charging=None, series=None)
        self.current = NS(injection=None, from_=None, to=None, series=None)
        self.status = 0 if self.batch == 1 else np.zeros(self.batch, dtype=np.int32)
        self.objective = self.iterations = self.residual = self.dual = self.gap = None
        self.rho = self.suspect = self.suspectCount = self.worst = None

    coefficient = property(lambda self: self.method.coefficient)
    mean = property(lambda self: self.method.mean)

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def close(self):
        if getattr(self, "_h", 0):
            _lib.lib().jg_pmulav_destroy(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        d = np.zeros(14, dtype=np.int64)
        _lib.check(_lib.lib().jg_pmulav_dims(self._h, d))
        return dict(zip(("buses", "pmus", "batch", "ld", "gainEntries", "entries", "factorLevels", "forwardLevels", "backwardLevels", "sweepLaunches", "bytesPerLane",
                         "inservice", "factorizations", "lastIterations"), map(int, d)))

    def time_kernel(self, kernel: int, reps: int = 20) -> np.ndarray:
        """milliseconds of `reps` runs (HIP events), every lane running: 0 .. 4 as DcLavStateEstimation.time_kernel, 5 polar -> rectangular readings,
        6 rectangular -> polar voltages, 7 the branch and bus pass (after power_ or current_), 8 the suspect pass"""
        ms = np.zeros(int(reps))
        _lib.check(_lib.lib().jg_pmulav_time_kernel(self._h, int(kernel), int(reps), ms))
        return ms

    def _refresh(self, i: int, magnitude: bool, angle: bool):
        """the analysis follows its Measurement container for ONE PMU: a changed status re-runs the start of the next solve_ on the changed row set
        (nothing symbolic); a channel that was given a new reading (`magnitude`, `angle`) moves that reading of every lane, and a lane's readings of a
        channel that was not given stay what setReadings_ made them"""
        p = self.monitoring.pmu
        st = int(p.magnitude.status[i]) * int(p.angle.status[i])
        if st != self._status[i]:
            self._status[i] = st
            self._status_dirty = True
        if magnitude:
            self.magnitude[:, i] = p.magnitude.mean[i]
        if angle:
            self.angle[:, i] = p.angle.mean[i]
        self._readings_dirty = self._readings_dirty or magnitude or angle
        se, rows = self.method, np.repeat(self._status, 2)
        se.inservice = int(rows.sum())
        se.mean[2 * i], se.mean[2 * i + 1] = st * p.magnitude.mean[i] * np.cos(p.angle.mean[i]), st * p.magnitude.mean[i] * np.sin(p.angle.mean[i])
        se.coefficient.nzval[:] = (self._val * rows[self._row])[self._order]


def pmuLavStateEstimation(monitoring: Measurement, batch: int = 1, iteration: int = 50, tolerance: float = 1e-8, weighted: bool = False,
                          device: int = 0) -> PmuLavStateEstimation:
    """pmuLavStateEstimation(monitoring, optimizer) without an optimizer: the LAV model of the PMU-only framework for `batch` realisations, its gain
    pattern analysed once on the device.  iteration, tolerance: the limits of solve_; weighted: rows scaled by 1 / sigma of the stored readings, one
    scale for every lane (the reference's model is unweighted)."""
    if monitoring.pmu.number == 0:
        raise ValueError("the measurement set holds no PMU")
    if int(iteration) < 0 or not float(tolerance) > 0.0:
        raise ValueError("pmuLavStateEstimation: iteration must not be negative, tolerance positive")
    return PmuLavStateEstimation(monitoring, batch, iteration, tolerance, weighted, device)


def _sync(an: PmuLavStateEstimation):
    L = _lib.lib()
    if an._status_dirty:
        _lib.check(L.jg_pmulav_set_status(an._h, np.ascontiguousarray(an._status, dtype=np.int32)))
        an._status_dirty = False
    if an._readings_dirty:
        _lib.check(L.jg_pmulav_set_readings(an._h, 0, an.batch, np.ascontiguousarray(an.magnitude).reshape(-1), np.ascontiguousarray(an.angle).reshape(-1)))
        an._readings_dirty = False


def solve_(an: PmuLavStateEstimation):
    """solve!(analysis) for every lane; analysis.status as in the module's head.  Every call starts anew from the start rule (or from setInitialPoint_,
    once): interior-point iterations are not warm-started, so a second solve_ after setReadings_ equals a fresh analysis."""
    _sync(an)
    L = _lib.lib()
    _lib.check(L.jg_pmulav_solve(an._h, an.iteration, an.tolerance))
    n, m, T = an.system.bus.number, 2 * an.monitoring.pmu.number, an.batch
    vm, va, st, obj, it = np.zeros((T, n)), np.zeros((T, n)), np.zeros(T, dtype=np.int32), np.zeros(T), np.zeros(T, dtype=np.int32)
    _lib.check(L.jg_pmulav_get_voltage(an._h, vm.ctypes.data_as(_lib.VP), va.ctypes.data_as(_lib.VP), st.ctypes.data_as(_lib.VP), obj.ctypes.data_as(_lib.VP),
                                       it.ctypes.data_as(_lib.VP)))
    r, y, gap = np.zeros((T, m)), np.zeros((T, m)), np.zeros(T)
    _lib.check(L.jg_pmulav_get_residual(an._h, r.reshape(-1)))
    _lib.check(L.jg_pmulav_get_dual(an._h, y.ctypes.data_as(_lib.VP), gap.ctypes.data_as(_lib.VP)))
    an.voltage.magnitude, an.voltage.angle = an._shape(vm), an._shape(va)
    an.residual, an.dual = an._shape(r), an._shape(y)
    if T == 1:
        an.status, an.objective, an.iterations, an.gap = int(st[0]), float(obj[0]), int(it[0]), float(gap[0])
    else:
        an.status, an.objective, an.iterations, an.gap = st, obj, it, gap


def stateEstimation_(an: PmuLavStateEstimation, power: bool = False, current: bool = False):
    """stateEstimation!(analysis; power, current)."""
    solve_(an)
    if power:
        power_(an)
    if current:
        current_(an)


def setReadings_(an: PmuLavStateEstimation, magnitude, angle, scenario0: int = 0):
    """the phasors of lanes scenario0 .. as the PMUs deliver them: magnitude, angle [count, pmus] in device order"""
    mag, ang = np.atleast_2d(np.asarray(magnitude, dtype=np.float64)), np.atleast_2d(np.asarray(angle, dtype=np.float64))
    if mag.shape != ang.shape or mag.shape[1] != an.monitoring.pmu.number or scenario0 < 0 or scenario0 + mag.shape[0] > an.batch:
        raise ValueError("setReadings_: magnitude and angle must be [count, pmus] with scenario0 + count <= batch")
    an.magnitude[scenario0:scenario0 + mag.shape[0]], an.angle[scenario0:scenario0 + mag.shape[0]] = mag, ang
    an._readings_dirty = True


def setInitialPoint_(an: PmuLavStateEstimation, other=None):
    """setInitialPoint!(analysis[, source]): the NEXT solve_ starts from these voltages instead of the unit-weight least-squares estimate -- the bus
    voltages of the power system (None), magnitude and angle of an AC analysis, or the angles of a DC analysis with the analysis' own magnitudes kept
    (one lane is given to every lane)."""
    n, T = an.system.bus.number, an.batch
    bus = an.system.bus.voltage
    if other is None:
        vm, va = bus.magnitude, bus.angle
    elif getattr(other.voltage, "magnitude", None) is not None:
        vm, va = other.voltage.magnitude, other.voltage.angle
    else:
        vm, va = an.voltage.magnitude, other.voltage.angle
    vm, va = np.atleast_2d(np.asarray(vm, dtype=np.float64)), np.atleast_2d(np.asarray(va, dtype=np.float64))
    if vm.shape[1] != n or va.shape[1] != n or vm.shape[0] not in (1, T) or va.shape[0] not in (1, T):
        raise ValueError("setInitialPoint_: the source holds voltages of another grid or another batch")
    vm, va = np.ascontiguousarray(np.broadcast_to(vm, (T, n))), np.ascontiguousarray(np.broadcast_to(va, (T, n)))
    _lib.check(_lib.lib().jg_pmulav_set_initial(an._h, vm.reshape(-1), va.reshape(-1)))
    an.voltage.magnitude, an.voltage.angle = an._shape(vm.copy()), an._shape(va.copy())


def updatePmu_(an: PmuLavStateEstimation, label, magnitude=None, angle=None, status=None, statusMagnitude=None, statusAngle=None):
    """updatePmu!(analysis; label, magnitude, angle, status, statusMagnitude, statusAngle): the container and the analysis' two rows follow.  A status
    change re-runs the start of the next solve_ and nothing symbolic, and leaves the lanes' readings alone; a new `magnitude` or `angle` becomes that
    reading of EVERY lane."""
    _se.updatePmu_(an.monitoring, label, magnitude=magnitude, angle=angle, status=status, statusMagnitude=statusMagnitude, statusAngle=statusAngle)
    an._refresh(int(label) - 1, magnitude is not None, angle is not None)


def _flows(an: PmuLavStateEstimation, *want):
    """[batch, rows, 2] host buffers for the wanted slots of jg_pmulav_get_flows (from, to, series current; from, to, series, charging, injected power)"""
    sysm = an.system
    L = _lib.lib()
    if not an._branches_on_device:
        lay, sh = sysm.branch.layout, sysm.bus.shunt
        _lib.check(L.jg_pmulav_set_branches(an._h, sysm.branch.number, np.ascontiguousarray(lay.from_, dtype=np.int64), np.ascontiguousarray(lay.to, dtype=np.int64),
                                            np.ascontiguousarray(lay.status, dtype=np.int8).ctypes.data_as(_lib.VP), np.ascontiguousarray(_branch_table(sysm).reshape(-1)),
                                            np.ascontiguousarray(sh.conductance, dtype=np.float64), np.ascontiguousarray(sh.susceptance, dtype=np.float64)))
        an._branches_on_device = True
    bufs = [np.zeros((an.batch, sysm.bus.number if k == 7 else sysm.branch.number, 2)) if w else None for k, w in enumerate(want)]
    _lib.check(L.jg_pmulav_get_flows(an._h, *[b.ctypes.data_as(_lib.VP) if b is not None else None for b in bufs]))
    return bufs


def power_(an: PmuLavStateEstimation):
    """power!(analysis) of a state estimation (acAnalysis.jl:221-262) for every lane: branch powers and the bus injections (a bus's branch ends plus its
    shunt) on the device from the rectangular estimate; on the host the shunt power |V|^2 conj(g + jb) and supply = injection + demand at EVERY bus.
    The reference forms no generator powers for an estimate, and neither does this."""
    bus = an.system.bus
    _, _, _, fr, to, se, ch, inj = _flows(an, False, False, False, True, True, True, True, True)
    vm = np.atleast_2d(an.voltage.magnitude)
    v2 = vm * vm
    shunt = np.stack([v2 * bus.shunt.conductance[None, :], -v2 * bus.shunt.susceptance[None, :]], axis=2)
    pw = an.power
    pw.injection, pw.shunt = _ns2(an, inj), _ns2(an, shunt)
    pw.supply = NS(active=an._shape(inj[:, :, 0] + bus.demand.active[None, :]), reactive=an._shape(inj[:, :, 1] + bus.demand.reactive[None, :]))
    pw.from_, pw.to, pw.series, pw.charging = _ns2(an, fr), _ns2(an, to), _ns2(an, se), _ns2(an, ch)


def current_(an: PmuLavStateEstimation):
    """current!(analysis) for every lane: from, to and series currents (magnitude, angle) on the device; the injected current conj(S_i / V_i) on the host."""
    fi, ti, si, _, _, _, _, inj = _flows(an, True, True, True, False, False, False, False, True)
    vm, va = np.atleast_2d(an.voltage.magnitude), np.atleast_2d(an.voltage.angle)
    with np.errstate(divide="ignore", invalid="ignore"):
        I = np.conj((inj[:, :, 0] + 1j * inj[:, :, 1]) / (vm * np.exp(1j * va)))
    cur, names = an.current, ("magnitude", "angle")
    cur.injection = NS(magnitude=an._shape(np.abs(I)), angle=an._shape(np.angle(I)))
    cur.from_, cur.to, cur.series = _ns2(an, fi, names), _ns2(an, ti, names), _ns2(an, si, names)


def suspect_(an: PmuLavStateEstimation, threshold: float):
    """the devices whose phasor residual rho_i = |r_re + j r_im| exceeds `threshold` (absolute, per unit; rho = 0 for a PMU outside the model):
    analysis.rho [batch, pmus], analysis.suspect (per lane the 0-based device indices, ascending), analysis.suspectCount, analysis.worst (the device of
    the largest rho, the lowest on ties)."""
    T, P = an.batch, an.monitoring.pmu.number
    rho, flag, cnt, worst = np.zeros((T, P)), np.zeros((T, P), dtype=np.int32), np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    _lib.check(_lib.lib().jg_pmulav_suspect(an._h, float(threshold), rho.ctypes.data_as(_lib.VP), flag.ctypes.data_as(_lib.VP), cnt.ctypes.data_as(_lib.VP),
                                            worst.ctypes.data_as(_lib.VP)))
    lists = [np.flatnonzero(flag[s]) for s in range(T)]
    an.rho = an._shape(rho)
    if T == 1:
        an.suspect, an.suspectCount, an.worst = lists[0], int(cnt[0]), int(worst[0])
    else:
        an.suspect, an.suspectCount, an.worst = lists, cnt, worst
