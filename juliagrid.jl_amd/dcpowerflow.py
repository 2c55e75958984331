"""DC power flow and the batched DC N-1 screen (the reference's dcPowerFlow / solve! / power!(::DcPowerFlow)).

  dcPowerFlow(system)          src/powerFlow/dcPowerFlow.jl:42-61
  solve!(analysis)             src/powerFlow/dcPowerFlow.jl:63-101
  power!(analysis)             src/postprocessing/dcAnalysis.jl:27-75 and its branch part (:41-48 of allPowerBranch)
  updateBranch!(analysis; label, status = 0) -> solve!   per scenario: setOutages_ (one shared factor, a rank-1 correction per lane: csrc/jg_dc.hpp)

All numerics run in libjgrid_hip.so (csrc/jg_dc.hip); the O(n) bus / generator bookkeeping of power! runs here.  A batched analysis keeps
`batch` scenarios of ONE grid on the device; arrays are [batch, ...] (1-D for batch 1), as in the AC analysis.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from .system import PowerSystem, dcModel_


class DcPowerFlow:
    """DcPowerFlow (src/definition/analysis.jl): voltage.angle, power.{injection, supply, generator, from_, to}, method."""

    def __init__(self, system: PowerSystem, batch: int, device: int):
        if system.model.dc.nodalMatrix is None:
            dcModel_(system)                                           # dcPowerFlow.jl:44-46
        self.system, self.batch, self.device = system, int(batch), int(device)
        dc, bus, br = system.model.dc, system.bus, system.branch
        B = dc.nodalMatrix
        h = C.c_int64(0)
        _lib.check(_lib.lib().jg_dc_create(C.byref(h), bus.number, B.colptr, B.rowval, np.ascontiguousarray(B.nzval, dtype=np.float64),
                                           int(bus.layout.slack), float(bus.voltage.angle[bus.layout.slack - 1]), self.batch, self.device))
        self._h = h.value
        _lib.check(_lib.lib().jg_dc_set_branches(self._h, br.number, np.ascontiguousarray(br.layout.from_, dtype=np.int64),
                                                 np.ascontiguousarray(br.layout.to, dtype=np.int64), np.ascontiguousarray(dc.admittance),
                                                 np.ascontiguousarray(br.parameter.shiftAngle, dtype=np.float64)))
        self.voltage = NS(angle=self._shape(np.tile(bus.voltage.angle, (self.batch, 1))))
        self.power = NS(injection=NS(active=None), supply=NS(active=None), generator=NS(active=None), from_=NS(active=None), to=NS(active=None))
        self.method = NS(dcmodel=True)
        self.status = 0 if self.batch == 1 else np.zeros(self.batch, dtype=np.int32)
        self._outage_labels = np.zeros(self.batch, dtype=np.int64)
        self._injection = None                                          # [batch, n] net injections of the scenarios that have their own, NaN rows elsewhere
        self._rhs = None

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def close(self):
        if getattr(self, "_h", 0):
            _lib.lib().jg_dc_destroy(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        d = np.zeros(10, dtype=np.int64)
        _lib.check(_lib.lib().jg_dc_dims(self._h, d))
        return dict(zip(("n", "batch", "ld", "branches", "entries", "factorLevels", "forwardLevels", "backwardLevels", "sweepLaunches", "sweepTerms"), map(int, d)))

    def angle_device(self):
        """(device address of the angles [n][ld], ld, device address of the int32 status [ld])"""
        info = np.zeros(3, dtype=np.int64)
        _lib.check(_lib.lib().jg_dc_angle_device(self._h, info))
        return int(info[0]), int(info[1]), int(info[2])

    def pack_results_device(self, dst_ptr: int):
        """angle | status, [batch][n + 1] doubles, into device memory of the caller (the operand of Comm.allgather_device)"""
        _lib.check(_lib.lib().jg_dc_pack_results_device(self._h, _lib.VP(int(dst_ptr))))

    def screen_device(self, dst_ptr: int, rating=None):
        _set_rating(self, rating)
        _lib.check(_lib.lib().jg_dc_screen_device(self._h, _lib.VP(int(dst_ptr))))

    def time_kernel(self, kernel: int, reps: int = 20) -> np.ndarray:
        """milliseconds of `reps` runs (HIP events): 0 the whole chain of a batch, 1 the sweep pair, 2 the combine, 3 flows + summary"""
        ms = np.zeros(int(reps))
        _lib.check(_lib.lib().jg_dc_time_kernel(self._h, int(kernel), int(reps), ms))
        return ms


def dcPowerFlow(system: PowerSystem, batch: int = 1, device: int = 0) -> DcPowerFlow:
    """dcPowerFlow(system): builds the DC model if needed, factorises the nodal matrix (slack row / column removed) ONCE on the device."""
    return DcPowerFlow(system, batch, device)


def _base_rhs(system: PowerSystem) -> np.ndarray:
    bus = system.bus                                                    # dcPowerFlow.jl:82-88
    return bus.supply.active - bus.demand.active - bus.shunt.conductance - system.model.dc.shiftPower


def _set_rating(an: DcPowerFlow, rating):
    r = None if rating is None else np.ascontiguousarray(rating, dtype=np.float64)
    if r is not None and r.shape != (an.system.branch.number,):
        raise ValueError("rating: one value per branch")
    an._rating = r                                                      # (kept alive for the call)
    _lib.check(_lib.lib().jg_dc_set_rating(an._h, None if r is None else r.ctypes.data_as(_lib.VP)))


def solve_(an: DcPowerFlow):
    """solve!(analysis::DcPowerFlow) for every scenario; analysis.status: 0, or 3 where the outaged branch is a bridge (angles NaN)."""
    rhs = np.ascontiguousarray(_base_rhs(an.system), dtype=np.float64)
    if an._rhs is None or not np.array_equal(rhs, an._rhs):
        _lib.check(_lib.lib().jg_dc_set_rhs(an._h, rhs))
        an._rhs = rhs.copy()
        if an._injection is not None:
            _upload_injections(an)
    _lib.check(_lib.lib().jg_dc_solve(an._h))
    th = np.zeros((an.batch, an.system.bus.number))
    st = np.zeros(an.batch, dtype=np.int32)
    _lib.check(_lib.lib().jg_dc_get_angle(an._h, th.reshape(-1), st))
    an.voltage.angle = an._shape(th)
    an.status = int(st[0]) if an.batch == 1 else st


def powerFlow_(an: DcPowerFlow, power: bool = False):
    """powerFlow!(analysis::DcPowerFlow; power): solve!, then power! if asked."""
    solve_(an)
    if power:
        power_(an)


def setOutages_(an: DcPowerFlow, labels, scenario0: int = 0):
    """scenario scenario0 + s = base grid with branch labels[s] out of service (0 / None = base grid): the reference's
    updateBranch!(analysis; label, status = 0) per scenario, without touching the factor."""
    lab = np.array([int(x) if x else 0 for x in labels], dtype=np.int64)
    if lab.size and (lab.min() < 0 or lab.max() > an.system.branch.number):
        raise IndexError("setOutages_: branch label out of range")
    _lib.check(_lib.lib().jg_dc_set_outages(an._h, int(scenario0), int(lab.size), lab))
    an._outage_labels[scenario0:scenario0 + lab.size] = lab


def _upload_injections(an: DcPowerFlow):
    sys_ = an.system
    own = np.flatnonzero(~np.isnan(an._injection[:, 0]))
    if not own.size:
        return
    rhs = an._injection - sys_.bus.shunt.conductance[None, :] - sys_.model.dc.shiftPower[None, :]
    start = own[0]
    for a, b in zip(own, np.r_[own[1:], -1]):                           # runs of consecutive lanes: one upload each
        if b != a + 1:
            _lib.check(_lib.lib().jg_dc_set_injections(an._h, int(start), int(a - start + 1), np.ascontiguousarray(rhs[start:a + 1]).reshape(-1)))
            start = b


def setInjection_(an: DcPowerFlow, active, scenario0: int = 0):
    """Per-scenario net active injections (supply - demand per bus, [count, n]) for scenarios scenario0 .. : what a loop of updateBus!(analysis; active) /
    updateGenerator!(analysis; active) -> solve! over Monte-Carlo draws sets.  Shunts and phase shifters stay the system's."""
    p = np.atleast_2d(np.asarray(active, dtype=np.float64))
    if p.shape[1] != an.system.bus.number or scenario0 < 0 or scenario0 + p.shape[0] > an.batch:
        raise ValueError("setInjection_: active must be [count, buses] with scenario0 + count <= batch")
    if an._injection is None:
        an._injection = np.full((an.batch, an.system.bus.number), np.nan)
    an._injection[scenario0:scenario0 + p.shape[0]] = p
    if an._rhs is None:
        an._rhs = np.ascontiguousarray(_base_rhs(an.system), dtype=np.float64)
        _lib.check(_lib.lib().jg_dc_set_rhs(an._h, an._rhs))
    _upload_injections(an)


def power_(an: DcPowerFlow):
    """power!(analysis::DcPowerFlow) (src/postprocessing/dcAnalysis.jl:27-75) for every scenario: branch flows on the device
    (from = y (theta_from - theta_to - shiftAngle), to = -from, 0 on a lane's outaged branch); the slack injection, supply and generator
    outputs on the host.  The slack injection sum_j B[slack, j] theta_j + shunt + shiftPower equals the flows that leave the slack bus plus its
    shunt, which is how a lane with an outage gets it without a matrix of its own."""
    sys_, bus, gen, br = an.system, an.system.bus, an.system.generator, an.system.branch
    fr = np.zeros((an.batch, br.number))
    _lib.check(_lib.lib().jg_dc_get_flows(an._h, fr.reshape(-1)))
    slack = bus.layout.slack - 1
    inj = np.tile(bus.supply.active - bus.demand.active, (an.batch, 1))
    if an._injection is not None:
        own = ~np.isnan(an._injection[:, 0])
        inj[own] = an._injection[own]
    out_f = br.layout.from_ - 1 == slack
    out_t = br.layout.to - 1 == slack
    inj[:, slack] = fr[:, out_f].sum(axis=1) - fr[:, out_t].sum(axis=1) + bus.shunt.conductance[slack]
    sup = np.tile(bus.supply.active, (an.batch, 1))
    sup[:, slack] = bus.demand.active[slack] + inj[:, slack]
    gp = np.zeros((an.batch, gen.number))
    on = gen.layout.status == 1
    gp[:, on] = gen.output.active[on]
    lst = bus.supply.generator.get(slack + 1, [])
    if lst and gen.layout.status[lst[0] - 1] == 1:                      # dcAnalysis.jl:59-72
        gp[:, lst[0] - 1] = inj[:, slack] + bus.demand.active[slack] - sum(gen.output.active[j - 1] for j in lst[1:])
    pw = an.power
    pw.injection, pw.supply, pw.generator = NS(active=an._shape(inj)), NS(active=an._shape(sup)), NS(active=an._shape(gp))
    pw.from_, pw.to = NS(active=an._shape(fr)), NS(active=an._shape(-fr))


def screenSummary_(an: DcPowerFlow, rating=None) -> np.ndarray:
    """[batch, 5] per scenario: worst |from| / rating and its branch (1-based, 0: none rated), largest |from| and its branch, status; ties go to the
    lowest branch.  What the user loop reads off power!(analysis) after every solve!, reduced where the angles are."""
    _set_rating(an, rating)
    rec = np.zeros((an.batch, 5))
    _lib.check(_lib.lib().jg_dc_screen(an._h, rec.reshape(-1)))
    return rec


def dcContingencyAnalysis(system: PowerSystem, labels, device: int = 0, rating=None) -> DcPowerFlow:
    """Solved batched DC analysis, scenario s = outage of branch labels[s] (0 / None: base case): analysis.voltage.angle [batch, n],
    analysis.status [batch] (3: bridge), and analysis.screen [batch, 5] (screenSummary_) when `rating` is given."""
    labels = list(labels)
    an = dcPowerFlow(system, batch=len(labels), device=device)
    setOutages_(an, labels)
    solve_(an)
    an.screen = screenSummary_(an, rating) if rating is not None else None
    return an
