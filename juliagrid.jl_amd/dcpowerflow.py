"""DC power flow and the batched DC N-1 screen (the reference's dcPowerFlow / solve! / power!(::DcPowerFlow)).

  dcPowerFlow(system)          src/powerFlow/dcPowerFlow.jl:42-61
  solve!(analysis)             src/powerFlow/dcPowerFlow.jl:63-101
  power!(analysis)             src/postprocessing/dcAnalysis.jl:27-75 and its branch part (:41-48 of allPowerBranch)
  updateBranch!(analysis; label, status = 0) -> solve!   per scenario: setOutages_ (one shared factor, a rank-1 correction per lane: csrc/jg_dc.hpp;
                                                         a tuple (k, l) is a lane with two outages: a 2 x 2 correction; islands="shed": a bridge
                                                         outage is solved on the slack's island, which the reference cannot do)
  the same loop over ALL pairs of a candidate list          dcPairScreen (the DC N-2 screen: csrc/jg_dc_pair.hpp)
  the N-1 loop inside a loop over injection profiles        dcSeriesScreen (csrc/jg_dc_series.hpp)
  the N-1 loop while the injections move along a direction  dcTransferScreen (the transfer capability: csrc/jg_dc_transfer.hpp)
  updateGenerator!(g, status = 0) alone and around the N-1 loop   dcGeneratorScreen (dcgenerator.py; csrc/jg_dc_generator.hpp)

All numerics run in libjgrid_hip.so (csrc/jg_dc.hip); the O(n) bus / generator bookkeeping of power! runs here.  A batched analysis keeps
`batch` scenarios of ONE grid on the device; arrays are [batch, ...] (1-D for batch 1), as in the AC analysis.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
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
        if br.number:                                                   # a grid without a branch (the slack alone) has no branch table: jg_dc_set_branches refuses nbr = 0
            _lib.check(_lib.lib().jg_dc_set_branches(self._h, br.number, np.ascontiguousarray(br.layout.from_, dtype=np.int64),
                                                     np.ascontiguousarray(br.layout.to, dtype=np.int64), np.ascontiguousarray(dc.admittance),
                                                     np.ascontiguousarray(br.parameter.shiftAngle, dtype=np.float64)))
        self.voltage = NS(angle=self._shape(np.tile(bus.voltage.angle, (self.batch, 1))))
        self.power = NS(injection=NS(active=None), supply=NS(active=None), generator=NS(active=None), from_=NS(active=None), to=NS(active=None))
        self.method = NS(dcmodel=True)
        self.status = 0 if self.batch == 1 else np.zeros(self.batch, dtype=np.int32)
        self._outage_labels = np.zeros(self.batch, dtype=np.int64)
        self._outage_labels2 = np.zeros(self.batch, dtype=np.int64)
        self._injection = None                                          # [batch, n] net injections of the scenarios that have their own, NaN rows elsewhere
        self._rhs = None
        self._island_mode = 0                                           # what jg_dc_set_island_mode was last told
        self._island_table = None                                       # contingency.islandTable(system), once, when islands="shed" is first asked for
        self.island = None

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
    """solve!(analysis::DcPowerFlow) for every scenario; analysis.status: 0, or 3 where the outaged branch is a bridge (angles NaN); 4 on a bridge lane
    set with islands="shed" (solved on the slack's island, NaN on the buses that leave; analysis.island holds what was shed)."""
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
    an.island = _island_record(an) if an._island_table is not None else None


ISLAND_MODES = {"skip": 0, "shed": 1}


def _island_mode(islands) -> int:
    if islands not in ISLAND_MODES:
        raise ValueError("islands is 'skip' (a bridge outage gets status 3) or 'shed' (it is solved on the slack's island: status 4)")
    return ISLAND_MODES[islands]


def _island_record(an: DcPowerFlow):
    """analysis.island of a solved batch, [batch] each: buses shed (0: the lane shed nothing), injection = the lane's right-hand side summed over them
    (supply - demand - shunt conductance - shiftPower, of the lane's own injections where it has them), m = the bridge's end on the slack's side
    (1-based), flow = what left m over the bridge before the outage -- all from the device -- and demand / supply shed, prefix sums over the preorder
    of the system's own values (NaN on a shedding lane with injections of its own, which carry no such split)."""
    rec = np.zeros((an.batch, 4))
    _lib.check(_lib.lib().jg_dc_get_islands(an._h, rec.reshape(-1)))
    tb, bus = an._island_table, an.system.bus
    lab = an._outage_labels - 1
    isl = rec[:, 2] > 0
    lo = np.where(isl, tb.lo[lab], 0)
    hi = np.where(isl, tb.hi[lab], -1)
    own = np.zeros(an.batch, dtype=bool) if an._injection is None else ~np.isnan(an._injection[:, 0])
    out = {}
    for name, v in (("demand", bus.demand.active), ("supply", bus.supply.active)):
        cs = np.r_[0.0, np.cumsum(v[tb.order], dtype=np.longdouble)]   # (extended precision where the platform has it: the difference of two long sums)
        out[name] = np.where(isl & own, np.nan, (cs[hi + 1] - cs[lo]).astype(np.float64))
    return NS(buses=an._shape(rec[:, 0].astype(np.int64)), injection=an._shape(rec[:, 1].copy()), m=an._shape(rec[:, 2].astype(np.int64)),
              flow=an._shape(rec[:, 3].copy()), demand=an._shape(out["demand"]), supply=an._shape(out["supply"]))


def _shed_mask(an: DcPowerFlow):
    """[batch, n] True on the buses a lane shed, or None when no lane shed any"""
    if an.island is None or not np.any(np.atleast_1d(an.island.buses)):
        return None
    tb = an._island_table
    lab = an._outage_labels - 1
    isl = np.atleast_1d(an.island.buses) > 0
    lo = np.where(isl, tb.lo[lab], 1)
    hi = np.where(isl, tb.hi[lab], 0)
    pre = tb.preorder[None, :]
    return (pre >= lo[:, None]) & (pre <= hi[:, None])


def powerFlow_(an: DcPowerFlow, power: bool = False):
    """powerFlow!(analysis::DcPowerFlow; power): solve!, then power! if asked."""
    solve_(an)
    if power:
        power_(an)


def outagePairs(labels, branches: int):
    """labels of a scenario list as two int64 arrays (first, second outage; 0 = none): an entry is None / 0, a branch label, or a tuple (k, l) of two
    different labels ((k, 0): k alone).  Checked on the host: IndexError for a label outside 1 .. branches, ValueError for k == l or a tuple of another length."""
    a = np.zeros(len(labels), dtype=np.int64)
    b = np.zeros(len(labels), dtype=np.int64)
    for s, x in enumerate(labels):
        if isinstance(x, (tuple, list)):
            if len(x) != 2:
                raise ValueError("an outage pair is a tuple (k, l) of two branch labels")
            a[s], b[s] = (int(x[0]) if x[0] else 0), (int(x[1]) if x[1] else 0)
            if a[s] and a[s] == b[s]:
                raise ValueError(f"outage pair ({a[s]}, {b[s]}): the two branches must differ")
        else:
            a[s] = int(x) if x else 0
    if a.size and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) > branches):
        raise IndexError("branch label out of range")
    return a, b


def setOutages_(an: DcPowerFlow, labels, scenario0: int = 0, islands: str = "skip"):
    """scenario scenario0 + s = base grid with branch labels[s] out of service (0 / None = base grid; a tuple (k, l): BOTH branches): the reference's
    updateBranch!(analysis; label, status = 0) per scenario, without touching the factor.  islands="shed": a lane of THIS call whose one outage is a
    bridge is solved on the side of the bridge that holds the slack (status 4, NaN angles on the buses that leave, analysis.island after solve_) instead
    of being skipped with status 3; lanes with two outages keep status 3 for whatever islands."""
    mode = _island_mode(islands)                                        # refused on the host, before the device is touched
    lab, lab2 = outagePairs(list(labels), an.system.branch.number)
    if mode != an._island_mode:
        if mode and an._island_table is None:
            from .contingency import islandTable
            an._island_table = islandTable(an.system)
        _lib.check(_lib.lib().jg_dc_set_island_mode(an._h, mode))
        an._island_mode = mode
    if lab2.any():
        _lib.check(_lib.lib().jg_dc_set_outage_pairs(an._h, int(scenario0), int(lab.size), lab, lab2))
    else:
        _lib.check(_lib.lib().jg_dc_set_outages(an._h, int(scenario0), int(lab.size), lab))
    an._outage_labels[scenario0:scenario0 + lab.size] = lab
    an._outage_labels2[scenario0:scenario0 + lab.size] = lab2


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
    if br.number:                                                       # no branch: no flow kernel to launch (its grid would be empty), the flows are empty
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
    shed = _shed_mask(an)
    if shed is not None:                                                # what a lane shed is not solved for: NaN on its buses and on their generators
        inj[shed] = np.nan
        sup[shed] = np.nan
        gp[shed[:, gen.layout.bus - 1] & on[None, :]] = np.nan
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


def dcContingencyAnalysis(system: PowerSystem, labels, device: int = 0, rating=None, islands: str = "skip") -> DcPowerFlow:
    """Solved batched DC analysis, scenario s = outage of branch labels[s] (0 / None: base case; a tuple (k, l): both branches): analysis.voltage.angle [batch, n],
    analysis.status [batch] (3: bridge), and analysis.screen [batch, 5] (screenSummary_) when `rating` is given.  islands="shed": setOutages_."""
    labels = list(labels)
    outagePairs(labels, system.branch.number)                           # refused on the host, before the device is touched
    _island_mode(islands)
    an = dcPowerFlow(system, batch=len(labels), device=device)
    setOutages_(an, labels, islands=islands)
    solve_(an)
    an.screen = screenSummary_(an, rating) if rating is not None else None
    return an


class DcPairScreen:
    """What dcPairScreen returns.
      candidates  [K] branch labels (1-based, ascending); monitored rows are those of the call
      records     [m, 5] the pairs whose worst loading exceeds the threshold, sorted by (k, l): label k, label l, worst branch, worst |from| / rating,
                  number of monitored branches above the threshold
      islanding   [i, 2] int64 labels of the pairs that island a part of the grid (status 3); with islands="shed" only the pairs that STAY status 3: the
                  joint cuts of two non-bridges, and the pairs with a non-bridge whose |1 - Phi[l,l]| vanishes
      totals      dict(pairs, violating, islanding): exact also when a list overflowed
      overflow / islandingOverflow   a list was cut at its capacity: it holds the FIRST entries by (k, l)
      worst       [K] the worst loading over all screened pairs of each candidate (ranking)
      loading, branch, count, determinant   with dense=True: [K, K], the upper triangle mirrored (NaN loading on islanding pairs, diagonal 0); with
                  rows=(k0, k1): the block [k1 - k0, K] as screened, 0 where l <= k
      shed, shedBuses, shedM, shedFlow   with islands="shed" (else None), one entry per bridge among ALL the candidates (whatever `rows`): their labels
                  ascending, the number of buses that leave [S] int64, the bridge's end on the slack's side [S] (1-based bus) and the flow that left
                  that end over the bridge in the base case [S] (from the device).  A pair that holds a bridge is then screened on the slack's island:
                  finite loading, in the records, the counts and `worst` like any other
      recordShed  with islands="shed" (else None): [m, 2] int64, per record what pairShed gives for its pair
      info        dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def pairShed(system: PowerSystem, pairs, table=None) -> np.ndarray:
    """[m, 2] int64 for the pairs (k, l) of branch labels `pairs` [m, 2]: the labels of the bridges whose island leaves when both go out of service with
    islands="shed" -- column 0 holds k and column 1 holds l where that branch is a bridge, 0 where it is none; of two NESTED bridges only the outer one
    is named (what leaves behind the inner one is part of what leaves behind the outer).  Host only, from islandTable(system) (or `table`)."""
    from .contingency import islandTable
    tb = islandTable(system) if table is None else table
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(p.shape, dtype=np.int64)
    if not p.shape[0]:
        return out
    k, l = p[:, 0] - 1, p[:, 1] - 1
    bk, bl = tb.side[k] != 0, tb.side[l] != 0
    k_in_l = bk & bl & (tb.lo[l] <= tb.lo[k]) & (tb.hi[k] <= tb.hi[l])
    l_in_k = bk & bl & (tb.lo[k] <= tb.lo[l]) & (tb.hi[l] <= tb.hi[k])
    out[:, 0] = np.where(bk & ~k_in_l, p[:, 0], 0)
    out[:, 1] = np.where(bl & ~l_in_k, p[:, 1], 0)
    return out


def pairCandidates(system: PowerSystem) -> np.ndarray:
    """default candidates of the N-2 screen: labels of the in-service branches that are not bridges (and not self-loops), ascending"""
    from .contingency import bridges
    lay = system.branch.layout
    return (np.flatnonzero((lay.status == 1) & ~bridges(system) & (lay.from_ != lay.to)) + 1).astype(np.int64)


def shedCandidates(system: PowerSystem) -> np.ndarray:
    """default candidates of a screen with islands="shed": labels of the in-service branches that are not self-loops, bridges included, ascending"""
    lay = system.branch.layout
    return (np.flatnonzero((lay.status == 1) & (lay.from_ != lay.to)) + 1).astype(np.int64)


def _pair_lists(system: PowerSystem, candidates, monitored, rating, who: str = "dcPairScreen", least: int = 2, shed: bool = False):
    """candidate and monitored labels of a pair screen, checked on the host before anything touches the device"""
    nb, status = system.branch.number, system.branch.layout.status
    rating = np.ascontiguousarray(rating, dtype=np.float64)
    if rating.shape != (nb,):
        raise ValueError("rating: one value per branch")
    cand = (shedCandidates(system) if shed else pairCandidates(system)) if candidates is None else np.asarray(list(candidates), dtype=np.int64)
    if cand.size and (cand.min() < 1 or cand.max() > nb):
        raise IndexError(f"{who}: candidate branch label out of range")
    if np.unique(cand).size != cand.size:
        raise ValueError(f"{who}: a candidate is named twice" + (" (a pair needs two different branches)" if least == 2 else ""))
    if cand.size < least:
        raise ValueError(f"{who}: two or more candidates are needed" if least == 2 else f"{who}: one or more candidates are needed")
    off = cand[status[cand - 1] != 1]
    if off.size:
        raise ValueError(f"{who}: candidate branch {int(off[0])} is out of service")
    if monitored is None:
        mon = (np.flatnonzero((status == 1) & (rating > 0)) + 1).astype(np.int64)
    else:
        mon = np.unique(np.asarray(list(monitored), dtype=np.int64))
        if mon.size and (mon.min() < 1 or mon.max() > nb):
            raise IndexError(f"{who}: monitored branch label out of range")
    return np.sort(cand), mon, rating

SCREEN_INFO = ("rows", "ld", "phiBytes", "freeBytes", "budgetBytes", "buildMs", "sweepMs", "phiMs")     # info [0 .. 7] of every screen's build: the kept sensitivities


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_lib.VP)


def _screen_rows(who: str, last: int, rows, block, block_bytes: int, row_bytes: int):
    """(k0, k1, step) of a screen call: the candidate positions [k0, k1) it covers (`rows`, cut at `last`; default all of them) and the rows of one
    device call (`block`; default: `block_bytes` of dense result at `row_bytes` a row)"""
    k0, k1 = (0, last) if rows is None else (int(rows[0]), min(int(rows[1]), last))
    if k0 < 0 or k1 < k0:
        raise ValueError(f"{who}: rows = (k0, k1) with 0 <= k0 <= k1 <= candidates")
    step = max(1, block_bytes // row_bytes) if block is None else int(block)
    if step < 1:
        raise ValueError(f"{who}: block >= 1")
    return k0, k1, step


@contextmanager
def _screen_analysis(analysis_or_system, which: str, rating, device: int):
    """(analysis, library) of a screen call, the base right-hand side and the rating set: the caller's analysis, whose screen state (jg_dc_<which>_*) is
    released afterwards, or for a PowerSystem one of the call's own, closed afterwards"""
    own = isinstance(analysis_or_system, PowerSystem)
    an = dcPowerFlow(analysis_or_system, device=device) if own else analysis_or_system
    L = _lib.lib()
    try:
        if an._rhs is None:
            an._rhs = np.ascontiguousarray(_base_rhs(an.system), dtype=np.float64)
            _lib.check(L.jg_dc_set_rhs(an._h, an._rhs))
        _set_rating(an, rating)
        yield an, L
    finally:
        if own:
            an.close()
        else:
            _lib.check(getattr(L, f"jg_dc_{which}_release")(an._h))


def _screen_blocks(k0: int, k1: int, step: int, rec: np.ndarray, full: dict, screen):
    """The device calls of a screen, `step` rows at a time: screen(b0, b1, capacity, records, part) screens the rows [b0, b1) into what is left of the
    record buffer `rec` and the row slices `part` of the dense arrays `full`, and returns the call's totals ([:3] add up, [3] = records written).
    Returns (totals [3], records written)."""
    tot, nrec = np.zeros(3, dtype=np.int64), 0
    for b0 in range(k0, k1, step):
        b1 = min(b0 + step, k1)
        part = {name: a[b0 - k0:b1 - k0] for name, a in full.items()}                         # (row slices of a C-contiguous array are contiguous)
        r = rec[nrec:]
        t = screen(b0, b1, r.shape[0], _ptr(r) if r.shape[0] else None, part)
        tot += t[:3]
        nrec += int(t[3])
    return tot, nrec


def _shed_block(L, an, which: str, b0: int, b1: int, *shapes):
    """(labels, buses, m, ...) of the bridge candidates among the positions [b0, b1) of a screen built in shed mode, then what jg_dc_<which>_get_shed
    gives for them: one array of shape (bridges,) + s per s of `shapes`"""
    n = np.zeros(1, dtype=np.int64)
    lab, buses, m, side = (np.zeros(b1 - b0, dtype=np.int64) for _ in range(4))
    _lib.check(getattr(L, f"jg_dc_{which}_get_shed_table")(an._h, b0, b1, n, lab, buses, m, side))
    c = int(n[0])
    flows = [np.zeros((c,) + s) for s in shapes]
    if c:
        _lib.check(getattr(L, f"jg_dc_{which}_get_shed")(an._h, b0, b1, *(f.reshape(-1) for f in flows)))
    return (lab[:c], buses[:c], m[:c], *flows)


def _concat(blocks, *empty):
    """the columns of the blocks' tuples concatenated; `empty`: what a column is when there was no block"""
    return [np.concatenate([x[j] for x in blocks]) if blocks else e for j, e in enumerate(empty)]


PAIR_BLOCK_BYTES = 256 << 20                                           # default bound of the dense result of one device call (16 bytes per pair)


def dcPairScreen(analysis_or_system, candidates=None, monitored=None, rating=None, threshold: float = 1.0, rows=None, capacity: int = 1 << 20,
                 dense: bool = False, islandCapacity: int = 1 << 16, block=None, budget=None, device: int = 0, islands: str = "skip") -> DcPairScreen:
    """The DC N-2 screen: every pair k < l of `candidates` (labels; default pairCandidates(system)) out of service together, the worst |from| / rating over
    `monitored` (default: every in-service branch with a rating > 0) per pair -- the loop updateBranch!(k), updateBranch!(l), solve!, power! over all
    pairs, from ONE factor and one sweep pair per candidate (csrc/jg_dc_pair.hpp).
      rows       (k0, k1): only the pairs whose FIRST branch is candidate position k0 .. k1 - 1 (what one rank of a sharded screen takes: shard())
      block      candidate rows per device call (bounds the memory of a call; default: 256 MiB of dense result); the result does not depend on it
      capacity / islandCapacity   most records / islanding pairs kept (the first by (k, l); the totals stay exact)
      budget     bytes the kept sensitivities may take (default: 0.8 of the free device memory); JGridError code 5 with the sizes when they do not fit
      islands    "skip": a pair that holds a bridge is singular (status 3: `islanding`, NaN loading).  "shed": a candidate the graph calls a bridge
                 is shed as setOutages_(..., islands="shed") sheds a lane's -- the buses behind it leave with their injections, the pair's other
                 branch (where it stays) is solved on what is left, the worst loading, its branch and the count cover the branches that stay --
                 and the pair is screened like any other (no 2 x 2 solve: csrc/jg_dc_pair.hpp has the table).  The default candidates are then
                 shedCandidates(system), the result names what was shed (DcPairScreen: shed .. shedFlow, recordShed), and `islanding` keeps the
                 joint cuts of two non-bridges and the pairs with a singular non-bridge.  A pair of two non-bridges is bitwise what it is without
                 the keyword.  With dense=True the determinant of a pair with a bridge is the denominator of the branch that is solved (1: none)"""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    mode = _island_mode(islands)                                        # refused on the host, before the device is touched
    if rating is None:
        raise ValueError("dcPairScreen: rating (per branch, per unit of active power) is needed")
    if not threshold >= 0:
        raise ValueError("dcPairScreen: threshold >= 0")
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    cand, mon, rating = _pair_lists(system, candidates, monitored, rating, shed=bool(mode))
    nk = int(cand.size)
    k0, k1, step = _screen_rows("dcPairScreen", nk - 1, rows, block, PAIR_BLOCK_BYTES, (nk + 63) // 64 * 64 * (24 if dense else 16))     # (the last candidate is the first branch of no pair)
    with _screen_analysis(analysis_or_system, "pair", rating, device) as (an, L):
        info = np.zeros(8)
        _lib.check(L.jg_dc_pair_set_island_mode(an._h, mode))
        _lib.check(L.jg_dc_pair_build(an._h, nk, cand, int(mon.size), _ptr(mon), int(budget or 0), info))
        rec = np.zeros((max(int(capacity), 0), 5))
        isl = np.zeros((max(int(islandCapacity), 0), 2), dtype=np.int64)
        worst = np.zeros(nk)
        nisl = 0
        full = {name: np.zeros((k1 - k0, nk), dtype=dt) for name, dt in (("loading", np.float64), ("branch", np.int32), ("count", np.int32), ("determinant", np.float64))} if dense else {}

        def screen(b0, b1, cap, r, part):
            nonlocal nisl
            t6, i = np.zeros(6, dtype=np.int64), isl[nisl:]
            _lib.check(L.jg_dc_pair_screen(an._h, b0, b1, float(threshold), cap, r, i.shape[0], _ptr(i) if i.shape[0] else None, t6, _ptr(worst),
                                           _ptr(part.get("loading")), _ptr(part.get("branch")), _ptr(part.get("count")), _ptr(part.get("determinant"))))
            nisl += int(t6[4])
            return t6
        tot, nrec = _screen_blocks(k0, k1, step, rec, full, screen)
        res = DcPairScreen(candidates=cand, monitored=mon, records=rec[:nrec].copy(), islanding=isl[:nisl].copy(), worst=worst, threshold=float(threshold),
                           totals=dict(pairs=int(tot[0]), violating=int(tot[1]), islanding=int(tot[2])), overflow=bool(tot[1] > nrec),
                           islandingOverflow=bool(tot[2] > nisl), rows=(k0, k1), info=dict(zip(SCREEN_INFO, (float(x) for x in info))))
        for name, a in full.items():
            if rows is None:                                            # the upper triangle, mirrored ([nk - 1, nk] rows came back: the last candidate has none)
                a = np.vstack([a, np.zeros((1, nk), dtype=a.dtype)])
                a = (a + a.T).astype(a.dtype)
            setattr(res, name, a)
        res.shed = res.shedBuses = res.shedM = res.shedFlow = res.recordShed = None
        if mode:
            res.shed, res.shedBuses, res.shedM, res.shedFlow = _shed_block(L, an, "pair", 0, nk, ())
            res.recordShed = pairShed(system, res.records[:, :2])
        return res


class DcSeriesScreen:
    """What dcSeriesScreen returns.
      candidates  [K] branch labels (1-based, ascending); monitored the labels of the call; profiles = T; threshold; rows = (k0, k1)
      records     [r, 5] the cases (k, t) whose worst loading exceeds the threshold, sorted by (k, t): label k, profile index t (0-based row of
                  `injections`), worst branch label, worst |from| / rating, number of monitored branches above the threshold
      overflow    the record list was cut at its capacity: it holds the FIRST entries by (k, t)
      islanding   labels of the screened candidates that are bridges (status 3): NaN loading in every profile, never in `records`
      totals      dict(cases = rows screened x T, violating, islanding = bridge candidates): exact also when the list overflowed
      worst       [K] the worst loading over all profiles of each screened candidate (0 on a bridge and outside `rows`)
      shed, shedBuses, shedM, shedFlow, shedDemand, unserved   with islands="shed" (else None): the screened bridge candidates, which are then solved on
                  the slack's island and are cases like any other (no longer in `islanding`, which keeps what is still status 3): their labels
                  ascending, the number of buses that leave [S] int64, the bridge's end on the slack's side [S] (1-based bus), the flow that left that
                  end over the bridge before the outage [S, T] (from the device; the right-hand side summed over what leaves is -shedFlow, the meaning
                  of analysis.island.flow / .injection -- on a phase-shifting bridge less the bridge's own shiftPower entry at its end that leaves), and with `demand`: the demand summed over what leaves [S, T] and its sum over the profiles [S]
      worstProfile / violatingProfile   [T] per profile over the screened candidates: the worst loading (bridges aside) and the number of candidates
                  whose outage violates (int64)
      base        [T, 3] the base case of every profile, no outage: worst loading, its branch label, number of branches above the threshold
      loading, branch, count   with dense=True: [k1 - k0, T]
      info        dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs, f0Bytes, f0BuildMs, f0SweepMs, f0KernelMs)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


SERIES_BLOCK_BYTES = 256 << 20                                         # default bound of the dense result of one device call (16 bytes per case)


def _shed_demand(system: PowerSystem, labels: np.ndarray, demand: np.ndarray) -> np.ndarray:
    """[len(labels), T] the demand summed over the buses that leave with each bridge: prefix sums over the preorder per profile, a chunk of profiles at
    a time (32 MiB of prefix sums, in extended precision where the platform has it: the difference of two long sums)"""
    from .contingency import islandTable
    tb = islandTable(system)
    lo, hi = tb.lo[labels - 1].astype(np.int64), tb.hi[labels - 1].astype(np.int64)
    T, n = demand.shape[0], tb.order.size
    out = np.zeros((labels.size, T))
    step = max(1, (32 << 20) // (np.dtype(np.longdouble).itemsize * (n + 1)))
    for t0 in range(0, T, step):
        cs = np.zeros((min(step, T - t0), n + 1), dtype=np.longdouble)
        np.cumsum(demand[t0:t0 + step][:, tb.order], axis=1, dtype=np.longdouble, out=cs[:, 1:])
        out[:, t0:t0 + step] = (cs[:, hi + 1] - cs[:, lo]).T.astype(np.float64)
    return out


def dcSeriesScreen(analysis_or_system, injections, candidates=None, monitored=None, rating=None, threshold: float = 1.0, rows=None,
                   capacity: int = 1 << 20, dense: bool = False, block=None, budget=None, device: int = 0, islands: str = "skip",
                   demand=None) -> DcSeriesScreen:
    """The DC N-1 screen at every one of a series of injection profiles: branch k of `candidates` (labels; default pairCandidates(system); one is
    allowed) out of service under profile t of `injections` ([T, buses] net active injection per bus, supply - demand, the meaning of setInjection_;
    shunts and phase shifters stay the system's), the worst |from| / rating over `monitored` per case -- the loop updateBus! / updateGenerator! per
    profile around updateBranch!(k, status = 0), solve!, power! per branch, from ONE factor, one sweep pair per candidate and one per profile
    (csrc/jg_dc_series.hpp).  `monitored`, `rating`, `rows`, `block`, `budget` and `capacity` mean what they mean for dcPairScreen; the budget covers
    the sensitivities and the profiles' base flows, and a caller with more profiles than fit splits them (a profile's results do not depend on the others).
      islands    "skip": a bridge candidate gets status 3 (`islanding`, NaN loadings).  "shed": it is screened on the slack's island as setOutages_(...,
                 islands="shed") solves a lane: the buses behind it leave with their injections, the worst loading, its branch and the count cover the
                 branches that stay, and the case enters the records and every summary like any other; the default candidates are then
                 shedCandidates(system), and the result names what was shed (DcSeriesScreen).  A non-bridge whose |1 - Phi[k,k]| vanishes keeps status 3
      demand     [T, buses] with islands="shed": the demand of every profile, for shedDemand / unserved (host prefix sums)"""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    mode = _island_mode(islands)                                        # refused on the host, before the device is touched
    if rating is None:
        raise ValueError("dcSeriesScreen: rating (per branch, per unit of active power) is needed")
    if not threshold >= 0:
        raise ValueError("dcSeriesScreen: threshold >= 0")
    inj = np.asarray(injections, dtype=np.float64)
    if inj.ndim != 2 or inj.shape[0] < 1 or inj.shape[1] != system.bus.number:
        raise ValueError("dcSeriesScreen: injections must be [T, buses] with T >= 1")
    if not np.isfinite(inj).all():
        raise ValueError("dcSeriesScreen: injections must be finite")
    if demand is not None:
        if not mode:
            raise ValueError("dcSeriesScreen: demand goes with islands='shed'")
        demand = np.asarray(demand, dtype=np.float64)
        if demand.shape != inj.shape or not np.isfinite(demand).all():
            raise ValueError("dcSeriesScreen: demand must be [T, buses] like injections, and finite")
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    cand, mon, rating = _pair_lists(system, candidates, monitored, rating, who="dcSeriesScreen", least=1, shed=bool(mode))
    nk, T = int(cand.size), int(inj.shape[0])
    k0, k1, step = _screen_rows("dcSeriesScreen", nk, rows, block, SERIES_BLOCK_BYTES, (T + 63) // 64 * 64 * 16)
    with _screen_analysis(analysis_or_system, "series", rating, device) as (an, L):
        rhs = np.ascontiguousarray(inj - system.bus.shunt.conductance[None, :] - system.model.dc.shiftPower[None, :])
        info = np.zeros(12)
        _lib.check(L.jg_dc_series_set_island_mode(an._h, mode))
        _lib.check(L.jg_dc_series_build(an._h, nk, cand, int(mon.size), _ptr(mon), T, rhs.reshape(-1), int(budget or 0), info))
        del rhs
        rec = np.zeros((max(int(capacity), 0), 5))
        worst, worstProfile, violatingProfile, base = np.zeros(nk), np.zeros(T), np.zeros(T, dtype=np.int64), np.zeros((T, 3))
        bridges, shed = [], []
        full = {name: np.zeros((k1 - k0, T), dtype=dt) for name, dt in (("loading", np.float64), ("branch", np.int32), ("count", np.int32))} if dense else {}

        def screen(b0, b1, cap, r, part):
            t5, isl = np.zeros(5, dtype=np.int64), np.zeros(b1 - b0, dtype=np.int64)
            _lib.check(L.jg_dc_series_screen(an._h, b0, b1, float(threshold), cap, r, _ptr(isl), t5, _ptr(worst), _ptr(worstProfile), _ptr(violatingProfile),
                                             _ptr(base) if b0 == k0 else None, _ptr(part.get("loading")), _ptr(part.get("branch")), _ptr(part.get("count"))))
            bridges.append(isl[:int(t5[2])])
            if mode:
                shed.append(_shed_block(L, an, "series", b0, b1, (T,)))
            return t5
        tot, nrec = _screen_blocks(k0, k1, step, rec, full, screen)
        none = np.zeros(0, dtype=np.int64)
        res = DcSeriesScreen(candidates=cand, monitored=mon, profiles=T, threshold=float(threshold), rows=(k0, k1), records=rec[:nrec].copy(),
                             overflow=bool(tot[1] > nrec), islanding=np.concatenate(bridges) if bridges else none,
                             totals=dict(cases=int(tot[0]), violating=int(tot[1]), islanding=int(tot[2])), worst=worst, worstProfile=worstProfile,
                             violatingProfile=violatingProfile, base=base,
                             info=dict(zip(SCREEN_INFO + ("f0Bytes", "f0BuildMs", "f0SweepMs", "f0KernelMs"), (float(x) for x in info))))
        for name, a in full.items():
            setattr(res, name, a)
        res.shed = res.shedBuses = res.shedM = res.shedFlow = res.shedDemand = res.unserved = None
        if mode:
            res.shed, res.shedBuses, res.shedM, res.shedFlow = _concat(shed, none, none, none, np.zeros((0, T)))
            if demand is not None:
                res.shedDemand = _shed_demand(system, res.shed, demand)
                res.unserved = res.shedDemand.sum(axis=1)
        return res


class DcTransferScreen:
    """What dcTransferScreen returns.
      candidates  [K] branch labels (1-based, ascending); monitored the labels of the call; transfers = T; cutoff; rows = (k0, k1)
      capability  [T] the least transfer capability over the base case and the screened outages (+inf: nothing limits the transfer; negative: a
                  branch is beyond its rating at zero transfer), limitingOutage [T] the branch label whose outage gives it (0: the base case) and
                  limitingBranch [T] the branch that reaches its rating (0: none); ties go to the base case, then to the lowest candidate
      base        [T, 3] the base case of every transfer, no outage: capability, limiting branch label, monitored branches above their rating at zero transfer
      worst       [K] the least capability over all transfers of each screened candidate (NaN on a bridge, +inf outside `rows`)
      records     [r, 5] the cases (k, t) whose capability lies below amount[t], sorted by (k, t): label k, transfer index t (0-based row of
                  `transfers`), limiting branch label, capability, flow sensitivity g of the limiting branch; empty without `amount`
      overflow    the record list was cut at its capacity: it holds the FIRST entries by (k, t)
      islanding   labels of the screened candidates that are bridges (status 3): NaN capability for every transfer, never in `records` or a minimum
      totals      dict(cases = rows screened x T, limited = cases below their amount, islanding = bridge candidates): exact also when the list overflowed
      capabilityCases, branch   with dense=True: [k1 - k0, T]
      shed, shedBuses, shedM, shedFlow, shedTransfer   with islands="shed" (else None): the screened bridge candidates, which are then screened on the
                  slack's island and are cases like any other (no longer in `islanding`): their labels ascending, the number of buses that leave [S]
                  int64, the bridge's end on the slack's side [S] (1-based bus), the flow that left that end over the bridge at zero transfer [S] and
                  per unit of each transfer [S, T] (both from the device).  shedTransfer[k, t] != 0: direction t has a source or sink behind bridge k and
                  is partly shed with it; the capability of that case belongs to what remains of the direction
      info        dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs, gBytes, gBuildMs, gSweepMs, gKernelMs)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


TRANSFER_BLOCK_BYTES = 256 << 20                                       # default bound of the dense result of one device call (12 bytes per case)


def transferDirection(system: PowerSystem, source, sink, sourceShare=None, sinkShare=None) -> np.ndarray:
    """A transfer direction [buses] for dcTransferScreen: +1 spread over the buses `source` (labels) and -1 over the buses `sink`, by the shares given
    (normalised to sum 1 on each side; equal by default).  A bus may stand on both sides."""
    d = np.zeros(system.bus.number)
    for name, labels, share, sign in (("source", source, sourceShare, 1.0), ("sink", sink, sinkShare, -1.0)):
        labels = [int(x) for x in np.atleast_1d(np.asarray(labels)).ravel()]
        if not labels:
            raise ValueError(f"transferDirection: {name} names no bus")
        missing = [x for x in labels if x not in system.bus.label]
        if missing:
            raise KeyError(f"The bus label {missing[0]} that has been specified does not exist.")
        w = np.ones(len(labels)) if share is None else np.asarray(share, dtype=np.float64).ravel()
        if w.shape != (len(labels),) or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
            raise ValueError(f"transferDirection: {name}Share needs one finite value >= 0 per bus and a positive sum")
        np.add.at(d, [system.bus.label[x] - 1 for x in labels], sign * w / w.sum())
    return d


def dcTransferScreen(analysis_or_system, transfers, candidates=None, monitored=None, rating=None, amount=None, cutoff: float = 1e-6, injection=None,
                     rows=None, capacity: int = 1 << 20, dense: bool = False, block=None, budget=None, device: int = 0,
                     islands: str = "skip") -> DcTransferScreen:
    """The DC transfer-capability screen: how far the injections can move along direction t of `transfers` ([T, buses] net active injection per unit of
    transfer, the meaning of setInjection_; transferDirection builds one; the slack takes what a direction does not balance) before the first monitored
    branch reaches its rating, in the base case and with branch k of `candidates` (labels; default pairCandidates(system)) out of service -- the loop
    that raises updateBus! / updateGenerator! along a direction around updateBranch!(k, status = 0), solve!, power! per branch, from ONE factor, one
    sweep pair per candidate and one per direction (csrc/jg_dc_transfer.hpp).  A branch limits only where its flow moves by more than `cutoff` per unit
    of transfer.  `injection` ([buses], default: the system's own) is the base operating point; `amount` (a value or [T]) asks for the records of the
    cases that cannot carry that much.  `monitored`, `rating`, `rows`, `block`, `budget` and `capacity` mean what they mean for dcSeriesScreen, and so
    does islands="shed": a bridge candidate is screened on the slack's island (a branch that leaves with it limits nothing; +inf and branch 0 when
    nothing eligible stays), the default candidates are shedCandidates(system).  The part of a direction that lies behind the bridge is shed with it
    (shedTransfer), and the capability of such a case is that of what remains of the direction."""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    who = "dcTransferScreen"
    mode = _island_mode(islands)                                        # refused on the host, before the device is touched
    if rating is None:
        raise ValueError(f"{who}: rating (per branch, per unit of active power) is needed")
    if not cutoff > 0:
        raise ValueError(f"{who}: cutoff > 0")
    d = np.asarray(transfers, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] != system.bus.number:
        raise ValueError(f"{who}: transfers must be [T, buses] with T >= 1")
    if not np.isfinite(d).all():
        raise ValueError(f"{who}: transfers must be finite")
    zero = np.flatnonzero(~d.any(axis=1))
    if zero.size:
        raise ValueError(f"{who}: transfer {int(zero[0])} is all zero: it moves nothing")
    T = int(d.shape[0])
    if amount is not None:
        amount = np.ascontiguousarray(np.broadcast_to(np.asarray(amount, dtype=np.float64), (T,)) if np.ndim(amount) == 0 else np.asarray(amount, dtype=np.float64))
        if amount.shape != (T,) or np.isnan(amount).any():
            raise ValueError(f"{who}: amount is one value, or one per transfer, and no NaN")
    if injection is not None:
        injection = np.asarray(injection, dtype=np.float64)
        if injection.shape != (system.bus.number,) or not np.isfinite(injection).all():
            raise ValueError(f"{who}: injection must be [buses] and finite")
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    cand, mon, rating = _pair_lists(system, candidates, monitored, rating, who=who, least=1, shed=bool(mode))
    nk = int(cand.size)
    k0, k1, step = _screen_rows(who, nk, rows, block, TRANSFER_BLOCK_BYTES, (T + 63) // 64 * 64 * 12)
    with _screen_analysis(analysis_or_system, "transfer", rating, device) as (an, L):
        base_rhs = None if injection is None else np.ascontiguousarray(injection - system.bus.shunt.conductance - system.model.dc.shiftPower)
        info = np.zeros(12)
        _lib.check(L.jg_dc_transfer_set_island_mode(an._h, mode))
        _lib.check(L.jg_dc_transfer_build(an._h, nk, cand, int(mon.size), _ptr(mon), T, np.ascontiguousarray(d).reshape(-1), _ptr(base_rhs), int(budget or 0), info))
        rec = np.zeros((max(int(capacity), 0) if amount is not None else 0, 5))
        worst, base = np.full(nk, np.inf), np.zeros((T, 3))
        cap, capOutage, capBranch = np.full(T, np.inf), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        bridges, shed = [], []
        full = {name: np.zeros((k1 - k0, T), dtype=dt) for name, dt in (("capabilityCases", np.float64), ("branch", np.int32))} if dense else {}

        def screen(b0, b1, room, r, part):
            t5, isl = np.zeros(5, dtype=np.int64), np.zeros(b1 - b0, dtype=np.int64)
            _lib.check(L.jg_dc_transfer_screen(an._h, b0, b1, float(cutoff), _ptr(amount), room, r, _ptr(isl), t5, _ptr(worst), _ptr(cap), _ptr(capOutage),
                                               _ptr(capBranch), _ptr(base) if b0 == k0 else None, _ptr(part.get("capabilityCases")), _ptr(part.get("branch"))))
            bridges.append(isl[:int(t5[2])])
            if mode:
                shed.append(_shed_block(L, an, "transfer", b0, b1, (), (T,)))
            return t5
        tot, nrec = _screen_blocks(k0, k1, step, rec, full, screen)
        none = np.zeros(0, dtype=np.int64)
        first = base[:, 0] <= cap                                       # ties go to the base case
        res = DcTransferScreen(candidates=cand, monitored=mon, transfers=T, cutoff=float(cutoff), rows=(k0, k1),
                               capability=np.where(first, base[:, 0], cap), limitingOutage=np.where(first, 0, capOutage),
                               limitingBranch=np.where(first, base[:, 1].astype(np.int64), capBranch), base=base, worst=worst, records=rec[:nrec].copy(),
                               overflow=bool(tot[1] > nrec), islanding=np.concatenate(bridges) if bridges else none,
                               totals=dict(cases=int(tot[0]), limited=int(tot[1]), islanding=int(tot[2])),
                               info=dict(zip(SCREEN_INFO + ("gBytes", "gBuildMs", "gSweepMs", "gKernelMs"), (float(x) for x in info))))
        for name, a in full.items():
            setattr(res, name, a)
        res.shed = res.shedBuses = res.shedM = res.shedFlow = res.shedTransfer = None
        if mode:
            res.shed, res.shedBuses, res.shedM, res.shedFlow, res.shedTransfer = _concat(shed, none, none, none, np.zeros(0), np.zeros((0, T)))
        return res
