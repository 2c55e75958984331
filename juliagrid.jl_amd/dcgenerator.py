"""The DC generator-outage screen: the loss of a generating unit alone (G-1) and with a branch out of service beside it (generator x branch).

  the loop updateGenerator!(system, analysis; label = g, status = 0), solve!, power!          src/powerSystem/generator.jl:262-360, :433-446
  around updateBranch!(...; label = k, status = 0), solve!, power! per branch k                dcGeneratorScreen (csrc/jg_dc_generator.hpp)
  the slack bus's last unit cannot go (generator.jl:441-445 throws)                            generatorCandidates, ValueError

The loss of a unit moves the right-hand side alone.  Who replaces the lost output is a host matter (pickupShare): the slack (the reference), or
the remaining units by participation factors with their headroom as caps.  The result is the sparse matrix A [distinct generator buses x G] of net
injection changes; everything else runs in libjgrid_hip.so (csrc/jg_dc_generator.hip) on the factor, the sensitivities and the record protocol the other DC
screens use.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .dcpowerflow import (SCREEN_INFO, SERIES_BLOCK_BYTES, _concat, _island_mode, _pair_lists, _ptr, _screen_analysis, _screen_blocks, _screen_rows,
                          _shed_block, _shed_demand)
from .system import PowerSystem, dcModel_

PICKUPS = ("slack", "participation")


def generatorCandidates(system: PowerSystem) -> np.ndarray:
    """default generators of dcGeneratorScreen: labels of the in-service generators whose removal leaves the slack bus with at least one in-service
    generator (the reference refuses the loss of the slack bus's last unit and this screen picks no new slack), ascending"""
    gen, slack = system.generator, int(system.bus.layout.slack)
    on = gen.layout.status == 1
    last = on & (gen.layout.bus == slack) & (int((on & (gen.layout.bus == slack)).sum()) <= 1)
    return (np.flatnonzero(on & ~last) + 1).astype(np.int64)


def _generator_list(system: PowerSystem, generators, who: str = "dcGeneratorScreen") -> np.ndarray:
    """generator labels of a screen, checked on the host before anything touches the device"""
    gen = system.generator
    if generators is None:
        g = generatorCandidates(system)
    else:
        g = np.asarray(list(generators), dtype=np.int64)
        if g.size and (g.min() < 1 or g.max() > gen.number):
            raise IndexError(f"{who}: generator label out of range")
        ok = generatorCandidates(system)
        for label in g:
            if gen.layout.status[label - 1] != 1:
                raise ValueError(f"{who}: generator {int(label)} is out of service")
            if label not in ok:
                raise ValueError(f"{who}: generator {int(label)} is the last in-service unit of the slack bus: its loss needs a new slack, which this screen does not pick")
    if g.size < 1:
        raise ValueError(f"{who}: one or more generators are needed")
    return g


def shareLoss(lost: float, weight: np.ndarray, room: np.ndarray):
    """(take [units], shortfall): `lost` shared among units by `weight` (>= 0), no unit taking more than its `room` (>= 0); what a capped unit cannot
    take is shared again among the uncapped ones by the same weights until nothing moves; what nobody can take is the shortfall.  A negative `lost`
    (a unit that absorbed power) is shared by the weights alone: a share below 0 meets no cap."""
    weight, room = np.asarray(weight, dtype=np.float64), np.asarray(room, dtype=np.float64)
    take = np.zeros(weight.size)
    left = float(lost)
    free = weight > 0
    while left != 0.0 and free.any():
        share = np.where(free, left * weight / weight[free].sum(), 0.0)
        over = free & (share > room - take)
        if not over.any():
            take += share
            left = 0.0
            break
        left -= float((room - take)[over].sum())                       # the capped units fill up; the rest is shared again
        take[over] = room[over]
        free &= ~over
    return take, left


class PickupShare:
    """The split of every outage's lost output (pickupShare).
      generators  [G] labels; lost [G] = Pg
      take        scipy CSC [generators of the system x G]: what each remaining unit adds (empty with slack pickup)
      shortfall   [G] what nobody could take: it goes to the slack (0 with slack pickup, where nothing is asked of anybody)
      slackShare  [G] the net change of the slack bus's injection without the shortfall: what its own units take, less Pg where g sits there; with slack
                  pickup Pg (0 where g sits on the slack bus)
      buses       [B] the distinct generator buses that move (labels, ascending, the slack bus aside)
      A           scipy CSC [B x G]: the net change of the bus injections per outage, -Pg at g's bus included.  Over ALL buses the changes balance (the DC
                  model has no losses): sum_b A[b, g] + slackShare[g] + shortfall[g] = 0"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def pickupShare(system: PowerSystem, generators=None, pickup: str = "slack", participation=None) -> PickupShare:
    """Who replaces the output of each lost unit.  pickup="slack": the slack takes all of it (the reference).  pickup="participation": the remaining
    in-service units share it by `participation` ([generators of the system], >= 0; default each unit's maxActive), a unit taking no more than
    maxActive - active (shareLoss); the shortfall goes to the slack."""
    import scipy.sparse as sp
    who = "dcGeneratorScreen"
    if pickup not in PICKUPS:
        raise ValueError(f"{who}: pickup is 'slack' (the slack takes the lost output) or 'participation' (the remaining units share it)")
    gen, slack = system.generator, int(system.bus.layout.slack)
    g = _generator_list(system, generators, who)
    G, ng = int(g.size), gen.number
    on = gen.layout.status == 1
    pg = gen.output.active.astype(np.float64)
    lost = pg[g - 1].copy()
    rows, cols, vals = [], [], []
    shortfall = np.zeros(G)
    if pickup == "participation":
        w = gen.capability.maxActive if participation is None else np.asarray(participation, dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        if w.shape != (ng,):
            raise ValueError(f"{who}: participation needs one value per generator of the system")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError(f"{who}: participation must be finite and >= 0")
        room = np.maximum(np.asarray(gen.capability.maxActive, dtype=np.float64) - pg, 0.0)
        for j, label in enumerate(g):
            rest = on.copy()
            rest[label - 1] = False
            idx = np.flatnonzero(rest)
            take, shortfall[j] = shareLoss(lost[j], w[idx], room[idx])
            nz = take != 0
            rows.append(idx[nz]); cols.append(np.full(int(nz.sum()), j)); vals.append(take[nz])
    elif participation is not None:
        raise ValueError(f"{who}: participation goes with pickup='participation'")
    cat = lambda x, dt: np.concatenate(x).astype(dt) if x else np.zeros(0, dtype=dt)
    take = sp.csc_matrix((cat(vals, np.float64), (cat(rows, np.int64), cat(cols, np.int64))), shape=(ng, G))
    # net change per bus: the units' takes at their buses, -Pg at g's
    tc = take.tocoo()
    bus_r = np.r_[gen.layout.bus[tc.row], gen.layout.bus[g - 1]].astype(np.int64)
    col_r = np.r_[tc.col, np.arange(G)].astype(np.int64)
    val_r = np.r_[tc.data, -lost]
    at_slack = bus_r == slack
    slack_share = np.zeros(G)
    np.add.at(slack_share, col_r[at_slack], val_r[at_slack])
    if pickup == "slack":
        slack_share = np.where(gen.layout.bus[g - 1] == slack, 0.0, lost)
    keep = ~at_slack & (val_r != 0)
    buses = np.unique(bus_r[keep])
    A = sp.csc_matrix((val_r[keep], (np.searchsorted(buses, bus_r[keep]), col_r[keep])), shape=(buses.size, G))
    A.sum_duplicates()
    A.sort_indices()
    return PickupShare(generators=g, lost=lost, take=take, shortfall=shortfall, slackShare=slack_share, buses=buses.astype(np.int64), A=A, pickup=pickup)


def _slack_generation(system: PowerSystem) -> float:
    """the slack bus's generation in the base case, from the balance of the lossless DC model: what all buses inject sums to the shunts' and the phase
    shifters' terms (the nodal matrix has zero column sums)"""
    bus, slack = system.bus, int(system.bus.layout.slack) - 1
    other = np.delete(bus.supply.active, slack)
    return float(bus.demand.active.sum() + bus.shunt.conductance.sum() + system.model.dc.shiftPower.sum() - other.sum())


class DcGeneratorScreen:
    """What dcGeneratorScreen returns.  A column g is the outage of generators[g]; row 0 is that outage alone (G-1), row k that outage with candidate
    branch k out of service beside it.
      generators  [G] generator labels; candidates [K] branch labels (ascending); monitored the labels of the call; threshold; rows = (k0, k1); pickup
      base        [G, 3] the G-1 cases: worst loading, its branch label, number of monitored branches above the threshold
      violating   [r, 5] the cases whose worst loading exceeds the threshold, sorted by (k, g) with the G-1 cases first: branch label k (0: the G-1
                  case), column g (0-based index into `generators`), worst branch label, worst |from| / rating, number of branches above the threshold;
                  the G-1 cases are part of it when rows start at 0
      overflow    the list was cut at its capacity: it holds the FIRST entries by (k, g)
      totals      dict(cases, violating, islanding = bridge candidates): exact also when the list overflowed
      worst       [K] the worst loading over all generators of each screened candidate (0 on a bridge and outside `rows`)
      worstGenerator / violatingGenerator   [G] per generator: the worst loading over the rows screened, the G-1 row included, and the number of
                  candidates whose outage beside the unit's violates (int64)
      bridges     labels of the screened candidates that are bridges (status 3): NaN loading for every generator, never in `violating`
      shed, shedBuses, shedM, shedFlow, shedDemand   with islands="shed" (else None), as DcSeriesScreen: the screened bridge candidates, solved on the
                  slack's island; shedFlow [S, G]; shedDemand [S] the system's demand summed over what leaves.  A unit behind such a bridge leaves with
                  it: its column there is the shed case without the outage
      lost        [G] Pg of each unit; shortfall [G] what no unit could pick up (it goes to the slack); slackActive [G] the slack bus's generation after
                  each G-1 case; pickupShare the PickupShare of the call (pickupShare(...)) when asked for with share=True
      loading, branch, count   with dense=True: [k1 - k0, G]
      info        dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs, f0Bytes, psiBuildMs, psiSweepMs, psiKernelMs, psiBytes,
                  flowKernelMs, busesSwept, entries)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


GENERATOR_INFO = SCREEN_INFO + ("f0Bytes", "psiBuildMs", "psiSweepMs", "psiKernelMs", "psiBytes", "flowKernelMs", "busesSwept", "entries")


def _build(L, an, cand, mon, share: PickupShare, mode: int, budget) -> np.ndarray:
    """jg_dc_generator_build for the split `share`; returns info [16]"""
    A = share.A
    info = np.zeros(16)
    _lib.check(L.jg_dc_generator_set_island_mode(an._h, mode))
    _lib.check(L.jg_dc_generator_build(an._h, int(cand.size), cand, int(mon.size), _ptr(mon), int(share.generators.size), int(share.buses.size),
                                       np.ascontiguousarray(share.buses, dtype=np.int64), np.ascontiguousarray(A.indptr, dtype=np.int64),
                                       np.ascontiguousarray(A.indices, dtype=np.int64), np.ascontiguousarray(A.data, dtype=np.float64), int(budget or 0), info))
    return info


def dcGeneratorScreen(analysis_or_system, generators=None, candidates=None, monitored=None, rating=None, threshold: float = 1.0, pickup: str = "slack",
                      participation=None, rows=None, capacity: int = 1 << 20, dense: bool = False, islands: str = "skip", block=None, budget=None,
                      device: int = 0, share: bool = False, flows: bool = False) -> DcGeneratorScreen:
    """The DC generator-outage screen: every generator of `generators` (labels; default generatorCandidates(system)) out of service alone (G-1) and with
    branch k of `candidates` out beside it -- the loop updateGenerator!(g, status = 0) around updateBranch!(k, status = 0), solve!, power! per branch --
    from ONE factor, one sweep pair per candidate and one per DISTINCT generator bus (csrc/jg_dc_generator.hpp).  `candidates`, `monitored`, `rating`,
    `threshold`, `rows`, `block`, `budget`, `capacity`, `dense` and `islands` mean what they mean for dcSeriesScreen (islands="shed": the default candidates
    are shedCandidates(system)).
      pickup         "slack": the slack takes the lost output (the reference).  "participation": the remaining in-service units share it by
                     `participation` ([generators of the system]; default maxActive), each up to maxActive - active; what nobody can take goes to the
                     slack and is reported as `shortfall` (pickupShare)
      share / flows  keep the PickupShare of the call as `pickupShare` / the G-1 flows [rows of the build, G] as `flow` with their branch labels `flowRows`
    The slack bus's last in-service unit cannot be lost (the reference throws; no new slack is picked here): it is not among the default generators, and
    naming it, or a unit that is out of service, raises ValueError."""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    who = "dcGeneratorScreen"
    mode = _island_mode(islands)                                        # refused on the host, before the device is touched
    if rating is None:
        raise ValueError(f"{who}: rating (per branch, per unit of active power) is needed")
    if not threshold >= 0:
        raise ValueError(f"{who}: threshold >= 0")
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    sh = pickupShare(system, generators, pickup, participation)
    cand, mon, rating = _pair_lists(system, candidates, monitored, rating, who=who, least=1, shed=bool(mode))
    nk, G = int(cand.size), int(sh.generators.size)
    k0, k1, step = _screen_rows(who, nk, rows, block, SERIES_BLOCK_BYTES, (G + 63) // 64 * 64 * 16)
    with _screen_analysis(analysis_or_system, "generator", rating, device) as (an, L):
        info = _build(L, an, cand, mon, sh, mode, budget)
        rec = np.zeros((max(int(capacity), 0), 5))
        worst, worstGenerator, violatingGenerator, base = np.zeros(nk), np.zeros(G), np.zeros(G, dtype=np.int64), np.zeros((G, 3))
        bridges, shed = [], []
        full = {name: np.zeros((k1 - k0, G), dtype=dt) for name, dt in (("loading", np.float64), ("branch", np.int32), ("count", np.int32))} if dense else {}

        def screen(b0, b1, cap, r, part):
            t5, isl = np.zeros(5, dtype=np.int64), np.zeros(b1 - b0, dtype=np.int64)
            _lib.check(L.jg_dc_generator_screen(an._h, b0, b1, float(threshold), cap, r, _ptr(isl), t5, _ptr(worst), _ptr(worstGenerator), _ptr(violatingGenerator),
                                                _ptr(base) if b0 == k0 else None, _ptr(part.get("loading")), _ptr(part.get("branch")), _ptr(part.get("count"))))
            bridges.append(isl[:int(t5[2])])
            if mode:
                shed.append(_shed_block(L, an, "generator", b0, b1, (G,)))
            return t5
        tot, nrec = _screen_blocks(k0, k1, step, rec, full, screen)
        none = np.zeros(0, dtype=np.int64)
        res = DcGeneratorScreen(generators=sh.generators, candidates=cand, monitored=mon, threshold=float(threshold), rows=(k0, k1), pickup=pickup, base=base,
                                violating=rec[:nrec].copy(), overflow=bool(tot[1] > nrec), bridges=np.concatenate(bridges) if bridges else none,
                                totals=dict(cases=int(tot[0]), violating=int(tot[1]), islanding=int(tot[2])), worst=worst, worstGenerator=worstGenerator,
                                violatingGenerator=violatingGenerator, lost=sh.lost, shortfall=sh.shortfall,
                                slackActive=_slack_generation(system) + sh.slackShare + sh.shortfall, pickupShare=sh if share else None,
                                info=dict(zip(GENERATOR_INFO, (float(x) for x in info))))
        for name, a in full.items():
            setattr(res, name, a)
        res.flow = res.flowRows = None
        if flows:
            in_rows = np.zeros(system.branch.number, dtype=bool)
            in_rows[mon - 1] = True
            in_rows[cand - 1] = True
            res.flowRows = (np.flatnonzero(in_rows) + 1).astype(np.int64)
            res.flow = np.zeros((res.flowRows.size, G))
            _lib.check(L.jg_dc_generator_get_flows(an._h, res.flow.reshape(-1)))
        res.shed = res.shedBuses = res.shedM = res.shedFlow = res.shedDemand = None
        if mode:
            res.shed, res.shedBuses, res.shedM, res.shedFlow = _concat(shed, none, none, none, np.zeros((0, G)))
            res.shedDemand = _shed_demand(system, res.shed, system.bus.demand.active[None, :])[:, 0]
        return res
