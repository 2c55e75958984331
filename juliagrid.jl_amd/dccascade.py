"""The DC cascading-outage screen: an initiating outage of 1 to `most` branches, then every overloaded monitored branch trips and the flows are formed
again, stage after stage, on the one shared factor (csrc/jg_dc_cascade.hpp).

Reference counterpart: the user loop updateBranch!(analysis; label = s, status = 0) for the initiating outage, solve!, power!, then updateBranch! for what
is overloaded and solve! again until nothing is overloaded -- one rebuild and one refactorisation per stage and per initiating event.  Here: the kept
sensitivities Phi of the union of the initiating members and the monitored branches, and ONE kernel launch per block of cascades; the outage set grows on
the device."""
from types import SimpleNamespace

import numpy as np

from . import _lib
from .dcgroup import DC_GROUP_MAX
from .dcpowerflow import SCREEN_INFO, _island_mode, _ptr, _screen_analysis
from .system import PowerSystem, dcModel_

DC_CASCADE_MAX = DC_GROUP_MAX                                           # csrc/jg_dc_cascade.hpp
DC_CASCADE_TRUNCATED = 5                                                # status: the next stage would exceed `most`
_RULES = {"all": 0, "worst": 1}


def _event_lists(system: PowerSystem, events, most: int):
    """the events as label tuples and as a CSR (offsets, members), checked on the host before anything touches the device: dcGroupScreen's rules"""
    nb, status = system.branch.number, system.branch.layout.status
    out = []
    for g, members in enumerate(events):
        try:
            labels = tuple(members)
        except TypeError:
            labels = (members,)
        who = f"dcCascadeScreen: event {g} {labels!r}"
        if not labels:
            raise ValueError(f"{who} is empty")
        if len(labels) > most:
            raise ValueError(f"{who} has {len(labels)} members, {most} at the most")
        for lab in labels:
            if not isinstance(lab, (int, np.integer)) or isinstance(lab, bool) or lab < 1 or lab > nb:
                raise ValueError(f"{who}: {lab!r} is no branch label (1 .. {nb})")
        labels = tuple(int(x) for x in labels)
        if len(set(labels)) != len(labels):
            raise ValueError(f"{who} names a branch twice")
        off = [lab for lab in labels if status[lab - 1] != 1]
        if off:
            raise ValueError(f"{who}: branch {off[0]} is out of service")
        out.append(labels)
    if not out:
        raise ValueError("dcCascadeScreen: one or more events are needed")
    offsets = np.zeros(len(out) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in out])
    return out, offsets, np.array([lab for x in out for lab in x], dtype=np.int64)


def dcCascadeScreen(analysis_or_system, events, monitored=None, rating=None, trip: float = 1.0, rule: str = "all", most: int = DC_CASCADE_MAX, rows=None,
                    dense: bool = False, budget=None, device: int = 0, islands: str = "skip"):
    """The DC cascading-outage screen: every event of `events` -- a list of tuples of 1 to `most` branch labels, in service, no label twice within an event
    (the output of outageList / parallelGroups can be passed as it is) -- is the initiating outage of one cascade.  Per cascade, stage 0 being the initiating
    set S: the |S| x |S| system of the common-mode screen is solved; a singular one means S islands a part of the grid (status 3, the cascade ends; there is
    no shed mode); else the flows of the monitored branches not in S are formed and a branch trips when |flow| > trip * rating (strict).
      monitored  the branches that can trip and that are reported (default: every in-service branch with a rating > 0); an unrated or unmonitored branch
                 never trips
      rule       "all": every overloaded branch leaves at once, ascending by branch within a stage; "worst": only the most loaded one, ties to the lowest
      most       2 to 8: branches out of service in one cascade, initiating ones included; a stage that would exceed it ends the cascade with status 5
                 (truncated), the set stays as it is and `pending` holds how many were overloaded
      rows       cascades per device call (default: all of them); the result does not depend on it, bit for bit
      budget     bytes the kept sensitivities may take (default: 80 % of the free device memory).  The candidates are the sorted union of all initiating
                 members and all monitored branches in service -- whatever can trip needs its column -- so they cannot be blocked: ValueError with the
                 bytes needed and available when they do not fit, before any sweep
    Returns a namespace:
      events, candidates, monitored, trip, rule, most
      status [C]    0: stable, 3: the set islands a part of the grid, 5: truncated
      stages [C]    stages of trips applied;  size [C]  branches out at the end;  pending [C]
      tripped [C, most]   labels in the order they left: the initiating members as given, then by stage, ascending within a stage; 0: unused
      stage [C, most]     the stage at which each left (0: initiating, -1: unused);  loading [C, most]  the loading that tripped it (NaN: initiating, unused)
      worst [C], worstBranch [C]   the final state: <= trip for status 0, the overloaded state for status 5, NaN and 0 for status 3
      base          [monitored] the base-case flows of the monitored branches
      flows         with dense=True: [C, monitored] the final flows, 0 on what is out, NaN rows for status 3
      totals        dict(cascades, stable, islanding, truncated, trips)
      buildMs, screenMs   HIP events: the build of the sensitivities; the cascade kernel, summed over the device calls
      info          dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs)"""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    if _island_mode(islands):
        raise ValueError("dcCascadeScreen: islands='shed' is not available: the cascade screen has no shed mode (a set that islands a part of the grid "
                         "ends its cascade with status 3)")
    if rating is None:
        raise ValueError("dcCascadeScreen: rating (per branch, per unit of active power) is needed")
    if not trip >= 0:
        raise ValueError("dcCascadeScreen: trip >= 0")
    if rule not in _RULES:
        raise ValueError(f"dcCascadeScreen: rule is \"all\" or \"worst\", not {rule!r}")
    if isinstance(most, bool) or not isinstance(most, (int, np.integer)) or most < 2 or most > DC_CASCADE_MAX:
        raise ValueError(f"dcCascadeScreen: most is 2 to {DC_CASCADE_MAX}, not {most!r}")
    most = int(most)
    nb, status = system.branch.number, system.branch.layout.status
    rating = np.ascontiguousarray(rating, dtype=np.float64)
    if rating.shape != (nb,):
        raise ValueError("rating: one value per branch")
    labels, offsets, members = _event_lists(system, list(events), most)
    if monitored is None:
        mon = (np.flatnonzero((status == 1) & (rating > 0)) + 1).astype(np.int64)
    else:
        mon = np.unique(np.asarray(list(monitored), dtype=np.int64))
        if mon.size and (mon.min() < 1 or mon.max() > nb):
            raise IndexError("dcCascadeScreen: monitored branch label out of range")
    C = len(labels)
    step = C if rows is None else int(rows)
    if step < 1:
        raise ValueError("dcCascadeScreen: rows >= 1")
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    with _screen_analysis(analysis_or_system, "cascade", rating, device) as (an, L):
        info = np.zeros(8)
        try:
            _lib.check(L.jg_dc_cascade_build(an._h, C, offsets, members, int(mon.size), _ptr(mon), int(budget or 0), info))
        except _lib.JGridError as e:
            if e.code == 5:                                             # the sensitivities do not fit: the message has the bytes needed and available
                raise ValueError(f"dcCascadeScreen: {e}") from None
            raise
        dims = np.zeros(6, dtype=np.int64)
        _lib.check(L.jg_dc_cascade_get_dims(an._h, dims))
        cand = np.zeros(int(dims[2]), dtype=np.int64)
        _lib.check(L.jg_dc_cascade_get_candidates(an._h, cand))
        nm = int(dims[4])
        st, stages, size, pending = (np.zeros(C, dtype=np.int32) for _ in range(4))
        worst, branch = np.zeros(C), np.zeros(C, dtype=np.int32)
        tripped, stage, loading = np.zeros((C, most), dtype=np.int64), np.zeros((C, most), dtype=np.int32), np.zeros((C, most))
        flows = np.zeros((C, nm)) if dense else None
        screen_ms = 0.0
        for c0 in range(0, C, step):
            c1 = min(c0 + step, C)
            ms = np.zeros(1)
            _lib.check(L.jg_dc_cascade_run(an._h, c0, c1, float(trip), _RULES[rule], most, _ptr(st[c0:c1]), _ptr(stages[c0:c1]), _ptr(size[c0:c1]),
                                           _ptr(tripped[c0:c1]), _ptr(stage[c0:c1]), _ptr(loading[c0:c1]), _ptr(worst[c0:c1]), _ptr(branch[c0:c1]),
                                           _ptr(pending[c0:c1]), _ptr(flows[c0:c1]) if dense and nm else None, _ptr(ms)))
            screen_ms += float(ms[0])
        base = np.zeros(nm)
        if nm:
            _lib.check(L.jg_dc_cascade_get_base(an._h, base))
        totals = dict(cascades=C, stable=int((st == 0).sum()), islanding=int((st == 3).sum()), truncated=int((st == DC_CASCADE_TRUNCATED).sum()),
                      trips=int((stage > 0).sum()))
        res = SimpleNamespace(events=labels, candidates=cand, monitored=mon, trip=float(trip), rule=rule, most=most, status=st, stages=stages, size=size,
                              tripped=tripped, stage=stage, loading=loading, worst=worst, worstBranch=branch.astype(np.int64), pending=pending, base=base,
                              totals=totals, buildMs=float(info[5]), screenMs=screen_ms, info=dict(zip(SCREEN_INFO, (float(x) for x in info))))
        if dense:
            res.flows = flows
        return res
