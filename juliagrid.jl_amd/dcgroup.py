"""The DC common-mode screen: named outage groups of 1 to DC_GROUP_MAX branches, each group one case, on the one shared factor (csrc/jg_dc_group.hpp).

Reference counterpart: the user loop updateBranch!(analysis; label = s, status = 0) for every member s of a group, then solve!, power! -- one rebuild and one
refactorisation per group.  Here: the kept sensitivities Phi of the union of all members, a k x k solve and one pass over the monitored branches per group."""
from types import SimpleNamespace

import numpy as np

from . import _lib
from .dcpowerflow import SCREEN_INFO, _ptr, _screen_analysis
from .system import PowerSystem, dcModel_

DC_GROUP_MAX = 8                                                        # csrc/jg_dc_group.hpp


def parallelGroups(system: PowerSystem):
    """(groups, rest): the default common-mode list -- every set of two or more IN-SERVICE branches that join the same unordered pair of buses (the
    circuits of one tower) is a group, a tuple of branch labels in ascending order; the groups are sorted by their first member.  A set of more than
    DC_GROUP_MAX = 8 branches keeps its first 8 labels as the group, and the labels left over are reported in `rest`, a list of tuples in the order of
    the groups they were cut from (empty when no set is that large): nothing is dropped silently and nothing is raised.  Self-loops form no group."""
    lay = system.branch.layout
    sets = {}
    for k in np.flatnonzero((lay.status == 1) & (lay.from_ != lay.to)):
        a, b = int(lay.from_[k]), int(lay.to[k])
        sets.setdefault((min(a, b), max(a, b)), []).append(int(k) + 1)
    groups, rest = [], []
    for labels in sorted((v for v in sets.values() if len(v) >= 2), key=lambda v: v[0]):
        groups.append(tuple(labels[:DC_GROUP_MAX]))
        if len(labels) > DC_GROUP_MAX:
            rest.append(tuple(labels[DC_GROUP_MAX:]))
    return groups, rest


def _group_lists(system: PowerSystem, groups):
    """the groups as label tuples and as a CSR (offsets, members), checked on the host before anything touches the device"""
    nb, status = system.branch.number, system.branch.layout.status
    out = []
    for g, members in enumerate(groups):
        try:
            labels = tuple(members)
        except TypeError:
            labels = (members,)
        who = f"dcGroupScreen: group {g} {labels!r}"
        if not labels:
            raise ValueError(f"{who} is empty")
        if len(labels) > DC_GROUP_MAX:
            raise ValueError(f"{who} has {len(labels)} members, {DC_GROUP_MAX} at the most")
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
        raise ValueError("dcGroupScreen: one or more groups are needed")
    offsets = np.zeros(len(out) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in out])
    return out, offsets, np.array([lab for x in out for lab in x], dtype=np.int64)


def dcGroupScreen(analysis_or_system, groups, monitored=None, rating=None, threshold: float = 1.0, rows=None, capacity=None, dense: bool = False,
                  budget=None, device: int = 0):
    """The DC common-mode screen: every group of `groups` -- a list of tuples of 1 to 8 branch labels, in service, no label twice within a group -- out of
    service as ONE case: both circuits of a tower, a corridor, the feeders a bus-section fault clears, a user's own N-k list (parallelGroups(system) gives
    the parallel circuits).  The candidates of the kept sensitivities are the sorted union of all members.  `monitored` (default: every in-service branch
    with a rating > 0), `rating`, `threshold` and `dense` mean what they mean in dcPairScreen.
      rows       groups per device call (bounds the memory of a call; default: all of them); the result does not depend on it
      capacity   most records kept (default: 1 << 20; the first by (group, branch); the total stays exact)
    A group that holds a bridge or whose members form a joint cut islands a part of the grid: status 3, no shedding.  Returns a namespace:
      groups        the groups as tuples of labels, as screened;  candidates  the union of the members, ascending;  monitored  the monitored labels, ascending
      status [G]    0: screened, 3: the group islands a part of the grid
      worst [G], worstBranch [G]   the largest |flow| / rating over the monitored branches that stay and the branch that has it (NaN and 0 for status 3)
      count [G]     monitored branches above the threshold
      violating     [v, 4] group index (0-based), branch label, flow, loading, sorted by (group, branch); totals = dict(groups, violating, islanding):
                    exact also when `capacity` cut the list (overflow)
      islanding     indices of the status-3 groups, ascending
      base          [monitored] the base-case flows of the monitored branches
      flows         with dense=True: [G, monitored] the flows, 0 on a group's members, NaN rows for status 3
      buildMs, screenMs   HIP events: the build of the sensitivities; the solves and the screen kernel, summed over the device calls
      info          dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs)"""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    if rating is None:
        raise ValueError("dcGroupScreen: rating (per branch, per unit of active power) is needed")
    if not threshold >= 0:
        raise ValueError("dcGroupScreen: threshold >= 0")
    nb, status = system.branch.number, system.branch.layout.status
    rating = np.ascontiguousarray(rating, dtype=np.float64)
    if rating.shape != (nb,):
        raise ValueError("rating: one value per branch")
    labels, offsets, members = _group_lists(system, list(groups))
    if monitored is None:
        mon = (np.flatnonzero((status == 1) & (rating > 0)) + 1).astype(np.int64)
    else:
        mon = np.unique(np.asarray(list(monitored), dtype=np.int64))
        if mon.size and (mon.min() < 1 or mon.max() > nb):
            raise IndexError("dcGroupScreen: monitored branch label out of range")
    G = len(labels)
    step = G if rows is None else int(rows)
    if step < 1:
        raise ValueError("dcGroupScreen: rows >= 1")
    cap = (1 << 20) if capacity is None else max(int(capacity), 0)
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    with _screen_analysis(analysis_or_system, "group", rating, device) as (an, L):
        info = np.zeros(8)
        _lib.check(L.jg_dc_group_build(an._h, G, offsets, members, int(mon.size), _ptr(mon), int(budget or 0), info))
        dims = np.zeros(6, dtype=np.int64)
        _lib.check(L.jg_dc_group_get_dims(an._h, dims))
        cand = np.zeros(int(dims[2]), dtype=np.int64)
        _lib.check(L.jg_dc_group_get_candidates(an._h, cand))
        nm = int(dims[4])
        st, worst, branch, count = np.zeros(G, dtype=np.int32), np.zeros(G), np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
        flows = np.zeros((G, nm)) if dense else None
        rec, isl = np.zeros((cap, 4)), np.zeros(G, dtype=np.int64)
        tot, nrec, nisl, screen_ms = np.zeros(3, dtype=np.int64), 0, 0, 0.0
        for g0 in range(0, G, step):
            g1 = min(g0 + step, G)
            r, i, t6, ms = rec[nrec:], isl[nisl:], np.zeros(6, dtype=np.int64), np.zeros(1)
            _lib.check(L.jg_dc_group_screen(an._h, g0, g1, float(threshold), r.shape[0], _ptr(r) if r.shape[0] else None, i.shape[0], _ptr(i) if i.shape[0] else None,
                                            t6, _ptr(st[g0:g1]), _ptr(worst[g0:g1]), _ptr(branch[g0:g1]), _ptr(count[g0:g1]),
                                            _ptr(flows[g0:g1]) if dense and nm else None, _ptr(ms)))
            tot += t6[:3]
            nrec += int(t6[3]); nisl += int(t6[4])
            screen_ms += float(ms[0])
        base = np.zeros(nm)
        if nm:
            _lib.check(L.jg_dc_group_get_base(an._h, base))
        res = SimpleNamespace(groups=labels, candidates=cand, monitored=mon, status=st, worst=worst, worstBranch=branch.astype(np.int64), count=count,
                              violating=rec[:nrec].copy(), islanding=isl[:nisl].copy(), base=base, threshold=float(threshold),
                              totals=dict(groups=int(tot[0]), violating=int(tot[1]), islanding=int(tot[2])), overflow=bool(tot[1] > nrec),
                              buildMs=float(info[5]), screenMs=screen_ms, info=dict(zip(SCREEN_INFO, (float(x) for x in info))))
        if dense:
            res.flows = flows
        return res
