"""Branch status tests of a DC measurement set (topology errors), on the factor of the gain matrix the estimator already holds.

residualTest_ asks "which METER is wrong"; a wrong breaker status spreads over the two flow meters of the branch and the injection meters at its ends, and
no single meter explains it.  The hypothesis for branch k adds one unknown to the model, z = c + H theta + m_k phi + e: phi is the flow k really carries
from -> to minus the flow the model gives it, m_k is +1 on the from-end wattmeters of k and the injection wattmeters on from(k), -1 on the to-end
wattmeters and the injection wattmeters on to(k) (csrc/jg_dcse_topology.hpp).  With r the residuals of the full set's estimate:

  D_k = m_k' W m_k - (H' W m_k)' G^-1 (H' W m_k)      once per factor, one sweep pair per 512 candidates
  flowError_kl = m_k' W r_l / D_k                       the estimate of phi in lane l
  statistic_kl = m_k' W r_l / sqrt(D_k)                 N(0, 1) without an error; its square is the drop of the objective when phi is freed
  status 0 testable, 1 critical branch (D_k <= 1e-6 m_k' W m_k: a status error on it moves the estimate and leaves no residual), 2 unseen (m_k = 0)

All numerics run in libjgrid_hip.so (csrc/jg_dcse_topology.hip); m_k is built here on the host from the container's wattmeters.  The reference has no
counterpart (its bad-data processing is per measurement).
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from .dcstateestimation import DcStateEstimation, _sync, dcStateEstimation, solve_
from .measurement import Measurement


def _meter_columns(an: DcStateEstimation):
    """per branch (0-based) the rows (0-based, ascending) and signs of m_k, whatever the meters' status: the library masks rows out of service"""
    sysm = an.system
    br, w = sysm.branch, an.monitoring.wattmeter
    f = np.asarray(br.layout.from_, dtype=np.int64) - 1
    t = np.asarray(br.layout.to, dtype=np.int64) - 1
    at_bus = [[] for _ in range(sysm.bus.number)]                       # rows of the injection wattmeters at a bus: two meters, both counted
    cols = [[] for _ in range(br.number)]
    for r, (fam, i) in enumerate(an._devs):
        if fam != "w":
            continue                                                    # PMUs: 0
        k = int(w.layout.index[i]) - 1
        if w.layout.bus[i]:
            at_bus[k].append(r)
        else:
            cols[k].append((r, 1 if w.layout.from_[i] else -1))
    for k in range(br.number):
        if f[k] == t[k]:
            continue                                                    # a branch from a bus to itself carries nothing the injections see
        cols[k] += [(r, 1) for r in at_bus[f[k]]] + [(r, -1) for r in at_bus[t[k]]]
        cols[k].sort()
    return cols


def dcTopologyScreen(analysis_or_monitoring, candidates=None, threshold: float = 3.0, capacity: int = 65536, dense: bool = False, correct: bool = False,
                     labels: bool = False):
    """The status test of every candidate branch in every lane of a solved DcStateEstimation (its lanes must not have removed rows), or of a Measurement
    container (an analysis is built, solved and closed).

    candidates    branch labels (1-based), in or out of service, in the order they are tested and reported; None: every branch that at least one meter
                  in service sees, ascending
    threshold     a (lane, branch) with |statistic| >= threshold is a record
    capacity      records delivered at the most; `total` is exact whatever it is
    dense         also statisticAll [count, lanes]
    correct       also angle [lanes, n]: lanes with |statistic| >= threshold carry the estimate of the augmented problem for their `best` branch,
                  theta' = theta^ - G^-1 H' W m_k flowError; the others the analysis' estimate bit for bit.  The analysis itself is left as it is
    labels        critical and unseen as "Branch 7" instead of numbers

    Returns candidates [count], status [count] (0 / 1 / 2), denominator, norm [count] (D_k and m_k' W m_k), critical, unseen (the branches of status 1
    and 2), best [lanes] (the branch of the largest |statistic|, the first of `candidates` on ties -- parallel circuits that only injection meters see
    share a column and always tie; -1 where no candidate is testable), statistic, flowError [lanes] (NaN there), count [lanes] (candidates at or above the
    threshold), records [k, 4] = (lane, branch, statistic, flowError), 1-based, sorted by (lane, position in `candidates`) with the exact `total`, and
    largestResidual [lanes]: the lane's largest normalised residual as residualTest_ sees it -- where |statistic| exceeds it, one branch explains the
    residuals better than any single meter."""
    who = "dcTopologyScreen"
    own = isinstance(analysis_or_monitoring, Measurement)
    if not own and not isinstance(analysis_or_monitoring, DcStateEstimation):
        raise TypeError(f"{who}: a DcStateEstimation or a Measurement container is needed")
    if not float(threshold) > 0.0:
        raise ValueError(f"{who}: threshold > 0, not {threshold!r}")
    if int(capacity) < 0:
        raise ValueError(f"{who}: capacity >= 0")
    an = dcStateEstimation(analysis_or_monitoring) if own else analysis_or_monitoring
    try:
        if own:
            solve_(an)
        elif an.objective is None:
            raise ValueError(f"{who}: solve the analysis first")
        _sync(an)                                                       # a changed status or variance: the denominators follow the new set
        L, check = _lib.lib(), _lib.check
        nbr, lanes, n = an.system.branch.number, an.batch, an.system.bus.number
        cols = _meter_columns(an)
        if candidates is None:
            seen = [k for k in range(nbr) if any(an._status[r] for r, _ in cols[k])]
            if not seen:
                raise ValueError(f"{who}: no meter in service sees a branch")
            cand = np.array(seen, dtype=np.int64) + 1
        else:
            cand = np.atleast_1d(np.asarray(candidates))
            if cand.ndim != 1 or cand.size == 0 or not np.issubdtype(cand.dtype, np.integer):
                raise TypeError(f"{who}: candidates is a list of branch labels (integers)")
            cand = cand.astype(np.int64)
            bad = cand[(cand < 1) | (cand > nbr)]
            if bad.size:
                raise ValueError(f"{who}: the branch label {int(bad[0])} does not exist")
            if np.unique(cand).size != cand.size:
                raise ValueError(f"{who}: a branch is listed twice")
        count = cand.size
        ptr = np.r_[0, np.cumsum([len(cols[k - 1]) for k in cand])].astype(np.int64)
        row = np.array([r + 1 for k in cand for r, _ in cols[k - 1]] or [0], dtype=np.int64)
        sign = np.array([s for k in cand for _, s in cols[k - 1]] or [1], dtype=np.int32)
        check(L.jg_dcse_topology_set(an._h, count, cand, ptr, row, sign))
        D, norm, status = np.zeros(count), np.zeros(count), np.zeros(count, dtype=np.int32)
        check(L.jg_dcse_topology_denominators(an._h, D.ctypes.data_as(_lib.VP), norm.ctypes.data_as(_lib.VP), status.ctypes.data_as(_lib.VP), None))
        rec = np.zeros((max(int(capacity), 1), 4))
        totals = np.zeros(2, dtype=np.int64)
        best, cnt = np.zeros(lanes, dtype=np.int32), np.zeros(lanes, dtype=np.int32)
        stat, phi = np.zeros(lanes), np.zeros(lanes)
        all_t = np.zeros((count, lanes)) if dense else None
        check(L.jg_dcse_topology_screen(an._h, float(threshold), int(capacity), rec.reshape(-1), totals, best, stat, phi, cnt,
                                        all_t.ctypes.data_as(_lib.VP) if dense else None))
        kept = int(min(totals[0], int(capacity)))
        records = rec[:kept].copy()
        records[:, 1] = cand[records[:, 1].astype(np.int64) - 1]
        largest, index = np.zeros(lanes), np.zeros(lanes, dtype=np.int32)
        check(L.jg_dcse_residual_test(an._h, np.inf, 0, largest, index))
        name = (lambda ks: [f"Branch {int(k)}" for k in ks]) if labels else (lambda ks: ks)
        out = NS(candidates=cand, status=status, denominator=D, norm=norm, critical=name(cand[status == 1]), unseen=name(cand[status == 2]),
                 best=np.where(best > 0, cand[np.maximum(best, 1) - 1], -1), statistic=stat, flowError=phi, count=cnt.astype(np.int64), records=records,
                 total=int(totals[0]), largestResidual=largest)
        if dense:
            out.statisticAll = all_t
        if correct:
            with np.errstate(invalid="ignore"):
                pick = np.where(np.abs(stat) >= float(threshold), best, 0).astype(np.int32)
            angle = np.zeros((lanes, n))
            check(L.jg_dcse_topology_correct(an._h, pick, angle.reshape(-1)))
            out.angle = angle
        return out
    finally:
        if own:
            an.close()


def topologyRuns(an: DcStateEstimation) -> int:
    """how often the handle has formed the denominators of its candidates (the counter beside dims()["omegaRuns"]); 0 before the first screen"""
    runs = np.zeros(1, dtype=np.int64)
    _lib.check(_lib.lib().jg_dcse_topology_denominators(an._h, None, None, None, runs.ctypes.data_as(_lib.VP)))      # the counter alone: nothing is formed
    return int(runs[0])
