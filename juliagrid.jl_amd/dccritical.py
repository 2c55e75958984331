"""Critical measurements and critical pairs of a DC measurement set, on the factor of the gain matrix the estimator already holds.

With Omega = W^-1 - H G^-1 H' the covariance of the residuals of the FULL set (csrc/jg_dcse.hpp):

  a critical measurement   w_i Omega_ii <= 1e-6: its residual is 0 whatever it reads, residualTest_ is blind to it, without it the grid is unobservable
  a critical pair i < j    w_j (Omega_jj - Omega_ij^2 / Omega_ii) <= 1e-6: the two normalised residuals are equal up to their sign for an error on either
                           meter, so the test removes the wrong one as easily as the right one; removing both loses observability (a lane that does so
                           through removeMeasurement_ gets status 1 -- the same pivot, csrc/jg_dcse_critical.hpp)
  gamma_ij                 Omega_ij / sqrt(Omega_ii Omega_jj) below that limit: which other meter a bad reading on meter i will be mistaken for

All numerics run in libjgrid_hip.so (csrc/jg_dcse_critical.hip): per block of 512 rows j of H one sweep pair on the shared factor gives G^-1 h_j', one
pass over all rows of H against it gives Omega_ij.  The reference has no counterpart (its observability analysis is topological).
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from .dcstateestimation import DcStateEstimation, _label, _sync, dcStateEstimation
from .measurement import Measurement


def dcCriticalScreen(analysis_or_monitoring, correlation=None, capacity: int = 65536, labels: bool = False):
    """The screen of a DcStateEstimation (any batch; its lanes must not have removed rows) or of a Measurement container (an analysis is built and closed).

    correlation   None: critical pairs only; c in [0, 1]: also every pair with |gamma| >= c
    capacity      pairs delivered at the most; the totals are exact whatever it is
    labels        critical measurements as "Wattmeter 3" / "PMU 7" instead of rows

    Returns critical (rows, 1-based, or labels), pairs [k, 3] = (i, j, gamma) sorted by (i, j) with gamma = +-1 for the critical pairs and only for them,
    totalSingles, totalPairs, totalCorrelated (the further pairs at or above `correlation`), partner [m] (1-based row of the largest |gamma_ij|, the lowest
    row on ties; -1 for rows out of service, critical rows and a row without any other) with partnerCorrelation [m] (NaN there), and variance [m], the
    Omega_ii it used (1 / w_i for a row out of service)."""
    own = isinstance(analysis_or_monitoring, Measurement)
    an = dcStateEstimation(analysis_or_monitoring) if own else analysis_or_monitoring
    if not isinstance(an, DcStateEstimation):
        raise TypeError("dcCriticalScreen: a DcStateEstimation or a Measurement container is needed")
    if correlation is not None and not 0.0 <= float(correlation) <= 1.0:
        raise ValueError(f"dcCriticalScreen: correlation is None or in [0, 1], not {correlation!r}")
    if int(capacity) < 0:
        raise ValueError("dcCriticalScreen: capacity >= 0")
    try:
        _sync(an)                                                           # a changed status or variance: the screen sees the new set
        m = an.method.number
        rec = np.zeros((max(int(capacity), 1), 3))
        totals = np.zeros(3, dtype=np.int64)
        single, partner, gamma = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m)
        _lib.check(_lib.lib().jg_dcse_critical_screen(an._h, -1.0 if correlation is None else float(correlation), int(capacity), rec.reshape(-1), totals,
                                                      single, partner, gamma))
        kept = int(min(totals[1] + totals[2], int(capacity)))
        rows = np.flatnonzero(single) + 1
        variance = np.zeros(m)
        _lib.check(_lib.lib().jg_dcse_get_variance(an._h, variance))
        return NS(critical=[_label(an, int(i)) for i in rows] if labels else rows, pairs=rec[:kept].copy(), totalSingles=int(totals[0]),
                  totalPairs=int(totals[1]), totalCorrelated=int(totals[2]), partner=np.where(partner > 0, partner, -1).astype(np.int64),
                  partnerCorrelation=gamma, variance=variance)
    finally:
        if own:
            an.close()
