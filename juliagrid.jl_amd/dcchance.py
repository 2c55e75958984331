"""The DC probabilistic N-1 screen under Gaussian injection uncertainty: with branch k out of service, how likely is branch m to exceed its rating?
(csrc/jg_dc_chance.hpp has the algebra.)

Reference counterpart: the user loop that samples injections, updateBus! / updateGenerator! per sample around updateBranch!(analysis; label = k, status = 0),
solve!, power! per branch, and counts -- dcSeriesScreen over thousands of sampled profiles, whose answer is a frequency with sampling noise and no tail
below 1 / T.  In the DC model the flows are linear in the injections, so Gaussian injections p0 + L' xi, xi ~ N(0, I_r), give Gaussian post-contingency
flows: their mean and standard deviation come from the kept sensitivities and ONE sweep pair per factor, and no sample is drawn."""
from types import SimpleNamespace

import numpy as np

from . import _lib
from .dcpowerflow import SCREEN_INFO, _island_mode, _pair_lists, _ptr, _screen_analysis, _screen_blocks, _screen_rows
from .system import PowerSystem, dcModel_

DC_CHANCE_MAX = 32                                                      # csrc/jg_dc_chance.hpp
CHANCE_BLOCK_BYTES = 256 << 20                                         # default bound of the dense result of one device call (24 bytes per case and branch)


def injectionFactors(system: PowerSystem, buses, std, correlation: float = 0.0) -> np.ndarray:
    """Factors [len(buses), system buses] for dcChanceScreen: the rows of the Cholesky factor L of the covariance C = L' L of uncertain net injections at
    the buses `buses` (labels, none twice) with standard deviations `std` (one value or one per bus, >= 0) and ONE common correlation between every two of
    them.  Host only.  ValueError for more than DC_CHANCE_MAX = 32 buses (truncate a larger covariance yourself: a PCA keeps the largest factors) and
    for a correlation that makes the matrix indefinite (below -1 / (len(buses) - 1), or above 1)."""
    who = "injectionFactors"
    labels = [int(x) for x in np.atleast_1d(np.asarray(buses)).ravel()]
    m = len(labels)
    if m < 1:
        raise ValueError(f"{who}: one or more buses are needed")
    if m > DC_CHANCE_MAX:
        raise ValueError(f"{who}: {m} buses, {DC_CHANCE_MAX} at the most (one factor per bus)")
    if len(set(labels)) != m:
        raise ValueError(f"{who}: a bus is named twice")
    missing = [x for x in labels if x not in system.bus.label]
    if missing:
        raise KeyError(f"The bus label {missing[0]} that has been specified does not exist.")
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(std, dtype=np.float64), (m,))) if np.ndim(std) == 0 else np.asarray(std, dtype=np.float64)
    if sd.shape != (m,) or not np.isfinite(sd).all() or (sd < 0).any():
        raise ValueError(f"{who}: std is one finite value >= 0, or one per bus")
    rho = float(correlation)
    corr = np.full((m, m), rho)
    np.fill_diagonal(corr, 1.0)
    if not np.isfinite(rho) or abs(rho) > 1 or np.linalg.eigvalsh(corr).min() < -1e-12:
        raise ValueError(f"{who}: correlation {rho!r} makes the covariance of {m} buses indefinite (-1 / (buses - 1) <= correlation <= 1)")
    w, v = np.linalg.eigh(corr)
    if w.min() > 1e-12:
        lower = np.linalg.cholesky(corr)                                # corr = lower lower'
    else:                                                               # semidefinite (correlation 1, or at the lower bound): a QR of the square root gives the triangle
        root = (v * np.sqrt(np.maximum(w, 0.0))).T                      # corr = root' root
        rr = np.linalg.qr(root, mode="r")
        lower = (rr * np.where(np.diag(rr) < 0, -1.0, 1.0)[:, None]).T
    cols = np.array([system.bus.label[x] - 1 for x in labels], dtype=np.int64)
    out = np.zeros((m, system.bus.number))
    out[:, cols] = (sd[:, None] * lower).T                              # C = D corr D = (D lower)(D lower)', the factors are the columns of D lower
    return out


def dcChanceScreen(analysis_or_system, factors, candidates=None, monitored=None, rating=None, probability: float = 0.05, injection=None, rows=None,
                   capacity: int = 1 << 20, dense: bool = False, device: int = 0, block=None, budget=None, islands: str = "skip"):
    """The DC probabilistic N-1 screen: with branch k of `candidates` (labels; default pairCandidates(system); one is allowed) out of service and the
    injections p0 + factors' xi, xi ~ N(0, I_r), the probability that each branch of `monitored` exceeds its rating -- exact in the DC model, from ONE
    factor, one sweep pair per candidate and one per factor, no sample.
      factors      [r, buses] with 1 <= r <= DC_CHANCE_MAX = 32, laid out like `injections` of dcSeriesScreen: net active injection per unit of xi_j
                   (a truncated PCA of a forecast-error covariance; injectionFactors builds the Cholesky rows of a simple one).  The slack takes what a
                   factor does not balance: a factor's slack entry is taken as 0
      probability  a (k, m) with P >= probability is a record and counts
      injection    [buses] the operating point p0 (net active injection, the meaning of setInjection_); default: the system's own
      rows         (k0, k1): only the candidate positions k0 .. k1 - 1;  block: candidates per device call (the result does not depend on it)
    `monitored`, `rating`, `budget`, `capacity` and `dense` mean what they mean for dcSeriesScreen.  A bridge candidate gets status 3 (`bridges`, NaN);
    there is no shed mode: islands="shed" raises ValueError.  Returns a namespace:
      candidates [K], monitored [M]   labels, ascending;  factors = r;  threshold = `probability`;  rows = (k0, k1)
      status [K]    0: screened, 3: a bridge (0 outside `rows`)
      worst [K], worstBranch [K]   the largest P over the monitored branches and the branch that has it (ties: the lowest label; NaN and 0 for status 3)
      count [K]     monitored branches with P >= probability
      records       [v, 5] label k, label m, mean, std, P of every (k, m) with P >= probability, sorted by (k, m); total: their exact number, also when
                    `capacity` cut the list (overflow)
      bridges       labels of the screened candidates with status 3
      base          namespace(mean, std, probability), each [M]: the base case, no outage
      mean, std, probability   with dense=True: [k1 - k0, M]; 0 at m = k, NaN rows for status 3
      info          dict(rows, ld, phiBytes, freeBytes, budgetBytes, buildMs, sweepMs, phiMs, sBytes, sBuildMs, sSweepMs, sKernelMs)"""
    own = isinstance(analysis_or_system, PowerSystem)
    system = analysis_or_system if own else analysis_or_system.system
    who = "dcChanceScreen"
    if _island_mode(islands):
        raise ValueError(f"{who}: islands='shed' is not available: the probabilistic screen has no shed mode (a bridge candidate gets status 3)")
    if rating is None:
        raise ValueError(f"{who}: rating (per branch, per unit of active power) is needed")
    if not 0 < probability <= 1:
        raise ValueError(f"{who}: 0 < probability <= 1")
    L_ = np.asarray(factors, dtype=np.float64)
    if L_.ndim != 2 or L_.shape[1] != system.bus.number:
        raise ValueError(f"{who}: factors must be [r, buses]")
    if L_.shape[0] < 1 or L_.shape[0] > DC_CHANCE_MAX:
        raise ValueError(f"{who}: {L_.shape[0]} factors, 1 to {DC_CHANCE_MAX} are screened (truncate the covariance's factorisation)")
    if not np.isfinite(L_).all():
        raise ValueError(f"{who}: factors must be finite")
    if injection is not None:
        injection = np.asarray(injection, dtype=np.float64)
        if injection.shape != (system.bus.number,) or not np.isfinite(injection).all():
            raise ValueError(f"{who}: injection must be [buses] and finite")
    if own and system.model.dc.nodalMatrix is None:
        dcModel_(system)
    cand, mon, rating = _pair_lists(system, candidates, monitored, rating, who=who, least=1)
    nk, nm, r = int(cand.size), int(mon.size), int(L_.shape[0])
    k0, k1, step = _screen_rows(who, nk, rows, block, CHANCE_BLOCK_BYTES, max(1, nm) * 24)
    with _screen_analysis(analysis_or_system, "chance", rating, device) as (an, L):
        base_rhs = None if injection is None else np.ascontiguousarray(injection - system.bus.shunt.conductance - system.model.dc.shiftPower)
        info = np.zeros(12)
        _lib.check(L.jg_dc_chance_build(an._h, r, np.ascontiguousarray(L_).reshape(-1), nk, cand, nm, _ptr(mon), _ptr(base_rhs), int(budget or 0), info))
        rec = np.zeros((max(int(capacity), 0), 5))
        status, worst, branch, count = np.zeros(nk, dtype=np.int32), np.zeros(nk), np.zeros(nk, dtype=np.int32), np.zeros(nk, dtype=np.int32)
        full = {name: np.zeros((k1 - k0, nm)) for name in ("mean", "std", "probability")} if dense else {}

        def screen(b0, b1, cap, rp, part):
            t5 = np.zeros(5, dtype=np.int64)
            want = dense and nm > 0
            _lib.check(L.jg_dc_chance_screen(an._h, b0, b1, float(probability), cap, rp, t5, _ptr(worst[b0:b1]), _ptr(branch[b0:b1]), _ptr(count[b0:b1]),
                                             _ptr(status[b0:b1]), _ptr(part["mean"]) if want else None, _ptr(part["std"]) if want else None,
                                             _ptr(part["probability"]) if want else None))
            return t5
        tot, nrec = _screen_blocks(k0, k1, step, rec, full, screen)
        base = SimpleNamespace(mean=np.zeros(nm), std=np.zeros(nm), probability=np.zeros(nm))
        if nm:
            _lib.check(L.jg_dc_chance_get_base(an._h, _ptr(base.mean), _ptr(base.std), _ptr(base.probability)))
        res = SimpleNamespace(candidates=cand, monitored=mon, factors=r, threshold=float(probability), rows=(k0, k1), status=status, worst=worst,
                              worstBranch=branch.astype(np.int64), count=count, records=rec[:nrec].copy(), total=int(tot[1]), overflow=bool(tot[1] > nrec),
                              bridges=cand[status == 3], base=base, totals=dict(cases=int(tot[0]), records=int(tot[1]), bridges=int(tot[2])),
                              info=dict(zip(SCREEN_INFO + ("sBytes", "sBuildMs", "sSweepMs", "sKernelMs"), (float(x) for x in info))))
        for name, a in full.items():
            setattr(res, name, a)
        return res
