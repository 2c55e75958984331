"""What the DC cascading-outage screen (dcCascadeScreen, csrc/jg_dc_cascade.hip) is held against: the cascade rule stated once in numpy, on two routes to
the flows of an outage set that are independent of each other and of the library (tests/test_dc_cascade_host.py, tests/test_dc_cascade_gpu.py).

  (a) cascade_rebuild(t, S0, rating, monitored, trip, rule, most)       every stage runs dc_group_reference.group_solve on the current set: the members out
                                                                       of service in a copy of the case table, the matrix rebuilt and refactorised; a set
                                                                       that islands a part of the grid is found by the graph oracle, not by linear algebra
  (b) cascade_formula(Phi, f0, S0, rating, monitored, trip, rule, most) the same through dc_group_reference.group_flows on a dense Phi

The rule (stage 0 = the initiating set S0): the set islands -> status 3, end.  Else a monitored, rated branch not in the set is overloaded when
|flow| / rating > trip (strict).  rule "all": every overloaded branch trips, ascending by branch; rule "worst": the most loaded one, ties to the lowest
branch.  No trip -> status 0.  |S| + trips > most -> status 5 (truncated), the set stays, pending = the overloaded branches.  Else append, next stage.

Both return a namespace: status, stages, tripped / stage / loading (lists in the order the branches left; initiating members have stage 0 and loading
NaN), flows (final, [branches]; None for status 3), worst, worstBranch (1-based, 0: none), pending, sets (every set the cascade passed through, for the
pivot condition of the tests), and the MARGIN of the cascade: the smallest |loading - trip| over every stage and monitored rated branch still in service,
and for rule "worst" also the gap between the two largest loadings of every stage that trips.  A cascade makes discrete decisions; one whose margin is
tiny is ambiguous, and the tests leave it out of the comparison of sequences.

S0 and monitored hold 0-based branch indices."""
from types import SimpleNamespace

import numpy as np

import dc_group_reference as Q
import dc_reference as R

TRUNCATED = 5
AMBIGUOUS = 1e-6                    # a cascade whose margin by route (a) is below it is left out of the comparison of sequences


def ratings(t, seed=11):
    """the ratings of the cascade tests: (1.2 + 0.2 u) |f0| + 0.02 with a seeded jitter u (a flat 1.2 |f0| + 0.02 makes the parallel circuits of
    pegaseShaped 160 tie exactly under rule "worst"), every seventh branch unrated"""
    f0 = R.solve(t)[1]
    r = (1.2 + 0.2 * np.random.default_rng(seed).random(f0.size)) * np.abs(f0) + 0.02
    r[::7] = 0.0
    return r


def default_monitored(t, rating):
    return np.flatnonzero((np.asarray(t["br_status"]) == 1) & (rating > 0))


def in_service(t):
    return [int(k) for k in np.flatnonzero(np.asarray(t["br_status"]) == 1)]


def _cascade(flows_of, S0, rating, monitored, trip, rule, most):
    nb = rating.size
    can = np.zeros(nb, dtype=bool)
    can[np.asarray(monitored, dtype=np.int64)] = True
    can &= rating > 0
    inv = np.where(can, 1.0 / np.where(can, rating, 1.0), 0.0)
    S = [int(s) for s in S0]
    out = SimpleNamespace(status=0, stages=0, tripped=list(S), stage=[0] * len(S), loading=[np.nan] * len(S), flows=None, worst=np.nan, worstBranch=0,
                          pending=0, sets=[tuple(S)], margin=np.inf)
    while True:
        fr = flows_of(S)
        if fr is None:
            out.status, out.flows, out.worst, out.worstBranch = 3, None, np.nan, 0
            return out
        load = np.abs(fr) * inv
        load[S] = 0.0
        left = can.copy()
        left[S] = False
        out.flows = fr
        out.worst = float(load.max())
        out.worstBranch = int(np.argmax(load)) + 1 if out.worst > 0 else 0
        if left.any():
            out.margin = min(out.margin, float(np.abs(load[left] - trip).min()))
        over = np.flatnonzero(left & (load > trip))
        if over.size == 0:
            out.status = 0
            return out
        if rule == "worst":
            top = np.sort(load[left])[::-1]
            if top.size > 1:
                out.margin = min(out.margin, float(top[0] - top[1]))
            now = [int(over[np.argmax(load[over])])]              # (argmax: ties go to the lowest branch)
        else:
            now = [int(k) for k in over]
        if len(S) + len(now) > most:
            out.status, out.pending = TRUNCATED, int(over.size)
            return out
        out.stages += 1
        for k in now:
            S.append(k)
            out.tripped.append(k); out.stage.append(out.stages); out.loading.append(float(load[k]))
        out.sets.append(tuple(S))


def cascade_rebuild(t, S0, rating, monitored, trip=1.0, rule="all", most=8, base=None):
    base = Q.base_components(t) if base is None else base
    return _cascade(lambda S: Q.group_solve(t, S, base), S0, rating, monitored, trip, rule, most)


def cascade_formula(Phi, f0, S0, rating, monitored, trip=1.0, rule="all", most=8):
    """also .pivots: the smallest |pivot| of every set the cascade passed through"""
    pivots = []

    def flows_of(S):
        fr, small = Q.group_flows(Phi, f0, S)
        pivots.append(small)
        return fr
    out = _cascade(flows_of, S0, rating, monitored, trip, rule, most)
    out.pivots = pivots
    return out


def same_sequence(a, b):
    """the discrete outcome of two cascades: status, stages, the ordered trips with their stages, pending"""
    return (a.status, a.stages, a.tripped, a.stage, a.pending) == (b.status, b.stages, b.tripped, b.stage, b.pending)


def shares(results):
    """(stable, islanding, truncated) of a list of cascades"""
    st = [r.status for r in results]
    return st.count(0), st.count(3), st.count(TRUNCATED)
