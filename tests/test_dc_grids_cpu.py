"""The shared DC factor's schedule on degenerate and seeded grids, without a GPU (tests/dc_grids.py has the grids and the replay).

Three things are held here: the schedule of every family is race-free and solves the system (a numpy replay with "final" flags against
dc_reference.solve); the families TOGETHER reach every branch of the sweep kernels that the issue names (asserted per class, so that a change of the
ordering that drops one is named); and dc_reference.solve itself is not the limit of the comparisons of tests/test_dc_grids_gpu.py (a dense solve in
extended precision)."""
import numpy as np
import pytest

import dc_grids as G
import dc_reference as R

REPLAY_TOL = 1e-12       # two f64 eliminations of a well-conditioned matrix with fewer than 800 rows
REFERENCE_TOL = 1e-11    # dc_reference.solve against a dense solve in numpy.longdouble: a condition on the INPUTS (change a family's reactances, not this)


@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_the_schedule_replays_without_a_race_and_solves_the_system(jg, name):
    t = G.family(name, jg)
    th = G.replay(t, jg=jg)                                          # raises ScheduleError on a term that reads a value that is not final
    ref, _ = R.solve(t)
    dev = R.worst(th, ref)
    print(name, "replay against dc_reference.solve", dev)
    assert dev <= REPLAY_TOL


def test_the_replay_notices_a_row_scheduled_too_early(jg):
    """the check checks: a backward level moved down by one makes a row read a value that is not final"""
    t = G.family("ring 17", jg)
    real = jg._lib.Plan.get

    def moved(self, which):
        a = real(self, which)
        if which == "bwd_level":
            a = a.copy()
            a[np.argmax(a)] -= 1
        return a
    jg._lib.Plan.get = moved
    try:
        with pytest.raises(G.ScheduleError):
            G.replay(t, jg=jg)
    finally:
        jg._lib.Plan.get = real


def test_the_families_reach_every_branch_of_the_sweep_kernels(jg):
    """Coverage is asserted, not assumed.  If a change of the ordering drops a class, this names it: add a family that reaches it (choose it with
    dc_grids.sweep_levels on the CPU); do not delete the assertion."""
    reached = {}
    for name in G.FAMILIES:
        for c in G.classes(G.sweep_levels(G.family(name, jg), jg)):
            reached.setdefault(c, []).append(name)
    for c in G.COVERAGE:
        print(f"{c}: {', '.join(reached.get(c, [])) or 'NOT REACHED'}")
    missing = [c for c in G.COVERAGE if c not in reached]
    assert not missing, missing
    # and not by one family alone where the issue's own check asks for it: without the tree and the path a class is lost
    rest = set()
    for name in G.FAMILIES:
        if name not in ("binary tree 63", "path 40"):
            rest |= G.classes(G.sweep_levels(G.family(name, jg), jg))
    assert [c for c in G.COVERAGE if c not in rest], "the tree and the path no longer add a class of their own"


def test_sweep_levels_is_what_the_tables_say(jg):
    """forward_levels restated in numpy against the analysis's own export of the same levels (y_level), and the launch rule on hand-made widths"""
    for name in ("mesh 8x8", "pegaseShaped 160"):
        t = G.family(name, jg)
        plan = G._plan(t, jg)[0]
        lv = G.sweep_levels(t, jg)
        assert lv["forward"].sum() == lv["backward"].sum() == plan.n and sorted(lv["perm"]) == list(range(plan.n))
        assert lv["lower"].sum() == lv["upper"].sum()                # a structurally symmetric factor
        assert np.array_equal(G._forward_levels(plan.n, plan.get("l_ptr"), plan.get("l_col")), plan.get("y_level"))
    assert G.launches([16, 17, 3, 1, 40, 16]) == [(0, 1, 1), (1, 2, 0), (2, 4, 1), (4, 5, 0), (5, 6, 1)]
    assert [G._wpi(c) for c in (1, 2, 3, 4, 5, 8, 9, 16)] == [16, 8, 4, 4, 2, 2, 1, 1]


def _dense_longdouble(t):
    """theta of dc_reference.solve's system by plain Gaussian elimination with partial pivoting in numpy.longdouble"""
    B, _, psh = R.assemble(t)
    n = t["bus_type"].size
    slack = R.slack_of(t)
    keep = np.r_[0:slack, slack + 1:n]
    th = np.zeros(n, dtype=np.longdouble)
    if keep.size:
        A = B.toarray()[np.ix_(keep, keep)].astype(np.longdouble)
        b = R.rhs_of(t, psh)[keep].astype(np.longdouble)
        m = keep.size
        for k in range(m):
            p = k + int(np.argmax(np.abs(A[k:, k])))
            if p != k:
                A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
            f = A[k + 1:, k] / A[k, k]
            A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
            b[k + 1:] -= f * b[k]
        x = np.zeros(m, dtype=np.longdouble)
        for k in range(m - 1, -1, -1):
            x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
        th[keep] = x
    return th + np.longdouble(np.asarray(t["bus_va"], dtype=np.float64)[slack])


@pytest.mark.parametrize("name", [k for k in G.FAMILIES if k not in ("pegaseShaped 160", "pegaseShaped 777")])
def test_the_reference_is_not_the_limit(jg, name):
    t = G.family(name, jg)
    assert t["bus_type"].size <= 100
    ref, _ = R.solve(t)
    ld = _dense_longdouble(t)
    dev = float(np.abs(ref.astype(np.longdouble) - ld).max() / max(np.longdouble(1.0), np.abs(ld).max()))
    print(name, "dc_reference.solve against the extended-precision dense solve", dev)
    assert dev <= REFERENCE_TOL
