"""AC grids for the block-LU Newton-Raphson and Gauss-Newton engines (csrc/jg_nr.hip, csrc/jg_gn.hip, csrc/jg_engine.hip): the dressed degenerate graphs
of tests/gs_grids.py and seven larger ones Gauss-Seidel could not afford -- the helper of tests/test_nr_grids_host.py, tests/test_nr_grids_gpu.py and
tests/test_gn_grids_gpu.py.

  FAMILIES                      name -> builder of a table: gs_grids.FAMILIES, then the larger families
  family / system / labels      as in gs_grids, over FAMILIES (labels: base lane 0 first, then twins, slack branch, off copies, tap, shift, a bridge,
                                three plain branches)
  bridge(name)                  the labels of a family whose outage islands a bus
  classes(t)                    the branches of k_assemble / k_assemble1 (and of the row loops that share their shape) a grid reaches, read off the nodal
                                matrix's pattern as jg_nr_create gets it, the bus types and the slack: names of COVERAGE
  osys(name)                    the family's OracleSystem, built once
  patched(name, label)          a fresh OracleNR of the family with the branch `label` out through outagePatch (0: the base grid)
  first(name, label)            the oracle's first Newton step of that lane, computed once, read-only: mismatch, Jacobian, increment, V, theta after it
  run(name, label)              the oracle's powerFlow! of that lane at (ITERATION, TOLERANCE), computed once, read-only
  margins_hold(r)               the rule of test_wide_batches_gpu._margins_hold on such a run
  dense_longdouble(...)         Gaussian elimination with partial pivoting in numpy.longdouble, as _dense_longdouble of tests/test_dc_grids_cpu.py
  GN_FAMILIES, gn_table(name)   the Gauss-Newton families and their all-families measurement tables from the oracle's converged power flow
  GN_DEV_REF                    per GN family max|increment - increment_orthogonal| / max|.| of the oracle at the start point, as
                                tests/test_nr_grids_host.py measured and printed it (the yardstick of tests/test_gn_grids_gpu.py)
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

import dc_grids as D
import gs_grids as G
from gs_grids import _made, kinds

ITERATION = 20
# ONE tolerance for every family and lane.  At 1e-8 two lanes of "ring 12 with twins" (0 and 15) stop with a last check of 1.0e-8, within MARGIN of the
# tolerance; at 1e-9 every non-bridge lane of every family stops clear of it on both sides, by a factor 1.23 or more (asserted on the oracle alone, tests/test_nr_grids_host.py)
TOLERANCE = 1e-9
MARGIN = 1e-3


def complete(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def tree(n):
    return [((i - 1) // 2, i) for i in range(1, n)]


FAMILIES = dict(G.FAMILIES)
FAMILIES.update({
    "complete 12 AC": _made(12, complete(12), 11, 41, units=[2, 7], shifts=2),
    "complete 24 AC": _made(24, complete(24), 0, 42, units=[5, 13, 20], shifts=2, load=0.5),
    "mesh 8x8 AC": _made(64, D._mesh(8, 8), 27, 43, units=[3, 40, 60], twins=2, off=1, shifts=3, load=0.3),
    "binary tree 63 AC": _made(63, tree(63) + [(0, 1), (1, 3), (2, 6)], 62, 44, units=[0, 10, 30], load=0.3),
    "comb 16 x 2 AC": _made(48, D._comb(16, 2) + [(0, 1), (7, 8)], 47, 45, units=[3, 12], off=1, shifts=2, load=0.3),
    "star 17 all PV": _made(17, D._star(17) + [(0, 3)], 0, 46, units=range(1, 17)),
    "path 40 AC": _made(40, D._path(40) + [(0, 1), (20, 21)], 0, 47, units=[13, 30], shifts=2, load=0.15),
})
NAMES = list(FAMILIES)

_TABLES = {}


def family(name, jg=None):
    """the table of a family, built once; callers get copies"""
    if name not in _TABLES:
        _TABLES[name] = FAMILIES[name](jg)
    return {k: np.array(v) for k, v in _TABLES[name].items()}


def system(name, jg=None):
    jg = D._jg(jg)
    s = jg.powerSystem(family(name, jg))
    jg.acModel_(s)
    return s


@functools.lru_cache(maxsize=None)
def labels(name):
    return G.labels(family(name))


@functools.lru_cache(maxsize=None)
def bridge(name):
    kd = kinds(family(name))
    return frozenset(k for k in labels(name)[1:] if "bridge" in kd[k])


LONG = 20                      # a "long" row: past the "<= 19" k_assemble's own comment assumes

COVERAGE = ([f"row longer than 4, length mod 4 = {r}" for r in range(4)] + [f"row length mod 8 = {r}" for r in range(8)] +
            ["row of 20 or more entries", "row of 64 or more entries", "long row, diagonal first", "long row, diagonal last",
             "n = 1", "n = 2", "n < 16", "n mod 16 = 0", "n mod 16 = 1", "n mod 16 = 15", "n = 64", "64 < n < 80",
             "no PQ bus", "no PV bus", "slack first bus", "slack last bus", "slack hub", "slack leaf"])


def classes(t, jg=None):
    """the names of COVERAGE the grid reaches.  The rows are those of the nodal matrix as jg_nr_create gets it (CSC of a structurally symmetric pattern:
    a column is the row, ascending); k_assemble walks a row in chunks of 4, k_assemble1 gives lane q of a quad the entries q, q + 4 | q + 8, q + 12 | ...
    (a trip is 8 entries), both take 16 rows per chunk maximum and k_assemble1 64 rows per workgroup"""
    jg = D._jg(jg)
    s = jg.powerSystem({k: np.array(v) for k, v in t.items()})
    jg.acModel_(s)
    Y = s.model.ac.nodalMatrix
    colptr, rowval = np.asarray(Y.colptr) - 1, np.asarray(Y.rowval) - 1
    n = s.bus.number
    typ = np.asarray(t["bus_type"])
    slack = int(np.flatnonzero(typ == 3)[0])
    ln = np.diff(colptr)
    got = set()
    for i in range(n):
        row = rowval[colptr[i]:colptr[i + 1]]
        assert np.all(np.diff(row) > 0) and i in row
        got.add(f"row length mod 8 = {ln[i] % 8}")
        if ln[i] > 4:
            got.add(f"row longer than 4, length mod 4 = {ln[i] % 4}")
        if ln[i] >= LONG:
            got.add("row of 20 or more entries")
            if row[0] == i:
                got.add("long row, diagonal first")
            if row[-1] == i:
                got.add("long row, diagonal last")
        if ln[i] >= 64:
            got.add("row of 64 or more entries")
    for name, hit in (("n = 1", n == 1), ("n = 2", n == 2), ("n < 16", n < 16), ("n mod 16 = 0", n % 16 == 0), ("n mod 16 = 1", n % 16 == 1),
                      ("n mod 16 = 15", n % 16 == 15), ("n = 64", n == 64), ("64 < n < 80", 64 < n < 80), ("no PQ bus", not np.any(typ == 1)),
                      ("no PV bus", not np.any(typ == 2)), ("slack first bus", slack == 0 and n > 1), ("slack last bus", slack == n - 1 and n > 1),
                      ("slack hub", ln[slack] == ln.max() and ln[slack] > 3), ("slack leaf", ln[slack] == 2)):
        if hit:
            got.add(name)
    return got


# ---- the oracle's side, once per family and lane ----------------------------------------------------------------------------------------------------
def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def osys(name):
    return _oracle().OracleSystem(family(name))


@functools.lru_cache(maxsize=None)
def _system(name):
    return system(name)


@functools.lru_cache(maxsize=None)
def patch(name, label):
    """(0-based pointers, deltas) of the lane's edit of the nodal matrix; nothing for the base lane"""
    if not label:
        return (), ()
    ptr, dy = D._jg().outagePatch(_system(name), int(label))
    return tuple(int(p) - 1 for p in ptr), tuple(complex(d) for d in dy)


def patched(name, label, types=None, qs=None):
    """a fresh OracleNR of the lane; types: a bus-type vector of its own (the lane-valued types of setBusType_), qs: its reactive supply"""
    O = _oracle()
    sy = osys(name)
    if types is not None:
        sy = O.OracleSystem(family(name))
        sy.type = np.asarray(types, dtype=np.int8).copy()
    o = O.OracleNR(sy)
    for p, d in zip(*patch(name, label)):
        o.add_ybus(p, d)
    if qs is not None:
        o.set_power(sy.ps, qs, sy.pd, sy.qd)
    return o


def _frozen(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return ns


@functools.lru_cache(maxsize=None)
def first(name, label):
    """the oracle's first step of the lane from newtonRaphson()'s start point: mismatch! then solve!"""
    o = patched(name, label)
    vm0, va0 = o.voltage()
    dp, dq = o.mismatch()
    f = o.vectors()[1]
    if o.dim:
        o.solve()
    j, _, inc = o.vectors()
    vm, va = o.voltage()
    return _frozen(NS(dim=o.dim, nnzJ=o.nnzJ, pq=o.pq, pvpq=o.pvpq, pcount=o.pcount, jcolptr=o.jcolptr, jrowval=o.jrowval, dp=dp, dq=dq, f=f, J=j, inc=inc,
                      vm0=vm0, va0=va0, vm=vm, va=va))


def finish(o, status):
    vm, va = o.voltage()
    return _frozen(NS(status=int(status), iteration=o.iteration, vm=vm, va=va, history=o.history.max(axis=1).copy()))


@functools.lru_cache(maxsize=None)
def run(name, label, tolerance=TOLERANCE):
    o = patched(name, label)
    return finish(o, o.power_flow(iteration=ITERATION, tolerance=tolerance))


def margins_hold(r, tolerance=TOLERANCE):
    h = r.history
    return bool(h[-1] * (1.0 + MARGIN) <= tolerance and (h.size < 2 or h[-2] >= tolerance * (1.0 + MARGIN)))


def dense_longdouble(dim, colptr, rowval, nzval, rhs):
    """x of J x = rhs, J given by its CSC arrays (1-based): plain Gaussian elimination with partial pivoting in numpy.longdouble"""
    A = np.zeros((dim, dim), dtype=np.longdouble)
    for c in range(dim):
        for p in range(colptr[c] - 1, colptr[c + 1] - 1):
            A[rowval[p] - 1, c] += np.longdouble(nzval[p])
    b = np.asarray(rhs, dtype=np.longdouble).copy()
    for k in range(dim):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(dim, dtype=np.longdouble)
    for k in range(dim - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


# ---- Gauss-Newton on the same grids --------------------------------------------------------------------------------------------------------------------
GN_FAMILIES = ["two buses, PQ", "all PV ring 9", "all PQ mesh 4x4", "complete 24 AC", "star 40, hub first PV", "star 71, hub last", "mesh 8x8 AC"]
# max|increment() - increment_orthogonal()| / max|increment_orthogonal()| of the oracle at the start point (tests/test_nr_grids_host.py prints them)
GN_DEV_REF = {"two buses, PQ": 3.9e-14, "all PV ring 9": 1.4e-14, "all PQ mesh 4x4": 1.0e-13, "complete 24 AC": 9.9e-12, "star 40, hub first PV": 1.4e-13,
              "star 71, hub last": 2.1e-12, "mesh 8x8 AC": 1.1e-13}
GN_TOLERANCE = 1e-11           # stateEstimation_ of the known-answer test (tests/test_random_grids_gpu.py: test_wls_known_answer)


def lu_bound(name):
    """first increment under LU against OracleGN.increment(), relative to max|ref|: 10 x the family's yardstick, floored at the 1e-9 bar of the NR increment"""
    return max(10.0 * GN_DEV_REF[name], 1e-9)


def orthogonal_bound(name):
    """first increment under Orthogonal against increment_orthogonal(), relative to max|ref|: methods_reference.increment_bound's rule on the family's
    yardstick -- 10 x, never looser than 1e-6"""
    return min(10.0 * GN_DEV_REF[name], 1e-6)
# The tables' own start (V = 1, theta = 0 everywhere) leaves a plain branch without current, and the magnitude of a zero current has no derivative: an
# ammeter row there is 0 / 0 on the oracle and on the device alike.  The Gauss-Newton grids therefore start from seeded voltages around the flat point
# (+- 0.02 pu, +- 0.05 rad), written into bus_vm / bus_va of the table so that both sides read the same start.
GN_START_SEED = 4711


@functools.lru_cache(maxsize=None)
def gn_grid(name):
    """(table, OracleSystem with the power flow's types and slack, vm, va) of the family's converged power flow; shared, read-only"""
    O = _oracle()
    t = family(name)
    rng = np.random.default_rng(GN_START_SEED)
    n = t["bus_type"].size
    t["bus_vm"] = 1.0 + 0.02 * rng.uniform(-1, 1, n)
    t["bus_va"] = 0.05 * rng.uniform(-1, 1, n)
    s = O.OracleSystem(t)
    pf = O.OracleNR(s)
    assert pf.power_flow(iteration=ITERATION, tolerance=TOLERANCE) == 0
    vm, va = pf.voltage()
    s.type = pf.type.copy(); s.slack = pf.slack
    vm.flags.writeable = va.flags.writeable = False
    return t, s, vm, va


def gn_table(name):
    """voltmeters, ammeters, wattmeters, varmeters and PMUs at every place, reading the power flow exactly (methods_reference.all_families)"""
    import methods_reference as R
    t, s, vm, va = gn_grid(name)
    return R.all_families(_oracle(), s, vm, va)
