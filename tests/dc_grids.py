"""Hand-made and seeded grids for the shared DC factor (csrc/jg_dc_sweep.hip), what their elimination structures reach in the sweep kernels, and a numpy
replay of the factor's schedule -- the helper of tests/test_dc_grids_cpu.py and tests/test_dc_grids_gpu.py.

  table(n, edges, slack, seed, ...)   a table dict in the fixture layout (the keys of tests/golden/cases/*.npz): seeded reactances in [0.05, 0.5], seeded
                                      demands met by ONE unit at the slack bus (further units elsewhere carry a fixed share, the slack's takes the rest),
                                      optional parallel twins, out-of-service copies and shift angles
  FAMILIES                            name -> builder of a table: degenerate graphs with their slack at the first bus, the last bus, the hub or a leaf,
                                      and three seeded pegaseShaped grids (the seeds of tests/test_random_grids_gpu.py)
  sweep_levels(table)                 what the DC handle's factor looks like for this grid: row counts of the forward and backward levels, the launches
                                      build_sweep makes of them, the rows' list lengths.  The analysis is asked for exactly as jg_dc.hip asks: the row
                                      form of dcModel_'s nodal matrix (structurally symmetric, diagonal included), policy 255 << 8 (no top tasks)
  launches(widths)                    build_sweep's launch rule restated: a run of levels of at most 16 rows is one chain launch, a wider level its own
  classes(levels)                     the branches of the sweep kernels these levels reach, as a set of names (COVERAGE lists all of them)
  plan_of / plan_levels / replay_plan the three above for any analysed pattern and its row-form values (sweep_levels and replay go through them)
  replay(table, rhs)                  the schedule replayed in numpy: factorise level by level from t_ptr / t_a / t_b / t_d / e_level, sweep level by
                                      level over the padded lists (pad column n, value 0).  Every entry and every row carries a "final" flag that is
                                      set when its level is over; a term that reads a value that is not final raises ScheduleError
"""
import numpy as np
import scipy.sparse as sp

import dc_reference as R

DC_T = 4                 # csrc/jg_dc_sweep.hpp
DC_CHAIN_WAVES = 16
DC_POLICY_NO_TOP = 255 << 8


class ScheduleError(AssertionError):
    pass


def _jg(jg=None):
    if jg is None:
        import juliagrid.jl_amd as jg
    return jg


def table(n, edges, slack, seed, twins=0, off=0, shifts=0, units=3):
    """n buses (0-based in `edges` and `slack`), one branch per edge, then `twins` parallel copies of seeded edges with reactances of their own, then
    `off` out-of-service copies (parallel to an edge, so that the pattern of the nodal matrix stays the graph's); `shifts` seeded in-service branches
    get a shift angle; `units` generators besides the slack's at seeded other buses"""
    rng = np.random.default_rng(seed)
    e = [(int(a), int(b)) for a, b in edges]
    m0 = len(e)
    extra = twins + off if m0 else 0
    pick = rng.choice(m0, size=extra, replace=extra > m0) if extra else np.zeros(0, dtype=np.int64)
    e += [e[int(k)] for k in pick]
    m = len(e)
    status = np.ones(m, dtype=np.int8)
    if off and m0:
        status[m0 + twins:] = 0
    x = rng.uniform(0.05, 0.5, m)
    shift = np.zeros(m)
    if shifts and m0:
        on = np.flatnonzero(status == 1)
        shift[rng.choice(on, size=min(shifts, on.size), replace=False)] = rng.uniform(-0.05, 0.05, min(shifts, on.size))
    pd = rng.uniform(0.01, 0.1, n)
    pd[slack] = 0.0
    others = np.array([b for b in range(n) if b != slack], dtype=np.int64)
    ubus = np.sort(rng.choice(others, size=min(units, others.size), replace=False)) if others.size else others
    upg = np.full(ubus.size, pd.sum() / (ubus.size + 2.0))
    gen_bus = np.r_[slack, ubus].astype(np.int64)
    gen_pg = np.r_[pd.sum() - upg.sum(), upg]                     # the slack's unit balances the demand
    bus_type = np.ones(n, dtype=np.int8)
    bus_type[ubus] = 2
    bus_type[slack] = 3
    f = np.array([a for a, _ in e], dtype=np.int64)
    to = np.array([b for _, b in e], dtype=np.int64)
    ng = gen_bus.size
    return dict(
        base_power=np.array(1.0e8), bus_label=np.arange(1, n + 1, dtype=np.int64), bus_type=bus_type, bus_pd=pd, bus_qd=np.zeros(n), bus_gs=np.zeros(n),
        bus_bs=np.zeros(n), bus_vm=np.ones(n), bus_va=np.zeros(n), br_from=f + 1, br_to=to + 1, br_status=status, br_r=np.zeros(m), br_x=x,
        br_g=np.zeros(m), br_b=np.zeros(m), br_tap=np.ones(m), br_shift=shift, gen_bus=gen_bus + 1, gen_status=np.ones(ng, dtype=np.int8), gen_pg=gen_pg,
        gen_qg=np.zeros(ng), gen_vg=np.ones(ng), gen_qmax=np.ones(ng), gen_qmin=-np.ones(ng))


def _path(n):
    return [(i, i + 1) for i in range(n - 1)]


def _star(n):
    return [(0, i) for i in range(1, n)]


def _mesh(r, c):
    return [(i * c + j, i * c + j + 1) for i in range(r) for j in range(c - 1)] + [(i * c + j, (i + 1) * c + j) for i in range(r - 1) for j in range(c)]


def _cliques(a, b):
    return ([(i, j) for i in range(a) for j in range(i + 1, a)] + [(a + i, a + j) for i in range(b) for j in range(i + 1, b)] + [(a - 1, a)])


def _comb(spine, leaves):
    return _path(spine) + [(i, spine + leaves * i + j) for i in range(spine) for j in range(leaves)]


def _pegase(n, nb, ng, seed):
    def make(jg=None):
        return _jg(jg).pegaseShaped(n=n, nb=nb, ng=ng, seed=seed, load_scale=0.15)
    return make


def _made(*a, **kw):
    return lambda jg=None: table(*a, **kw)


# the slack: first bus, last bus, the hub, a leaf
FAMILIES = {
    "one bus": _made(1, [], 0, 1),
    "two buses": _made(2, [(0, 1)], 1, 2),
    "path 40": _made(40, _path(40), 0, 3, twins=2, shifts=2),                                       # the slack is a leaf: the first bus
    "star 33, hub slack": _made(33, _star(33), 0, 4, off=1),
    "star 71, leaf slack": _made(71, _star(71), 70, 5, twins=1, shifts=2),
    "complete 12": _made(12, [(i, j) for i in range(12) for j in range(i + 1, 12)], 11, 6, shifts=3),
    "ring 17": _made(17, _path(17) + [(16, 0)], 0, 7, twins=1, off=1, shifts=2),
    "mesh 8x8": _made(64, _mesh(8, 8), 27, 8, twins=2, off=1, shifts=3),
    "binary tree 63": _made(63, [((i - 1) // 2, i) for i in range(1, 63)], 62, 9, twins=1),          # the slack is a leaf: the last bus
    "two cliques": _made(17, _cliques(8, 9), 0, 10, twins=1, shifts=2),
    "comb 16 x 2": _made(48, _comb(16, 2), 47, 11, off=1, shifts=2),                                # the slack is a leaf
    "pegaseShaped 72": _pegase(72, 118, 12, 11),
    "pegaseShaped 160": _pegase(160, 270, 25, 12),
    "pegaseShaped 777": _pegase(777, 1300, 120, 13),
}

_TABLES = {}


def family(name, jg=None):
    """the table of a family, built once; callers get copies"""
    if name not in _TABLES:
        _TABLES[name] = FAMILIES[name](jg)
    return {k: np.array(v) for k, v in _TABLES[name].items()}


def launches(widths):
    """build_sweep's rule: [(first level, end level, chain)]"""
    out, l, nlev = [], 0, len(widths)
    while l < nlev:
        narrow = widths[l] <= DC_CHAIN_WAVES
        e = l + 1
        if narrow:
            while e < nlev and widths[e] <= DC_CHAIN_WAVES:
                e += 1
        out.append((l, e, 1 if narrow else 0))
        l = e
    return out


def _plan(t, jg=None):
    """(plan, row-form values of the handle's matrix, slack, system): what jg_dc_create analyses and factorises"""
    jg = _jg(jg)
    s = jg.powerSystem({k: np.array(v) for k, v in t.items()})
    jg.dcModel_(s)
    B = s.model.dc.nodalMatrix
    n = s.bus.number
    plan = plan_of(n, B.colptr - 1, B.rowval - 1, jg)
    # the pattern is structurally symmetric: entry q of the row form is the entry (column, row) of the CSC arrays, value by value
    M = sp.csc_matrix((np.asarray(B.nzval, dtype=np.float64), np.asarray(B.rowval) - 1, np.asarray(B.colptr) - 1), shape=(n, n))
    At = M.T.tocsc()                                               # CSC of the transpose: column r of it holds row r of M in ascending columns
    At.sort_indices()
    assert np.array_equal(At.indptr, B.colptr - 1) and np.array_equal(At.indices, B.rowval - 1), "the nodal matrix pattern is not structurally symmetric"
    A = At.data.copy()
    slack = int(s.bus.layout.slack) - 1
    row = np.repeat(np.arange(n), np.diff(At.indptr))
    hit = (row == slack) | (At.indices == slack)
    A[hit] = np.where(row[hit] == At.indices[hit], 1.0, 0.0)       # the slack row and column: an identity row
    return plan, A, slack, s


def _forward_levels(n, l_ptr, l_col):
    flev = np.ones(n, dtype=np.int64)
    for r in range(n):
        for p in range(l_ptr[r], l_ptr[r + 1]):
            flev[r] = max(flev[r], flev[l_col[p]] + 1)
    return flev


def plan_of(n, rowptr, col, jg=None):
    """the analysis of a structurally symmetric pattern with a full diagonal (row form, 0-based), asked for as the DC handles ask: no top tasks"""
    return _jg(jg)._lib.Plan(n, rowptr, col, policy=DC_POLICY_NO_TOP)


def plan_levels(plan):
    """sweep_levels of an analysis, whatever matrix it is of (tests/dc_lane_grids.py: the gain pattern of the lane-valued factor)"""
    n = plan.n
    l_ptr, l_col, u_ptr = plan.get("l_ptr"), plan.get("l_col"), plan.get("u_ptr")
    flev, blev = _forward_levels(n, l_ptr, l_col), plan.get("bwd_level").astype(np.int64)
    fw, bw = np.bincount(flev, minlength=2)[1:], np.bincount(blev, minlength=2)[1:]
    return dict(forward=fw, backward=bw, forwardLaunches=launches(fw), backwardLaunches=launches(bw), lower=np.diff(l_ptr), upper=np.diff(u_ptr),
                perm=plan.get("perm").copy(), terms=int(((np.diff(l_ptr) + DC_T - 1) // DC_T * DC_T).sum() + ((np.diff(u_ptr) + DC_T - 1) // DC_T * DC_T).sum()))


def sweep_levels(t, jg=None):
    """dict(forward, backward: rows per level; forwardLaunches, backwardLaunches; lower, upper: list lengths per row; perm)"""
    return plan_levels(_plan(t, jg)[0])


def _wpi(cnt):
    w = DC_CHAIN_WAVES
    while cnt * w > DC_CHAIN_WAVES:
        w >>= 1
    return w


COVERAGE = ([f"{d} chain level with {w} waves per row" for d in ("forward", "backward") for w in (16, 8, 4, 2, 1)] +
            [f"{d} level of {c} rows" for d in ("forward", "backward") for c in ("exactly 16", "17 or 18")] +
            [f"{d} wide level, rows mod 4 = {r}" for d in ("forward", "backward") for r in range(4)] +
            [f"list length mod 4 = {r}" for r in range(4)] + ["empty list", "list of 64 or more terms", "backward launches chain, wide, chain"])


def classes(lv):
    """the names of COVERAGE these levels reach"""
    got = set()
    for d in ("forward", "backward"):
        for w in lv[d]:
            if w <= DC_CHAIN_WAVES:
                got.add(f"{d} chain level with {_wpi(int(w))} waves per row")
            else:
                got.add(f"{d} wide level, rows mod 4 = {int(w) % 4}")
            if w == 16:
                got.add(f"{d} level of exactly 16 rows")
            if w in (17, 18):
                got.add(f"{d} level of 17 or 18 rows")
    for ln in np.r_[lv["lower"], lv["upper"]]:
        got.add("empty list" if ln == 0 else f"list length mod 4 = {int(ln) % 4}")
        if ln >= 64:
            got.add("list of 64 or more terms")
    kinds = "".join("c" if c else "w" for _, _, c in lv["backwardLaunches"])
    if "cw" in kinds and "wc" in kinds[kinds.index("cw"):]:        # a chain, one or more wide levels, a chain again
        got.add("backward launches chain, wide, chain")
    return got


def _padded(n, n_entries, ptr, ent, col, upper):
    """build_sweep's lists: (ptr, col, ent, dpiv) padded to DC_T with column n / entry n_entries"""
    ln = np.diff(ptr)
    pp = np.r_[0, np.cumsum((ln + DC_T - 1) // DC_T * DC_T)]
    pc, pe, pd = np.full(pp[-1], n, dtype=np.int64), np.full(pp[-1], n_entries, dtype=np.int64), np.zeros(pp[-1], dtype=np.int64)
    for k in range(n):
        q = pp[k] + np.arange(ln[k])
        pc[q], pe[q] = col[ptr[k]:ptr[k + 1]], ent[ptr[k]:ptr[k + 1]]
        pd[q] = k if upper else col[ptr[k]:ptr[k + 1]]
    return pp, pc, pe, pd


def _sweep(n, level, pp, pc, val, start, W, final):
    """one triangle, level by level: W[k] = start(k) - sum val * W[col]; a term must read a row that is final (row n, the zero row, always is)"""
    for l in range(1, int(level.max()) + 1):
        rows = np.flatnonzero(level == l)
        new = {}
        for k in rows:
            cols = pc[pp[k]:pp[k + 1]]
            if not final[cols].all():
                raise ScheduleError(f"sweep level {l}: row {k} reads rows {cols[~final[cols]].tolist()} that are not final")
            acc = start(k)
            for p in range(pp[k], pp[k + 1]):
                acc = acc - val[p] * W[pc[p]]
            new[k] = acc
        for k, v in new.items():
            W[k] = v
        final[rows] = True
    if not final.all():
        raise ScheduleError("rows without a level")


def replay_plan(plan, A, r):
    """the schedule of `plan` replayed on the row-form values A of its pattern: x = M^-1 r ([n] or [n, k]), both in the matrix's own order"""
    n = plan.n
    g = plan.get
    perm, e_src, t_ptr, t_a, t_b, t_d, e_level, diag = g("perm"), g("e_src"), g("t_ptr"), g("t_a"), g("t_b"), g("t_d"), g("e_level"), g("diag")
    ne = e_src.size
    X = np.zeros(ne + 1)
    X[:ne] = np.where(e_src >= 0, A[np.maximum(e_src, 0)], 0.0)
    done = np.zeros(ne, dtype=bool)
    for l in range(int(e_level.max()) + 1 if ne else 0):          # factor_numeric: a launch per level, a thread per entry
        ents = np.flatnonzero(e_level == l)
        new = np.zeros(ents.size)
        for i, e in enumerate(ents):
            q = slice(t_ptr[e], t_ptr[e + 1])
            src = np.r_[t_a[q], t_b[q], t_d[q]]
            if not done[src].all():
                raise ScheduleError(f"factorisation level {l}: entry {e} reads entries {src[~done[src]].tolist()} that are not final")
            acc = X[e]
            for a, b, d in zip(t_a[q], t_b[q], t_d[q]):
                acc -= X[a] * X[b] / X[d]
            new[i] = acc
        X[ents] = new
        done[ents] = True
    if not done.all():
        raise ScheduleError("entries without a level")
    piv = X[diag]
    if not (np.isfinite(piv).all() and (piv != 0).all()):
        raise ScheduleError("zero or non-finite pivot")
    dinv = 1.0 / piv
    l_ptr, l_col = g("l_ptr"), g("l_col")
    fp, fc, fe, fd = _padded(n, ne, l_ptr, g("l_ent"), l_col, False)
    bp, bc, be, bd = _padded(n, ne, g("u_ptr"), g("u_ent"), g("u_col"), True)
    fval = np.where(fe < ne, X[fe] * dinv[fd], 0.0)                # k_dc_compact
    bval = np.where(be < ne, X[be] * dinv[bd], 0.0)
    W = np.zeros((n + 1,) + r.shape[1:])
    final = np.zeros(n + 1, dtype=bool)
    final[n] = True
    _sweep(n, _forward_levels(n, l_ptr, l_col), fp, fc, fval, lambda k: r[perm[k]], W, final)
    Y = W.copy()
    final[:n] = False                                              # the backward sweep overwrites W in place: a row not yet final holds the forward value
    _sweep(n, g("bwd_level").astype(np.int64), bp, bc, bval, lambda k: Y[k] * dinv[k], W, final)
    x = np.zeros_like(r)
    x[perm] = W[:n]
    return x


def replay(t, rhs=None, jg=None):
    """the angles [n] (or [n, m] for rhs [n, m]) the schedule gives: the slack's angle added, as dc_reference.solve.  rhs: bus order, default the
    table's own right-hand side"""
    plan, A, slack, s = _plan(t, jg)
    if rhs is None:
        rhs = R.rhs_of(t, R.assemble(t)[2])
    r = np.array(rhs, dtype=np.float64)
    r[slack] = 0.0
    th = replay_plan(plan, A, r)
    th = th + float(np.asarray(t["bus_va"], dtype=np.float64)[slack])
    th[slack] = float(np.asarray(t["bus_va"], dtype=np.float64)[slack])
    return th
