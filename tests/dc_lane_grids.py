"""Measurement sets on the grids of tests/dc_grids.py for the lane-valued factor (csrc/jg_dc_lanefactor.hip) and the two robust estimators on it
(csrc/jg_dclav.hip, csrc/jg_dchuber.hip), what their GAIN patterns reach in the factorisation and sweep kernels, and the lanes the tests compare -- the
helper of tests/test_dc_lane_grids_cpu.py and of the device tests on these pairs.

  measurement_set(t, th, kind)    kind "full": dcse_reference.full_set (gain pattern: the two-hop graph; complete on a star); "flows": a flow meter on
                                  every in-service branch and a PMU at the slack (the graph's own pattern); "tree": flow meters on a spanning tree and
                                  the slack's PMU (just determined); ("sized", m): a seeded subset of "full" with exactly m rows that keeps the flow
                                  meters of a spanning tree, so every bus stays observed (m >= buses - 1)
  setup(name, kind)               everything of one (grid, set) pair, built once: table, angles, set, H and z of both estimators, the gain pattern
  gain_pattern(ent, n)            the pattern dclav_create / dchuber_create build: the union over ALL rows of their column pairs plus the whole diagonal
  lane_levels(pattern)            dc_grids.plan_levels of that pattern, plus the widths of the factorisation levels, the entries without update terms
                                  and the fill entries
  lane_classes(lv, n, m)          the names of LANE_COVERAGE these reach
  gain_values / replay_gain       H'QH on the pattern (the slack's row and column the identity) and dc_grids.replay_plan on it
  lav_readings / huber_readings   the four kinds of lanes of the existing GPU tests (exact, gross errors only, noisy, noisy with gross errors), seeded
  lav_break_trace(t, ms, z)       the start of the LAV solve on finite readings that overflow, in the device's operations: what the status-3 test rests on
  fair(margins)                   no verdict of a restatement (its `margins`) lies within 1 +- FAIR of its bound
"""
import numpy as np

import dc_grids as G
import dc_reference as R
import dcse_reference as S
import dclav_reference as L
import dchuber_reference as U

ROWS = 32                # DCLAV_ROWS = DCHUBER_ROWS: rows of H per wavefront
COLS = 8                 # DCLAV_COLS = DCHUBER_COLS: states per wavefront
THRESHOLD = 1.345
TOL = 1e-8
FAIR = 1e-6              # test_dchuber_host.FAIR

FAMILY_NAMES = [k for k in G.FAMILIES if k != "pegaseShaped 777"]
# the grids of the state-count classes: paths whose slack is the first bus
PATHS = {f"path {n}": (lambda n=n: G.table(n, G._path(n), 0, 40 + n)) for n in (2, 8, 9, 32, 33)}

LANE_COVERAGE = (G.COVERAGE + [f"factor level, entries mod 4 = {r}" for r in range(4)] + ["entry without update terms", "fill entry"] +
                 [f"n mod 4 = {r}" for r in range(4)] + ["m < 32", "m = 32", "m = 33", "m = 128", "m = 129"] + [f"n = {n}" for n in (1, 2, 8, 9, 32, 33)])

# the (grid, set) pairs of the factor and estimator tests: chosen with lane_levels on the CPU so that, with EDGE_PAIRS, they reach every class of
# LANE_COVERAGE (tests/test_dc_lane_grids_cpu.py asserts it and prints which pair reaches which class)
PAIRS = [
    ("two buses", "flows"),
    ("path 40", "flows"),
    ("star 33, hub slack", "full"),
    ("star 71, leaf slack", "full"),
    ("star 71, leaf slack", "flows"),
    ("complete 12", "full"),
    ("ring 17", "full"),
    ("mesh 8x8", "full"),
    ("mesh 8x8", "flows"),
    ("binary tree 63", "flows"),
    ("two cliques", "full"),
    ("comb 16 x 2", "flows"),
    ("pegaseShaped 72", "flows"),
    ("pegaseShaped 72", "tree"),
    ("pegaseShaped 160", "tree"),
]
# the chunk edges of the iteration passes: m = 31, 32, 33 need a grid of at most m + 1 buses to stay observed (ring 17), m = 128, 129 run on mesh 8x8
EDGE_PAIRS = ([("ring 17", ("sized", m)) for m in (31, 32, 33)] + [("mesh 8x8", ("sized", m)) for m in (128, 129)] + [(p, "flows") for p in PATHS])


def label(kind):
    return kind if isinstance(kind, str) else f"{kind[0]}({kind[1]})"


def table_of(name, jg=None):
    return PATHS[name]() if name in PATHS else G.family(name, jg)


def _tree_branches(t):
    """0-based indices of in-service branches that form a spanning tree, breadth first from the slack"""
    n = t["bus_type"].size
    f, to = np.asarray(t["br_from"]).astype(int) - 1, np.asarray(t["br_to"]).astype(int) - 1
    on = np.asarray(t["br_status"]) == 1
    seen, order, tree = {R.slack_of(t)}, [R.slack_of(t)], []
    for b in order:
        for k in np.flatnonzero(on & ((f == b) | (to == b))):
            o = int(to[k] if f[k] == b else f[k])
            if o not in seen:
                seen.add(o)
                order.append(o)
                tree.append(int(k))
    assert len(seen) == n, "the grid is not connected"
    return np.array(sorted(tree), dtype=np.int64)


def _subset(ms, rows, nw):
    """the rows `rows` (ascending; wattmeters first, then PMUs) of a set"""
    w, p = rows[rows < nw], rows[rows >= nw] - nw
    return S.meters(ms.w_kind[w], ms.w_index[w], ms.w_mean[w], ms.w_variance[w], None, ms.p_index[p], None, ms.p_angle[p], ms.p_variance[p])


def measurement_set(t, th, kind, var_w=1e-2, var_p=1e-5):
    full = S.full_set(t, th, var_w, var_p)
    if kind == "full":
        return full
    n = t["bus_type"].size
    slack = R.slack_of(t)
    fr = R.power(t, th)["from_"]
    if kind in ("flows", "tree"):
        br = np.flatnonzero(np.asarray(t["br_status"]) == 1) if kind == "flows" else _tree_branches(t)
        return S.meters(np.ones(br.size), br + 1, fr[br], np.full(br.size, var_w), None, [slack + 1], None, [th[slack]], [var_p])
    m = int(kind[1])
    nw = full.w_index.size
    keep = n + 2 * _tree_branches(t)                                 # the from-end meters of a spanning tree: rows n + 2 k of full_set
    assert keep.size <= m <= nw + n, f"a set of {m} rows cannot observe {n} buses / the full set has {nw + n} rows"
    rest = np.setdiff1d(np.arange(nw + n), keep)
    rows = np.sort(np.r_[keep, np.random.default_rng(1000 + m).choice(rest, m - keep.size, replace=False)]).astype(np.int64)
    return _subset(full, rows, nw)


def gain_pattern(ent, n):
    """(rowptr, col) of the gain matrix's pattern, 0-based, columns ascending; ent: per row of H its columns (dcse_reference.rows)"""
    adj = [{j} for j in range(n)]
    for cols, _ in ent:
        for a in cols:
            adj[int(a)].update(int(b) for b in cols)
    rowptr = np.r_[0, np.cumsum([len(a) for a in adj])].astype(np.int64)
    return rowptr, np.array([c for a in adj for c in sorted(a)], dtype=np.int64)


def lane_levels(pattern, jg=None):
    """dc_grids.plan_levels of the pattern's analysis, plus factor (entries per factorisation level), noTerms, fill, entries, plan"""
    rowptr, col = pattern
    plan = G.plan_of(rowptr.size - 1, rowptr, col, jg)
    lv = G.plan_levels(plan)
    e_level, t_ptr, e_src = plan.get("e_level"), plan.get("t_ptr"), plan.get("e_src")
    lv.update(factor=np.bincount(e_level), noTerms=int((np.diff(t_ptr) == 0).sum()), fill=int((e_src < 0).sum()), entries=int(e_src.size), plan=plan)
    return lv


def lane_classes(lv, n, m):
    got = G.classes(lv)
    got |= {f"factor level, entries mod 4 = {int(w) % 4}" for w in lv["factor"] if w}
    if lv["noTerms"]:
        got.add("entry without update terms")
    if lv["fill"]:
        got.add("fill entry")
    got.add(f"n mod 4 = {n % 4}")
    got |= {c for c, hit in (("m < 32", m < 32), ("m = 32", m == 32), ("m = 33", m == 33), ("m = 128", m == 128), ("m = 129", m == 129)) if hit}
    if n in (1, 2, 8, 9, 32, 33):
        got.add(f"n = {n}")
    return got


_SETUP = {}


class Setup:
    """one (grid, set) pair: t, th, ms, n, m, slack, va; H, z, on of the LAV rows; Hs, zs, sigma of the Huber rows (scaled by 1 / sigma); ent, pattern"""

    def __init__(self, name, kind, jg=None):
        self.name, self.kind = name, kind
        self.t = t = table_of(name, jg)
        self.th, _ = R.solve(t)
        self.ms = ms = measurement_set(t, self.th, kind)
        self.H, self.z, self.on, self.slack = L.lav_rows(t, ms)
        self.Hs, self.zs, _, _, self.sigma = U.huber_rows(t, ms)
        self.m, self.n = self.H.shape
        self.va = float(np.asarray(t["bus_va"], dtype=np.float64)[self.slack])
        self.ent = S.rows(t, ms)[0]
        self.pattern = gain_pattern(self.ent, self.n)
        self._lv = None

    def levels(self, jg=None):
        if self._lv is None:
            self._lv = lane_levels(self.pattern, jg)
        return self._lv


def setup(name, kind, jg=None):
    key = (name, label(kind))
    if key not in _SETUP:
        _SETUP[key] = Setup(name, kind, jg)
    return _SETUP[key]


def gain(H, q, slack):
    Gm = H.T @ (q[:, None] * H)
    Gm[slack, slack] = 1.0
    return Gm


def gain_values(pattern, Gm):
    """the row-form values of a dense gain matrix on the pattern"""
    rowptr, col = pattern
    return Gm[np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr)), col]


def replay_gain(su, q, rhs, jg=None):
    Gm = gain(su.H, q, su.slack)
    assert np.count_nonzero(Gm) <= su.pattern[1].size
    return G.replay_plan(su.levels(jg)["plan"], gain_values(su.pattern, Gm), np.array(rhs, dtype=np.float64))


def dense_longdouble(A, b):
    """A^-1 b by plain Gaussian elimination with partial pivoting in numpy.longdouble (_dense_longdouble of tests/test_dc_grids_cpu.py for any matrix)"""
    A, b = A.astype(np.longdouble), b.astype(np.longdouble)
    m = b.size
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
    return x


def factor_inputs(su, batch, seed=11):
    """(q [batch, m], rhs [batch, n]) of the factor tests: a seeded Q per lane over twelve decades (10^-6 .. 10^6, as test_the_lane_valued_factor_alone), a
    seeded right-hand side, 0 at the slack"""
    rng = np.random.default_rng(seed)
    q = 10.0 ** rng.uniform(-6.0, 6.0, (batch, su.m))
    rhs = rng.standard_normal((batch, su.n))
    rhs[:, su.slack] = 0.0
    return q, rhs


FACTOR_LANES = (0, 1, 31, 63, 64)
LANE_SEEDS = (7, 11)     # the two seeds of the eight lanes (every lane of every pair meets the conditions of tests/test_dc_lane_grids_cpu.py with them)


def lav_kinds(su, seed):
    """[4, m] readings of the LAV lanes: exact, gross errors only (+5 on up to three rows), noisy (1e-2), noisy with up to two gross errors of -4"""
    z, m = su.z, su.m
    rng = np.random.default_rng(seed)
    kinds = [z.copy() for _ in range(4)]
    kinds[1][rng.choice(m, min(3, m), replace=False)] += 5.0
    kinds[2] += 1e-2 * rng.standard_normal(m)
    kinds[3] += 1e-2 * rng.standard_normal(m)
    kinds[3][rng.choice(m, min(2, m), replace=False)] -= 4.0
    return np.stack(kinds)


def huber_kinds(su, seed):
    """[4, m] UNSCALED readings of the Huber lanes: exact, up to four gross errors of 40 sigma, noisy (one sigma), noisy with up to three of -40 sigma"""
    z, m = su.zs, su.m
    rng = np.random.default_rng(seed)
    kinds = [z.copy() for _ in range(4)]
    k = min(4, m)
    kinds[1][rng.choice(m, k, replace=False)] += 40.0 * rng.choice([-1.0, 1.0], k)
    kinds[2] += rng.standard_normal(m)
    kinds[3] += rng.standard_normal(m)
    kinds[3][rng.choice(m, min(3, m), replace=False)] -= 40.0
    return np.stack(kinds) * su.sigma[None, :]


def lav_readings(su, count=8):
    """[count, m]: the four kinds with the pair's first seed, then with its second, in turn"""
    k = np.concatenate([lav_kinds(su, s) for s in LANE_SEEDS])
    return np.stack([k[s % 8] for s in range(count)])


def huber_readings(su, count=8):
    k = np.concatenate([huber_kinds(su, s) for s in LANE_SEEDS])
    return np.stack([k[s % 8] for s in range(count)])


def fair(margins):
    return all(abs(g - 1.0) > FAIR for g in margins)


_REF = {}


def lav_refs(su, count=8):
    """per lane of lav_readings: (z, lav_ipm's result, its margins)"""
    key = (su.name, label(su.kind), "lav", count)
    if key not in _REF:
        out = []
        for z in lav_readings(su, count):
            z = z * su.on
            ref = L.lav_ipm(su.H, z, su.on, su.slack, tolerance=TOL)
            out.append((z, ref, ref.margins))
        _REF[key] = out
    return _REF[key]


def huber_refs(su, count=8):
    """per lane of huber_readings: (unscaled z, huber_ipm's result on the scaled rows with kappa = THRESHOLD)"""
    key = (su.name, label(su.kind), "huber", count)
    if key not in _REF:
        _REF[key] = [(z, U.huber_ipm(su.Hs, z / su.sigma * su.on, THRESHOLD, su.on, su.slack, tolerance=TOL)) for z in huber_readings(su, count)]
    return _REF[key]


# ---- the lane that breaks mid-iteration (status 3): the start of csrc/jg_dclav.hip traced with the device's own operations ---------------------------
def _fma(a, b, c):
    """fma(a, b, c) as far as overflow goes: one rounding of a * b + c (numpy.longdouble has the range; the last bit does not matter here)"""
    with np.errstate(all="ignore"):
        return np.float64(np.longdouble(a) * np.longdouble(b) + np.longdouble(c))


def lav_break_trace(t, ms, z, jg=None, scale=None):
    """What the start of lav_solve makes of finite readings z that overflow: k_lav_prep -> k_lav_col<false> -> the sweeps on the factor of H'H ->
    k_lav_row<true> -> k_lav_start_finish -> k_lav_init -> Q of iteration 0, every sum in the device's order with fma where the device fuses, and
    fmax dropping NaN as C's does.  -> dict(theta, r0, objective, s, q, zero_pivot_states)"""
    H, _, on, slack = L.lav_rows(t, ms)
    if scale is not None:                                            # the Huber rows: H and z scaled by 1 / sigma, the same start up to k_hub_row<true>
        H = H * scale[:, None]
    m, n = H.shape
    ent = S.rows(t, ms)[0]                                           # a row's stored columns: the slack's is kept with the value 0, and 0 x NaN is NaN
    pattern = gain_pattern(ent, n)
    plan = G.plan_of(n, pattern[0], pattern[1], jg)
    g = plan.get
    perm, e_src, t_ptr, t_a, t_b, t_d, e_level, diag = g("perm"), g("e_src"), g("t_ptr"), g("t_a"), g("t_b"), g("t_d"), g("e_level"), g("diag")
    A = gain_values(pattern, gain(H, on.astype(np.float64), slack))
    ne = e_src.size
    X = np.zeros(ne + 1)
    X[:ne] = np.where(e_src >= 0, A[np.maximum(e_src, 0)], 0.0)
    for l in range(int(e_level.max()) + 1):                          # k_lf_level: finite values, as dc_grids.replay_plan
        for e in np.flatnonzero(e_level == l):
            for a, b, d in zip(*(x[t_ptr[e]:t_ptr[e + 1]] for x in (t_a, t_b, t_d))):
                X[e] -= X[a] * X[b] / X[d]
    dinv = 1.0 / X[diag]
    assert np.isfinite(dinv).all()
    T = np.where(on, z, 0.0)
    B = np.zeros(n)
    for j in range(n):                                               # k_lav_col<false>: rows ascending, fma
        for i in np.flatnonzero(H[:, j]):
            B[j] = _fma(H[i, j], T[i], B[j])
    W = np.zeros(n + 1)

    def sweep(level, ptr, col, ent, upper, start):
        for l in range(1, int(level.max()) + 1):
            new = {}
            for k in np.flatnonzero(level == l):
                acc = start(k)
                for p in range(ptr[k], ptr[k + 1]):
                    with np.errstate(all="ignore"):
                        v = X[ent[p]] * dinv[k if upper else col[p]]
                    acc = _fma(-v, W[col[p]], acc)
                new[k] = acc
            for k, v in new.items():
                W[k] = v
    l_ptr, l_col = g("l_ptr"), g("l_col")
    sweep(G._forward_levels(n, l_ptr, l_col), l_ptr, l_col, g("l_ent"), False, lambda k: B[perm[k]])
    with np.errstate(all="ignore"):
        sweep(g("bwd_level").astype(np.int64), g("u_ptr"), g("u_col"), g("u_ent"), True, lambda k: W[k] * dinv[k])
    theta = np.zeros(n)
    theta[perm] = W[:n]
    r0 = np.zeros(m)
    for i in np.flatnonzero(on):                                     # k_lav_row<true>: lav_dot is an fma chain over the row's columns
        s = 0.0
        for j in sorted(int(c) for c in ent[i][0]):
            s = _fma(H[i, j], theta[j], s)
        with np.errstate(all="ignore"):
            r0[i] = z[i] - s
    with np.errstate(all="ignore"):
        obj = float(np.sum(np.abs(r0[on])))                          # (NaN if a residual is NaN, inf if one is inf and none NaN: whatever the order)
        s = float(np.fmax(obj / int(on.sum()), L.START_FLOOR))       # fmax drops NaN
        u, v = np.fmax(r0, 0.0) + s, np.fmax(-r0, 0.0) + s
        q = np.where(on, 1.0 / (u + v), 0.0)
    dead = [j for j in range(n) if j != slack and not (q[H[:, j] != 0.0] != 0.0).any()]
    return dict(theta=theta, r0=r0, objective=obj, s=s, q=q, zero_pivot_states=dead)


BREAK_ROWS, BREAK_LANE = ((5, 1e308), (30, -1e308)), 5                # the readings of the lane that breaks on case14test: finite, but H'z overflows
