"""Dressed grids for the batched DC optimal power flow (csrc/jg_dcopf.hip): the degenerate graphs of tests/dc_grids.py and case118 with seeded costs,
capacities, ratings, angle limits and a second unit at one bus; what the factor of K looks like on them; a polish of the restatement's solution that
shares no iteration with it -- the helper of tests/test_dcopf_grids_host.py and tests/test_dcopf_grids_gpu.py.

  dress(table_or_case, seed)   a PowerSystem with seeded optimal-power-flow data.  The table's own dispatch (the slack's unit balancing the demand) and
                               its DC flows are a feasible point by construction: every capacity lies above the unit's output there, every rating and
                               angle limit above the branch's flow and angle difference there (by 8 % at the least, so that a demand of 1.05 stays
                               feasible).  The costs pull the optimum away from that point, so some limits bind
  GRIDS                        name -> (family or case, seed)
  grid(name)                   the dressed system, its restatement model and the table, built once
  lanes(name)                  the 65 demand factors of the device test, seeded per grid, in [0.85, 1.05]; lane 0 is 1.0
  k_pattern(md)                the pattern of K = P + sigma I + A' rho A: that of A'A plus the diagonal
  k_levels(md)                 dc_grids.sweep_levels for K: jg_dcopf_create's analysis (the same pattern, policy DC_POLICY_NO_TOP) and build_sweep's launches
  active(md, r)                the active set of a restatement result: rows whose multiplier has a sign and whose z sits on the bound of that sign
  polish(md, r)                the equality-constrained QP on that set by one dense solve of its KKT system
  MEASURED, bounds(name)       per grid the figures of tools/dcopf_grids_measure.py and the device test's bounds: these x 10 (the rules of test_dcopf_gpu.py
                               and test_dcopf_host.py)
"""
import importlib
import os
from types import SimpleNamespace as NS

import numpy as np
import scipy.sparse as sp

import dc_grids as G
import dc_reference as D
import dcopf_reference as R

SEED_LANES, LANES = 65, 65
REFERENCE_LANES = (0, 63, 64)           # the lanes held against the restatement: the first, the last of group 0, the one alone in group 1
TIGHT = 3                           # ratings per grid that lie close to the flows of the table's dispatch
ACTIVE = 1e-3                       # a row counts as active with a multiplier above this x the largest nodal price

# name -> (family of dc_grids or case fixture, seed of the dressing)
GRIDS = {
    "two buses": ("two buses", 13),
    "path 40": ("path 40", 11),
    "star 71, leaf slack": ("star 71, leaf slack", 14),
    "star 33, hub slack": ("star 33, hub slack", 11),
    "binary tree 63": ("binary tree 63", 11),
    "two cliques": ("two cliques", 11),
    "mesh 8x8": ("mesh 8x8", 27),
    "ring 17": ("ring 17", 12),
    "case118": ("case118", 8),
}
LARGEST = "case118"


def _jg():
    return importlib.import_module("juliagrid.jl_amd")


def _table(source):
    if isinstance(source, dict):
        return {k: np.array(v) for k, v in source.items()}
    if source in G.FAMILIES:
        return G.family(source, _jg())
    with np.load(os.path.join(R.GOLDEN, "cases", source + ".npz")) as z:
        return {k: z[k] for k in z.files}


def dressed_table(source, seed):
    """The table with a second unit at the bus of a seeded existing unit (the two share the first one's output) and the slack's first unit balancing
    the demand, and the generator drawn."""
    t = _table(source)
    rng = np.random.default_rng(seed)
    ng = t["gen_bus"].size
    on = np.flatnonzero(np.asarray(t["gen_status"]) == 1)
    k = int(rng.choice(on))
    for name in [key for key in t if key.startswith("gen_") and np.ndim(t[key]) >= 1 and np.shape(t[key])[0] == ng and not key.startswith("gen_cost")]:
        t[name] = np.concatenate((t[name], t[name][k:k + 1]))
    t["gen_pg"] = np.asarray(t["gen_pg"], dtype=np.float64).copy()
    t["gen_pg"][k] *= 0.5
    t["gen_pg"][ng] = t["gen_pg"][k]
    slack = D.slack_of(t)
    at = np.flatnonzero((np.asarray(t["gen_bus"]) - 1 == slack) & (np.asarray(t["gen_status"]) == 1))
    live = np.asarray(t["gen_status"]) == 1
    need = float(np.sum(t["bus_pd"]) + np.sum(t["bus_gs"]))                 # a DC grid has no losses; the shift powers sum to zero
    t["gen_pg"][at[0]] += need - float(t["gen_pg"][live].sum())
    return t, k, rng


def dress(source, seed):
    """The dressed PowerSystem (dcModel_ done).  Its `dressing` says what was put where."""
    jg = _jg()
    sysmod = importlib.import_module("juliagrid.jl_amd.system")
    t, twin_of, rng = dressed_table(source, seed)
    theta, flow = D.solve(t)
    s = jg.powerSystem(t)
    gen, br = s.generator, s.branch
    demand = float(np.sum(t["bus_pd"]))
    units = np.flatnonzero(gen.layout.status == 1)
    pg = np.asarray(t["gen_pg"], dtype=np.float64)
    assert np.all(pg[units] >= 0.0), "the table's dispatch has a negative output"
    # capacities: above the table's dispatch, about twice the demand in all
    cap = np.zeros(gen.number)
    cap[units] = rng.uniform(1.7, 2.3, units.size) * pg[units] + 0.1 * demand / units.size
    for j, k in enumerate(units):
        k = int(k)
        jg.updateGeneratorSystem_(s, k + 1, minActive=0.0, maxActive=float(cap[k]))
        if j % 3 == 2:                                                      # four points, convex: slopes ascending
            x = cap[k] * np.array([0.0, 0.3, 0.7, 1.0])
            slope = np.sort(rng.uniform(8.0, 45.0, 3))
            y = np.r_[0.0, np.cumsum(slope * np.diff(x))] + rng.uniform(0.0, 5.0)
            sysmod.cost_(s, k + 1, piecewise=np.stack((x, y), axis=1))
        else:
            sysmod.cost_(s, k + 1, polynomial=[rng.uniform(4.0, 30.0) / cap[k], rng.uniform(8.0, 40.0), rng.uniform(0.0, 5.0)])
    live = np.flatnonzero(br.layout.status == 1)
    fl = np.abs(np.asarray(flow, dtype=np.float64))
    diff = np.abs(theta[br.layout.from_ - 1] - theta[br.layout.to - 1])
    scale = max(float(fl[live].max()), 1e-6)
    rated = np.sort(rng.choice(live, size=max(1, int(round(0.4 * live.size))), replace=False))
    tight = set(rng.choice(rated, size=min(TIGHT, rated.size), replace=False).tolist())
    for k in rated:                                                         # a few close to the table's flows, the others well above them
        f = rng.uniform(1.08, 1.4) if int(k) in tight else rng.uniform(1.8, 3.0)
        jg.updateBranchSystem_(s, int(k) + 1, rating=float(f * fl[k] + 0.02 * scale))
    rest = np.array([k for k in live if k not in set(rated.tolist())], dtype=np.int64)
    angled = np.zeros(0, dtype=np.int64)
    if rest.size:
        heavy = rest[np.argsort(-diff[rest], kind="stable")][:max(1, rest.size // 2)]        # where a limit can bind
        angled = np.sort(rng.choice(heavy, size=min(3, heavy.size), replace=False))
        for k in angled:
            lim = float(rng.uniform(1.08, 1.3) * diff[k] + 1e-3)
            jg.updateBranchSystem_(s, int(k) + 1, minDiffAngle=-lim, maxDiffAngle=lim)
    jg.dcModel_(s)
    s.dressing = NS(table=t, twin_of=twin_of + 1, twin=gen.number, rated=rated + 1, angled=angled + 1, capacity=cap)
    return s


_grids, _solved, _polished = {}, {}, {}


def grid(name):
    """(system, restatement model at the base demand), built once"""
    if name not in _grids:
        s = dress(*GRIDS[name])
        _grids[name] = (s, R.model(s))
    return _grids[name]


def lanes(name):
    f = np.random.default_rng(SEED_LANES + GRIDS[name][1]).uniform(0.85, 1.05, LANES)
    f[0] = 1.0
    return f


def lane_model(name, j):
    s, _ = grid(name)
    return R.model(s, demand=s.bus.demand.active * lanes(name)[j])


def solved(name, j=0, tolerance=1e-9):
    """The restatement's solution of lane j (rho = 0.1, not adapted), computed once"""
    key = (name, j, tolerance)
    if key not in _solved:
        md = lane_model(name, j)
        _solved[key] = (md, R.admm(md, adapt_every=0, tolerance=tolerance, iteration=6000 if tolerance == 1e-9 else 100000))
    return _solved[key]


# ---- the factor of K ----------------------------------------------------------------------------------------------------------------------------
def k_pattern(md):
    """CSR (= CSC: symmetric) of the pattern of A'A plus the diagonal, columns ascending"""
    S = sp.csr_matrix((md.A != 0).astype(np.int64))
    K = (S.T @ S + sp.identity(md.n, dtype=np.int64, format="csr")).tocsr()
    K.sort_indices()
    return K.indptr.astype(np.int64), K.indices.astype(np.int64)


def k_levels(md):
    """dc_grids.sweep_levels for the pattern of K: the analysis jg_dcopf_create asks for"""
    ptr, idx = k_pattern(md)
    plan = _jg()._lib.Plan(md.n, ptr, idx, policy=G.DC_POLICY_NO_TOP)
    l_ptr, l_col, u_ptr = plan.get("l_ptr"), plan.get("l_col"), plan.get("u_ptr")
    flev, blev = G._forward_levels(md.n, l_ptr, l_col), plan.get("bwd_level").astype(np.int64)
    fw, bw = np.bincount(flev, minlength=2)[1:], np.bincount(blev, minlength=2)[1:]
    return dict(forward=fw, backward=bw, forwardLaunches=G.launches(fw), backwardLaunches=G.launches(bw), lower=np.diff(l_ptr), upper=np.diff(u_ptr))


def k_classes(lv):
    """The four classes of dc_grids.COVERAGE the set has to reach on K, by the names of this module"""
    got = G.classes(lv)
    out = set()
    if any(c.startswith("forward wide level") for c in got):
        out.add("wide forward level")
    if any(c.startswith("backward wide level") for c in got):
        out.add("wide backward level")
    if any("chain level" in c for c in got):
        out.add("chain level")
    if "list of 64 or more terms" in got:
        out.add("list of 64 or more terms")
    if "backward launches chain, wide, chain" in got:
        out.add("backward launches chain, wide, chain")
    return out


# "wide backward level" is not in the list.  Over every family of dc_grids.FAMILIES up to 200 variables and case118, dressed, K's widest backward level
# has 16 rows or fewer (the tree: 15 or 16 by seed; case118: 13) except on "pegaseShaped 160" (194 variables, 22 rows), and there the restatement does
# not end within 6 000 iterations at rho = 0.1 under the seeds 1 .. 8 of this dressing: that grid stays out by the set's first condition -- DESIGN.md 3.23.1
K_COVERAGE = ("wide forward level", "chain level", "list of 64 or more terms")


# ---- the active set and the polish -----------------------------------------------------------------------------------------------------------------
def active(md, r, l=None, u=None):
    """(upper, lower): masks of the inequality rows active at their upper / lower bound -- a multiplier of that sign above 1e-9 of the largest and z
    on the bound -- plus the equality rows in `upper`"""
    l = md.l if l is None else l
    u = md.u if u is None else u
    top = np.abs(r.y).max()
    near = 1e-6 * max(1.0, np.abs(r.z).max())
    up = (~md.eq) & (r.y > 1e-9 * top) & (np.abs(r.z - u) <= near)
    lo = (~md.eq) & (r.y < -1e-9 * top) & (np.abs(r.z - l) <= near)
    return up | md.eq, lo


def polish(md, r, l=None, u=None):
    """x, y of  min 1/2 x'Px + q'x  s.t. the active rows at their bounds, by ONE dense solve of [[P, Aa'], [Aa, 0]]; y is zero off the set"""
    l = md.l if l is None else l
    u = md.u if u is None else u
    up, lo = active(md, r, l, u)
    rows = np.flatnonzero(up | lo)
    Aa = md.A[rows]
    b = np.where(up[rows], u[rows], l[rows])
    k = rows.size
    M = np.block([[np.diag(md.P), Aa.T], [Aa, np.zeros((k, k))]])
    sol = np.linalg.solve(M, np.r_[-md.q, b])
    y = np.zeros(md.m)
    y[rows] = sol[md.n:]
    x = sol[:md.n]
    return NS(x=x, y=y, z=md.A @ x, upper=up, lower=lo, rows=rows, objective=0.5 * x @ (md.P * x) + md.q @ x + md.constant)


def polished(name):
    if name not in _polished:
        md, r = solved(name)
        _polished[name] = polish(md, r)
    return _polished[name]


def distance(md, x, y, x2, y2):
    """(angles, outputs and helpers, nodal prices): largest differences"""
    b = md.kind == "balance"
    return np.array([np.abs(x[:md.buses] - x2[:md.buses]).max(), np.abs(x[md.buses:] - x2[md.buses:]).max(), np.abs(y[b] - y2[b]).max()])


def active_kinds(md, y):
    """Rows by kind with a multiplier above ACTIVE x the largest nodal price; capability rows at their upper limit only"""
    top = np.abs(y[md.kind == "balance"]).max()
    big = np.abs(y) > ACTIVE * top
    return {"flow": int((big & (md.kind == "flow")).sum()), "capability upper": int(((y > ACTIVE * top) & (md.kind == "capability")).sum()),
            "piecewise": int((big & (md.kind == "piecewise")).sum()), "angle": int((big & (md.kind == "angle")).sum())}


# ---- measured on the CPU by tools/dcopf_grids_measure.py (rho = 0.1, not adapted); move and polish over REFERENCE_LANES, certificate over all lanes ------------------------------------------------
# move: the restatement between tolerance 1e-9 and 1e-10 (angles, outputs and helpers, nodal prices, objective relative); certificate: R.kkt of the
# restatement, the worst over ALL 65 lanes, as the device test holds all 65 to it (bound, stationarity, complementarity, wrong side); polish: lane 0's restatement from the polished point (as move)
MEASURED = {
    "two buses": dict(move=(1.05e-10, 4.79e-08, 1.36e-07, 3.43e-09), certificate=(2.77e-08, 1.90e-07, 4.51e-08, 6.51e-17), polish=(1.28e-11, 3.53e-08, 1.75e-08, 3.70e-09)),
    "path 40": dict(move=(3.57e-08, 1.68e-07, 4.43e-07, 2.90e-09), certificate=(6.16e-08, 5.22e-10, 6.76e-08, 1.02e-17), polish=(3.19e-08, 1.51e-07, 3.96e-07, 2.75e-09)),
    "star 71, leaf slack": dict(move=(1.03e-08, 3.77e-07, 3.15e-07, 1.94e-08), certificate=(2.41e-07, 7.29e-09, 9.43e-06, 1.82e-18), polish=(1.06e-08, 3.74e-07, 3.24e-07, 1.88e-08)),
    "star 33, hub slack": dict(move=(3.32e-09, 1.03e-07, 4.01e-07, 7.59e-09), certificate=(8.27e-09, 4.71e-10, 3.24e-07, 1.26e-17), polish=(1.98e-09, 8.90e-08, 2.02e-07, 6.79e-09)),
    "binary tree 63": dict(move=(1.67e-08, 1.25e-07, 2.33e-07, 6.21e-09), certificate=(3.54e-09, 5.79e-10, 1.62e-07, 7.80e-18), polish=(1.68e-08, 1.32e-07, 1.67e-07, 6.56e-09)),
    "two cliques": dict(move=(1.75e-09, 3.53e-07, 1.73e-06, 2.39e-08), certificate=(4.33e-08, 1.79e-07, 1.34e-07, 3.13e-17), polish=(9.86e-10, 3.40e-08, 1.93e-06, 2.57e-08)),
    "mesh 8x8": dict(move=(1.76e-09, 8.52e-08, 2.78e-07, 1.10e-08), certificate=(9.32e-08, 1.81e-08, 1.36e-07, 1.44e-18), polish=(2.02e-09, 9.80e-08, 3.20e-07, 1.26e-08)),
    "ring 17": dict(move=(4.94e-09, 7.33e-09, 5.54e-07, 3.26e-09), certificate=(4.57e-09, 4.52e-10, 1.11e-07, 2.10e-17), polish=(5.20e-09, 7.71e-09, 5.83e-07, 3.04e-09)),
    "case118": dict(move=(8.37e-08, 2.81e-05, 2.81e-06, 1.02e-08), certificate=(3.83e-07, 8.17e-07, 1.11e-05, 2.43e-16), polish=(2.02e-08, 3.96e-06, 3.20e-06, 6.71e-09)),
}
WRONG_SIDE = 1e-11          # a multiplier on a side without a bound: the rounding of one multiplier step (tests/test_dcopf_host.py), not a measurement x 10


def bounds(name):
    """The device test's bounds: the measured figures x 10"""
    g = MEASURED[name]
    cert = tuple(10 * v for v in g["certificate"][:3]) + (WRONG_SIDE,)
    return NS(move=tuple(10 * v for v in g["move"]), certificate=cert, polish=tuple(10 * v for v in g["polish"]))
