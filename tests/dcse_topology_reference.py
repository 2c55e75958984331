"""Dense numpy restatement of the branch status tests (dcTopologyScreen, csrc/jg_dcse_topology.hip), the check of tests/test_dcse_topology_host.py and
tests/test_dcse_topology_gpu.py, built on tests/dcse_reference.py (matrices, rows, gain, full_set, meters) and tests/dc_reference.py.

  columns(t, ms)            m_k of every branch from the meter table, [rows, branches]: +1 from-end wattmeters of k and injection wattmeters on from(k),
                            -1 to-end wattmeters and injection wattmeters on to(k), 0 on PMUs and rows out of service
  Dense(t, ms)              H, W, a DENSE INVERSE of the gain and the columns, kept for several calls:
    .screen(cand)           D_k = m' W m - g' G^-1 g, N_k = m' W m, status 0 / 1 / 2 -- never the library's blocks of 512 candidates on a sparse factor
    .statistics(Z, cand)    r = z - H theta^ with the angles relative to the slack, c = m' W r, t = c / sqrt(D), phi = c / D, [candidates, lanes]
    .augmented(z, k)        independently of those formulas: numpy.linalg.lstsq on [sqrt(W) H, sqrt(W) m_k] -> phi, theta', the drop of the objective
  fixture(name)             the measurement sets of the tests; readings(fx, toggle) the exact readings of the grid with one branch status flipped

Rows, branches and lanes are 0-based here; angles carry the slack's angle as analysis.voltage.angle does.
"""
from types import SimpleNamespace as NS

import numpy as np

import dc_grids
import dc_reference as R
import dcse_critical_reference as C
import dcse_reference as S

SINGULAR = 1e-6                  # DCSE_SINGULAR, csrc/jg_dcse.hpp


def columns(t, ms):
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    m = ms.w_index.size + int(np.sum(ms.p_bus))
    M = np.zeros((m, f.size))
    for r in range(ms.w_index.size):
        if not ms.w_status[r]:
            continue
        j = int(ms.w_index[r]) - 1
        if ms.w_kind[r] == 0:
            M[r, (f == j) & (to != j)] += 1.0
            M[r, (to == j) & (f != j)] -= 1.0
        else:
            M[r, j] = 1.0 if ms.w_kind[r] == 1 else -1.0
    return M


class Dense:
    def __init__(self, t, ms):
        H, w, _, self.slack = S.matrices(t, ms)
        self.status = np.asarray(S.rows(t, ms)[1], dtype=np.float64)
        self.H, self.w = H.toarray(), w * self.status
        self.Gi = np.linalg.inv(S.gain(t, ms).toarray())
        self.M = columns(t, ms)
        self.va = float(np.asarray(t["bus_va"], dtype=np.float64)[self.slack])

    def screen(self, cand):
        Mk = self.M[:, cand]
        g = self.H.T @ (self.w[:, None] * Mk)
        self.X = self.Gi @ g                                           # x_k = G^-1 H' W m_k, [n, candidates]
        norm = (self.w[:, None] * Mk * Mk).sum(axis=0)
        D = norm - (g * self.X).sum(axis=0)
        status = np.where(norm == 0.0, 2, np.where(D > SINGULAR * norm, 0, 1))
        return NS(D=D, norm=norm, status=status, cand=np.asarray(cand))

    def estimate(self, Z):
        """theta^ [lanes, n] relative to the slack, residuals [lanes, m]; Z = se.mean per lane"""
        Z = np.atleast_2d(Z) * self.status[None, :]
        th = (self.Gi @ (self.H.T @ (self.w[:, None] * Z.T))).T
        th[:, self.slack] = 0.0
        return th, Z - th @ self.H.T

    def statistics(self, Z, sc):
        th, r = self.estimate(Z)
        c = (self.w[:, None] * self.M[:, sc.cand]).T @ r.T            # [candidates, lanes]
        ok = sc.status == 0
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(ok[:, None], c / np.sqrt(np.where(ok, sc.D, 1.0))[:, None], np.nan)
            phi = np.where(ok[:, None], c / np.where(ok, sc.D, 1.0)[:, None], np.nan)
        return NS(t=t, phi=phi, theta=th + self.va, residual=r, objective=(self.w[None, :] * r * r).sum(axis=1))

    def corrected(self, st, sc, q, lane):
        """theta^ - x_k phi^ for candidate position q in lane `lane` (screen(sc.cand) came last)"""
        th = st.theta[lane] - self.X[:, q] * st.phi[q, lane]
        th[self.slack] = self.va
        return th

    def augmented(self, z, k):
        """(phi, theta' with the slack's angle, drop of the objective) of branch k for ONE lane by least squares on the widened matrix"""
        z = np.asarray(z, dtype=np.float64) * self.status
        keep = np.r_[0:self.slack, self.slack + 1:self.H.shape[1]]
        sw = np.sqrt(self.w)
        A = sw[:, None] * np.c_[self.H[:, keep], self.M[:, k]]
        sol, _, rank, _ = np.linalg.lstsq(A, sw * z, rcond=None)
        assert rank == A.shape[1], (k, rank, A.shape)
        r1 = sw * z - A @ sol
        A0 = A[:, :-1]
        r0 = sw * z - A0 @ np.linalg.lstsq(A0, sw * z, rcond=None)[0]
        th = np.zeros(self.H.shape[1])
        th[keep] = sol[:-1]
        return float(sol[-1]), th + self.va, float(r0 @ r0 - r1 @ r1)


# ---- the measurement sets of the tests -------------------------------------------------------------------------------------------------------------
def _fixture(t, keep_w, keep_p, off_rows, batch, cand=None, var=(1e-2, 1e-5)):
    th, _ = R.solve(t)
    ms = C._subset(S.full_set(t, th, *var), keep_w, keep_p)
    ms.w_status[list(off_rows)] = 0
    _, status, variance, _, off, _ = S.rows(t, ms)
    nbr = np.asarray(t["br_from"]).size
    return NS(t=t, ms=ms, keep_w=keep_w, keep_p=keep_p, off_rows=list(off_rows), status=status.astype(np.float64), sigma=np.sqrt(variance), off=off, var=var,
              cand=np.arange(nbr) if cand is None else np.asarray(cand), batch=batch)


def _case14(load_case, slack_angle, batch):
    """the construction of dcse_critical_reference.thinned_case14 (the leaf, bus 8, keeps only the two wattmeters of its branch: a critical branch; bus
    `lonely` keeps only its PMU), with the slack's angle as given and branch 4 out of service in the model"""
    t = dict(load_case("case14"))
    t["bus_va"] = np.asarray(t["bus_va"], dtype=np.float64).copy()
    t["bus_va"][R.slack_of(t)] = slack_angle
    t["br_status"] = np.asarray(t["br_status"]).copy()
    t["br_status"][3] = 0
    th, _ = R.solve(t)
    full = S.full_set(t, th)
    n = t["bus_type"].size
    f, to = np.asarray(t["br_from"]).astype(int) - 1, np.asarray(t["br_to"]).astype(int) - 1
    leaf, = C._leaves(t)
    keep_w, keep_p = C._plan(t, full, pair_leaf=leaf)
    deg = np.bincount(np.r_[f, to], minlength=n)
    lonely = next(int(b) for b in np.argsort(deg, kind="stable") if b not in leaf[:2] and b != R.slack_of(t) and deg[b] == 2)
    for k in np.flatnonzero((f == lonely) | (to == lonely)):
        keep_w[[n + 2 * k, n + 2 * k + 1, int(f[k] if to[k] == lonely else to[k])]] = False
    keep_w[lonely] = False
    return _fixture(t, keep_w, keep_p, [3], batch)


def _case118(load_case):
    t = dict(load_case("case118"))
    t["br_status"] = np.asarray(t["br_status"]).copy()
    t["br_status"][10] = 0
    n, nb = t["bus_type"].size, np.asarray(t["br_from"]).size
    return _fixture(t, np.ones(n + 2 * nb, dtype=bool), np.ones(n, dtype=bool), [40], 70)


def _seeded(name, seed, share_w, share_p, batch, slack_angle=0.0, leaves_without_pmu=0, var=(1e-2, 1e-5), switch_off=0):
    """a grid of tests/dc_grids.py with a randomly thinned full set (dcse_critical_reference.seeded_grid's rule); `leaves_without_pmu`: that many
    leaves lose their PMU whatever the draw, so that their only branch is a critical branch"""
    t = dc_grids.family(name)
    t["bus_va"][R.slack_of(t)] = slack_angle
    ends = [tuple(sorted(p)) for p in zip(t["br_from"].tolist(), t["br_to"].tolist())]
    twin = [k for k, p in enumerate(ends) if p in ends[:k]]          # the later circuit of a parallel pair: opening it islands nothing
    t["br_status"][twin[:switch_off]] = 0
    n, nb = t["bus_type"].size, np.asarray(t["br_from"]).size
    rng = np.random.default_rng(seed)
    keep_w = rng.random(n + 2 * nb) < share_w
    keep_p = rng.random(n) < share_p
    for b, _, _ in C._leaves(t)[:leaves_without_pmu]:
        keep_p[b] = False
    off = rng.choice(int(keep_w.sum()), size=2, replace=False)
    return _fixture(t, keep_w, keep_p, off, batch, var=var)


FIXTURES = {
    "case14": lambda lc: _case14(lc, 0.0, 5),
    "case14 slack": lambda lc: _case14(lc, -0.17, 1),
    "case118": _case118,
    # a PMU on every bus at 1e-9 against wattmeters at 1: the grid's stiffest branches (admittances up to 5 128) are otherwise within a decade of the limit
    "pegase777": lambda lc: _seeded("pegaseShaped 777", 21, 0.7, 1.0, 3, var=(1.0, 1e-9), switch_off=2),
    "mesh": lambda lc: _seeded("mesh 8x8", 5, 0.6, 0.2, 5, slack_angle=0.1),
    "comb": lambda lc: _seeded("comb 16 x 2", 3, 0.8, 0.3, 5, leaves_without_pmu=3),
}
_FX = {}


def fixture(name, load_case):
    """built once and shared; callers do not change it.  .dense, .screen: the restatement of the set and of all its candidates"""
    if name not in _FX:
        fx = FIXTURES[name](load_case)
        fx.name = name
        fx.dense = Dense(fx.t, fx.ms)
        fx.sc = fx.dense.screen(fx.cand)
        _FX[name] = fx
    return _FX[name]


def readings(fx, toggle=None):
    """se.mean [m] of one lane: the exact readings of the grid with branch `toggle` (0-based) flipped against the model, None where that islands the grid.
    The constants the model takes out of a reading (shift, shunt, the slack's angle) are the MODEL's"""
    t = {k: np.array(v) for k, v in fx.t.items()}
    if toggle is not None:
        t["br_status"][toggle] = 1 - t["br_status"][toggle]
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    on = np.asarray(t["br_status"]) == 1
    n = t["bus_type"].size
    graph = sp.coo_matrix((np.ones(int(on.sum())), (t["br_from"][on] - 1, t["br_to"][on] - 1)), shape=(n, n))
    if connected_components(graph, directed=False)[0] != 1:
        return None, None, None                                      # (the sparse solve does not always notice the singular matrix of an islanded grid)
    th, fl = R.solve(t)
    ms = C._subset(S.full_set(t, th, *fx.var), fx.keep_w, fx.keep_p)
    raw = np.r_[ms.w_mean, ms.p_angle[ms.p_bus]]
    return fx.status * (raw + fx.off), th, fl


def plantable(fx, in_service=True, count=2):
    """the testable branches (0-based) with the largest true flow whose flip does not island the grid: in service in the model (they open) or out of
    service (they close)"""
    st = np.asarray(fx.t["br_status"]).astype(int)
    pos = {int(k): q for q, k in enumerate(fx.cand)}
    out = []
    for k in np.flatnonzero(st == (1 if in_service else 0)):
        if int(k) not in pos or fx.sc.status[pos[int(k)]] != 0:
            continue
        z, th, fl = readings(fx, int(k))
        if z is None:
            continue
        base = R.solve(fx.t)[1] if in_service else fl                # the flow that disappears, or appears
        out.append((abs(float(base[k])), int(k)))
        if len(out) >= 12:
            break
    return [k for _, k in sorted(out, key=lambda p: (-p[0], p[1]))[:count]]


def lanes(fx, seed=3, scale=0.01):
    """Z [batch, m] and the lanes' roles: [("open", k), ("meter", row), ("clean", None), ("close", k), ("open", k2), then noise only] (a tree has
    no branch that can open); every lane carries
    seeded noise of `scale` sigma"""
    rng = np.random.default_rng(seed)
    opens, closes = plantable(fx, True, 2), plantable(fx, False, 1)
    plan = [("open", k) for k in opens[:1]] + [("meter", None), ("clean", None)] + [("close", k) for k in closes] + [("open", k) for k in opens[1:]]
    roles, Z = [], []
    for l in range(fx.batch):
        kind, k = plan[l] if l < len(plan) else ("clean", None)
        z = readings(fx, k if kind in ("open", "close") else None)[0].copy()
        z += fx.status * scale * fx.sigma * rng.standard_normal(z.size)
        if kind == "meter":
            k = int(np.flatnonzero(fx.status > 0)[len(z) // 3])
            z[k] += 30.0 * fx.sigma[k]
        roles.append((kind, k))
        Z.append(z)
    return np.array(Z), roles
