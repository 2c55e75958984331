"""AC grids for the Gauss-Seidel power flow (csrc/jg_gs.hip): the graph builders of tests/dc_grids.py dressed for AC -- the helper of
tests/test_gs_grids_host.py and tests/test_gs_grids_gpu.py.

  dress(t, seed, units, taps)   a table of dc_grids.table(..., units=0) made an AC one with a seeded generator: br_r a fraction of br_x, line charging on
                                some branches, taps != 1 on a few, bus_qd a fraction of bus_pd, a few shunts, units at the buses named (each with a
                                fixed share of the demand, the slack's takes the rest) and gen_vg in [0.98, 1.05].  The shift angles are table's own
  FAMILIES                      name -> builder of a table.  Small on purpose: Gauss-Seidel needs on the order of n^2 sweeps on a path.  Trees carry
                                parallel twins, so that outages that are no bridges exist on them
  kinds(t)                      per branch label, what an outage of it is: "twin", "slack", "off", "tap", "shift", "bridge" (a set of them)
  labels(t)                     the outage labels of a family, by one rule (below); 0, the base grid, comes first
  system(name)                  the family's PowerSystem with its AC model built (a new one per call)
  restated(name, limit)         the restatement's run of the family's lanes, one per label: (out, v), computed once, shared by the tests, read-only
  contraction(out)              per lane of a run of the restatement, the ratio of its last two mismatch maxima (NaN: not converged; 0: converged at
                                the first check, nothing was iterated)
"""
import functools

import numpy as np

import dc_grids as D
import gs_reference as R

TOL = 1e-8


def dress(t, seed, units=(), taps=None):
    rng = np.random.default_rng(seed)
    n, m = t["bus_type"].size, t["br_from"].size
    slack = int(np.flatnonzero(t["bus_type"] == 3)[0])
    on = np.flatnonzero(t["br_status"] == 1)
    t["br_r"] = rng.uniform(0.1, 0.4, m) * t["br_x"]
    t["br_b"] = np.where(rng.random(m) < 0.4, rng.uniform(0.01, 0.06, m), 0.0)
    tap = np.ones(m)
    if taps is None:
        taps = rng.choice(on, size=min(3, on.size), replace=False) if on.size else []
    for k in taps:
        tap[int(k)] = rng.choice([0.94, 0.97, 1.03, 1.06])
    t["br_tap"] = tap
    t["bus_qd"] = rng.uniform(0.2, 0.5, n) * t["bus_pd"]
    shunt = rng.choice(n, size=min(3, n), replace=False)
    t["bus_gs"][shunt] = rng.uniform(0.0, 0.02, shunt.size)
    t["bus_bs"][shunt] = rng.uniform(0.01, 0.1, shunt.size)
    ubus = np.array(sorted(int(b) for b in units), dtype=np.int64)
    assert slack not in ubus
    total = float(t["bus_pd"].sum())
    upg = np.full(ubus.size, total / (ubus.size + 2.0))
    t["bus_type"][ubus] = 2
    t["gen_bus"] = np.r_[slack, ubus].astype(np.int64) + 1
    ng = ubus.size + 1
    t["gen_pg"] = np.r_[total - upg.sum(), upg]
    t["gen_status"], t["gen_qg"] = np.ones(ng, dtype=np.int8), np.zeros(ng)
    t["gen_qmax"], t["gen_qmin"] = np.ones(ng), -np.ones(ng)
    t["gen_vg"] = rng.uniform(0.98, 1.05, ng)
    return t


def _made(n, edges, slack, seed, units=(), taps=None, load=1.0, **kw):
    def make(jg=None):
        t = D.table(n, edges, slack, seed, units=0, **kw)
        t["bus_pd"] *= load
        return dress(t, seed + 1000, units, taps)
    return make


def _pegase(n, nb, ng, seed):
    return lambda jg=None: D._jg(jg).pegaseShaped(n=n, nb=nb, ng=ng, seed=seed, load_scale=0.15)


def _ring(n):
    return D._path(n) + [(n - 1, 0)]


# edges listed twice are parallel twins; table's `off` appends out-of-service copies of seeded edges, `shifts` draws shift angles
FAMILIES = {
    "one bus": _made(1, [], 0, 21),                                                                       # npq == npv == 0, no branch
    "two buses, PQ": _made(2, [(0, 1), (0, 1)], 0, 22, off=1, taps=[1]),                                    # npv == 0
    "two buses, PV": _made(2, [(0, 1), (1, 0)], 1, 23, units=[0], off=1, shifts=1),                         # npq == 0, the slack is the last bus
    "star 33, hub slack": _made(33, D._star(33) + [(0, 7), (0, 7), (0, 20)], 0, 24, units=[3, 20, 31], off=1, shifts=2, taps=[6, 19, 33]),
    # the hub is the last bus and a demand bus: a row of 71 entries, its diagonal last; the slack is leaf 5
    "star 71, hub last": _made(71, [(70, i) for i in range(70)] + [(70, 5), (12, 70), (70, 40)], 5, 35, units=[12, 33, 60], off=1, shifts=2,
                               taps=[4, 70, 71], load=0.4),
    # the hub is bus 0 with a unit: a row of 40 entries, its diagonal first; the slack is the last bus
    "star 40, hub first PV": _made(40, D._star(40) + [(0, 39), (0, 17), (17, 0)], 39, 26, units=[0, 9, 17], off=1, shifts=2, taps=[38, 40]),
    "all PV ring 9": _made(9, _ring(9), 0, 27, units=range(1, 9), shifts=1),
    "all PQ mesh 4x4": _made(16, D._mesh(4, 4), 5, 28, shifts=2),
    "ring 12 with twins": _made(12, _ring(12) + [(0, 1), (6, 7)], 0, 29, units=[4, 9], off=1, shifts=2),
    "path 12": _made(12, D._path(12) + [(0, 1), (5, 6), (10, 11)], 0, 30, units=[7], off=1, shifts=1, taps=[5, 13]),
    "two cliques 5+6": _made(11, D._cliques(5, 6), 2, 31, units=[0, 8], shifts=2),
    "pegaseShaped 60": _pegase(60, 96, 10, 32),
}

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
def restated(name, limit):
    s = system(name)
    lab = labels(family(name))
    g = R.problem(s)
    yt, v, P, Q = R.lanes(g, len(lab), R.lane_values(s, lab))
    out = R.run(g, yt, v, P, Q, limit, TOL)
    for a in (v, out.iteration, out.status, out.before, *out.stop):
        a.flags.writeable = False
    return out, v


def _connected(n, f, to, keep):
    comp = np.arange(n)
    for a, b in zip(f[keep], to[keep]):
        ca, cb = comp[a], comp[b]
        if ca != cb:
            comp[comp == cb] = ca
    return np.unique(comp).size == 1


def kinds(t):
    """label -> set of what the branch is: a parallel "twin" (another in-service branch joins the same buses), at the "slack", "off" (out of service),
    with a "tap" != 1 or a "shift" != 0, a "bridge" (in service, and the in-service graph falls apart without it)"""
    n = t["bus_type"].size
    f, to, on = t["br_from"] - 1, t["br_to"] - 1, t["br_status"] == 1
    slack = int(np.flatnonzero(t["bus_type"] == 3)[0])
    out = {}
    for k in range(f.size):
        s = set()
        same = ((f == f[k]) & (to == to[k])) | ((f == to[k]) & (to == f[k]))
        same[k] = False
        if not on[k]:
            s.add("off")
        elif np.any(same & on):
            s.add("twin")
        if slack in (f[k], to[k]):
            s.add("slack")
        if t["br_tap"][k] != 1.0:
            s.add("tap")
        if t["br_shift"][k] != 0.0:
            s.add("shift")
        keep = on.copy()
        keep[k] = False
        if on[k] and not _connected(n, f, to, keep):
            s.add("bridge")
        out[k + 1] = s
    return out


def labels(t):
    """0 (the base grid), then by ONE rule for every family: up to four twins, the first in-service branch at the slack, every out-of-service copy, the
    first tapped and the first shifted branch in service, the first bridge if none of these is one, and the first three in-service branches that are
    nothing of the kind"""
    kd = kinds(t)
    first = lambda want, count=1: [k for k, s in kd.items() if want(s)][:count]
    pick = ([0] + first(lambda s: "twin" in s, 4) + first(lambda s: "slack" in s and "off" not in s) + first(lambda s: "off" in s, 99) +
            first(lambda s: "tap" in s and "off" not in s) + first(lambda s: "shift" in s and "off" not in s))
    if not any("bridge" in kd[k] for k in pick[1:]):
        pick += first(lambda s: "bridge" in s)
    return tuple(dict.fromkeys(pick + first(lambda s: not s, 3)))


def contraction(out):
    c = np.full(out.status.shape, np.nan)
    ok = out.status == 0
    with np.errstate(all="ignore"):
        c[ok] = np.where(np.isnan(out.before[ok]), 0.0, np.maximum(out.stop[0], out.stop[1])[ok] / out.before[ok])
    return c
