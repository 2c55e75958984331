"""What the DC generator-outage screen is held against (tests/test_dc_generator_host.py, tests/test_dc_generator_gpu.py): a numpy restatement of the
reference's user loop, one REBUILD per case -- never the sensitivities the library screens with.

  candidates(t)             0-based in-service generators whose loss leaves the slack bus an in-service unit (what generatorCandidates must give)
  pmax_of(t)                the units' maxActive: the table's gen_pmax, else 5 x the output (the reference's addGenerator! default)
  share_loss(lost, w, room) the capped re-sharing, unit by unit in plain loops: (take, shortfall)
  change(t, g, pickup, w)   (d [buses], take [generators], shortfall): the change of the net bus injections when unit g is lost.  "slack": -Pg at g's bus
                            (updateGenerator!(...; status = 0) takes Pg out of bus.supply.active; the slack's entry of a right-hand side is dropped, so
                            the slack picks it up).  "participation": the units still in service add their takes at their buses
  flows(t, g, k, ...)       from-end flows of the case: the table with the injections moved by `change`, branch k (0-based, or None) out of service, by
                            dc_reference.solve (rebuild, refactorise); shed=True: dc_island_reference.solve, the model of the slack's component alone
  expect(...)               every case of a screen: loading / branch / count [1 + K, G] (row 0: G-1), and the two guards of the comparison per case: `tie`
                            (the two largest loadings lie within 1e-9: the worst branch is not compared) and `near` (a loading lies within 1e-9 of the
                            threshold: counts and records are not compared)
  slack_generation(t, d)    the slack bus's generation after the change d, from the flows that leave it (power! of the reference)

Column sums.  Over ALL buses the changes of an outage balance, because the DC model has no losses: what the lost unit no longer injects is injected
somewhere else.  Written per outage g with A[:, g] the changes at the generator buses other than the slack:
    sum_b A[b, g] + (what the slack bus's own units take - Pg where g sits on the slack bus) + shortfall[g] = 0
so A's column sums are -shortfall - (the slack's share).  With slack pickup nothing is asked of any unit: shortfall = 0 and the slack's share is Pg.
"""
import numpy as np

import dc_island_reference as I
import dc_pair_reference as P
import dc_reference as R

TOL = 1e-9


def _gen(t):
    return np.asarray(t["gen_bus"]).astype(np.int64) - 1, np.asarray(t["gen_status"]).astype(np.int64) == 1, np.asarray(t["gen_pg"], dtype=np.float64)


def candidates(t):
    bus, on, _ = _gen(t)
    slack = R.slack_of(t)
    at_slack = [g for g in range(bus.size) if on[g] and bus[g] == slack]
    return np.array([g for g in range(bus.size) if on[g] and not (len(at_slack) == 1 and g == at_slack[0])], dtype=np.int64)


def pmax_of(t):
    return np.asarray(t["gen_pmax"], dtype=np.float64) if "gen_pmax" in t else 5.0 * np.asarray(t["gen_pg"], dtype=np.float64)


def share_loss(lost, w, room):
    take = [0.0] * len(w)
    live = [i for i in range(len(w)) if w[i] > 0]
    left = float(lost)
    while live and left != 0.0:
        total = sum(w[i] for i in live)
        capped = [i for i in live if left * w[i] / total > room[i]]
        if not capped:
            for i in live:
                take[i] = left * w[i] / total
            left = 0.0
            break
        for i in capped:
            take[i] = room[i]
            left -= room[i]
        live = [i for i in live if i not in capped]
    return np.array(take), left


def change(t, g, pickup="slack", weight=None):
    bus, on, pg = _gen(t)
    d = np.zeros(t["bus_type"].size)
    d[bus[g]] -= pg[g]
    take = np.zeros(bus.size)
    if pickup == "slack":
        return d, take, 0.0
    pmax = pmax_of(t)
    w = pmax if weight is None else np.asarray(weight, dtype=np.float64)
    rest = [u for u in range(bus.size) if on[u] and u != g]
    tk, short = share_loss(pg[g], [w[u] for u in rest], [max(pmax[u] - pg[u], 0.0) for u in rest])
    for u, v in zip(rest, tk):
        take[u] = v
        d[bus[u]] += v
    return d, take, short


def flows(t, d, k=None, shed=False):
    inj = R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64) + d
    if shed:
        return I.solve(t, out=k, injection=inj)[1]
    return R.solve(t, out=k, injection=inj)[1]


def slack_generation(t, d):
    slack = R.slack_of(t)
    fr = flows(t, d)
    f, to = np.asarray(t["br_from"]).astype(np.int64) - 1, np.asarray(t["br_to"]).astype(np.int64) - 1
    return float(fr[f == slack].sum() - fr[to == slack].sum() + t["bus_gs"][slack] + t["bus_pd"][slack])


def summary(fr, rating, thr, monitored=None):
    """(worst loading, its branch, count, tie, near) of one case"""
    w, b, load = P.loading(fr, rating, monitored)
    scale = max(1.0, w)
    top = np.sort(load)[-2:] if load.size > 1 else np.array([0.0, w])
    return w, b, int((load > thr).sum()), bool(top[1] - top[0] <= TOL * scale), bool((np.abs(load - thr) <= TOL * scale).any())


def expect(t, rating, gens, cands, thr, pickup="slack", weight=None, shed=False, monitored=None):
    """gens: 0-based generators; cands: 0-based branches (ascending).  Arrays [1 + K, G]; row 0 the G-1 cases"""
    K, G = len(cands), len(gens)
    out = dict(load=np.zeros((1 + K, G)), branch=np.zeros((1 + K, G), dtype=np.int64), count=np.zeros((1 + K, G), dtype=np.int64),
               tie=np.zeros((1 + K, G), dtype=bool), near=np.zeros((1 + K, G), dtype=bool), shortfall=np.zeros(G), slack=np.zeros(G), flow0=[])
    for j, g in enumerate(gens):
        d, _, out["shortfall"][j] = change(t, int(g), pickup, weight)
        for i, k in enumerate([None] + [int(k) for k in cands]):
            fr = flows(t, d, k, shed)
            if i == 0:
                out["flow0"].append(fr)
            out["load"][i, j], out["branch"][i, j], out["count"][i, j], out["tie"][i, j], out["near"][i, j] = summary(fr, rating, thr, monitored)
        out["slack"][j] = slack_generation(t, d)
    out["flow0"] = np.stack(out["flow0"], axis=1)
    return out


def excluded_share(e):
    """the share of the cases one of the two guards takes out of a comparison"""
    return float((e["tie"] | e["near"]).mean())


def records(e, labels_k, thr):
    """the record list the expectation implies, sorted by (k, g) with row 0 (label 0) first: rows (label k, g, branch, loading, count)"""
    lab = np.r_[0, labels_k]
    return np.array([(lab[i], j, e["branch"][i, j], e["load"][i, j], e["count"][i, j]) for i in range(lab.size) for j in range(e["load"].shape[1])
                     if e["load"][i, j] > thr], dtype=np.float64).reshape(-1, 5)


def with_generators(t, buses, pg, pmax=None, status=None):
    """a copy of the table with generators appended at `buses` (1-based bus indices)"""
    t2 = {k: np.array(v) for k, v in t.items()}
    m = len(buses)
    if "gen_pmax" not in t2:
        t2["gen_pmax"] = pmax_of(t)
    add = dict(gen_bus=np.asarray(buses), gen_pg=np.asarray(pg, dtype=np.float64), gen_status=np.ones(m) if status is None else np.asarray(status),
               gen_qg=np.zeros(m), gen_vg=np.ones(m), gen_qmax=np.ones(m), gen_qmin=-np.ones(m),
               gen_pmax=5.0 * np.asarray(pg, dtype=np.float64) if pmax is None else np.asarray(pmax, dtype=np.float64))
    for k, v in add.items():
        t2[k] = np.concatenate([t2[k], v.astype(t2[k].dtype)])
    return t2


def with_feeder(t, at, pg, x=0.1):
    """a copy of the table with one new bus hung on bus `at` (1-based) by a single branch -- a bridge -- and a generator of output `pg` on the new bus"""
    t2 = {k: np.array(v) for k, v in t.items()}
    n = t2["bus_type"].size
    one = dict(bus_type=2, bus_pd=0.02, bus_qd=0.0, bus_gs=0.0, bus_bs=0.0, bus_vm=1.0, bus_va=0.0)
    if "bus_label" in t2:
        one["bus_label"] = int(np.max(t2["bus_label"])) + 1
    for k, v in one.items():
        t2[k] = np.concatenate([t2[k], np.array([v]).astype(t2[k].dtype)])
    for k, v in dict(br_from=at, br_to=n + 1, br_status=1, br_r=0.0, br_x=x, br_g=0.0, br_b=0.0, br_tap=1.0, br_shift=0.0).items():
        t2[k] = np.concatenate([t2[k], np.array([v]).astype(t2[k].dtype)])
    return with_generators(t2, [n + 1], [pg])
