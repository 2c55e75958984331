"""numpy restatement of a bridge candidate of the DC series and transfer screens solved on the slack's island (islands="shed"): what
tests/test_dc_series_shed_host.py holds against the rebuild route of tests/dc_island_reference.py, and what the GPU tests take their bridge lists from.

  adjacency(t)              in-service bus graph as lists (self-loops aside)
  split(t, k, adj)          (S mask [n], m, s) of in-service branch k by a SEARCH from both of its ends with k deleted, a step at a time on either side:
                            the two searches meet (None: k is no bridge) or one runs out of buses -- that side, or the other when it holds the slack,
                            is the side S that leaves; m is k's end on the slack's side, s = +1 / -1: m is the from / to end.  No DFS numbering, no
                            low-link: not the library's table
  bridges(t, adj)           {k: (S, m, s)} over the in-service branches
  unit_columns(t, ms)       z = B^-1 e_m on the UNSPLIT grid (slack row / column removed, the slack's own column 0) for the buses ms
  shed_flows(t, k, sp, z, F0)     f_l = F0[l] + y_l a_l' z s F0[k] for the branches with both ends on the slack's side, 0 for k and what left; F0 [branches]
                            or [branches, T]
  shed_sensitivity(...)     the same without the base flows' shift angle: g_l = G[l] + Z[l] s G[k]
  one_side(t, S, k)         the claim the device mask rests on: every in-service branch other than k with one end in S has both ends there
"""
import numpy as np
import scipy.sparse.linalg as sla

import dc_reference as R


def _ends(t):
    return np.asarray(t["br_from"]).astype(np.int64) - 1, np.asarray(t["br_to"]).astype(np.int64) - 1


def adjacency(t):
    f, to = _ends(t)
    on = np.asarray(t["br_status"]).astype(np.int64) == 1
    adj = [[] for _ in range(t["bus_type"].size)]
    for k in np.flatnonzero(on & (f != to)):
        adj[f[k]].append((int(to[k]), int(k)))
        adj[to[k]].append((int(f[k]), int(k)))
    return adj


def split(t, k, adj=None):
    adj = adjacency(t) if adj is None else adj
    f, to = _ends(t)
    a, b = int(f[k]), int(to[k])
    if a == b or int(np.asarray(t["br_status"])[k]) != 1:
        return None
    seen = [{a}, {b}]
    front = [[a], [b]]
    side = 0
    while front[0] and front[1]:
        nxt = []
        for v in front[side]:
            for u, e in adj[v]:
                if e == k or u in seen[side]:
                    continue
                if u in seen[1 - side]:
                    return None                                    # the searches met: a way round k
                seen[side].add(u)
                nxt.append(u)
        front[side] = nxt
        side = 1 - side
    done = 0 if not front[0] else 1                               # this side ran out of buses: it is complete
    slack = R.slack_of(t)
    if slack in seen[done]:                                        # the slack's side is complete: finish the search of the other one, which leaves
        done = 1 - done
        while front[done]:
            nxt = []
            for v in front[done]:
                for u, e in adj[v]:
                    if e != k and u not in seen[done]:
                        seen[done].add(u)
                        nxt.append(u)
            front[done] = nxt
    S = np.zeros(t["bus_type"].size, dtype=bool)
    S[list(seen[done])] = True
    m = a if not S[a] else b
    return S, m, (1.0 if m == a else -1.0)


def bridges(t, adj=None):
    adj = adjacency(t) if adj is None else adj
    out = {}
    for k in np.flatnonzero(np.asarray(t["br_status"]).astype(np.int64) == 1):
        sp = split(t, int(k), adj)
        if sp is not None:
            out[int(k)] = sp
    return out


def unit_columns(t, ms):
    B, y, _ = R.assemble(t)
    n = t["bus_type"].size
    slack = R.slack_of(t)
    keep = np.r_[0:slack, slack + 1:n]
    lu = sla.splu(B[keep][:, keep].tocsc())
    ms = sorted(set(int(m) for m in ms))
    E = np.zeros((n, len(ms)))
    for j, m in enumerate(ms):
        if m != slack:
            E[m, j] = 1.0
    Z = np.zeros((n, len(ms)))
    if ms:
        Z[keep] = lu.solve(E[keep])
    return {m: Z[:, j] for j, m in enumerate(ms)}, y


def _gone(t, S, k):
    f, to = _ends(t)
    gone = S[f] | S[to]
    gone[k] = True
    return gone


def shed_sensitivity(t, k, sp, z, y, G):
    """G [branches] or [branches, T] on the unsplit grid -> the same with bridge k out and its side S shed"""
    S, _, s = sp
    f, to = _ends(t)
    Zk = y * (z[f] - z[to])
    g = s * G[k]
    out = G + (Zk[:, None] * g[None, :] if np.ndim(G) == 2 else Zk * g)
    out[_gone(t, S, k)] = 0.0
    return out


shed_flows = shed_sensitivity                                      # the base flows carry their shift angle already; the update has none


def one_side(t, S, k):
    f, to = _ends(t)
    on = (np.asarray(t["br_status"]).astype(np.int64) == 1) & (f != to)
    on[k] = False
    return bool(np.all(S[f[on]] == S[to[on]]))


def sample(t, count=32, seed=11, adj=None):
    """`count` seeded bridges of a large grid (0-based, ascending) with what leaves: {k: (S, m, s)}"""
    br = bridges(t, adj)
    pick = np.sort(np.random.default_rng(seed).choice(np.array(sorted(br)), count, replace=False))
    return {int(k): br[int(k)] for k in pick}, br
