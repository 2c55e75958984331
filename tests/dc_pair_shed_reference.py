"""A PAIR of DC outages of which one or both are bridges, solved on the island that keeps the slack (dcPairScreen(..., islands="shed")): the check of
tests/test_dc_pair_shed_host.py and tests/test_dc_pair_shed_gpu.py.  The reference's own loop has no answer here (solve! meets a singular matrix), so this
states the behaviour from first principles, in the style of tests/dc_island_reference.py:

  Grid(t)                    the branch table of a case as arrays, made once
  component(g, outs)         the buses the slack still reaches with the branches `outs` deleted, by a breadth-first SEARCH over adjacency lists (no DFS
                             numbering, not the library's table)
  rebuild(g, k, l)           the DC model REBUILT on that component alone (its buses, the in-service branches with both ends in it, k and l deleted), slack
                             row / column removed, scipy splu: (from [branches], component mask); 0 on k, l and every branch with an end outside.  It never
                             uses the identity the kernel solves these pairs by
  Restatement(t, cols)       numpy restatement of the table of csrc/jg_dc_pair.hpp on the UNSPLIT grid: Phi of the candidates `cols`, Z = y a' B^-1 e_m for
                             the bridges among them, g = s f0; .flows(i, j) -> (from or None: status 3, kind)
  kind(br, g, k, l)          "plain" (no bridge), "outside" (one bridge, the other branch stays), "inside" (one bridge, the other branch leaves with it),
                             "disjoint" / "nested" (two bridges), from the searched sides S of tests/dc_series_shed_reference.py
  joint_cut(g, k, l)         the pair splits the grid (a search with both deleted reaches fewer buses than the base search)
  hand_rating(t), sample(t, br, bridges, others, seed)
"""
from collections import deque

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

import dc_pair_reference as P
import dc_reference as R
import dc_series_shed_reference as H

SINGULAR = P.SINGULAR


class Grid:
    def __init__(self, t):
        self.t = t
        self.n = int(t["bus_type"].size)
        self.f = np.asarray(t["br_from"]).astype(np.int64) - 1
        self.to = np.asarray(t["br_to"]).astype(np.int64) - 1
        self.y = R.admittance(t)                                   # 0 on a branch out of service
        self.shift = np.asarray(t["br_shift"], dtype=np.float64)
        self.slack = R.slack_of(t)
        self.net = R.supply(t) - np.asarray(t["bus_pd"], dtype=np.float64) - np.asarray(t["bus_gs"], dtype=np.float64)
        self.adj = [[] for _ in range(self.n)]
        for k in np.flatnonzero((self.y != 0) & (self.f != self.to)):
            self.adj[self.f[k]].append((int(self.to[k]), int(k)))
            self.adj[self.to[k]].append((int(self.f[k]), int(k)))
        self.base = component(self, ())


def component(g, outs):
    """boolean [n]: True on the buses the slack reaches once the branches `outs` (0-based) are deleted"""
    outs = set(int(o) for o in outs)
    keep = np.zeros(g.n, dtype=bool)
    keep[g.slack] = True
    q = deque([g.slack])
    while q:
        v = q.popleft()
        for u, e in g.adj[v]:
            if e not in outs and not keep[u]:
                keep[u] = True
                q.append(u)
    return keep


def joint_cut(g, k, l):
    return int(component(g, (k, l)).sum()) < int(g.base.sum())


def rebuild(g, k, l=None):
    """(from [branches], component mask) with the branches k and l out of service, on the slack's component alone"""
    outs = [o for o in (k, l) if o is not None]
    keep = component(g, outs)
    y = np.where(keep[g.f] & keep[g.to], g.y, 0.0)                 # the model of the component: a branch with an end outside is not in it
    y[outs] = 0.0
    idx = np.flatnonzero(keep)
    pos = np.full(g.n, -1)
    pos[idx] = np.arange(idx.size)
    live = np.flatnonzero(y != 0)
    ff, tt, yy = pos[g.f[live]], pos[g.to[live]], y[live]
    B = sp.coo_matrix((np.r_[yy, yy, -yy, -yy], (np.r_[ff, tt, ff, tt], np.r_[ff, tt, tt, ff])), shape=(idx.size, idx.size)).tocsc()
    psh = np.zeros(idx.size)
    np.add.at(psh, ff, -g.shift[live] * yy)
    np.add.at(psh, tt, g.shift[live] * yy)
    rhs = g.net[idx] - psh
    rest = np.flatnonzero(idx != g.slack)
    x = np.zeros(idx.size)
    if rest.size:
        x[rest] = sla.splu(B[rest][:, rest].tocsc()).solve(rhs[rest])
    th = np.zeros(g.n)
    th[idx] = x
    fr = np.zeros(g.f.size)
    fr[live] = y[live] * (th[g.f[live]] - th[g.to[live]] - g.shift[live])
    return fr, keep


def kind(br, g, k, l):
    bk, bl = k in br, l in br
    if not bk and not bl:
        return "plain"
    if bk and bl:
        Sk, Sl = br[k][0], br[l][0]
        return "nested" if (not (Sk & ~Sl).any() or not (Sl & ~Sk).any()) else "disjoint"
    b, o = (k, l) if bk else (l, k)
    S = br[b][0]
    return "inside" if (S[g.f[o]] and S[g.to[o]]) else "outside"


class Restatement:
    """the table of csrc/jg_dc_pair.hpp for the candidates `cols` (0-based branches); `br` = {bridge: (S, m, s)} of tests/dc_series_shed_reference.py"""

    def __init__(self, t, cols, br=None, g=None):
        self.g = Grid(t) if g is None else g
        self.cols = [int(c) for c in cols]
        self.br = H.bridges(t) if br is None else br
        self.Phi, self.f0, y = P.sensitivities(t, self.cols)
        z, _ = H.unit_columns(t, [self.br[c][1] for c in self.cols if c in self.br])
        self.gk = {}
        for i, c in enumerate(self.cols):                         # a bridge's column holds Z[:,c] = y a' B^-1 e_m, as the shed build writes it
            if c in self.br:
                _, m, s = self.br[c]
                self.Phi[:, i] = y * (z[m][self.g.f] - z[m][self.g.to])
                self.gk[c] = s * self.f0[c]

    def gone(self, k, l):
        """the branches that carry 0: k, l and every branch with an end in what left"""
        S = np.zeros(self.g.n, dtype=bool)
        for c in (k, l):
            if c in self.br:
                S |= self.br[c][0]
        out = S[self.g.f] | S[self.g.to]
        out[[k, l]] = True
        return out, S

    def flows(self, i, j):
        k, l = self.cols[i], self.cols[j]
        kd = kind(self.br, self.g, k, l)
        P_, f0 = self.Phi, self.f0
        if kd == "plain":
            fr, _ = P.pair_flows(P_, f0, self.cols, i, j)
            return fr, kd
        if kd in ("disjoint", "nested"):
            ck, cl = self.gk[k], self.gk[l]
            if kd == "nested":
                if not (self.br[k][0] & ~self.br[l][0]).any():     # k's side inside l's
                    ck = 0.0
                else:
                    cl = 0.0
        else:
            bi, oi = (i, j) if k in self.br else (j, i)
            b, o = self.cols[bi], self.cols[oi]
            cb, co = self.gk[b], 0.0
            if kd == "outside":
                den = 1.0 - P_[o, oi]
                if abs(den) < SINGULAR:
                    return None, kd
                co = (f0[o] + P_[o, bi] * cb) / den
            ck, cl = (cb, co) if bi == i else (co, cb)
        fr = f0 + P_[:, i] * ck + P_[:, j] * cl
        fr[self.gone(k, l)[0]] = 0.0
        return fr, kd


def hand_rating(t):
    """ratings at the scale of each branch's own base flow (so that the worst branch differs from pair to pair), every seventh branch not rated"""
    r = 0.05 + 1.2 * np.abs(R.solve(t)[1])
    r[::7] = 0.0
    return r


def sample(t, br, bridges, others, seed=5):
    """0-based candidates, ascending: `bridges` seeded bridges (None: all of them) and `others` seeded in-service non-bridges (self-loops aside)"""
    rng = np.random.default_rng(seed)
    f, to = H._ends(t)
    on = np.flatnonzero((np.asarray(t["br_status"]).astype(np.int64) == 1) & (f != to))
    b = np.array(sorted(br), dtype=np.int64)
    o = np.array([k for k in on if int(k) not in br], dtype=np.int64)
    if bridges is not None:
        b = rng.choice(b, bridges, replace=False)
    o = rng.choice(o, min(others, o.size), replace=False)
    return np.sort(np.r_[b, o])
