"""numpy / scipy restatement of a DC outage that splits the grid, solved on the island that keeps the slack: the check of tests/test_dc_island_host.py and
tests/test_dc_island_gpu.py.  The reference itself has no answer here (its solve! meets a singular matrix), so this states the behaviour from first
principles, in the style of tests/dc_reference.py:

  component(t, out)      the buses the slack still reaches with branch `out` deleted, by a breadth-first SEARCH of the in-service graph (no DFS numbering)
  solve(t, out, ...)     the DC model REBUILT on that component alone (its buses, the in-service branches with both ends in it, `out` deleted), slack
                         row / column removed, scipy splu; NaN angles outside the component, flows 0 on `out` and on every branch with an end outside
  shed(t, out, ...)      what left: buses, the right-hand side, demand and supply summed over them
  power(t, th, fr, ...)  injection / supply / generator of power!(analysis) on the component, NaN on what left

It never uses the identity the library solves these lanes by (theta_M = x_M + g z_M on the ONE factor of the whole grid).
`t` is a table dict of tests/conftest.py: load_case; hand_grid() builds the 200-bus grid of the tests.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
import scipy.sparse.linalg as sla

import dc_reference as R


def _ends(t):
    return np.asarray(t["br_from"]).astype(np.int64) - 1, np.asarray(t["br_to"]).astype(np.int64) - 1


def component(t, out=None):
    """boolean [n]: True on the buses of the slack's component once branch `out` (0-based, or None) is deleted"""
    n = t["bus_type"].size
    f, to = _ends(t)
    on = np.asarray(t["br_status"]).astype(np.int64) == 1
    if out is not None:
        on[out] = False
    g = sp.coo_matrix((np.ones(int(on.sum())), (f[on], to[on])), shape=(n, n)).tocsr()
    order = csg.breadth_first_order(g, R.slack_of(t), directed=False, return_predecessors=False)
    keep = np.zeros(n, dtype=bool)
    keep[order] = True
    return keep


def solve(t, out=None, injection=None):
    """theta [n] (NaN outside the slack's component), from [branches] (0 on `out` and on branches that touch what left), the component mask"""
    n = t["bus_type"].size
    f, to = _ends(t)
    keep = component(t, out)
    slack = R.slack_of(t)
    shift = np.asarray(t["br_shift"], dtype=np.float64)
    y = R.admittance(t, out)
    y = np.where(keep[f] & keep[to], y, 0.0)                       # the model of the component: branches with an end outside are not in it
    idx = np.flatnonzero(keep)
    pos = np.full(n, -1)
    pos[idx] = np.arange(idx.size)
    live = np.flatnonzero(y != 0)
    ff, tt, yy = pos[f[live]], pos[to[live]], y[live]
    B = sp.coo_matrix((np.r_[yy, yy, -yy, -yy], (np.r_[ff, tt, ff, tt], np.r_[ff, tt, tt, ff])), shape=(idx.size, idx.size)).tocsc()
    psh = np.zeros(idx.size)
    np.add.at(psh, ff, -shift[live] * yy)
    np.add.at(psh, tt, shift[live] * yy)
    net = (R.supply(t) - t["bus_pd"]) if injection is None else np.asarray(injection, dtype=np.float64)
    rhs = (net - t["bus_gs"])[idx] - psh
    rest = np.flatnonzero(idx != slack)
    x = np.zeros(idx.size)
    if rest.size:
        x[rest] = sla.splu(B[rest][:, rest].tocsc()).solve(rhs[rest])
    th = np.full(n, np.nan)
    th[idx] = x + np.asarray(t["bus_va"], dtype=np.float64)[slack]
    fr = np.zeros(f.size)
    fr[live] = y[live] * (th[f[live]] - th[to[live]] - shift[live])
    return th, fr, keep


def shed(t, out, injection=None, keep=None):
    """dict(buses, injection, demand, supply) of what branch `out` takes with it: the count and the sums over the buses outside the slack's component;
    injection is the right-hand side of the UNSPLIT model, supply - demand (or the lane's own net injection) - shunt conductance - shiftPower"""
    gone = ~(component(t, out) if keep is None else keep)
    _, _, psh = R.assemble(t)
    rhs = R.rhs_of(t, psh, injection)
    return dict(buses=int(gone.sum()), injection=float(rhs[gone].sum()), demand=float(np.asarray(t["bus_pd"])[gone].sum()), supply=float(R.supply(t)[gone].sum()))


def power(t, th, fr, keep, injection=None):
    """injection / supply / generator on the slack's component (the slack's from the flows that leave it), NaN on the buses that left"""
    f, to = _ends(t)
    slack = R.slack_of(t)
    sup = R.supply(t)
    inj = (sup - t["bus_pd"]) if injection is None else np.asarray(injection, dtype=np.float64).copy()
    inj[slack] = fr[f == slack].sum() - fr[to == slack].sum() + t["bus_gs"][slack]
    sup = sup.copy()
    sup[slack] = t["bus_pd"][slack] + inj[slack]
    gen_bus = np.asarray(t["gen_bus"]).astype(np.int64) - 1
    on = np.asarray(t["gen_status"]) == 1
    pg = np.asarray(t["gen_pg"], dtype=np.float64)
    g = np.where(on, pg, 0.0)
    at_slack = [k for k in range(gen_bus.size) if on[k] and gen_bus[k] == slack]
    if at_slack:
        g[at_slack[0]] = inj[slack] + t["bus_pd"][slack] - sum(pg[k] for k in at_slack[1:])
    inj[~keep] = np.nan
    sup[~keep] = np.nan
    g[on & ~keep[gen_bus]] = np.nan
    return dict(injection=inj, supply=sup, generator=g)


def worst(a, ref, keep):
    """tests/dc_reference.py: worst on the entries of the slack's component, the scaling and bound of tests/test_dc_gpu.py"""
    return R.worst(np.asarray(a)[keep], np.asarray(ref)[keep])


def hand_grid(seed=11):
    """A 200-bus grid built for the island lanes, bus numbers shuffled so that no side of a bridge is a run of bus indices.  In construction order
    (before the shuffle; `marks` names the branches, 0-based):
      core        buses 0 .. 99, a ring with 40 chords; the slack is bus 0; a phase shifter on a ring branch
      at_slack    bridge slack -> 100, one bus behind it: m is the slack, S is one bus
      pocket      buses 101 .. 185 (85 buses: more than a lane group) as a ring with 30 chords and a phase shifter inside, hung on core bus 10 by a
                  bridge that is itself a phase shifter and runs FROM the pocket TO the core: m is the to-end
      chain       core bus 20 -> 186 -> 187: two nested bridges (S of two buses, and of one), m the from-end
      doubled     core bus 30 = 188 by TWO parallel branches (neither is a bridge), then the bridge 188 -> 189
      open_loop   189 - core bus 31, OUT of service: in service it would close a loop and 188 -> 189 would be no bridge
      far         core bus 50 -> 190 .. 199, a path of ten bridges
    Loads on every bus, generators scattered over the core and the parts that leave; the slack's angle is not zero."""
    rng = np.random.default_rng(seed)
    n = 200
    br, marks = [], {}

    def add(a, b, shift=0.0, status=1, name=None):
        br.append((a, b, 0.02 + 0.2 * rng.random(), 1.0 if rng.random() < 0.7 else 0.95 + 0.1 * rng.random(), shift, status))
        if name:
            marks.setdefault(name, []).append(len(br) - 1)

    for i in range(100):
        add(i, (i + 1) % 100, shift=0.04 if i == 40 else 0.0, name="core_shifter" if i == 40 else None)
    for _ in range(40):
        a, b = rng.choice(100, 2, replace=False)
        add(int(a), int(b))
    add(0, 100, name="at_slack")
    for i in range(101, 186):
        add(i, 101 + (i - 101 + 1) % 85, shift=-0.03 if i == 120 else 0.0, name="pocket_shifter" if i == 120 else None)
    for _ in range(30):
        a, b = rng.choice(85, 2, replace=False)
        add(101 + int(a), 101 + int(b))
    add(130, 10, shift=0.05, name="pocket")
    add(20, 186, name="chain")
    add(186, 187, name="chain")
    add(30, 188, name="doubled")
    add(30, 188, name="doubled")
    add(188, 189, name="behind_doubled")
    add(189, 31, status=0, name="open_loop")
    prev = 50
    for i in range(190, 200):
        add(prev, i, name="far")
        prev = i
    perm = rng.permutation(n)                                      # construction bus -> bus index of the table
    z = np.zeros(n)
    pd = 0.05 + 0.1 * rng.random(n)
    gens = np.r_[rng.choice(100, 12, replace=False), [0, 100, 110, 150, 187, 189, 195]]
    pg = 0.5 + rng.random(gens.size)
    bt = np.ones(n, dtype=np.int8)
    bt[gens] = 2
    bt[0] = 3
    inv = np.argsort(perm)                                         # table bus -> construction bus
    a = np.array(br, dtype=np.float64)
    t = dict(base_power=np.array([1e8]), bus_type=bt[inv], bus_pd=pd[inv], bus_qd=z.copy(), bus_gs=(0.01 * rng.random(n))[inv], bus_bs=z.copy(),
             bus_vm=np.ones(n), bus_va=np.full(n, 0.1), br_from=perm[a[:, 0].astype(np.int64)] + 1, br_to=perm[a[:, 1].astype(np.int64)] + 1,
             br_status=a[:, 5].astype(np.int8), br_r=np.zeros(len(br)), br_x=a[:, 2].copy(), br_g=np.zeros(len(br)), br_b=np.zeros(len(br)),
             br_tap=a[:, 3].copy(), br_shift=a[:, 4].copy(), gen_bus=perm[gens] + 1, gen_status=np.ones(gens.size, dtype=np.int8), gen_pg=pg,
             gen_qg=np.zeros(gens.size), gen_vg=np.ones(gens.size), gen_qmax=np.ones(gens.size), gen_qmin=-np.ones(gens.size))
    return t, marks, perm
