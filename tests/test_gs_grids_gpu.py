"""Gauss-Seidel power flow on the device (csrc/jg_gs.hip) on the grids of tests/gs_grids.py and under edits of a live batch, against the numpy
restatement (tests/gs_reference.py).  What the restatement gives on these grids, and why the bounds hold on them, is asserted on the host in
tests/test_gs_grids_host.py; its LIMIT and COUNTS are used here.

Bounds, those of tests/test_gs_gpu.py unchanged (compare_lanes is its function): status and sweep count equal on every lane, voltages of converged lanes
within 1e-10, single steps within 1e-12, lanes with the same inputs equal bit for bit.  Every full run of the restatement is first checked to stop clear of
the tolerance (gs_reference.margins_hold), so that no count hangs on a rounding.

Measured on an MI355X, worst |dV| per family: DESIGN.md section 3.15.1.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import gs_grids as G
import gs_reference as R
from conftest import load_case
from test_gs_gpu import compare_lanes
from test_gs_grids_host import COUNTS, LIMIT, NAMES

pytestmark = pytest.mark.gpu

TOL = G.TOL


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def deviation(got, want):
    """worst |got - want| where `want` is finite; where it is not (a lane an outage left without admittance), `got` is not finite either"""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


class Pair:
    """a device analysis of `batch` lanes and the restatement's state of the same lanes, edited together.  dry: the restatement alone (no device)"""

    def __init__(self, jg, s, batch, dry=False):
        self.jg, self.s, self.batch = jg, s, batch
        self.an = None if dry else jg.gaussSeidel(s, batch=batch)
        self.labs = np.zeros(batch, dtype=np.int64)
        self.g = R.problem(s)
        self.yt, self.v, self.P, self.Q = R.lanes(self.g, batch)
        self.step_dev = self.run_dev = 0.0

    def values(self):
        """the lanes' matrices again, each from a system REBUILT without the lane's branch -- after any edit of the system, a new pattern included"""
        self.g = R.problem(self.s)
        self.yt = R.lane_values(self.s, self.labs)

    def outages(self, labs, s0=0):
        self.labs[s0:s0 + len(labs)] = labs
        if self.an is not None:
            self.jg.setOutages_(self.an, labs, s0)
        self.values()

    def injection(self, factor, s0=0):
        """lanes s0 .. get the system's injections with the demand scaled by factor[k]"""
        bus = self.s.bus
        P = np.stack([bus.supply.active - f * bus.demand.active for f in factor])
        Q = np.stack([bus.supply.reactive - f * bus.demand.reactive for f in factor])
        self.P[s0:s0 + len(factor)], self.Q[s0:s0 + len(factor)] = P, Q
        if self.an is not None:
            self.jg.setInjection_(self.an, P, Q, s0)

    def steps(self, count):
        for step in range(count):
            rp, rq = R.mismatch(self.g, self.yt, self.v, self.P, self.Q)
            R.sweep(self.g, self.yt, self.v, self.P, self.Q)
            if self.an is None:
                continue
            p, q = (np.atleast_1d(x) for x in self.jg.mismatch_(self.an))
            self.jg.solve_(self.an)
            dv = np.atleast_2d(self.an.method.voltage)
            dev = max(deviation(p, rp), deviation(q, rq), deviation(dv.real, self.v.real), deviation(dv.imag, self.v.imag))
            assert dev <= 1e-12, (step, dev)
            self.step_dev = max(self.step_dev, dev)

    def full(self, limit):
        # the restatement runs every DISTINCT lane once (lanes with the same matrix, voltages and injections are one lane to it)
        seen, inv = {}, np.zeros(self.batch, dtype=np.int64)
        for b in range(self.batch):
            inv[b] = seen.setdefault(self.yt[b].tobytes() + self.v[b].tobytes() + self.P[b].tobytes() + self.Q[b].tobytes(), len(seen))
        u = np.array([int(np.flatnonzero(inv == k)[0]) for k in range(len(seen))])
        vu = self.v[u].copy()
        one = R.run(self.g, self.yt[u], vu, self.P[u], self.Q[u], limit, TOL)
        assert R.margins_hold(one, TOL)
        out = NS(iteration=one.iteration[inv], status=one.status[inv], stop=(one.stop[0][inv], one.stop[1][inv]), before=one.before[inv])
        self.v[:] = vu[inv]
        assert out.status[0] == 0 and np.mean(out.status == 0) >= 0.5
        if self.an is not None:
            self.jg.powerFlow_(self.an, iteration=limit, tolerance=TOL)
            self.run_dev = max(self.run_dev, compare_lanes(self.an, out, self.v, np.arange(self.batch)))
        return out


def lane_labels(name, batch):
    lab = np.array(G.labels(G.family(name)))
    return lab, lab[np.arange(batch) % lab.size]


@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("name", NAMES)
def test_every_family(jg, name, batch):
    """lane b loses branch labels[b mod len(labels)] (0: none); the limit is the one the host file recorded"""
    out, v = G.restated(name, LIMIT[name])
    lab, labs = lane_labels(name, batch)
    pick = np.arange(batch) % lab.size
    assert [(int(out.status[k]), int(out.iteration[k])) for k in range(lab.size)] == list(COUNTS[name].values())
    an = jg.gaussSeidel(G.system(name, jg), batch=batch)
    jg.setOutages_(an, labs)
    jg.powerFlow_(an, iteration=LIMIT[name], tolerance=TOL)
    dev = compare_lanes(an, out, v, pick)
    print(f"{name}, batch {batch}: sweeps {out.iteration.tolist()} worst |dV| device - restatement {dev:.3e}")
    if batch == 65:
        volt = an.method.voltage
        assert an.status[64] == 3 or same_bits(volt[64], volt[64 % lab.size])
        for b in range(lab.size, batch):
            if an.status[b] != 3:
                assert same_bits(volt[b], volt[b % lab.size]), b


@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("name", ["one bus", "two buses, PQ", "two buses, PV"])
def test_single_steps_with_an_empty_bus_list(jg, name, batch):
    pair = Pair(jg, G.system(name, jg), batch)
    pair.outages(lane_labels(name, batch)[1])
    assert deviation(np.atleast_2d(pair.an.method.voltage), pair.v) <= 1e-15
    pair.steps(5)
    assert np.all(np.atleast_1d(pair.an.method.iteration) == 5)
    print(f"{name}, batch {batch}: worst single-step deviation {pair.step_dev:.3e}")
    slack = int(pair.s.bus.layout.slack) - 1
    assert np.all(np.atleast_2d(pair.an.method.voltage)[:, slack] == pair.g.v0[slack])     # nobody walks the slack's row


def lane_ranges(jg, name, batch, edit, dry=False):
    """one kind of edit of lanes lane0 .. of a batch whose lanes carry outages; five single steps after every edit, then a full run; lanes outside the
    range keep the bits of a second analysis that never saw the edit"""
    lab, labs = lane_labels(name, batch)
    rng = np.random.default_rng(7 * batch + len(edit))
    pair = Pair(jg, G.system(name, jg), batch, dry)
    pair.outages(labs)
    other = None
    if not dry:
        other = jg.gaussSeidel(G.system(name, jg), batch=batch)
        jg.setOutages_(other, labs)
    edited = np.zeros(batch, dtype=bool)
    sweeps = 0
    if edit == "injection":
        # from lane 1, 63 and 64: across the wave boundary where the batch has lanes beyond it, and short of the last lane where the range can be
        for s0, count in ((1, 65), (63, 3), (64, 65)):
            count = max(1, min(count, batch - 1 - s0))
            pair.injection(rng.choice([0.9, 0.96, 1.04, 1.1], count), s0)
            edited[s0:s0 + count] = True
            pair.steps(5)
            sweeps += 5
        assert not edited[0] and (batch == 65 or (not edited[-1] and edited[63:129].all()))
    elif edit == "outages":
        s0, count = 60, min(8, batch - 1 - 60)                    # 60 .. 63 of 65 lanes, 60 .. 67 of 130: scenario0 > 0, across the boundary
        new = np.roll(lab, 3)[np.arange(count) % lab.size]
        assert np.any(new != labs[s0:s0 + count])
        pair.outages(new, s0)
        edited[s0:s0 + count] = True
        pair.steps(5)
        sweeps += 5
    elif edit == "one lane":
        new = int(lab[(64 + 2) % lab.size])
        assert new != labs[64] and labs[63] != 0 and (batch == 65 or labs[65] != 0)
        pair.labs[64] = new
        if not dry:
            jg.setOutage_(pair.an, 64, new)
        pair.values()
        pair.steps(5)
        pair.labs[64] = 0                                         # lane 64 back on the base grid; 63 and 65 keep their outage
        if not dry:
            jg.setOutage_(pair.an, 64, None)
        pair.values()
        pair.steps(5)
        sweeps += 10
        edited[64] = True
    elif edit == "voltage":
        g = pair.g
        slack = int(pair.s.bus.layout.slack) - 1
        kinds = np.where(rng.random((4, g.n)) < 0.3, rng.choice([0.98, 1.02], (4, g.n)), 1.0)      # four start points, dealt to the lanes by a seeded draw
        kinds[:, slack] = 1.0
        deal = rng.integers(0, 4, batch)
        deal[64] = (deal[63] + 1) % 4
        scale = kinds[deal]
        vm, va = np.abs(g.v0)[None, :] * scale, np.broadcast_to(np.angle(g.v0), (batch, g.n)).copy()
        assert len({tuple(r) for r in scale}) == 4 and np.any(scale[63] != scale[64])             # the lanes do differ, on both sides of the wave boundary
        pair.v[:] = vm * (np.cos(va) + 1j * np.sin(va))
        if not dry:
            jg.setInitialPoint_(pair.an, NS(voltage=NS(magnitude=vm, angle=va)))
            assert deviation(pair.an.method.voltage, pair.v) <= 1e-15
            assert deviation(pair.an.voltage.magnitude, vm) <= 1e-15
        edited[:] = True
        pair.steps(5)
        sweeps += 5
    else:
        raise ValueError(edit)
    if not dry:
        for _ in range(sweeps):
            jg.solve_(other)
        keep = ~edited
        assert same_bits(pair.an.method.voltage[keep], other.method.voltage[keep])
        if edited.any() and edit != "one lane":
            assert not same_bits(pair.an.method.voltage[edited], other.method.voltage[edited])
    out = pair.full(LIMIT[name])
    if not dry:
        jg.powerFlow_(other, iteration=LIMIT[name], tolerance=TOL)
        assert same_bits(pair.an.method.voltage[keep], other.method.voltage[keep])
        assert np.array_equal(pair.an.method.iteration[keep], other.method.iteration[keep])
        if edit == "one lane":                                    # restored: lane 64 ends where a base lane that took the same detour would; not lane 0's bits
            assert pair.an.status[64] == 0
    print(f"{name}, batch {batch}, {edit}: worst single step {pair.step_dev:.3e}, worst |dV| of the full run {pair.run_dev:.3e}, "
          f"converged {int(np.sum(out.status == 0))} of {batch}")
    return out


@pytest.mark.parametrize("edit", ["injection", "outages", "one lane", "voltage"])
@pytest.mark.parametrize("batch", [65, 130])
@pytest.mark.parametrize("name", ["ring 12 with twins", "star 71, hub last"])
def test_lane_ranges(jg, name, batch, edit):
    lane_ranges(jg, name, batch, edit)


CASE14_LANES = (0, 1, 2, 4, 5, 7, 9, 10, 13)                       # labels that converge on case14test (CASE14_COUNTS of tests/test_gs_gpu.py)


def live_system(jg, name):
    if name == "case14test":
        s = jg.powerSystem(load_case(name))
        jg.acModel_(s)
        return s, np.array(CASE14_LANES), 2500
    return G.system(name, jg), np.array(G.labels(G.family(name))), 6000


def live_edits(jg, name, dry=False):
    """a batch of 65 with outages and per-lane injections in place; every edit is mirrored by rebuilding the lanes' matrices from the edited system"""
    batch = 65
    s, lab, limit = live_system(jg, name)
    labs = lab[np.arange(batch) % lab.size]
    assert {7, 13} <= set(lab.tolist())
    pair = Pair(jg, s, batch, dry)
    pair.outages(labs)
    pair.injection(np.random.default_rng(14).uniform(0.95, 1.05, batch))
    pair.steps(3)
    an, bus, br = pair.an, s.bus, s.branch
    label_of = {idx - 1: l for l, idx in bus.label.items()}
    # 1. a shunt: the diagonal moves, the bus starts again from the system's voltage (bus.jl:350-362), every lane keeps its outage and its injections
    i = int(pair.g.pq[1])
    if dry:
        jg.updateBusSystem_(s, label_of[i], susceptance=float(bus.shunt.susceptance[i]) + 0.05)
    else:
        jg.updateBus_(an, label_of[i], susceptance=float(bus.shunt.susceptance[i]) + 0.05)
    pair.values()
    pair.v[:, i] = bus.voltage.magnitude[i] * (np.cos(bus.voltage.angle[i]) + 1j * np.sin(bus.voltage.angle[i]))
    pair.steps(3)
    # 2. the reactance of branch 7: out in some lanes, in service in the others
    x = float(br.parameter.reactance[6]) * 1.25
    jg.updateBranchSystem_(s, 7, reactance=x) if dry else jg.updateBranch_(an, 7, reactance=x)
    pair.values()
    pair.steps(3)
    # 3. branch 13 leaves the system; the lanes that had it as their outage must not lose it twice
    jg.updateBranchSystem_(s, 13, status=0) if dry else jg.updateBranch_(an, 13, status=0)
    pair.values()
    pair.steps(3)
    # 4. a branch parallel to branch 2: the same pattern, new values only
    f, t = int(br.layout.from_[1]) - 1, int(br.layout.to[1]) - 1
    kw = dict(from_=label_of[f], to=label_of[t], resistance=0.02, reactance=0.3, susceptance=0.02)
    pattern = s.model.revision.acPattern
    jg.addBranchSystem_(s, **kw) if dry else jg.addBranch_(an, **kw)
    assert s.model.revision.acPattern == pattern
    pair.values()
    pair.steps(3)
    # 5. a branch between two buses that had no entry: the pattern grows.  The reference goes on (its solve! reads the system's matrix, _addBranch!
    # only checks the bus types, syncTopology! takes the new revision): the analysis rebuilds its handle and continues from the same voltages
    Y = s.model.ac.nodalMatrix
    slack = int(bus.layout.slack) - 1
    a, b = next((a, b) for a in range(bus.number) for b in range(a + 2, bus.number) if slack not in (a, b) and not Y.has(a + 1, b + 1))
    kw = dict(from_=label_of[b], to=label_of[a], resistance=0.03, reactance=0.25, turnsRatio=0.98)
    jg.addBranchSystem_(s, **kw) if dry else jg.addBranch_(an, **kw)
    assert s.model.revision.acPattern == pattern + 1
    nnz = pair.yt.shape[1]
    pair.values()
    assert pair.yt.shape[1] == nnz + 2
    if not dry:
        before, count = an.method.voltage.copy(), an.method.iteration
        jg.mismatch_(an)                                          # the first call that meets the new pattern rebuilds
        assert an.method.signature.acPattern == pattern + 1
        assert same_bits(an.method.voltage, before) and an.method.iteration == count
        assert np.array_equal(an._P, pair.P) and np.array_equal(an._Q, pair.Q) and np.array_equal(an._outage_labels, labs)
    pair.steps(3)                                                 # per-lane injections and outages hold on the new pattern
    out = pair.full(limit)
    print(f"{name}: live edits, worst single step {pair.step_dev:.3e}, worst |dV| of the full run {pair.run_dev:.3e}, sweeps "
          f"{out.iteration[:lab.size].tolist()} status {out.status[:lab.size].tolist()}")
    return out


@pytest.mark.parametrize("name", ["ring 12 with twins", "case14test"])
def test_live_edits_of_a_batch(jg, name):
    live_edits(jg, name)


def test_hand_off_per_lane(jg):
    """setInitialPoint_(gs, nr) and (nr, gs) with [65, n] voltages of lanes that differ by an outage.  nr <- gs copies magnitude and angle: equal bit for
    bit.  gs <- nr forms magnitude * cis(angle) per lane, so what is bitwise there is the lane against a one-lane analysis given the same magnitude
    and angle through the [n] path; against numpy's cis the bound is one rounding"""
    name, batch = "pegaseShaped 60", 65
    lab = np.array([k for k, (status, _) in COUNTS[name].items() if status == 0])
    labs = lab[np.arange(batch) % lab.size]
    s = G.system(name, jg)
    nr = jg.newtonRaphson(s, batch=batch)
    jg.setOutages_(nr, labs)
    jg.powerFlow_(nr)
    assert np.all(nr.status == 0)
    assert np.abs(nr.voltage.magnitude[1] - nr.voltage.magnitude[0]).max() > 1e-6          # lanes differ
    gs = jg.gaussSeidel(s, batch=batch)
    jg.setOutages_(gs, labs)
    jg.setInitialPoint_(gs, nr)
    want = nr.voltage.magnitude * (np.cos(nr.voltage.angle) + 1j * np.sin(nr.voltage.angle))
    assert deviation(gs.method.voltage, want) <= 1e-15
    for lane in (0, 1, 63, 64):
        one = jg.gaussSeidel(s, batch=1)
        jg.setInitialPoint_(one, NS(voltage=NS(magnitude=nr.voltage.magnitude[lane], angle=nr.voltage.angle[lane])))
        assert same_bits(gs.method.voltage[lane], one.method.voltage), lane
    p, q = jg.mismatch_(gs)
    print("Gauss-Seidel mismatch at the Newton-Raphson solutions, worst lane", float(p.max()), float(q.max()))
    assert p.max() < 1e-8 and q.max() < 1e-8
    jg.setInitialPoint_(gs)
    jg.powerFlow_(gs, iteration=5)
    assert np.all(gs.status == 1) and not same_bits(gs.method.voltage[1], gs.method.voltage[0])
    jg.setInitialPoint_(nr, gs)
    assert same_bits(nr.voltage.magnitude, gs.voltage.magnitude) and same_bits(nr.voltage.angle, gs.voltage.angle)
