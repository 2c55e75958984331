"""Batched DC optimal power flow: one convex QP per lane, solved on the device by ADMM on one shared factor (csrc/jg_dcopf.hip).

  dcOptimalPowerFlow(system, optimizer)     src/optimalPowerFlow/dcOptimalPowerFlow.jl:44-198
  solve!(analysis)                          :298-370
  setInitialPoint!(target, source)          :445-476
  power!(analysis)                          src/postprocessing/dcAnalysis.jl

The reference hands the model to a JuMP solver, one problem at a time.  Here `modelRows` states the same model as  min 1/2 x' P x + q' x,
l <= A x <= u  with x = (bus angles, outputs of the in-service generators, one helper per piecewise-linear cost of more than two points) and the
rows in the order piecewise, balance, slack, capability, flow, angle difference.  P, q and A are shared by the lanes of a batch; a lane's own data are
its bounds: the demand profile in the balance rows, generator limits and generator outages in the capability rows.  A branch outage of one lane
changes A by a rank-1 term p d' (setBranchOutages_): the lane keeps the shared factor and corrects every solve by a rank-2 update; the branch's own
flow and angle rows become free rows and the two balance rows lose its shift power.

This module is product host code (numpy); the iteration runs in libjgrid_hip.so.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from . import _lib
from .system import PowerSystem, dcModel_

STATUS = {0: "solved", 2: "primal infeasible", 3: "singular", 5: "iteration limit"}
_TWO_PI = 2 * np.pi


def _angle_limited(lo: float, hi: float) -> bool:
    """addAngle (acOptimalPowerFlow.jl:495-514): a limit that is finite and neither 0 nor the full turn."""
    return bool((np.isfinite(lo) and lo not in (0.0, -_TWO_PI)) or (np.isfinite(hi) and hi not in (0.0, _TWO_PI)))


def _flow_limited(lo: float, hi: float) -> bool:
    """addFlow (dcOptimalPowerFlow.jl:258-277)."""
    return bool((lo != 0.0 and np.isfinite(lo)) or (hi != 0.0 and np.isfinite(hi)))


def modelRows(system: PowerSystem) -> NS:
    """The QP of dcOptimalPowerFlow(system): P (diagonal), q, the constant of the objective, A as 0-based CSR (rowptr, col, val), the base
    bounds l, u, the rows' class (1: equality) and where each kind of row and variable lies."""
    if system.model.dc.nodalMatrix is None:
        dcModel_(system)
    bus, br, gen, dc = system.bus, system.branch, system.generator, system.model.dc
    n = bus.number
    gens = np.flatnonzero(gen.layout.status == 1)
    var_pg = {int(k): n + j for j, k in enumerate(gens)}
    cost = gen.cost.active
    helper = {}
    nvar = n + gens.size
    for k in gens:
        if cost.model[k] == 1 and cost.piecewise[int(k) + 1].shape[0] > 2:
            helper[int(k)] = nvar
            nvar += 1
    P, q, c0 = np.zeros(nvar), np.zeros(nvar), 0.0
    rows = []                                                          # (kind, reference, columns, values, lower, upper)
    for k in gens:                                                     # addObjective (:201-226), addPiecewise (acOptimalPowerFlow.jl:436-484)
        k = int(k)
        if cost.model[k] == 2:
            c = cost.polynomial[k + 1]
            if c.size > 3:
                raise ValueError(f"dcOptimalPowerFlow: generator {k + 1} has a polynomial cost of degree {c.size - 1}; the DC model takes degree 2 at the most")
            if c.size == 3:
                P[var_pg[k]], q[var_pg[k]], c0 = 2.0 * c[0], c[1], c0 + c[2]
            elif c.size == 2:
                q[var_pg[k]], c0 = c[0], c0 + c[1]
            elif c.size == 1:
                c0 += c[0]
        elif cost.model[k] == 1:
            pts = cost.piecewise[k + 1]
            slope = np.diff(pts[:, 1]) / np.diff(pts[:, 0])
            if not np.all(np.isfinite(slope)):
                raise ValueError(f"dcOptimalPowerFlow: generator {k + 1} has a piecewise cost with a slope that is not finite")
            if pts.shape[0] == 2:                                      # the linear cost it is
                q[var_pg[k]], c0 = slope[0], c0 + pts[0, 1] - pts[0, 0] * slope[0]
            else:
                q[helper[k]] = 1.0
                for s in range(slope.size):
                    rows.append(("piecewise", (k + 1, s), [var_pg[k], helper[k]], [slope[s], -1.0], -np.inf, slope[s] * pts[s, 0] - pts[s, 1]))
    B = dc.nodalMatrix
    at_bus = {}
    for k in gens:
        at_bus.setdefault(int(gen.layout.bus[k]) - 1, []).append(var_pg[int(k)])
    for i in range(n):                                                 # B is symmetric: row i = column i
        lo, hi = B.colptr[i] - 1, B.colptr[i + 1] - 1
        cols = [int(r) - 1 for r in B.rowval[lo:hi]] + at_bus.get(i, [])
        vals = [float(v) for v in B.nzval[lo:hi]] + [-1.0] * len(at_bus.get(i, []))
        keep = [p for p in range(len(cols)) if vals[p] != 0.0 or cols[p] == i]
        rhs = -(bus.demand.active[i] + bus.shunt.conductance[i] + dc.shiftPower[i])
        rows.append(("balance", i + 1, [cols[p] for p in keep], [vals[p] for p in keep], rhs, rhs))
    s = bus.layout.slack - 1
    rows.append(("slack", s + 1, [s], [1.0], float(bus.voltage.angle[s]), float(bus.voltage.angle[s])))
    for k in gens:
        k = int(k)
        rows.append(("capability", k + 1, [var_pg[k]], [1.0], float(gen.capability.minActive[k]), float(gen.capability.maxActive[k])))
    on = np.flatnonzero(br.layout.status == 1)
    for k in on:
        k = int(k)
        lo, hi = float(br.flow.minFromBus[k]), float(br.flow.maxFromBus[k])
        if _flow_limited(lo, hi):
            y, f, t = float(dc.admittance[k]), int(br.layout.from_[k]) - 1, int(br.layout.to[k]) - 1
            off = y * float(br.parameter.shiftAngle[k])
            rows.append(("flow", k + 1, [f, t], [y, -y], lo + off, hi + off))
    for k in on:
        k = int(k)
        lo, hi = float(br.voltage.minDiffAngle[k]), float(br.voltage.maxDiffAngle[k])
        if _angle_limited(lo, hi):
            rows.append(("angle", k + 1, [int(br.layout.from_[k]) - 1, int(br.layout.to[k]) - 1], [1.0, -1.0], lo, hi))
    rowptr, col, val = [0], [], []
    for _, _, c, v, _, _ in rows:
        order = np.argsort(c)
        col += [c[p] for p in order]
        val += [v[p] for p in order]
        rowptr.append(len(col))
    kind = [r[0] for r in rows]
    where = {name: np.array([i for i, kd in enumerate(kind) if kd == name], dtype=np.int64) for name in ("piecewise", "balance", "slack", "capability", "flow", "angle")}
    m = len(rows)
    return NS(n=nvar, m=m, buses=n, generators=gens, var_pg=var_pg, helper=helper, P=P, q=q, constant=float(c0),
              rowptr=np.array(rowptr, dtype=np.int64), col=np.array(col, dtype=np.int64), val=np.array(val, dtype=np.float64),
              l=np.array([r[4] for r in rows], dtype=np.float64), u=np.array([r[5] for r in rows], dtype=np.float64),
              equality=np.array([1 if r[0] in ("balance", "slack") else 0 for r in rows], dtype=np.int32),
              kind=kind, ref=[r[1] for r in rows], rows=where)


def denseRows(model: NS) -> np.ndarray:
    A = np.zeros((model.m, model.n))
    for i in range(model.m):
        A[i, model.col[model.rowptr[i]:model.rowptr[i + 1]]] = model.val[model.rowptr[i]:model.rowptr[i + 1]]
    return A


def hostModel(model: NS, rho: float, sigma: float = 1e-6):
    """The library's host set-up alone (no device): K = P + sigma I + A' rho A dense from its term lists, the objective's scale, the rows' scales."""
    K, c, E = np.zeros(model.n * model.n), np.zeros(1), np.zeros(model.m)
    _lib.check(_lib.lib().jg_dcopf_host_model(model.n, model.m, model.P, model.q, model.rowptr, model.col + 1, model.val, model.equality, float(rho),
                                              float(sigma), K, c, E))
    return K.reshape(model.n, model.n), float(c[0]), E


class DcOptimalPowerFlow:
    """DcOptimalPowerFlow of the reference (definition/analysis.jl) with a batch: arrays are [batch, ...] (1-D for batch 1)."""

    def __init__(self, system, model, batch, h, adapt, check, adapt_every):
        self.system, self.model, self.batch, self._h = system, model, int(batch), h
        self.adapt, self.check, self.adapt_every = bool(adapt), int(check), int(adapt_every)
        gen = system.generator
        self.voltage = NS(angle=self._shape(np.tile(system.bus.voltage.angle, (self.batch, 1))))
        gp = np.where(gen.layout.status == 1, gen.output.active, 0.0)
        self.power = NS(generator=NS(active=self._shape(np.tile(gp, (self.batch, 1)))), injection=NS(active=None), supply=NS(active=None),
                        from_=NS(active=None), to=NS(active=None))
        self.dual = NS(balance=None, flow=None, capability=None, angle=None, piecewise=None, slack=None)
        self.objective = self.iterations = self.status = None
        self.refactorisations = 0
        self._l = np.tile(model.l, (self.batch, 1))
        self._u = np.tile(model.u, (self.batch, 1))
        self._demand = np.tile(system.bus.demand.active, (self.batch, 1))
        self._shift = np.zeros((self.batch, system.bus.number))        # what the lanes' outaged branches take out of the balance rows' shift power
        self.outage = np.zeros(self.batch, dtype=np.int64)             # the lanes' outaged branch (label, 0: none)
        self._outage_state = np.zeros(self.batch, dtype=np.int32)      # 0 none, 1 outage, 3 the outage is a bridge
        self._outage_dirty = False
        self._dirty = True
        self._x = self._y = self._z = None

    def _shape(self, a):
        return a[0] if self.batch == 1 else a

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().jg_dcopf_destroy(self._h)
            self._h = None

    @property
    def rho(self):
        r = np.zeros(1)
        _lib.check(_lib.lib().jg_dcopf_get_rho(self._h, r))
        return float(r[0])


def dcOptimalPowerFlow(system: PowerSystem, batch: int = 1, rho: float = 0.1, sigma: float = 1e-6, alpha: float = 1.6, tolerance: float = 1e-9,
                       iteration: int = 100000, adapt: bool = True, check: int = 25, adapt_every: int = 200, device: int = 0) -> DcOptimalPowerFlow:
    """dcOptimalPowerFlow(system, optimizer): builds the model rows on the host and the device handle (one symbolic analysis and one numeric
    factorisation of K).  `batch` lanes share P, q, A and rho; adapt=False keeps rho where it is, and then a lane's result does not depend on
    which other lanes share its batch."""
    if adapt_every % check:
        raise ValueError("dcOptimalPowerFlow: adapt_every must be a multiple of check")
    model = modelRows(system)
    h = C.c_int64(0)
    _lib.check(_lib.lib().jg_dcopf_create(C.byref(h), model.n, model.m, model.P, model.q, model.rowptr, model.col + 1, model.val, model.equality,
                                          int(batch), float(rho), float(sigma), float(alpha), int(device)))
    an = DcOptimalPowerFlow(system, model, batch, h.value, adapt, check, adapt_every)
    an.tolerance, an.iteration = float(tolerance), int(iteration)
    return an


def _lanes(an, a, width, what):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = np.tile(a, (an.batch, 1))
    if a.shape != (an.batch, width):
        raise ValueError(f"{what}: expected [{width}] or [{an.batch}, {width}], got {a.shape}")
    return a


def setInjection_(an: DcOptimalPowerFlow, demand) -> None:
    """The lanes' active demand, [buses] or [batch, buses] in per unit: the right-hand sides of the balance rows."""
    bus, dc = an.system.bus, an.system.model.dc
    d = _lanes(an, demand, bus.number, "setInjection_")
    rows = an.model.rows["balance"]
    an._demand = d.copy()
    _balance(an)


def _balance(an) -> None:
    """The balance rows' right-hand sides from the lanes' demand and the shift power their outaged branches no longer carry."""
    bus, dc = an.system.bus, an.system.model.dc
    rows = an.model.rows["balance"]
    an._l[:, rows] = an._u[:, rows] = -(an._demand + bus.shunt.conductance[None, :] + dc.shiftPower[None, :]) + an._shift
    an._dirty = True


def setCapability_(an: DcOptimalPowerFlow, lower=None, upper=None) -> None:
    """The lanes' generator limits, [generators] or [batch, generators] in per unit over ALL generators (those out of service are not read)."""
    gens, rows = an.model.generators, an.model.rows["capability"]
    if lower is not None:
        an._l[:, rows] = _lanes(an, lower, an.system.generator.number, "setCapability_")[:, gens]
    if upper is not None:
        an._u[:, rows] = _lanes(an, upper, an.system.generator.number, "setCapability_")[:, gens]
    if np.any(an._l[:, rows] > an._u[:, rows]):
        raise ValueError("setCapability_: a lower limit lies above its upper limit")
    an._dirty = True


def setOutages_(an: DcOptimalPowerFlow, generators=None, branches=None) -> None:
    """Per-lane generator outages: lane s runs without generator generators[s] (0 / None: none), through l = u = 0 on its capability row."""
    if branches is not None:
        raise ValueError("setOutages_: a branch outage of one lane changes the constraint matrix A, which the lanes of a DcOptimalPowerFlow share (with it "
                         "the one factor); setBranchOutages_ runs such lanes on the shared factor by a low-rank correction; or take the branch out of the system "
                         "(updateBranchSystem_) and build an analysis of its own")
    if generators is None:
        return
    lab = [int(g) if g else 0 for g in generators]
    if len(lab) != an.batch:
        raise ValueError(f"setOutages_: expected {an.batch} generator labels")
    row_of = {int(k) + 1: int(r) for k, r in zip(an.model.generators, an.model.rows["capability"])}
    for s, g in enumerate(lab):
        if g == 0:
            continue
        if not 1 <= g <= an.system.generator.number:
            raise IndexError("setOutages_: generator label out of range")
        if g in row_of:                                                # (one that is out of service in the system already has no row)
            an._l[s, row_of[g]] = an._u[s, row_of[g]] = 0.0
    an._dirty = True


def setBranchOutages_(an: DcOptimalPowerFlow, branches) -> None:
    """Per-lane branch outages: lane s runs without branch branches[s] (0 / None: none; one label: every lane), on the shared factor.  The lane's
    matrix is A + p d' (csrc/jg_dcopf.hpp); here its bounds: the branch's flow and angle rows are free, the balance rows of its two buses lose its
    shift power.  A lane whose branch is a bridge (islandTable) is not run: status 3, NaN.  A branch that is out of service in the system is no
    outage.  A call replaces the set, None clears it; x, y, z stay, so the next solve_ starts from the last solution."""
    br, dc, md = an.system.branch, an.system.model.dc, an.model
    if branches is None or np.isscalar(branches):
        branches = [branches] * an.batch
    lab = np.array([int(b) if b else 0 for b in branches], dtype=np.int64)
    if lab.shape != (an.batch,):
        raise ValueError(f"setBranchOutages_: expected {an.batch} branch labels")
    if np.any((lab < 0) | (lab > br.number)):
        raise IndexError("setBranchOutages_: branch label out of range")
    lab[lab > 0] = np.where((br.layout.status[lab[lab > 0] - 1] == 1) & (br.layout.from_[lab[lab > 0] - 1] != br.layout.to[lab[lab > 0] - 1]), lab[lab > 0], 0)
    state = np.zeros(an.batch, dtype=np.int32)
    if np.any(lab):
        from .contingency import islandTable
        tb = islandTable(an.system)
        state[lab > 0] = np.where(tb.lo[lab[lab > 0] - 1] <= tb.hi[lab[lab > 0] - 1], 3, 1)
    own = {}                                                            # the flow and angle rows of a branch
    for kind in ("flow", "angle"):
        for i in md.rows[kind]:
            own.setdefault(md.ref[i], []).append(int(i))
    for kind in ("flow", "angle"):                                      # the set before this one is gone
        an._l[:, md.rows[kind]], an._u[:, md.rows[kind]] = md.l[md.rows[kind]], md.u[md.rows[kind]]
    an._shift[:] = 0.0
    for s in np.flatnonzero(state == 1):
        k = int(lab[s]) - 1
        for i in own.get(k + 1, ()):
            an._l[s, i], an._u[s, i] = -np.inf, np.inf
        share = float(dc.admittance[k]) * float(br.parameter.shiftAngle[k])
        an._shift[s, br.layout.from_[k] - 1] -= share
        an._shift[s, br.layout.to[k] - 1] += share
    an.outage, an._outage_state, an._outage_dirty = lab, state, True
    _balance(an)


def _push_outages(an) -> None:
    br, dc, md = an.system.branch, an.system.model.dc, an.model
    L = _lib.lib()
    if not np.any(an._outage_state):
        _lib.check(L.jg_dcopf_set_branch_outages(an._h, None, None, None, None, None, None))
        return
    k = np.maximum(an.outage - 1, 0)
    f, t = br.layout.from_[k].astype(np.int64), br.layout.to[k].astype(np.int64)            # bus i is variable i; 1-based as the ABI counts
    rf, rt = md.rows["balance"][f - 1] + 1, md.rows["balance"][t - 1] + 1
    y = np.ascontiguousarray(dc.admittance[k], dtype=np.float64)
    arrays = [np.ascontiguousarray(a, dtype=np.int64) for a in (f, t, rf, rt)] + [y, np.ascontiguousarray(an._outage_state, dtype=np.int32)]
    _lib.check(L.jg_dcopf_set_branch_outages(an._h, *[a.ctypes.data for a in arrays]))


def outageCosts(system: PowerSystem, branches, demand=None, **kw) -> NS:
    """What each branch outage costs: ONE analysis with lane 0 the base case and lane j the outage of branches[j - 1] (demand: [buses] for every lane).
    Per outage its status, objective, cost (objective minus the base lane's), iterations and largest nodal price; `base` holds the base lane's."""
    branches = [int(b) for b in branches]
    an = dcOptimalPowerFlow(system, batch=len(branches) + 1, **kw)
    if demand is not None:
        setInjection_(an, np.asarray(demand, dtype=np.float64))
    setBranchOutages_(an, [0] + branches)
    solve_(an)
    st, obj, it, price = np.atleast_1d(an.status), np.atleast_1d(an.objective), np.atleast_1d(an.iterations), np.atleast_2d(an.dual.balance).max(axis=1)
    return NS(branches=np.array(branches, dtype=np.int64), status=st[1:].copy(), objective=obj[1:].copy(), cost=obj[1:] - obj[0], iterations=it[1:].copy(),
              price=price[1:].copy(), base=NS(status=int(st[0]), objective=float(obj[0]), iterations=int(it[0]), price=float(price[0])), analysis=an)


def setInitialPoint_(an: DcOptimalPowerFlow, source) -> None:
    """setInitialPoint!(target, source): angles and generator outputs from a DcPowerFlow or a DcOptimalPowerFlow; from the latter the duals too."""
    n, m, md = an.model.n, an.model.m, an.model
    x, y = np.zeros((an.batch, n)), np.zeros((an.batch, m))
    ang = np.asarray(source.voltage.angle, dtype=np.float64)
    x[:, :md.buses] = _lanes(an, ang, md.buses, "setInitialPoint_")
    gp = getattr(getattr(source.power, "generator", None), "active", None)
    if gp is not None:
        gp = _lanes(an, gp, an.system.generator.number, "setInitialPoint_")
        for k, j in md.var_pg.items():
            x[:, j] = gp[:, k]
    if isinstance(source, DcOptimalPowerFlow) and source._y is not None and source.model.m == m and source.model.n == n:
        x[:] = _lanes(an, source._x, n, "setInitialPoint_")
        y[:] = _lanes(an, source._y, m, "setInitialPoint_")
    else:                                                               # the helpers start on their costs' curves
        cost = an.system.generator.cost.active
        for k, j in md.helper.items():
            pts = cost.piecewise[k + 1]
            x[:, j] = np.interp(x[:, md.var_pg[k]], pts[:, 0], pts[:, 1])
    _lib.check(_lib.lib().jg_dcopf_set_start(an._h, x.reshape(-1), y.reshape(-1)))


def solve_(an: DcOptimalPowerFlow, iteration: int | None = None, tolerance: float | None = None) -> None:
    """solve!(analysis): runs every lane until it is solved, shown infeasible or at the iteration limit.  A first solve starts at zero (or at
    setInitialPoint_'s point); a later one goes on from where the last one ended -- the warm start after new bounds."""
    L, md = _lib.lib(), an.model
    if an._outage_dirty:
        _push_outages(an)
        an._outage_dirty = False
    if an._dirty:
        _lib.check(L.jg_dcopf_set_bounds(an._h, np.ascontiguousarray(an._l).reshape(-1), np.ascontiguousarray(an._u).reshape(-1)))
        an._dirty = False
    it, st, rf = np.zeros(an.batch, dtype=np.int32), np.zeros(an.batch, dtype=np.int32), np.zeros(1, dtype=np.int64)
    _lib.check(L.jg_dcopf_run(an._h, float(an.tolerance if tolerance is None else tolerance), int(an.iteration if iteration is None else iteration),
                              an.check, an.adapt_every if an.adapt else 0, it, st, rf))
    x, y, z, obj = np.zeros((an.batch, md.n)), np.zeros((an.batch, md.m)), np.zeros((an.batch, md.m)), np.zeros(an.batch)
    if not np.all(st == 3):
        _lib.check(L.jg_dcopf_get(an._h, x.ctypes.data, y.ctypes.data, z.ctypes.data, obj.ctypes.data))
    else:
        x[:], y[:], z[:], obj[:] = np.nan, np.nan, np.nan, np.nan
    out = np.flatnonzero(an._outage_state == 1)
    for s in out:                                                       # the outaged branch's own rows are free rows: no multiplier
        for i in np.concatenate((md.rows["flow"], md.rows["angle"])):
            if md.ref[i] == an.outage[s]:
                y[s, i] = 0.0
    an._x, an._y, an._z = x, y, z
    an.iterations, an.status, an.refactorisations = an._shape(it), an._shape(st), int(rf[0])
    an.objective = an._shape(obj + md.constant)
    gen = an.system.generator
    gp = np.zeros((an.batch, gen.number))
    for k, j in md.var_pg.items():
        gp[:, k] = x[:, j]
    an.voltage.angle = an._shape(x[:, :md.buses].copy())
    an.power.generator.active = an._shape(gp)
    # the reference's (JuMP's) signs: the multiplier of a row is d objective / d right-hand side.  The balance rows are stated here with the
    # opposite sign of the reference's, so their y is the nodal price as it is; every other row is the reference's own and gets -y
    rows = md.rows
    cap = np.zeros((an.batch, gen.number))
    cap[:, md.generators] = -y[:, rows["capability"]]
    an.dual = NS(balance=an._shape(y[:, rows["balance"]].copy()), slack=an._shape(-y[:, rows["slack"]]),
                 capability=an._shape(cap), flow={md.ref[i]: an._shape(-y[:, i]) for i in rows["flow"]},
                 angle={md.ref[i]: an._shape(-y[:, i]) for i in rows["angle"]}, piecewise={md.ref[i]: an._shape(-y[:, i]) for i in rows["piecewise"]})


def power_(an: DcOptimalPowerFlow) -> None:
    """power!(analysis::DcOptimalPowerFlow) (dcAnalysis.jl): from = y (theta_from - theta_to - shiftAngle), to = -from, the injection as the flows
    that leave a bus plus its shunt, supply = injection + demand; the generators' outputs are the solution's.  O(branches) per lane, on the host."""
    if an._x is None:
        raise RuntimeError("power_: solve_ first")
    bus, br, dc = an.system.bus, an.system.branch, an.system.model.dc
    th = an._x[:, :an.model.buses]
    f, t = br.layout.from_ - 1, br.layout.to - 1
    fr = dc.admittance[None, :] * (th[:, f] - th[:, t] - br.parameter.shiftAngle[None, :])
    out = np.flatnonzero(getattr(an, "_outage_state", np.zeros(0)) == 1)
    if out.size:
        fr[out, an.outage[out] - 1] = 0.0                              # a lane's outaged branch carries nothing
    inj = np.tile(bus.shunt.conductance, (an.batch, 1))
    for s in range(an.batch):
        np.add.at(inj[s], f, fr[s])
        np.add.at(inj[s], t, -fr[s])
    pw = an.power
    pw.from_, pw.to = NS(active=an._shape(fr)), NS(active=an._shape(-fr))
    pw.injection, pw.supply = NS(active=an._shape(inj)), NS(active=an._shape(inj + an._demand))


def powerFlow_(an: DcOptimalPowerFlow, iteration: int | None = None, tolerance: float | None = None, power: bool = False) -> None:
    """powerFlow!(analysis; iteration, tolerance, power) (:536-556)."""
    solve_(an, iteration, tolerance)
    if power:
        power_(an)
