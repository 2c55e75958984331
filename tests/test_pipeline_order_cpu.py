"""The ordering protocol of the two batch pipelines (juliagrid.jl_amd/pipeline.py: OrderedRun) and the straggler pools of ContingencyPipeline
(contingency._StragglerPools), on a CPU: stub handles, events instead of sleeps, a time limit on every wait -- a protocol bug is a failed assertion,
never a hung suite.  Nothing here loads libjgrid_hip.so."""
import threading

import numpy as np
import pytest

import juliagrid.jl_amd.contingency as contingency
from juliagrid.jl_amd import pipeline
from juliagrid.jl_amd.contingency import ContingencyPipeline, _Pool, _StragglerPools
from juliagrid.jl_amd.montecarlo import MonteCarloPipeline
from juliagrid.jl_amd.pipeline import OrderedRun

T = 20.0            # seconds: the limit of every wait and join below (none is ever reached by a correct protocol)


def _call(f):
    """f() on a thread of its own, joined within T: ("ok", value) or ("error", exception)."""
    box = []

    def target():
        try:
            box.append(("ok", f()))
        except BaseException as e:
            box.append(("error", e))
    t = threading.Thread(target=target, daemon=True)
    t.start()
    t.join(T)
    assert not t.is_alive(), "run() hangs"
    return box[0]


def _wait(ev, what):
    assert ev.wait(T), f"timed out waiting for {what}"


class _Pipe:
    """Stands where a pipeline stands: it keeps the handles, every run() is one OrderedRun."""

    def __init__(self, nh):
        self.handles = [f"handle{k}" for k in range(nh)]

    def run(self, nj, solve, on_done=None, hold=False, ring=0, **hooks):
        return OrderedRun(self.handles, nj, hold=hold, ring=ring).run(solve, on_done, **hooks)


def test_the_runner_is_device_free():
    """pipeline.py stands on the standard library alone: no binding, no torch, none of the modules that load the HIP library."""
    import types
    assert {v.__name__ for v in vars(pipeline).values() if isinstance(v, types.ModuleType)} <= {"threading"}
    assert not any(getattr(v, "__module__", "").startswith("juliagrid") and v.__module__ != pipeline.__name__ for v in vars(pipeline).values())


@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("nh,nj", [(1, 1), (1, 3), (2, 5), (3, 2), (3, 7), (2, 0)])
def test_order_and_stride(nh, nj, hold):
    pipe = _Pipe(nh)
    ran, seen = {}, []

    def solve(k, j):
        ran[j] = (k, threading.get_ident())
        return ("result", j)
    before = threading.active_count()
    kind, res = _call(lambda: pipe.run(nj, solve, lambda j, h: seen.append((j, h)), hold=hold))
    assert kind == "ok" and res == [("result", j) for j in range(nj)]
    assert seen == [(j, pipe.handles[j % nh]) for j in range(nj)]
    assert all(ran[j][0] == j % nh for j in range(nj))
    assert all(ran[j][1] == ran[j % nh][1] for j in range(nj)), "a handle has one host thread"
    assert threading.active_count() == before


@pytest.mark.parametrize("hook", [False, True])
def test_ring_keeps_a_record_until_it_is_delivered(hook):
    """nh = 2, ring = 2, nj = 5, on_done(0) blocks: jobs 2 and 3 wait for the deliveries of 0 and 1 although their handles are free."""
    pipe = _Pipe(2)
    log, lock = [], threading.Lock()
    gate, at_ring_wait, started = threading.Event(), threading.Event(), [threading.Event() for _ in range(5)]

    def note(x):
        with lock:
            log.append(x)

    def solve(k, j):
        note(("start", j))
        started[j].set()
        return j

    def on_done(j, h):
        if j == 0:
            _wait(gate, "the gate")
        note(("seen", j))

    def before_ring_wait():
        note(("hook",))
        at_ring_wait.set()
    hooks = {"before_ring_wait": before_ring_wait} if hook else {}
    box = []
    t = threading.Thread(target=lambda: box.append(_call(lambda: pipe.run(5, solve, on_done, ring=2, **hooks))), daemon=True)
    t.start()
    _wait(started[1], "job 1")
    if hook:
        _wait(at_ring_wait, "the ring hook")                # a worker stands before its ring wait now
    assert not started[2].is_set() and not started[3].is_set()
    gate.set()
    t.join(T)
    assert not t.is_alive() and box[0] == ("ok", [0, 1, 2, 3, 4])
    for j in (2, 3, 4):
        assert log.index(("seen", j - 2)) < log.index(("start", j)), log
    if hook:
        assert log.index(("hook",)) < log.index(("start", 2))
    else:
        assert ("hook",) not in log


@pytest.mark.parametrize("hold", [True, False])
def test_hold_decides_when_a_handle_is_free(hold):
    """nh = 2, nj = 4, on_done(0) blocks: with hold the handle of job 0 waits for its delivery, without it job 2 starts at once."""
    pipe = _Pipe(2)
    log, lock = [], threading.Lock()
    gate, started = threading.Event(), [threading.Event() for _ in range(4)]

    def solve(k, j):
        with lock:
            log.append(("start", j))
        started[j].set()
        return j

    def on_done(j, h):
        if j == 0:
            if not hold:
                _wait(started[2], "job 2, whose handle is free")        # while on_done(0) has not returned
            _wait(gate, "the gate")
        with lock:
            log.append(("seen", j))
    box = []
    t = threading.Thread(target=lambda: box.append(_call(lambda: pipe.run(4, solve, on_done, hold=hold))), daemon=True)
    t.start()
    _wait(started[1], "job 1")
    if hold:
        assert not started[2].is_set()
    else:
        _wait(started[2], "job 2")
    gate.set()
    t.join(T)
    assert not t.is_alive() and box[0] == ("ok", [0, 1, 2, 3])
    if hold:
        assert log.index(("seen", 0)) < log.index(("start", 2)) and log.index(("seen", 1)) < log.index(("start", 3)), log
    else:
        assert log.index(("start", 2)) < log.index(("seen", 0)), log


def test_hold_rules_of_the_two_pipelines():
    """The table of the two rules, kept apart on purpose: they differ with a record AND an on_done without a pool, and with neither."""
    def cb(j, h):
        return None
    rec = lambda j: 0                                                   # noqa: E731
    for record in (None, rec):
        for on_done in (None, cb):
            for pool in (False, True):
                assert ContingencyPipeline._hold(pool, record, on_done) == (not (pool or (record is not None and on_done is None)))
            assert MonteCarloPipeline._hold(record, on_done) == (on_done is not None and record is None)
    #                                  record  on_done   contingency (no pool)  contingency (pool)  Monte Carlo
    table = [(None, None, True, False, False), (None, cb, True, False, True), (rec, None, False, False, False), (rec, cb, True, False, False)]
    for record, on_done, c_plain, c_pool, mc in table:
        assert ContingencyPipeline._hold(False, record, on_done) is c_plain
        assert ContingencyPipeline._hold(True, record, on_done) is c_pool
        assert MonteCarloPipeline._hold(record, on_done) is mc


@pytest.mark.parametrize("where", ["solve", "on_done", "complete"])
def test_errors_surface_join_every_thread_and_leave_the_pipeline_usable(where):
    """nh = 3, nj = 6.  solve raises at job 3; on_done raises at job 2 while a worker has raised as well (the caller's error wins); the complete hook raises."""
    pipe = _Pipe(3)
    in_on_done_2, worker_failed = threading.Event(), threading.Event()
    started = []

    def solve(k, j):
        started.append(j)
        if where == "solve" and j == 3:
            raise RuntimeError("solve failed at job 3")
        if where == "on_done" and j == 4:
            _wait(in_on_done_2, "on_done(2)")
            raise RuntimeError("worker failed at job 4")
        return j

    def on_done(j, h):
        if where == "on_done" and j == 2:
            in_on_done_2.set()
            _wait(worker_failed, "the worker's failure")
            raise KeyError("caller failed at job 2")

    def complete(j):
        if where == "complete" and j == 1:
            raise RuntimeError("complete failed at job 1")
    before = threading.active_count()
    kind, e = _call(lambda: pipe.run(6, solve, on_done, complete=complete, on_fail=worker_failed.set))
    assert kind == "error"
    expect = {"solve": (RuntimeError, "solve failed at job 3"), "on_done": (KeyError, "caller failed at job 2"), "complete": (RuntimeError, "complete failed at job 1")}[where]
    assert type(e) is expect[0] and expect[1] in str(e)
    assert threading.active_count() == before, "a thread of the failed run is still there"
    where = None
    assert _call(lambda: pipe.run(6, solve, on_done, complete=complete)) == ("ok", list(range(6)))
    assert threading.active_count() == before


def test_no_job_starts_after_a_failure():
    """hold: job 3 waits for the delivery of job 0, which fails: the wait is released and job 3 does not run."""
    pipe = _Pipe(3)
    started = []

    def solve(k, j):
        started.append(j)
        return j

    def on_done(j, h):
        raise RuntimeError("caller failed at job 0")
    kind, e = _call(lambda: pipe.run(6, solve, on_done, hold=True))
    assert kind == "error" and "job 0" in str(e) and 0 in started and set(started) <= {0, 1, 2}


# ---- the straggler pools, driven through ContingencyPipeline.run itself with fake handles ----------------------------------------------------------

OWN_IT, POOL_ST = 3, 9


class _FakeHandle:
    """What the pools and ContingencyPipeline._solve use of a handle, and a log of it."""

    def __init__(self, name, batch, log, script=None, gates=None):
        self.name, self.batch, self.log, self.script, self.gates = name, batch, log, script or {}, gates or {}
        self._outage_labels = 100 * (len(log.handles) + 1) + np.arange(batch)
        log.handles.append(self)
        self.method = type("M", (), {})()
        self.status = None
        self.job = None
        self.home = np.zeros(0, dtype=np.int32)
        self.lanes = {}                                   # pool lane -> (job, scenario, label)
        self.fail = None
        self.resume_entered, self.resume_gate = threading.Event(), None

    def restore_voltage(self):
        self.job = self.log.next_job(self)

    def run_defer(self, iteration, tolerance, defer_at):
        self.log.add(("run_defer", self.job))
        if self.job in self.gates:
            _wait(self.gates[self.job], f"the gate of job {self.job}")
        if self.fail == ("run_defer", self.job):
            raise RuntimeError("run_defer failed")
        left = self.script[self.job]
        assert left <= defer_at
        self.home = (2 * np.arange(left) + 1).astype(np.int32)          # the odd scenarios are the slow ones
        return left

    def finish(self):
        self.method.iteration = np.full(self.batch, OWN_IT, dtype=np.int32)
        self.status = np.zeros(self.batch, dtype=np.int32)
        self.status[self.home] = 4                                      # handed to a pool
        self.home = np.zeros(0, dtype=np.int32)

    def lockstep(self):
        self.log.add(("lockstep", self.job))
        if self.job in self.gates:
            _wait(self.gates[self.job], f"the gate of job {self.job}")
        self.finish()

    def take_lanes(self, src, lane0):
        home = src.home.copy()
        assert lane0 + home.size <= self.batch, "the pool overflows"
        for i, sc in enumerate(home):
            self.lanes[lane0 + i] = (src.job, int(sc), int(src._outage_labels[sc]))
        self.log.add(("take", src.job, self.name, lane0, tuple(home)))
        if src.job in self.log.taken:
            self.log.taken[src.job].set()
        return home

    def resume(self, lanes, iteration, tolerance):
        if self.fail == ("resume",):
            raise RuntimeError("resume failed")
        self.resume_entered.set()
        if self.resume_gate is not None:
            _wait(self.resume_gate, "the gate of resume")
        assert [int(x) for x in self._outage_labels[:lanes]] == [self.lanes[l][2] for l in range(lanes)], "the outage labels travel with the lanes"
        it = np.array([1000 * self.lanes[l][0] + self.lanes[l][1] + 1 for l in range(lanes)], dtype=np.int32)
        return it, np.full(lanes, POOL_ST, dtype=np.int32)

    def pack_results_device(self, ptr):
        self.log.add(("own", ptr, "state"))

    def screen_device(self, ptr):
        self.log.add(("own", ptr, "summary"))

    def pack_rows_device(self, ptr, lane0, rows):
        self.log.add(("rows", ptr, "state", lane0, tuple(int(x) for x in rows)))

    def screen_rows_device(self, ptr, lane0, rows):
        self.log.add(("rows", ptr, "summary", lane0, tuple(int(x) for x in rows)))


class _Log:
    def __init__(self, nh):
        self.lock, self.entries, self.handles, self.nh, self.taken = threading.Lock(), [], [], nh, {}
        self.count = {}

    def add(self, x):
        with self.lock:
            self.entries.append(x)

    def next_job(self, h):                                # a handle's jobs are k, k + nh, ...
        k = self.handles.index(h)
        self.count[k] = self.count.get(k, -1) + 1
        return k + self.nh * self.count[k]

    def new_run(self):
        self.entries, self.count = [], {}
        for ev in self.taken.values():
            ev.clear()


def _fake_pipeline(monkeypatch, script, nh=2, batch=8, lanes=4):
    """A ContingencyPipeline around fake handles: batches of 8, two pools of 4 lanes.  Job 1 pauses only after job 0 has handed its stragglers over, and job 2 after job 1,
    so the order in which the pools fill is fixed."""
    log = _Log(nh)
    log.taken[0], log.taken[1] = threading.Event(), threading.Event()
    pipe = object.__new__(ContingencyPipeline)
    pipe.batch, pipe.base, pipe.reactive_limit, pipe.defer_at = batch, None, 0, 4
    pipe.handles = [_FakeHandle(f"h{k}", batch, log, script, gates={1: log.taken[0], 2: log.taken[1]}) for k in range(nh)]
    pipe.pools = [_Pool(_FakeHandle(f"P{i}", lanes, log)) for i in range(2)]
    pipe._stragglers = _StragglerPools(pipe.pools, pipe.defer_at)
    monkeypatch.setattr(contingency, "powerFlow_", lambda an, iteration, tolerance, fetch: an.lockstep())
    return pipe, log


def _check_pool_run(pipe, log, res, nj, script, kind):
    nh = len(pipe.handles)
    e = log.entries
    deferring = [j for j in range(nj) if j + nh < nj]
    assert sorted(x[1] for x in e if x[0] == "run_defer") == deferring, "the last job of each handle never pauses"
    assert sorted(x[1] for x in e if x[0] == "lockstep") == [j for j in range(nj) if j not in deferring]
    takes = [x for x in e if x[0] == "take"]
    assert sorted(x[1] for x in takes) == [j for j in deferring if script[j] > 0]
    for j in range(nj):
        it, st = res[j]
        home = 2 * np.arange(script.get(j, 0) if j in deferring else 0) + 1
        want_it, want_st = np.full(pipe.batch, OWN_IT), np.zeros(pipe.batch, dtype=int)
        want_it[home], want_st[home] = 1000 * j + home + 1, POOL_ST
        assert np.array_equal(it, want_it) and np.array_equal(st, want_st), j
        own = e.index(("own", 7000 + j, kind))
        if home.size:
            (_, _, pool, off, _), = [x for x in takes if x[1] == j]
            assert own < e.index(("rows", 7000 + j, kind, off, tuple(int(x) for x in home))), "the pool's rows follow the job's own record write"
    assert len([x for x in e if x[0] == "rows"]) == len(takes)
    for p in pipe.pools:
        assert p.fill == 0 and p.routes == [] and not p.queued and p.idle.is_set()
    return takes


@pytest.mark.parametrize("summary", [False, True])
@pytest.mark.parametrize("nj,lefts", [(5, [3, 2, 0]), (6, [3, 2, 0, 3])])
def test_pool_routing_with_fake_handles(monkeypatch, nj, lefts, summary):
    script = dict(enumerate(lefts))
    pipe, log = _fake_pipeline(monkeypatch, script)
    if nj == 6:                                       # job 4, the last of its handle, flushes the filling pool: only after job 3 has found it full
        log.taken[3] = threading.Event()
        pipe.handles[0].gates[4] = log.taken[3]
    seen = []
    before = threading.active_count()
    kind, res = _call(lambda: pipe.run([None] * nj, on_done=lambda j, an: seen.append(j), record=lambda j: 7000 + j, records=nj, summary=summary))
    assert kind == "ok", res
    assert seen == list(range(nj)) and threading.active_count() == before
    takes = _check_pool_run(pipe, log, res, nj, script, "summary" if summary else "state")
    # job 0 fills P0 with 3 of 4 lanes; job 1's 2 do not fit: P0 is flushed, P1 is filled; job 3's 3 do not fit beside them: back to the emptied P0
    want = [("take", 0, "P0", 0, (1, 3, 5)), ("take", 1, "P1", 0, (1, 3))] + ([("take", 3, "P0", 0, (1, 3, 5))] if nj == 6 else [])
    assert takes == want


def test_pools_flip_when_the_filling_one_is_queued(monkeypatch):
    """A ring of 2 records: before worker 0 waits for the delivery of job 0 it flushes P0, which holds that job's stragglers.  While P0 is resumed job 1
    pauses with one straggler: it would fit into P0, but P0 is queued -- it goes to P1."""
    script = {0: 3, 1: 1, 2: 0}
    pipe, log = _fake_pipeline(monkeypatch, script)
    p0 = pipe.pools[0].handle
    p0.resume_gate = log.taken[1]
    pipe.handles[1].gates = {1: p0.resume_entered}
    kind, res = _call(lambda: pipe.run([None] * 5, on_done=lambda j, an: None, record=lambda j: 7000 + j, records=2))
    assert kind == "ok", res
    takes = _check_pool_run(pipe, log, res, 5, script, "state")
    assert takes == [("take", 0, "P0", 0, (1, 3, 5)), ("take", 1, "P1", 0, (1,))]


@pytest.mark.parametrize("what", ["resume", "run_defer"])
def test_a_failed_run_leaves_nothing_in_the_pools_for_the_next(monkeypatch, what):
    """A pool's resume raises, or a batch's run_defer does while a pool holds another job's stragglers: run() raises that error with no thread left behind --
    and the NEXT run of the same pipeline starts with empty pools (before, `routes` / `fill` / `queued` of the failed run survived: the next run handed
    stragglers to lanes behind the stale ones and waited for a pool that was never resumed)."""
    script = {0: 3, 1: 2, 2: 0}
    pipe, log = _fake_pipeline(monkeypatch, script)
    if what == "resume":
        pipe.pools[0].handle.fail = ("resume",)
    else:
        pipe.handles[1].fail = ("run_defer", 1)
    gates, pipe.handles[0].gates = pipe.handles[0].gates, {}              # (job 1 hands nothing over in this run: job 2 does not wait for it)
    before = threading.active_count()
    run = lambda: pipe.run([None] * 5, on_done=lambda j, an: None, record=lambda j: 7000 + j, records=5)         # noqa: E731
    kind, e = _call(run)
    assert kind == "error" and isinstance(e, RuntimeError) and f"{what} failed" in str(e)
    assert threading.active_count() == before
    assert any(x[0] == "take" and x[1] == 0 for x in log.entries), "the failed run did hand stragglers to a pool"
    pipe.pools[0].handle.fail = pipe.handles[1].fail = None
    pipe.handles[0].gates = gates
    log.new_run()
    kind, res = _call(run)
    assert kind == "ok", res
    assert threading.active_count() == before
    takes = _check_pool_run(pipe, log, res, 5, script, "state")
    assert takes == [("take", 0, "P0", 0, (1, 3, 5)), ("take", 1, "P1", 0, (1, 3))]
