"""The ordered runner under ContingencyPipeline and MonteCarloPipeline: a list of jobs solved on a few handles, one host thread per handle,
delivered to the caller in job order.

Nothing here knows what a job or a handle is: the pipelines give a `solve(k, j)` and their hooks, the straggler pool of the contingency pipeline
(contingency._StragglerPools) joins a run through `wait_solved` / `failed` / `fail`.  The module imports the standard library only, so the whole
ordering protocol runs under pytest with stub handles and without the HIP library (tests/test_pipeline_order_cpu.py).
"""
from __future__ import annotations

import threading


class OrderedRun:
    """One run of `nj` jobs on `len(handles)` handles.

    Workers: worker k calls solve(k, j) for j = k, k + nh, ... on its own thread; what solve returns is job j's entry in the list run() returns.
    Handle reuse: job j starts once the handle is released by job j - nh -- when its solve returned (hold=False: nothing of it lives in the handle any more;
        the worker's own order, no wait), or when the caller has delivered it (hold=True: on_done reads the handle).
    Ring: with ring > 0 job j starts once job j - ring is delivered (the caller's ring of record buffers: record(j) may be record(j - ring)'s memory);
        `before_ring_wait()` runs once before that wait, if there is a wait.
    Delivery: the caller's thread walks j = 0 .. nj - 1: waits for solve(j), runs `complete(j)`, calls on_done(j, handles[j % nh]), marks j delivered.
    Errors: an exception in a worker, a hook, on_done, or one handed in through fail() releases every wait (`on_fail()` releases the collaborator's own);
        no job starts afterwards, every worker is joined, then run() raises: the caller's own failure (on_done, complete) first, else the first recorded."""

    def __init__(self, handles, nj: int, hold: bool = False, ring: int = 0):
        self.handles = list(handles)
        self.nh, self.nj, self.hold, self.ring = len(self.handles), int(nj), bool(hold), max(0, int(ring))
        self.results = [None] * self.nj
        self.errors = []
        self._solved = [threading.Event() for _ in range(self.nj)]        # solve(j) has returned, results[j] is there
        self._delivered = [threading.Event() for _ in range(self.nj)]     # on_done(j) has returned
        self._on_fail = None

    @property
    def failed(self) -> bool:
        return bool(self.errors)

    def fail(self, error: BaseException, first: bool = False):
        """Records `error` and releases every wait of the run: surface in the caller, never hang it."""
        if first:
            self.errors.insert(0, error)
        else:
            self.errors.append(error)
        for ev in self._solved + self._delivered:
            ev.set()
        if self._on_fail is not None:
            self._on_fail()

    def solved(self, j: int) -> bool:
        return self._solved[j].is_set()

    def wait_solved(self, j: int):
        """Blocks until solve(j) has returned; its result, or None when the run has failed."""
        self._solved[j].wait()
        return None if self.errors else self.results[j]

    def _worker(self, k, solve, before_ring_wait):
        try:
            for j in range(k, self.nj, self.nh):
                if self.hold and j - self.nh >= 0:
                    self._delivered[j - self.nh].wait()
                if self.ring and j - self.ring >= 0 and not self._delivered[j - self.ring].is_set():
                    if before_ring_wait is not None:
                        before_ring_wait()
                    self._delivered[j - self.ring].wait()
                if self.errors:
                    return
                self.results[j] = solve(k, j)
                self._solved[j].set()
        except BaseException as e:
            self.fail(e)

    def run(self, solve, on_done=None, before_ring_wait=None, complete=None, on_fail=None) -> list:
        self._on_fail = on_fail
        threads = [threading.Thread(target=self._worker, args=(k, solve, before_ring_wait), daemon=True) for k in range(self.nh)]
        for t in threads:
            t.start()
        try:
            for j in range(self.nj):
                self._solved[j].wait()
                if complete is not None and not self.errors:
                    complete(j)
                if self.errors:
                    break
                if on_done is not None:
                    on_done(j, self.handles[j % self.nh])
                self._delivered[j].set()
        except BaseException as e:                 # the caller's own on_done failed: the workers must not wait for deliveries that never come
            self.fail(e, first=True)
        finally:
            for t in threads:
                t.join()
        if self.errors:
            raise self.errors[0]
        return self.results


def gatherBlocks(dist, packed):
    """ONE collective of a sharded run: every rank contributes its contiguous [rows, width] block and receives the global block in rank order.
    `dist` is an initialised torch.distributed module; the tensor must live on the backend's device."""
    packed = packed.contiguous()
    g = packed.new_empty((dist.get_world_size() * packed.shape[0], packed.shape[1]))
    dist.all_gather_into_tensor(g, packed)
    return g
