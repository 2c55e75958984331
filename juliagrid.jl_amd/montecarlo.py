"""Sharded Monte-Carlo state estimation: noisy realisations of ONE measurement set as the lanes of Gauss-Newton batches.

The reference draws a realisation inside `add<Meter>!(...; noise = true)` (/root/reference/src/measurement/utility.jl:70-73:
`mean + variance^(1/2) * randn`) and estimates one at a time (`stateEstimation!`, src/stateEstimation/acStateEstimation.jl:1286-1329);
a Monte-Carlo study is a user-level loop over both.  Realisations share rows, type codes, Jacobian and gain pattern and the symbolic
analysis: here `batch` of them advance together in one handle, several handles keep the GPU busy, the realisations of a study shard across
GPUs contiguously (contingency.shard) and ONE collective carries the result record of every batch (for the estimator what
ContingencyPipeline is for the power flow).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .measurement import Measurement
from .pipeline import OrderedRun, gatherBlocks
from .stateestimation import AcStateEstimation, drawNoise_, gaussNewton, setNoise_, stateEstimation_

RECORD_TAIL = 3         # iterations | status | objective behind magnitude[n] | angle[n]


class MonteCarloPipeline:
    """`inflight` batches of `batch` realisations each in flight on one GPU: a handle, a HIP stream and a host thread per batch (the narrow
    launches of one batch's factorisation are filled by the others').

    A job is one batch of realisations: an integer SEED or a pair (seed, first realisation) -- the handle draws realisations first .. first + batch - 1 of
    that seed ON THE DEVICE (stateestimation.drawNoise_: counter-based generator + the acWLS value rules, nothing over PCIe; a rank of a sharded study passes
    its own `first`) --, `host_noise=True` draws them with numpy's PCG64(seed) on the host instead (setNoise_: [batch, m] arrays over PCIe), or None (the
    handle keeps the realisations it holds: a timing loop).  Every job restarts from the pipeline's start point, which stays in HBM.  `on_done(job, analysis)` runs on the CALLER's thread in job order -- where a sharded
    run issues its gather (collectives must be issued in the same order on every rank)."""

    def __init__(self, monitoring: Measurement, batch: int, inflight: int = 2, device: int = 0, start=None, method=None, scale: float = 1.0, host_noise: bool = False):
        self.monitoring, self.batch, self.scale, self.host_noise = monitoring, int(batch), float(scale), bool(host_noise)
        kw = {} if method is None else {"method": method}
        self.handles = [gaussNewton(monitoring, batch=self.batch, device=device, **kw) for _ in range(max(1, int(inflight)))]
        n = monitoring.system.bus.number
        vm, va = (np.ones(n), np.zeros(n)) if start is None else start          # flat start (BASELINE config 4) unless told otherwise
        for h in self.handles:
            h.setVoltage(vm, va)
            h.snapshot_voltage()

    @property
    def record_width(self) -> int:
        return 2 * self.monitoring.system.bus.number + RECORD_TAIL

    def close(self):
        for h in self.handles:
            h.close()
        self.handles = []

    def run(self, jobs, iteration: int = 40, tolerance: float = 1e-8, on_done=None, record=None, records: int = 0):
        """jobs: sequence of seeds / None.  record: optional callable job -> DEVICE pointer of a [batch, 2 n + 3] float64 buffer, complete when
        on_done(job, .) is called; the caller owns a ring of `records` buffers (job j + records is not written before on_done(j) has returned).
        Returns per-job (iterations, status) arrays."""
        jobs = list(jobs)
        ring = int(records) if (record is not None and records) else 0
        run = OrderedRun(self.handles, len(jobs), hold=self._hold(record, on_done), ring=ring)
        return run.run(lambda k, j: self._solve(self.handles[k], j, jobs[j], iteration, tolerance, record), on_done)

    @staticmethod
    def _hold(record, on_done) -> bool:
        """Whether the handle of job j waits for the delivery of j before it starts job j + nh: without a record the results live in the handle until the
        caller's on_done has seen them.  (Not ContingencyPipeline's rule: with a record AND an on_done this handle goes on, and with neither it goes on too.)"""
        return on_done is not None and record is None

    def _prepare(self, h, job):
        if job is not None:
            seed, first = (job if isinstance(job, (tuple, list)) else (job, 0))
            if self.host_noise:
                setNoise_(h, np.random.Generator(np.random.PCG64(int(seed))), scale=self.scale)
            else:
                drawNoise_(h, int(seed), scale=self.scale, first=int(first))
        h.restore_voltage()

    def _solve(self, h, j, job, iteration, tolerance, record):
        """Job j on handle `h` (a worker's thread): (iterations, status) per realisation, and the job's record written."""
        self._prepare(h, job)
        stateEstimation_(h, iteration=iteration, tolerance=tolerance, fetch=False)
        result = (np.array(h.method.iteration), np.array(h.status))
        if record is not None:
            h.pack_results_device(record(j))
        return result


def gatherEstimates(dist, packed):
    """Final gather of a sharded Monte-Carlo batch: ONE collective.  `packed` is this rank's [realisations, 2 n + 3] record
    (AcStateEstimation.pack_results_device); returns (iterations, status, objective, magnitude, angle) of the global block in realisation order."""
    return unpackEstimates(gatherBlocks(dist, packed))


def gatherEstimatesDevice(an: AcStateEstimation, comm, out_ptr: int):
    """The same gather through the C ABI alone (jg_gn_allgather_results: pack + ncclAllGather of RCCL on the handle's stream); `out_ptr`: device
    memory for [world x batch][2 n + 3] doubles."""
    _lib.check(_lib.lib().jg_gn_allgather_results(an._h, comm.h, _lib.VP(int(out_ptr))))


def unpackEstimates(g):
    """(iterations, status, objective, magnitude, angle) of a [realisations, 2 n + 3] record."""
    n = (g.shape[1] - RECORD_TAIL) // 2
    return g[:, 2 * n].long(), g[:, 2 * n + 1].long(), g[:, 2 * n + 2], g[:, :n], g[:, n:2 * n]
