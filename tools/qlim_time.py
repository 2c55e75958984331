"""Timing of reactive limits on a batch (jgrid.h: jg_nr_set_bus_type, jg_nr_reactive_limit): on case_ACTIVSg10k with 512 lanes (N-1 outages started
from the base-case solution) it prints one JSON line with
  asm_plain_ms / asm_lane_typed_ms   the batched assembly (jg_nr_time_kernel 0) without and with per-lane bus types,
  limit_ms                           one jg_nr_reactive_limit call (host wall clock: kernels + the copies of violate / counts),
  nr_iter_ms                         one batched NR iteration of the first solve (wall clock / iterations of the slowest lane),
  screen_ms / screen_limit_ms        powerFlow_ of the batch, without and with one round of reactiveLimit_ + powerFlow_.
Usage: python tools/qlim_time.py [case] [lanes]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import juliagrid.jl_amd as jg  # noqa: E402
from conftest import load_case  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "case_ACTIVSg10k"
    lanes = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    t = load_case(name)
    system = jg.powerSystem(t)
    base = jg.newtonRaphson(jg.powerSystem(t))
    jg.powerFlow_(base)
    labels = [int(x) for x in jg.outageList(system, lanes, seed=17)]
    an = jg.contingencyAnalysis(system, labels)
    jg.setInitialPoint_(an, base)
    jg.powerFlow_(an, fetch=False)                               # warm-up: graphs, plan
    out = dict(case=name, lanes=lanes)
    out["asm_plain_ms"] = an.time_kernel(0, 50)
    # per-lane types: the first PV bus turned PQ in every lane (values only; the plan is the same)
    tp = system.bus.layout.type.copy()
    tp[np.flatnonzero(tp == 2)[0]] = 1
    jg.setBusType_(an, tp)
    out["asm_lane_typed_ms"] = an.time_kernel(0, 50)
    jg.setBusType_(an, None)
    jg.setInitialPoint_(an, base)
    t0 = time.perf_counter()
    jg.powerFlow_(an, fetch=False)
    out["screen_ms"] = 1e3 * (time.perf_counter() - t0)
    out["nr_iter_ms"] = out["screen_ms"] / max(1, int(np.max(an.method.iteration)))
    jg.powerflow._upload_generators(an)
    viol = np.zeros((an.batch, system.generator.number), dtype=np.int8)
    cnt = np.zeros(an.batch, dtype=np.int32)
    t0 = time.perf_counter()
    jg._lib.check(jg._lib.lib().jg_nr_reactive_limit(an._h, 0, viol.ctypes.data, cnt.ctypes.data))
    out["limit_ms"] = 1e3 * (time.perf_counter() - t0)
    out["violating_lanes"] = int(np.sum(cnt > 0))
    jg.setBusType_(an, None)
    jg.setInjection_(an)
    jg.setOutages_(an, labels)
    jg.setInitialPoint_(an, base)
    t0 = time.perf_counter()
    jg.powerFlow_(an, fetch=False)
    jg.reactiveLimit_(an)
    jg.powerFlow_(an, fetch=False)
    out["screen_limit_ms"] = 1e3 * (time.perf_counter() - t0)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
