#!/usr/bin/env python3
"""Times per-lane branch outages in the batched DC optimal power flow (setBranchOutages_, csrc/jg_dcopf.hip) on the 10k-bus grid of
tools/dcopf_time.py (the same synthetic costs, ratings and demand factors): 512 lanes of distinct non-bridge outages against the same 512 lanes
without outages.

    python tools/dcopf_outage_time.py [--out profiles/dcopf_outage_time.json] [--reps 25] [--lanes 512] [--case case_ACTIVSg10k]

The GPU step runs in a child process of its own under a time limit.  It records, for the handle without and with the outages, ms per iteration and per
kernel (jg_dcopf_time: HIP events, median of REPS; with outages also the correction of x~ and the build of W and the 2 x 2 inverses), and the set-up
of the outage set (host wall clock of the first solve_'s upload and build).  Nothing is compared against the code under test here; the tests do that
(tests/test_dcopf_outage_gpu.py).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("iteration", "rhs", "sweep_pair", "update", "residual_verdict", "assemble_refactorise", "outage_correction", "outage_build_w")


def kernels(jg, an, reps, count):
    from dcopf_time import stats
    L, check = jg._lib.lib(), jg._lib.check
    out = {}
    for k, name in enumerate(NAMES[:count]):
        warm = np.zeros(3)
        check(L.jg_dcopf_time(an._h, k, 3, warm))
        ms = np.zeros(reps)
        check(L.jg_dcopf_time(an._h, k, reps, ms))
        out[name + "_ms"] = stats(ms, reps)
    return out


def step_opf(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    from dcopf_time import build
    jg, s, demand = build(a)
    opf = jg.dcoptimalpowerflow
    labels = [int(k) for k in jg.outageList(s, a.lanes, seed=7)]          # non-bridge, in service; distinct while the grid has that many
    out = dict(lanes=a.lanes, distinct_outages=len(set(labels)))
    for name, outages in (("without", None), ("with", labels)):
        an = jg.dcOptimalPowerFlow(s, batch=a.lanes, tolerance=1e-6, iteration=a.iteration)
        opf.setInjection_(an, demand)
        if outages:
            opf.setBranchOutages_(an, outages)
        t0 = time.perf_counter()
        opf.solve_(an, iteration=25)                                    # uploads the bounds and the outage set, builds W; one check
        first = (time.perf_counter() - t0) * 1e3
        out[name] = dict(first_25_iterations_wall_ms=first, variables=an.model.n, rows=an.model.m, **kernels(jg, an, a.reps, 8 if outages else 6))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcopf_outage_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--iteration", type=int, default=20000)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=("opf",))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DCOPF_OUTAGE_TIME_JSON " + json.dumps(step_opf(a), default=str))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "opf", "--reps", str(a.reps), "--lanes", str(a.lanes), "--iteration", str(a.iteration),
           "--case", a.case]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)                    # a time limit of its own
    line = [l for l in r.stdout.splitlines() if l.startswith("DCOPF_OUTAGE_TIME_JSON ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"step opf failed (exit {r.returncode})")
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps, opf=json.loads(line[0][len("DCOPF_OUTAGE_TIME_JSON "):]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
