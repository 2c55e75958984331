#!/usr/bin/env python3
"""Times the batched PMU least-absolute-value estimator (pmuLavStateEstimation, csrc/jg_pmulav.hip) on the 10k-bus grid with a bus PMU at every bus and a
PMU at both ends of every in-service branch: LANES realisations with seeded noise of 1e-3 on magnitude and angle, three gross phasor errors (magnitude
x 1.5, angle + 0.5 rad) in every fourth lane.  The readings come from the Newton-Raphson state of the grid, solved on the device in the same step.

    python tools/pmulav_time.py [--out profiles/pmulav_time.json] [--reps 10] [--lanes 512] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  pmulav  set-up (host wall clock of pmuLavStateEstimation), the handle's dims (bytes per lane among them), wall clock of a solve of the batch, the
          lanes' iteration counts and statuses, ms per iteration split as tools/dclav_time.py splits it (jg_pmulav_time_kernel 0 .. 4) and of the four
          new kernels (5 .. 8: polar -> rectangular, rectangular -> polar, branches and buses, suspects); HIP events, median of REPS, every lane running
  dclav   the DC LAV iteration of tools/dclav_time.py on the same grid with the same number of lanes, for scale
Nothing is compared against the code under test here; the tests do that (tests/test_pmulav_gpu.py).
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

SEED = 13
ITERATION = ("iteration", "assembly", "factorisation", "sweep_pair", "passes")
KERNELS = ("k_pmu_rect", "k_pmu_polar", "k_pmu_branch", "k_pmu_suspect")


def step_pmulav(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    from conftest import load_case
    lav = jg.pmulavstateestimation
    system = jg.powerSystem(load_case(a.case))
    pf = jg.newtonRaphson(system)
    jg.powerFlow_(pf)
    mon = jg.measurement(system)
    jg.addPmu_(mon, pf)
    pf.close()
    t0 = time.perf_counter()
    an = jg.pmuLavStateEstimation(mon, batch=a.lanes)
    setup = time.perf_counter() - t0
    rng = np.random.default_rng(SEED)
    P = mon.pmu.number
    mag = np.array(mon.pmu.magnitude.mean)[None, :] + 1e-3 * rng.standard_normal((a.lanes, P))
    ang = np.array(mon.pmu.angle.mean)[None, :] + 1e-3 * rng.standard_normal((a.lanes, P))
    for s in range(0, a.lanes, 4):
        d = rng.choice(P, 3, replace=False)
        mag[s, d] *= 1.5
        ang[s, d] += 0.5
    lav.setReadings_(an, mag, ang)
    t0 = time.perf_counter()
    lav.stateEstimation_(an, power=True)
    wall = time.perf_counter() - t0
    lav.suspect_(an, 0.05)
    it = np.atleast_1d(an.iterations)
    out = dict(setup_s=setup, dims=an.dims(), pmus=P, solve_wall_s=wall, iterations=dict(min=int(it.min()), median=float(np.median(it)), max=int(it.max())),
               status={str(k): int(v) for k, v in zip(*np.unique(np.atleast_1d(an.status), return_counts=True))}, ms={})
    for k, name in enumerate(ITERATION + KERNELS):
        ms_k = an.time_kernel(k, a.reps)
        out["ms"][name] = dict(median=float(np.median(ms_k)), min=float(ms_k.min()), max=float(ms_k.max()), reps=int(a.reps))
    an.close()
    return out


def step_dclav(a):
    import dclav_time
    return dclav_time.step_lav(a)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pmulav_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", default=None)
    a = p.parse_args()
    if a.step:
        print("__RESULT__" + json.dumps({"pmulav": step_pmulav, "dclav": step_dclav}[a.step](a)))
        return
    result = dict(case=a.case, lanes=a.lanes, seed=SEED)
    for step, limit in (("pmulav", 900), ("dclav", 600)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        line = [l for l in r.stdout.splitlines() if l.startswith("__RESULT__")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"step {step} failed with code {r.returncode}: the run ends here")
        result[step] = json.loads(line[0][len("__RESULT__"):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
