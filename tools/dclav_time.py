#!/usr/bin/env python3
"""Times the batched DC least-absolute-value estimator (dcLavStateEstimation, csrc/jg_dclav.hip) on the 10k-bus grid's full measurement set (injection +
from + to wattmeters at 1e-2, bus PMUs at 1e-5): LANES realisations with seeded noise, three gross errors in every fourth lane.

    python tools/dclav_time.py [--out profiles/dclav_time.json] [--reps 10] [--lanes 128] [--case case_ACTIVSg10k] [--sample 2]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  lav    set-up (host wall clock of dcLavStateEstimation), the handle's dims (bytes per lane among them), wall clock of a solve of the batch, the
         lanes' iteration counts and statuses, ms per iteration and per part (jg_dclav_time_kernel: HIP events, median of REPS, every lane running)
  host   scipy.optimize.linprog (HiGHS) on SAMPLE lanes on one core: seconds per lane (no GPU); `extrapolated` = that x LANES, stated as such
Nothing is compared against the code under test here; the tests do that (tests/test_dclav_gpu.py).
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

SEED = 13
KERNELS = ("iteration", "assembly", "factorisation", "sweep_pair", "passes")


def build(a):
    import dc_reference as R
    import dcse_reference as S
    from conftest import load_case
    t = load_case(a.case)
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    z = S.model(t, ms).mean
    rng = np.random.default_rng(SEED)
    sigma = np.sqrt(np.r_[ms.w_variance, ms.p_variance])
    Z = z[None, :] + sigma[None, :] * rng.standard_normal((a.lanes, z.size))
    for s in range(0, a.lanes, 4):
        Z[s, rng.choice(ms.w_index.size, 3, replace=False)] += 5.0
    return t, ms, Z


def step_lav(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    from test_dcse_host import monitoring_of
    t, ms, Z = build(a)
    lav = jg.dclavstateestimation
    t0 = time.perf_counter()
    an = jg.dcLavStateEstimation(monitoring_of(jg, t, ms), batch=a.lanes)
    setup = time.perf_counter() - t0
    lav.setReadings_(an, Z)
    t0 = time.perf_counter()
    lav.solve_(an)
    wall = time.perf_counter() - t0
    it = np.atleast_1d(an.iterations)
    out = dict(setup_s=setup, dims=an.dims(), solve_wall_s=wall, iterations=dict(min=int(it.min()), median=float(np.median(it)), max=int(it.max())),
               status={str(k): int(v) for k, v in zip(*np.unique(np.atleast_1d(an.status), return_counts=True))}, ms={})
    for k, name in enumerate(KERNELS):
        ms_k = an.time_kernel(k, a.reps)
        out["ms"][name] = dict(median=float(np.median(ms_k)), min=float(ms_k.min()), max=float(ms_k.max()), reps=int(a.reps))
    an.close()
    return out


def step_host(a):
    import dclav_reference as L
    import dcse_reference as S
    t, ms, Z = build(a)
    H, _, on, slack = L.lav_rows(t, ms)
    secs = []
    for s in range(a.sample):
        t0 = time.perf_counter()
        L.lav_linprog(H, Z[s] * on, on, slack)
        secs.append(time.perf_counter() - t0)
    per = float(np.median(secs))
    return dict(linprog_s_per_lane=per, sample=a.sample, extrapolated_s_for_batch=per * a.lanes,
                note="linprog per lane on one core, dense constraint matrix; the batch figure is the sample's median x lanes, not a run")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dclav_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--lanes", type=int, default=128)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--sample", type=int, default=2)
    p.add_argument("--step", default=None)
    a = p.parse_args()
    if a.step:
        print("__RESULT__" + json.dumps({"lav": step_lav, "host": step_host}[a.step](a)))
        return
    result = dict(case=a.case, lanes=a.lanes, seed=SEED)
    for step, limit in (("lav", 600), ("host", 1200)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case, "--sample", str(a.sample)]
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
