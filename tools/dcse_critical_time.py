#!/usr/bin/env python3
"""Times the critical-measurement and critical-pair screen (dcCriticalScreen, csrc/jg_dcse_critical.hip) on the set of tools/dcse_time.py: the 10k-bus
grid, injection + from + to wattmeters at 1e-2, bus PMUs at 1e-5, m = 45 412 rows = 89 blocks of 512 columns.

    python tools/dcse_critical_time.py [--out profiles/dcse_critical_time.json] [--reps 25] [--case case_ACTIVSg10k] [--sample 64]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  screen   the sweep pair of 512 lanes and the Omega diagonal (jg_dcse_time_kernel 2 and 5: the same sweep pairs the screen runs), the cross pass over
           all rows against one block of columns (jg_dcse_critical_time_kernel, HIP events, median of REPS), the whole call (host wall clock around a
           call that ends in a device synchronise; critical pairs only, and with correlation 0.9, whose write pass repeats the sweep pairs of the blocks
           that hold a record), what it found, and the columns of the sample checked against the route below
  dense    the numpy route on SAMPLE columns on one core: splu of the gain, U = G^-1 h_j', Omega[:, j] = -H U, gamma and the arg-max; extrapolated to all
           m columns (no GPU)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dcse_time import build, stats  # noqa: E402

SINGULAR = 1e-6


def sample_columns(S, t, ms, cols):
    """(seconds, partner, gamma of the partner, Omega_jj) of the columns `cols` by sparse solves and dense algebra; the full diagonal comes first"""
    import scipy.sparse.linalg as sla
    rb = S.Rebuilt(t, ms)
    d = rb.variances(dense=True)
    t0 = time.perf_counter()
    lu = sla.splu(rb.G)
    U = lu.solve(rb.H[cols].T.toarray())
    Om = -(rb.H @ U)                                                # [m, sample]
    live = (rb.status > 0) & (rb.w * d > SINGULAR)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = Om / np.sqrt(np.outer(d, d[cols]))
    g[~live] = 0.0
    g[cols, np.arange(cols.size)] = 0.0
    i = np.argmax(np.abs(g), axis=0)
    sec = time.perf_counter() - t0
    return sec, i, g[i, np.arange(cols.size)], d


def step_screen(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    jg, R, S, t, ms, mon = build(a)
    an = jg.dcStateEstimation(mon, batch=512)
    jg.solveSE_(an)
    L, check = jg._lib.lib(), jg._lib.check
    m = an.method.number
    blocks = (m + 511) // 512
    out = dict(dims=an.dims(), rows=m, blocks=blocks)
    an.time_kernel(2, 5)
    out["sweep_pair_ms"] = stats(an.time_kernel(2, a.reps), a.reps)
    out["omega_diagonal_and_pass_ms"] = stats(an.time_kernel(5, 3), 3)
    ms_ = np.zeros(5)
    check(L.jg_dcse_critical_time_kernel(an._h, 5, ms_))             # warm-up
    ms_ = np.zeros(a.reps)
    check(L.jg_dcse_critical_time_kernel(an._h, a.reps, ms_))
    out["cross_pass_one_block_ms"] = stats(ms_, a.reps)
    out["cross_pass_all_blocks_ms"] = out["cross_pass_one_block_ms"]["median"] * blocks
    nnz = int(an._ptr[-1])
    out["gathered_bytes_per_block"] = nnz * 512 * 8
    out["gather_TB_per_s"] = out["gathered_bytes_per_block"] / (out["cross_pass_one_block_ms"]["median"] * 1e-3) / 1e12
    jg.dcCriticalScreen(an)                                         # warm-up
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = jg.dcCriticalScreen(an)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["whole_call_ms"] = dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall)), reps=3, clock="host wall")
    t0 = time.perf_counter()
    corr = jg.dcCriticalScreen(an, correlation=0.9, capacity=1 << 20)
    out["whole_call_correlation_0_9_ms"] = dict(value=(time.perf_counter() - t0) * 1e3, reps=1, clock="host wall")
    out["found"] = dict(singles=got.totalSingles, pairs=got.totalPairs, correlated_0_9=corr.totalCorrelated)
    cols = np.linspace(0, m - 1, a.sample).astype(np.int64)
    _, i, g, d = sample_columns(S, t, ms, cols)
    out["sample_worst_variance"] = float(np.abs(got.variance - d).max())
    out["sample_worst_partner_correlation"] = float(np.nanmax(np.abs(np.abs(got.partnerCorrelation[cols]) - np.abs(g))))
    out["sample_partners_equal"] = int(np.sum(got.partner[cols] == i + 1))
    out["sample"] = int(cols.size)
    an.close()
    return out


def step_dense(a):
    jg, R, S, t, ms, mon = build(a)
    m = S.model(t, ms).number
    cols = np.linspace(0, m - 1, a.sample).astype(np.int64)
    sec = sample_columns(S, t, ms, cols)[0]
    return dict(sample=int(cols.size), sample_ms=sec * 1e3, all_columns_ms_extrapolated=sec * 1e3 * m / cols.size, threads=1)


STEPS = {"screen": (step_screen, 900), "dense": (step_dense, 900)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcse_critical_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--sample", type=int, default=64)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DCSE_CRITICAL_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("screen", "dense"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--sample", str(a.sample), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "dense" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DCSE_CRITICAL_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DCSE_CRITICAL_TIME_JSON "):])
    sc = result["screen"]
    result["sweep_pairs_all_blocks_ms"] = sc["sweep_pair_ms"]["median"] * sc["blocks"]
    result["cross_over_sweep_pairs"] = sc["cross_pass_all_blocks_ms"] / result["sweep_pairs_all_blocks_ms"]
    result["speedup_over_dense_route"] = result["dense"]["all_columns_ms_extrapolated"] / sc["whole_call_ms"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
