#!/usr/bin/env python3
"""Times the branch status tests (dcTopologyScreen, csrc/jg_dcse_topology.hip) on the set of tools/dcse_time.py: the 10k-bus grid, injection + from + to
wattmeters at 1e-2, bus PMUs at 1e-5, m = 45 412 rows, every branch a candidate (12 706 = 25 blocks of 512), batch 512.

    python tools/dcse_topology_time.py [--out profiles/dcse_topology_time.json] [--reps 25] [--case case_ACTIVSg10k] [--sample 64]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  screen   the denominators (jg_dcse_topology_time 0: all blocks; 1, 2, 3: the right-hand sides, the sweep pair and the denominator kernel of one block),
           the statistic pass over candidates x lanes (4), the correction (5) -- HIP events, median of REPS --, the whole call (host wall clock, the
           denominators cached), what it found, and the candidates of the sample checked against the route below
  dense    the numpy route on SAMPLE candidates on one core: splu of the gain, x_k = G^-1 H' W m_k, D_k, and t for 512 lanes; extrapolated to all
           candidates (no GPU)
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

LANES = 512


def sample_candidates(S, t, ms, cand, Z):
    """(seconds, D, norm, t [sample, lanes]) of the candidates `cand` (0-based) by sparse solves; Z [lanes, m]"""
    import scipy.sparse.linalg as sla
    import dcse_topology_reference as T
    rb = S.Rebuilt(t, ms)
    M = T.columns(t, ms)[:, cand]
    w = rb.w * rb.status
    t0 = time.perf_counter()
    lu = sla.splu(rb.G)
    g = rb.H.T @ (w[:, None] * M)
    X = lu.solve(g)
    norm = (w[:, None] * M * M).sum(axis=0)
    D = norm - (g * X).sum(axis=0)
    th = lu.solve(rb.H.T @ (w[:, None] * Z.T))
    th[rb.slack] = 0.0
    r = Z.T * rb.status[:, None] - rb.H @ th
    tt = ((w[:, None] * M).T @ r) / np.sqrt(D)[:, None]
    return time.perf_counter() - t0, D, norm, tt


def readings(jg, an, seed=5):
    jg.setNoise_(an, np.random.default_rng(seed))
    return an.readings.copy()


def step_screen(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    jg, R, S, t, ms, mon = build(a)
    an = jg.dcStateEstimation(mon, batch=LANES)
    Z = readings(jg, an)
    jg.solveSE_(an)
    L, check = jg._lib.lib(), jg._lib.check
    got = jg.dcTopologyScreen(an)                                    # candidates, denominators: warm-up
    out = dict(dims=an.dims(), rows=an.method.number, candidates=int(got.candidates.size), blocks=(got.candidates.size + 511) // 512, lanes=LANES)

    def timed(kernel, reps):
        ms_ = np.zeros(3)
        check(L.jg_dcse_topology_time(an._h, kernel, 3, ms_))
        ms_ = np.zeros(reps)
        check(L.jg_dcse_topology_time(an._h, kernel, reps, ms_))
        return stats(ms_, reps)

    out["denominators_all_blocks_ms"] = timed(0, 5)
    out["rhs_one_block_ms"] = timed(1, a.reps)
    out["sweep_pair_one_block_ms"] = timed(2, a.reps)
    out["denominator_kernel_one_block_ms"] = timed(3, a.reps)
    out["statistic_pass_ms"] = timed(4, a.reps)
    out["correction_ms"] = timed(5, a.reps)
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = jg.dcTopologyScreen(an, dense=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["whole_call_cached_ms"] = dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall)), reps=3, clock="host wall")
    out["found"] = dict(status_counts=np.bincount(got.status, minlength=3).tolist(), records=got.total)
    cand = got.candidates[np.linspace(0, got.candidates.size - 1, a.sample).astype(np.int64)] - 1
    pos = np.searchsorted(got.candidates, cand + 1)
    _, D, norm, tt = sample_candidates(S, t, ms, cand, Z)
    ok = got.status[pos] == 0
    out["sample"] = int(cand.size)
    out["sample_worst_D_over_norm"] = float(np.abs(got.denominator[pos] / got.norm[pos] - D / norm).max())
    out["sample_worst_statistic_scaled"] = float(np.max(np.abs(got.statisticAll[pos][ok] - tt[ok]) / np.maximum(1.0, np.abs(tt[ok]))))
    an.close()
    return out


def step_dense(a):
    jg, R, S, t, ms, mon = build(a)
    an_rows = S.model(t, ms).number
    nbr = np.asarray(t["br_from"]).size
    cand = np.linspace(0, nbr - 1, a.sample).astype(np.int64)
    Z = np.random.default_rng(5).standard_normal((LANES, an_rows))
    sec = sample_candidates(S, t, ms, cand, Z)[0]
    return dict(sample=int(cand.size), sample_ms=sec * 1e3, all_candidates_ms_extrapolated=sec * 1e3 * nbr / cand.size, threads=1)


STEPS = {"screen": (step_screen, 900), "dense": (step_dense, 900)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcse_topology_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--sample", type=int, default=64)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DCSE_TOPOLOGY_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("screen", "dense"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--sample", str(a.sample), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "dense" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DCSE_TOPOLOGY_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DCSE_TOPOLOGY_TIME_JSON "):])
    sc = result["screen"]
    result["sweep_pairs_all_blocks_ms"] = sc["sweep_pair_one_block_ms"]["median"] * sc["blocks"]
    result["speedup_over_dense_route"] = result["dense"]["all_candidates_ms_extrapolated"] / (sc["denominators_all_blocks_ms"]["median"] + sc["statistic_pass_ms"]["median"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
