#!/usr/bin/env python3
"""Times DC state estimation with batched bad-data removal: the 10k-bus grid, the full set (injection + from + to wattmeters at 1e-2, bus PMUs at 1e-5,
m = 45 412), 512 noisy realisations, kernel times through HIP events after a warm-up, medians of REPS runs.

    python tools/dcse_time.py [--out profiles/dcse_time.json] [--reps 25] [--lanes 512] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  dcse   set-up (symbolic analysis + gain assembly + factorisation: host wall clock of dcStateEstimation), the Omega diagonal, the chain of a batch and
         its parts (jg_dcse_time_kernel), a removal round (residual test + one new column of U per lane + the compensated solve; host wall clock around
         calls that end in a device synchronise), angles checked against the restatement on a handful of lanes
  splu   the same work by the restatement on one core: assemble + splu + a solve per realisation; rebuild + refactorise per removal (no GPU)
The sweep pair runs the kernels of the DC screen on a denser factor: the ratio to its measured time (profiles/dc_time.json) is reported beside the
ratio of the padded sweep terms of the two factors.
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


def build(a):
    import juliagrid.jl_amd as jg
    import dc_reference as R
    import dcse_reference as S
    from conftest import load_case
    from test_dcse_host import monitoring_of
    t = load_case(a.case)
    t["bus_va"] = np.asarray(t["bus_va"], dtype=np.float64).copy()
    t["bus_va"][R.slack_of(t)] = 0.0                                 # (tests/test_dcse_gpu.py: at_zero)
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    return jg, R, S, t, ms, monitoring_of(jg, t, ms)


def stats(ms, reps):
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(reps))


def step_dcse(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    jg, R, S, t, ms, mon = build(a)
    t0 = time.perf_counter()
    an = jg.dcStateEstimation(mon, batch=a.lanes)
    create_ms = (time.perf_counter() - t0) * 1e3
    jg.setNoise_(an, np.random.default_rng(1))
    t0 = time.perf_counter()
    jg.solveSE_(an)
    first_ms = (time.perf_counter() - t0) * 1e3
    rb = S.Rebuilt(t, ms)
    worst = max(R.worst(an.voltage.angle[i], rb.solve(an.readings[i])) for i in (0, 1, a.lanes // 2, a.lanes - 1))
    assert worst <= 1e-9, worst
    out = dict(dims=an.dims(), create_ms=create_ms, first_solve_ms=first_ms, worst_angle_vs_restatement=worst)
    for name, k in (("chain", 0), ("rhs", 1), ("sweep_pair", 2), ("residual_pass", 3), ("normalised_pass", 4)):
        an.time_kernel(k, 5)                                        # warm-up
        out[name + "_ms"] = stats(an.time_kernel(k, a.reps), a.reps)
    out["omega_diagonal_and_pass_ms"] = stats(an.time_kernel(5, 3), 3)
    out["estimates_per_s"] = a.lanes / (out["chain_ms"]["median"] * 1e-3)
    # a removal round: every lane gets a gross error of its own, the test removes it, the next solve compensates
    m, n = an.method.number, an.system.bus.number
    rows = np.r_[np.arange(n), np.arange(m - n, m)]
    z = an.readings.copy()
    pick = rows[(np.arange(a.lanes) * 37) % rows.size]
    z[np.arange(a.lanes), pick] += 3000.0 / np.sqrt(an.method.precision[pick])
    jg.setReadings_(an, z)
    jg.solveSE_(an)
    t0 = time.perf_counter()
    res = jg.residualTest_(an, threshold=3.0)
    test_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    jg.solveSE_(an)
    solve_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(res.index - 1, pick), "the planted rows were not the ones removed"
    out["removal_round"] = dict(residual_test_and_new_columns_ms=test_ms, compensated_solve_with_copies_ms=solve_ms, lanes=int(a.lanes), clock="host wall, one run")
    an.time_kernel(0, 5)
    out["chain_with_one_removed_row_ms"] = stats(an.time_kernel(0, a.reps), a.reps)
    i = a.lanes // 3
    out["worst_removed_angle_vs_restatement"] = R.worst(an.voltage.angle[i], S.Rebuilt(t, ms, [int(pick[i])]).solve(z[i]))
    an.close()
    return out


def step_splu(a):
    jg, R, S, t, ms, mon = build(a)
    mo = S.model(t, ms)
    z = mo.mean[None, :] + np.random.default_rng(1).standard_normal((a.lanes, mo.number)) / np.sqrt(mo.precision)[None, :]
    t0 = time.perf_counter()
    rb = S.Rebuilt(t, ms)
    setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    for s in range(a.lanes):
        th = rb.solve(z[s])
        rb.objective(z[s], th)
    batch = time.perf_counter() - t0
    k = min(a.lanes, 16)
    t0 = time.perf_counter()
    for s in range(k):
        S.Rebuilt(t, ms, [s]).solve(z[s])
    per_removal = (time.perf_counter() - t0) / k
    return dict(assemble_and_splu_ms=setup * 1e3, batch_ms=batch * 1e3, estimates_per_s=a.lanes / batch, rebuild_refactorise_solve_ms_per_removal=per_removal * 1e3,
                removal_round_ms_extrapolated=per_removal * a.lanes * 1e3, removals_timed=k, threads=1)


STEPS = {"dcse": (step_dcse, 600), "splu": (step_splu, 600)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcse_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DCSE_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("dcse", "splu"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "splu" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DCSE_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DCSE_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    dc = os.path.join(ROOT, "profiles", "dc_time.json")
    if os.path.exists(dc):
        with open(dc) as fh:
            ref = json.load(fh)["dc"]
        result["sweep_pair_over_dc_screen"] = result["dcse"]["sweep_pair_ms"]["median"] / ref["sweep_pair_ms"]["median"]
        result["sweep_terms_over_dc_screen"] = result["dcse"]["dims"]["sweepTerms"] / ref["dims"]["sweepTerms"]
        result["dc_screen"] = dict(sweep_pair_ms=ref["sweep_pair_ms"]["median"], sweepTerms=ref["dims"]["sweepTerms"], sweepLaunches=ref["dims"]["sweepLaunches"])
    result["speedup_over_splu_batch"] = result["splu"]["batch_ms"] / result["dcse"]["chain_ms"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
