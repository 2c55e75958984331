#!/usr/bin/env python3
"""Times the DC N-1 screen: the 10k-bus grid, 512 outages from outageList, kernel times through HIP events after a warm-up, medians of REPS runs.

    python tools/dc_time.py [--out profiles/dc_time.json] [--reps 25] [--lanes 512] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  dc     the DC screen batch (jg_dc_time_kernel: whole chain / sweep pair / combine / flows + summary), statuses and angles checked against the
         restatement on a handful of lanes
  block  the 2 x 2-block shared-factor step of the AC screen on the same grid and lanes (jg_nr_time_kernel 4: correction + CompBase::solve), timed
         through the existing public calls in the same run
  splu   the same batch by the restatement: rebuild + scipy splu per outage on one core (no GPU)
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


def step_dc(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import dc_reference as R
    s = jg.powerSystem(a.case)
    labels = jg.outageList(s, a.lanes)
    t0 = time.perf_counter()
    an = jg.dcPowerFlow(s, batch=a.lanes)
    create_ms = (time.perf_counter() - t0) * 1e3
    jg.setOutages_(an, labels)
    t0 = time.perf_counter()
    jg.solve_(an)
    first_ms = (time.perf_counter() - t0) * 1e3
    rec = jg.dcpowerflow.screenSummary_(an, np.ones(s.branch.number))
    assert np.all(np.asarray(an.status) == 0)
    from conftest import load_case
    t = load_case(a.case)
    worst = max(R.worst(an.voltage.angle[i], R.solve(t, out=int(labels[i]) - 1)[0]) for i in (0, 1, a.lanes // 2, a.lanes - 1))
    assert worst <= 1e-9, worst
    out = dict(dims=an.dims(), create_ms=create_ms, first_solve_ms=first_ms, worst_angle_vs_restatement=worst, worst_loading=float(rec[:, 0].max()))
    for name, k in (("chain", 0), ("sweep_pair", 1), ("combine", 2), ("flows_summary", 3)):
        an.time_kernel(k, 5)                                        # warm-up
        ms = an.time_kernel(k, a.reps)
        out[name + "_ms"] = dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(a.reps))
    d = out["dims"]
    ld = d["ld"]
    # algorithmic bytes of the sweep pair: each sweep reads and writes n x ld doubles (2 x n x ld x 8), plus the factor (values + columns) once per lane group
    factor = d["sweepTerms"] * 12 * (ld // 64)
    out["sweep_pair_bytes"] = int(2 * (2 * d["n"] * ld * 8) + factor)
    out["sweep_pair_fraction_of_8TBs"] = out["sweep_pair_bytes"] / (out["sweep_pair_ms"]["median"] * 1e-3) / 8e12
    out["outages_per_s"] = a.lanes / (out["chain_ms"]["median"] * 1e-3)
    an.close()
    return out


def step_block(a):
    import torch  # noqa: F401
    import juliagrid.jl_amd as jg
    s = jg.powerSystem(a.case)
    single = jg.newtonRaphson(s)
    jg.powerFlow_(single)
    an = jg.contingencyAnalysis(s, jg.outageList(s, a.lanes))
    base = jg.BaseCase(single)
    base.attach(an)
    jg.startFromBase_(an)
    jg.powerFlow_(an, fetch=False)
    an.time_kernel(4, 5)
    ms = np.array([an.time_kernel(4, 1) for _ in range(a.reps)])
    out = dict(shared_factor_step_ms=dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(a.reps)), base=base.info)
    base.close()
    an.close()
    single.close()
    return out


def step_splu(a):
    import juliagrid.jl_amd as jg
    import dc_reference as R
    from conftest import load_case
    t = load_case(a.case)
    labels = jg.outageList(jg.powerSystem(a.case), a.lanes)
    t0 = time.perf_counter()
    for lab in labels:
        R.solve(t, out=int(lab) - 1)
    sec = time.perf_counter() - t0
    return dict(batch_ms=sec * 1e3, outages_per_s=a.lanes / sec, threads=1)


STEPS = {"dc": (step_dc, 300), "block": (step_block, 300), "splu": (step_splu, 600)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DC_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("dc", "block", "splu"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "splu" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    result["dc_over_block"] = result["dc"]["sweep_pair_ms"]["median"] / result["block"]["shared_factor_step_ms"]["median"]
    result["speedup_over_splu"] = result["splu"]["batch_ms"] / result["dc"]["chain_ms"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
