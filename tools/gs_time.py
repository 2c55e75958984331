#!/usr/bin/env python3
"""Times the Gauss-Seidel power flow: a fixed number of sweeps (tolerance 0, so no lane leaves early) of the base case in every lane, at 512 and 4 096
lanes, on case118 and case1354pegase, through jg_gs_time_kernel (HIP events around the ONE launch of powerFlow_), medians of REPS runs after a warm-up.

    python tools/gs_time.py [--out profiles/gs_time.json] [--reps 5]

The same run also times the numpy restatement (tests/gs_reference.py) on a sample of lanes and sweeps, one core, for the time per sweep and lane.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"case118": dict(sweeps=400, sample_lanes=64, sample_sweeps=20), "case1354pegase": dict(sweeps=40, sample_lanes=64, sample_sweeps=3)}
LANES = (512, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gs_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import gs_reference as R
    from conftest import load_case
    res = {"reps": a.reps, "cases": {}}
    for case, c in CASES.items():
        s = jg.powerSystem(load_case(case))
        jg.acModel_(s)
        g = R.problem(s)
        rec = {"buses": int(g.n), "stored_entries": int(g.rowval.size), "sweeps": c["sweeps"], "lanes": {}}
        for lanes in LANES:
            an = jg.gaussSeidel(s, batch=lanes)
            an.time_kernel(0, 2, 1)                                            # warm-up
            jg.setInitialPoint_(an)
            ms = an.time_kernel(0, c["sweeps"], a.reps)                        # sweeps x (mismatch + sweep) + the last mismatch, per launch
            jg.powerFlow_(an, iteration=0)
            med = float(np.median(ms))
            rec["lanes"][str(lanes)] = dict(ms=dict(median=med, min=float(ms.min()), max=float(ms.max())), us_per_sweep=med * 1e3 / c["sweeps"],
                                            ns_per_sweep_and_lane=med * 1e6 / c["sweeps"] / lanes, finite=bool(np.isfinite(np.asarray(an.method.voltage)).all()))
            print(case, lanes, rec["lanes"][str(lanes)], flush=True)
            an.close()
        yt, v, P, Q = R.lanes(g, c["sample_lanes"])
        t0 = time.perf_counter()
        R.run(g, yt, v, P, Q, c["sample_sweeps"], 0.0)
        dt = time.perf_counter() - t0
        rec["restatement"] = dict(lanes=c["sample_lanes"], sweeps=c["sample_sweeps"], seconds=dt, us_per_sweep_and_lane=dt * 1e6 / c["sample_sweeps"] / c["sample_lanes"])
        print(case, "restatement", rec["restatement"], flush=True)
        res["cases"][case] = rec
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
