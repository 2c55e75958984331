#!/usr/bin/env python3
"""Times a 512-lane batch of BRIDGE outages solved on the slack's island (islands="shed") next to a 512-lane batch of outageList outages (the batch
tools/dc_time.py times): the 10k-bus grid, kernel times through HIP events after a warm-up, medians of REPS runs, ROUNDS alternations of the two.

    python tools/dc_island_time.py [--out profiles/dc_island_time.json] [--reps 25] [--rounds 3] [--lanes 512] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  plain  outageList outages, no keyword: the parent's path (the kernels without the island flag)
  shed   bridges drawn by a seeded shuffle, islands="shed": every lane an island lane; a few lanes checked against the restatement
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = (("chain", 0), ("sweep_pair", 1), ("combine", 2), ("flows_summary", 3))


def step(a, shed):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    s = jg.powerSystem(a.case)
    if shed:
        tb = jg.islandTable(s)
        labels = np.flatnonzero(tb.side != 0) + 1
        np.random.default_rng(512).shuffle(labels)
        labels = np.resize(labels, a.lanes)
    else:
        labels = jg.outageList(s, a.lanes)
    an = jg.dcPowerFlow(s, batch=a.lanes)
    jg.setOutages_(an, labels, islands="shed" if shed else "skip")
    jg.solve_(an)
    jg.dcpowerflow.screenSummary_(an, np.ones(s.branch.number))
    assert np.all(np.asarray(an.status) == (4 if shed else 0))
    out = dict(lanes=int(a.lanes))
    if shed:
        import dc_island_reference as I
        from conftest import load_case
        t = load_case(a.case)
        worst = 0.0
        for i in (0, 1, a.lanes // 2, a.lanes - 1):
            rth, _, keep = I.solve(t, out=int(labels[i]) - 1)
            assert np.array_equal(np.isnan(an.voltage.angle[i]), ~keep)
            worst = max(worst, I.worst(an.voltage.angle[i], rth, keep))
        assert worst <= 1e-9, worst
        out.update(worst_angle_vs_restatement=worst, buses_shed=dict(min=int(an.island.buses.min()), median=float(np.median(an.island.buses)), max=int(an.island.buses.max())))
    for name, k in KERNELS:
        an.time_kernel(k, 5)                                        # warm-up
        ms = an.time_kernel(k, a.reps)
        out[name + "_ms"] = dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(a.reps))
    an.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_island_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=("plain", "shed"))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DC_ISLAND_TIME_JSON " + json.dumps(step(a, a.step == "shed")))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps, rounds=[])
    for _ in range(a.rounds):
        this = {}
        for name in ("plain", "shed"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)     # a time limit of its own
            line = [l for l in r.stdout.splitlines() if l.startswith("DC_ISLAND_TIME_JSON ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
            this[name] = json.loads(line[0][len("DC_ISLAND_TIME_JSON "):])
        result["rounds"].append(this)
    for name in ("plain", "shed"):
        for k, _ in KERNELS:
            v = [r[name][k + "_ms"]["median"] for r in result["rounds"]]
            result[f"{name}_{k}_ms"] = dict(median=float(np.median(v)), min=min(v), max=max(v))
    result["shed_over_plain_chain"] = result["shed_chain_ms"]["median"] / result["plain_chain_ms"]["median"]
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
