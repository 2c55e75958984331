#!/usr/bin/env python3
"""Times the DC common-mode screen (dcGroupScreen) on the 10k-bus grid: parallelGroups(system) plus seeded groups of 3 to 8 members, next to the same
number of cases as 512-lane two-outage batches (the detail path: one sweep pair per outage and lane) and to the numpy rebuild route on a sample.  Kernel
times through HIP events after a warm-up, medians of REPS runs.

    python tools/dc_group_time.py [--out profiles/dc_group_time.json] [--reps 25] [--seeded 2048] [--sample 8] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  group   build and screen of all groups; k_group_screen and k_group_solve alone (jg_dc_group_time_kernel); a sample against the rebuild route
  lanes   512 two-outage lanes (pairs of the same candidates): setOutages_, solve_, screenSummary_, wall clock and kernels
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


def groups_of(jg, s, seeded):
    par, rest = jg.parallelGroups(s)
    cand = jg.pairCandidates(s)
    rng = np.random.default_rng(8)
    more = [tuple(sorted(int(x) for x in rng.choice(cand, size=int(k), replace=False))) for k in rng.integers(3, 9, size=seeded)]
    return par, rest, par + more


def stats(ms, reps):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)), reps=int(reps))


def step_group(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import dc_group_reference as Q
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = Q.rating_of(t)
    par, rest, groups = groups_of(jg, s, a.seeded)
    an = jg.dcPowerFlow(s)
    jg.dcGroupScreen(an, groups[:64], rating=rating)               # warm-up
    t0 = time.perf_counter()
    res = jg.dcGroupScreen(an, groups, rating=rating)
    wall = time.perf_counter() - t0
    out = dict(groups=len(groups), parallel=len(par), parallel_cut=len(rest), seeded=int(a.seeded), candidates=int(res.candidates.size),
               rows=int(res.info["rows"]), phi_bytes=res.info["phiBytes"], islanding=int(res.totals["islanding"]), violating=int(res.totals["violating"]),
               build_ms=res.buildMs, screen_ms=res.screenMs, wall_s=wall)
    # the kernels alone, on a state this step builds and screens itself (dcGroupScreen releases its own)
    L = jg._lib.lib()
    off = np.zeros(len(groups) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(g) for g in groups])
    info = np.zeros(8)
    jg._lib.check(L.jg_dc_group_build(an._h, len(groups), off, np.array([x for g in groups for x in g], dtype=np.int64), 0, None, 0, info))
    t6 = np.zeros(6, dtype=np.int64)
    jg._lib.check(L.jg_dc_group_screen(an._h, 0, len(groups), 1.0, 0, None, 0, None, t6, None, None, None, None, None, None))
    for name, k in (("k_group_screen", 0), ("k_group_solve", 1)):
        ms = np.zeros(a.reps)
        jg._lib.check(L.jg_dc_group_time_kernel(an._h, k, 0, len(groups), 5, ms))       # warm-up
        jg._lib.check(L.jg_dc_group_time_kernel(an._h, k, 0, len(groups), a.reps, ms))
        out[name + "_ms"] = stats(ms, a.reps)
    jg._lib.check(L.jg_dc_group_release(an._h))
    an.close()
    # the numpy rebuild route on a sample: seconds per group, and the parity of the sample
    base = Q.base_components(t)
    pick = np.linspace(0, len(groups) - 1, a.sample).astype(int)
    sec, worst = [], 0.0
    for g in pick:
        S = tuple(x - 1 for x in groups[g])
        t0 = time.perf_counter()
        ref = Q.group_solve(t, S, base)
        sec.append(time.perf_counter() - t0)
        if ref is None:
            assert res.status[g] == 3, (g, S)
        else:
            w = Q.loading(ref, rating, res.monitored - 1)[0]
            worst = max(worst, abs(res.worst[g] - w) / max(1.0, w))
    assert worst <= 1e-9, worst
    out.update(rebuild_s_per_group=float(np.median(sec)), sample=int(a.sample), worst_loading_vs_rebuild=worst)
    return out


def step_lanes(a):
    import torch  # noqa: F401
    import juliagrid.jl_amd as jg
    import dc_group_reference as Q
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = Q.rating_of(t)
    cand = jg.pairCandidates(s)
    rng = np.random.default_rng(8)
    pairs = [tuple(sorted(int(x) for x in rng.choice(cand, size=2, replace=False))) for _ in range(512)]
    an = jg.dcPowerFlow(s, batch=512)
    wall = []
    for _ in range(3 + a.reps):
        t0 = time.perf_counter()
        jg.dcpowerflow.setOutages_(an, pairs)
        jg.dcpowerflow.solve_(an)
        jg.dcpowerflow.screenSummary_(an, rating)
        wall.append(time.perf_counter() - t0)
    out = dict(lanes=512, batch_wall_ms=stats(np.array(wall[3:]) * 1e3, a.reps))
    for name, k in (("chain", 0), ("sweep_pair", 1), ("combine", 2), ("flows_summary", 3)):
        an.time_kernel(k, 5)
        out[name + "_ms"] = stats(an.time_kernel(k, a.reps), a.reps)
    an.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_group_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--seeded", type=int, default=2048)
    p.add_argument("--sample", type=int, default=8)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=("group", "lanes"))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DC_GROUP_TIME_JSON " + json.dumps((step_group if a.step == "group" else step_lanes)(a)))
        return
    result = dict(case=a.case, reps=a.reps)
    for name in ("group", "lanes"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--seeded", str(a.seeded), "--sample", str(a.sample), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)        # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_GROUP_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_GROUP_TIME_JSON "):])
    g, l = result["group"], result["lanes"]
    result["group_ms_per_case"] = g["screen_ms"] / g["groups"]
    result["two_outage_lane_ms_per_case"] = l["batch_wall_ms"]["median"] / l["lanes"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
