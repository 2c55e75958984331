#!/usr/bin/env python3
"""Times the DC cascading-outage screen (dcCascadeScreen) on the 10k-bus grid: every non-bridge in-service branch is an initiating event, the ratings are
those of tests/dc_cascade_reference.py, trip = 1, most = 8, both rules.  Next to it, what a user can do without it: the host loop of dcGroupScreen calls,
one per stage, on the same events (wall clock), and the numpy rebuild route on a seeded sample of cascades (extrapolated to all events, and said to be).
Kernel times through HIP events after a warm-up, medians of REPS runs.

    python tools/dc_cascade_time.py [--out profiles/dc_cascade_time.json] [--reps 20] [--sample 6] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  cascade   per rule: build and screen of all events, k_cascade alone (jg_dc_cascade_time_kernel), the distribution of stages and statuses; the sample
            against the rebuild route
  loop      per rule: dcGroupScreen once per stage on the sets still running, the trips taken from its records on the host
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
RULES = ("all", "worst")


def stats(ms, reps):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)), reps=int(reps))


def setup(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import dc_cascade_reference as K
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = K.ratings(t)
    events = [(int(k),) for k in jg.pairCandidates(s)]
    return jg, K, t, s, rating, events


def step_cascade(a):
    jg, K, t, s, rating, events = setup(a)
    an = jg.dcPowerFlow(s)
    jg.dcCascadeScreen(an, events[:64], rating=rating)             # warm-up
    out = dict(events=len(events))
    L = jg._lib.lib()
    results = {}
    for rule in RULES:
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = jg.dcCascadeScreen(an, events, rating=rating, rule=rule)
            wall.append(time.perf_counter() - t0)
        results[rule] = res
        out[rule] = dict(candidates=int(res.candidates.size), rows=int(res.info["rows"]), phi_bytes=res.info["phiBytes"], build_ms=res.buildMs,
                         screen_ms=res.screenMs, wall_s=float(np.median(wall)), totals=res.totals,
                         stages={int(k): int(v) for k, v in zip(*np.unique(res.stages, return_counts=True))},
                         size={int(k): int(v) for k, v in zip(*np.unique(res.size, return_counts=True))})
    # the kernel alone, on a state this step builds and runs itself (dcCascadeScreen releases its own)
    off = np.arange(len(events) + 1, dtype=np.int64)
    mon = np.ascontiguousarray(results["all"].monitored)
    info = np.zeros(8)
    jg._lib.check(L.jg_dc_cascade_build(an._h, len(events), off, np.array([e[0] for e in events], dtype=np.int64), mon.size, mon.ctypes.data_as(jg._lib.VP), 0, info))
    jg._lib.check(L.jg_dc_cascade_run(an._h, 0, len(events), 1.0, 0, 8, *([None] * 11)))
    for k, rule in enumerate(RULES):
        ms = np.zeros(a.reps)
        jg._lib.check(L.jg_dc_cascade_time_kernel(an._h, k, 0, len(events), 3, ms))       # warm-up
        jg._lib.check(L.jg_dc_cascade_time_kernel(an._h, k, 0, len(events), a.reps, ms))
        out[rule]["k_cascade_ms"] = stats(ms, a.reps)
    jg._lib.check(L.jg_dc_cascade_release(an._h))
    an.close()
    # the numpy rebuild route on a seeded sample: seconds per cascade, and the parity of the sample
    import dc_group_reference as Q
    base = Q.base_components(t)
    mon0 = K.default_monitored(t, rating)
    pick = np.random.default_rng(19).choice(len(events), size=a.sample, replace=False)
    for rule in RULES:
        sec, stages, agree = [], [], 0
        for c in pick:
            t0 = time.perf_counter()
            ref = K.cascade_rebuild(t, (events[c][0] - 1,), rating, mon0, 1.0, rule, 8, base)
            sec.append(time.perf_counter() - t0)
            stages.append(ref.stages)
            res = results[rule]
            n = int(res.size[c])
            agree += (int(res.status[c]), [int(x) - 1 for x in res.tripped[c, :n]]) == (ref.status, ref.tripped) or ref.margin < K.AMBIGUOUS
        assert agree == len(pick), (rule, agree)
        out[rule].update(rebuild_sample=int(a.sample), rebuild_s_per_cascade=float(np.mean(sec)), rebuild_sample_stages=[int(x) for x in stages],
                         rebuild_s_all_events_extrapolated=float(np.mean(sec)) * len(events))
    return out


def host_loop(jg, an, events, rating, monitored, rule, trip=1.0, most=8):
    """the cascade by dcGroupScreen calls, one per stage: (status [C], size [C], stages run)"""
    sets = [list(e) for e in events]
    status = np.zeros(len(sets), dtype=np.int64)
    run = list(range(len(sets)))
    stage = 0
    while run:
        res = jg.dcGroupScreen(an, [tuple(sets[c]) for c in run], monitored=monitored, rating=rating, threshold=trip, capacity=1 << 22)
        assert not res.overflow
        rec = res.violating
        first = np.searchsorted(rec[:, 0], np.arange(len(run) + 1))
        nxt = []
        for g, c in enumerate(run):
            if res.status[g] == 3:
                status[c] = 3
                continue
            mine = rec[first[g]:first[g + 1]]
            if mine.shape[0] == 0:
                continue
            now = [int(x) for x in mine[:, 1]] if rule == "all" else [int(mine[np.argmax(mine[:, 3]), 1])]
            if len(sets[c]) + len(now) > most:
                status[c] = 5
                continue
            sets[c] += now
            nxt.append(c)
        run = nxt
        stage += 1
    return status, np.array([len(x) for x in sets]), stage


def step_loop(a):
    jg, K, t, s, rating, events = setup(a)
    an = jg.dcPowerFlow(s)
    jg.dcGroupScreen(an, events[:64], rating=rating)               # warm-up
    out = {}
    for rule in RULES:
        ref = jg.dcCascadeScreen(an, events, rating=rating, rule=rule)
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            status, size, calls = host_loop(jg, an, events, rating, ref.monitored, rule)
            wall.append(time.perf_counter() - t0)
        out[rule] = dict(group_screen_calls=int(calls), wall_s=float(np.median(wall)), same_status=int((status == ref.status).sum()),
                         same_size=int((size == ref.size).sum()), events=len(events))
    an.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_cascade_time.json"))
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--sample", type=int, default=6)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=("cascade", "loop"))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DC_CASCADE_TIME_JSON " + json.dumps((step_cascade if a.step == "cascade" else step_loop)(a)))
        return
    result = dict(case=a.case, reps=a.reps, trip=1.0, most=8)
    for name in ("cascade", "loop"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--sample", str(a.sample), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)        # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_CASCADE_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_CASCADE_TIME_JSON "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
