#!/usr/bin/env python3
"""Times the DC probabilistic N-1 screen (dcChanceScreen) on the 10k-bus grid: every non-bridge branch a candidate, every in-service branch monitored and
rated, r = 8 and r = 32 seeded factors.  Next to it, in the same run, the two routes it replaces: dcSeriesScreen over 1 024 profiles sampled from the same
factors, and the numpy rebuild route on 16 candidates, extrapolated.  Kernel times through HIP events after a warm-up, medians of REPS runs.  No ratio is
required of these numbers; they are written down.

    python tools/dc_chance_time.py [--out profiles/dc_chance_time.json] [--reps 25] [--sample 16] [--profiles 1024] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  chance  per r: the build (Phi, then S: one sweep pair per factor), k_chance_screen and k_chance_base alone (jg_dc_chance_time_kernel), the FMA rate the
          screen kernel reaches (2 R FMAs per candidate and rated row, R the instance), a whole call; for r = 8 a sample against the rebuild route
  series  dcSeriesScreen over the sampled profiles: wall clock, build and kernel times
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


def stats(ms, reps):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)), reps=int(reps))


def setting(a):
    import juliagrid.jl_amd as jg
    import dc_chance_reference as Q
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = Q.rating_of(t)
    rating[rating == 0] = 1.0                                      # every in-service branch is rated: every row of the walk does the full work
    mon = (np.flatnonzero(np.asarray(t["br_status"]) == 1) + 1).astype(np.int64)
    return jg, Q, t, s, rating, mon, jg.pairCandidates(s), Q.factors(t, 32, Q.SEED)


def step_chance(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    jg, Q, t, s, rating, mon, cand, L32 = setting(a)
    an = jg.dcPowerFlow(s)
    jg.dcChanceScreen(an, L32[:8], candidates=cand[:64], monitored=mon, rating=rating)          # warm-up
    out = dict(candidates=int(cand.size), monitored=int(mon.size))
    lib = jg._lib.lib()
    for r in (8, 32):
        t0 = time.perf_counter()
        res = jg.dcChanceScreen(an, L32[:r], candidates=cand, monitored=mon, rating=rating, probability=Q.PROBABILITY)
        wall = time.perf_counter() - t0
        lds = (r + 7) // 8 * 8
        one = dict(factors=r, rows=int(res.info["rows"]), phi_bytes=res.info["phiBytes"], s_bytes=res.info["sBytes"], phi_build_ms=res.info["buildMs"],
                   s_build_ms=res.info["sBuildMs"], s_sweep_ms=res.info["sSweepMs"], s_kernel_ms=res.info["sKernelMs"], records=int(res.total),
                   bridges=int(res.bridges.size), call_wall_s=wall)
        # the kernels alone, on a state this step builds and screens itself (dcChanceScreen releases its own)
        info, t5 = np.zeros(12), np.zeros(5, dtype=np.int64)
        jg._lib.check(lib.jg_dc_chance_build(an._h, r, np.ascontiguousarray(L32[:r]).reshape(-1), cand.size, cand, mon.size, jg.dcpowerflow._ptr(mon), None, 0, info))
        jg._lib.check(lib.jg_dc_chance_screen(an._h, 0, cand.size, Q.PROBABILITY, 0, None, t5, None, None, None, None, None, None, None))
        for name, k in (("k_chance_screen", 0), ("k_chance_base", 1)):
            ms = np.zeros(a.reps)
            jg._lib.check(lib.jg_dc_chance_time_kernel(an._h, k, 0, cand.size, 5, ms))          # warm-up
            jg._lib.check(lib.jg_dc_chance_time_kernel(an._h, k, 0, cand.size, a.reps, ms))
            one[name + "_ms"] = stats(ms, a.reps)
        jg._lib.check(lib.jg_dc_chance_release(an._h))
        fma = 2.0 * lds * cand.size * mon.size                     # per candidate and rated row: R for the combined sensitivity, R for its square
        one.update(instance=lds, fma=fma, erfc=2.0 * cand.size * mon.size, fma_per_s=fma / (one["k_chance_screen_ms"]["median"] * 1e-3))
        out[f"r{r}"] = one
        if r == 8:                                                 # the numpy rebuild route on a sample: seconds per candidate, and the parity of the sample
            dense = jg.dcChanceScreen(an, L32[:r], candidates=cand, monitored=mon, rating=rating, rows=(0, 64), dense=True)
            pick = np.linspace(0, 63, a.sample).astype(int)
            sec, worst, p0 = [], 0.0, Q.own_injection(t)
            for i in pick:
                t0 = time.perf_counter()
                mu, S = Q.rebuild(t, int(cand[i]) - 1, p0, L32[:r])
                sec.append(time.perf_counter() - t0)
                sigma = np.sqrt((S ** 2).sum(axis=1))
                worst = max(worst, float(np.abs(dense.mean[i] - mu[mon - 1]).max()) / max(1.0, float(np.abs(mu).max())),
                            float(np.abs(dense.std[i] - sigma[mon - 1]).max()) / max(1.0, float(sigma.max())))
            assert worst <= 1e-9, worst
            out.update(rebuild_s_per_candidate=float(np.median(sec)), rebuild_s_all_candidates=float(np.median(sec)) * cand.size, sample=int(a.sample),
                       worst_mean_std_vs_rebuild=worst)
    an.close()
    return out


def step_series(a):
    import torch  # noqa: F401
    jg, Q, t, s, rating, mon, cand, L32 = setting(a)
    inj = Q.own_injection(t)[None, :] + np.random.default_rng(99).standard_normal((a.profiles, 8)) @ L32[:8]
    an = jg.dcPowerFlow(s)
    jg.dcSeriesScreen(an, inj[:64], candidates=cand[:64], monitored=mon, rating=rating)        # warm-up
    t0 = time.perf_counter()
    res = jg.dcSeriesScreen(an, inj, candidates=cand, monitored=mon, rating=rating)
    wall = time.perf_counter() - t0
    an.close()
    return dict(profiles=int(a.profiles), factors=8, call_wall_s=wall, phi_build_ms=res.info["buildMs"], f0_build_ms=res.info["f0BuildMs"],
                violating=int(res.totals["violating"]), smallest_frequency=1.0 / a.profiles)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_chance_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--sample", type=int, default=16)
    p.add_argument("--profiles", type=int, default=1024)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=("chance", "series"))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DC_CHANCE_TIME_JSON " + json.dumps((step_chance if a.step == "chance" else step_series)(a)))
        return
    result = dict(case=a.case, reps=a.reps)
    for name in ("chance", "series"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--sample", str(a.sample), "--profiles", str(a.profiles), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)        # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_CHANCE_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_CHANCE_TIME_JSON "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
