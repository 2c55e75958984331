#!/usr/bin/env python3
"""Times the DC N-2 screen: the 10k-bus grid, ALL pairs of the default candidate list, HIP events after a warm-up, medians of REPS runs.

    python tools/dc_pair_time.py [--out profiles/dc_pair_time.json] [--reps 20] [--lanes 512] [--case case_ACTIVSg10k] [--block 1024]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  pair     build of the sensitivities (total / sweep pairs / Phi kernel, HIP events inside jg_dc_pair_build), the screen over all pairs (wall clock of
           the calls and the sum of the screen kernel's event times per row block), achieved f64 rate and the Phi bytes the kernel design predicts
  lanes    a 512-lane batch of two-outage lanes against the same batch of single outages (jg_dc_time_kernel 0), same run
  restate  the same pairs by the numpy restatement on one core, extrapolated from all pairs of a sample of candidates (no GPU)
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

TILE, WAVES = 4, 4                                                      # DC_PAIR_TILE of csrc/jg_dc_pair.hpp, DC_PAIR_WAVES of csrc/jg_dc_phi.hpp


def stats(ms, reps):
    ms = np.asarray(ms)
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(reps))


def step_pair(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    from conftest import load_case
    from juliagrid.jl_amd import _lib
    from juliagrid.jl_amd.dcpowerflow import _base_rhs, _set_rating
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    an = jg.dcPowerFlow(s)
    L = _lib.lib()
    an._rhs = np.ascontiguousarray(_base_rhs(s), dtype=np.float64)
    _lib.check(L.jg_dc_set_rhs(an._h, an._rhs))
    _set_rating(an, rating)
    cand = jg.pairCandidates(s)
    mon = (np.flatnonzero((s.branch.layout.status == 1) & (rating > 0)) + 1).astype(np.int64)
    nk = int(cand.size)
    builds = []
    for _ in range(4):                                                  # the first is the warm-up
        info = np.zeros(8)
        t0 = time.perf_counter()
        _lib.check(L.jg_dc_pair_build(an._h, nk, cand, int(mon.size), mon.ctypes.data_as(_lib.VP), 0, info))
        builds.append((info[5], info[6], info[7], (time.perf_counter() - t0) * 1e3))
    b = np.median(np.array(builds[1:]), axis=0)
    rows, ld = int(info[0]), int(info[1])
    out = dict(candidates=nk, monitored=int(mon.size), rows=rows, ld=ld, phi_bytes=int(info[2]), free_bytes=int(info[3]),
               build_ms=dict(total=float(b[0]), sweep_pairs=float(b[1]), phi_kernel=float(b[2]), call_wall=float(b[3]), lane_batches=-(-ld // 512)))
    rec = np.zeros((1 << 16, 5))
    isl = np.zeros((1 << 16, 2), dtype=np.int64)
    blocks = [(k0, min(k0 + a.block, nk - 1)) for k0 in range(0, nk - 1, a.block)]

    def screen_all():
        tot = np.zeros(3, dtype=np.int64)
        worst = np.zeros(nk)
        t0 = time.perf_counter()
        for k0, k1 in blocks:
            t6 = np.zeros(6, dtype=np.int64)
            _lib.check(L.jg_dc_pair_screen(an._h, k0, k1, 1.0, rec.shape[0], rec.ctypes.data_as(_lib.VP), isl.shape[0], isl.ctypes.data_as(_lib.VP), t6,
                                           worst.ctypes.data_as(_lib.VP), None, None, None, None))
            tot += t6[:3]
        return time.perf_counter() - t0, tot
    screen_all()                                                        # warm-up
    walls = []
    for _ in range(3):
        sec, tot = screen_all()
        walls.append(sec)
    kernel_ms = summary_ms = 0.0
    for k0, k1 in blocks:
        L.jg_dc_pair_screen(an._h, k0, k1, 1.0, 0, None, 0, None, np.zeros(6, dtype=np.int64), None, None, None, None, None)   # the block's rows in place
        ms = np.zeros(a.reps)
        _lib.check(L.jg_dc_pair_time_kernel(an._h, 0, k0, k1, 2, ms[:2].copy()))
        _lib.check(L.jg_dc_pair_time_kernel(an._h, 0, k0, k1, a.reps, ms))
        kernel_ms += float(np.median(ms))
        _lib.check(L.jg_dc_pair_time_kernel(an._h, 1, k0, k1, a.reps, ms))
        summary_ms += float(np.median(ms))
    pairs = int(tot[0])
    # what the design predicts: per live workgroup (WAVES x TILE candidates k, one chunk of 64 l) every row of Phi once, 512 bytes; 5 f64 operations per pair and row
    live = sum(1 for kt in range(0, nk - 1, TILE * WAVES) for c in range(ld // 64) if c * 64 + 63 > kt)
    out.update(pairs=pairs, violating=int(tot[1]), islanding=int(tot[2]), row_blocks=len(blocks), block_rows=a.block,
               screen_wall_s=stats(walls, 3), screen_kernel_s=kernel_ms * 1e-3, summary_kernels_s=summary_ms * 1e-3,
               pairs_per_s_wall=pairs / float(np.median(walls)), pairs_per_s_kernel=pairs / (kernel_ms * 1e-3),
               f64_operations=5.0 * pairs * rows, f64_tflops_kernel=5.0 * pairs * rows / (kernel_ms * 1e-3) / 1e12,
               phi_bytes_predicted=float(live) * rows * 512, phi_tbs_kernel=float(live) * rows * 512 / (kernel_ms * 1e-3) / 1e12)
    an.close()
    return out


def step_lanes(a):
    import torch  # noqa: F401
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    singles = [int(x) for x in jg.outageList(s, a.lanes)]
    second = [int(x) for x in jg.outageList(s, a.lanes, seed=77)]
    pairs = [(k, l) if k != l else (k, 0) for k, l in zip(singles, second)]
    out = {}
    for name, labels in (("single", singles), ("pair", pairs)):
        an = jg.dcPowerFlow(s, batch=a.lanes)
        jg.setOutages_(an, labels)
        jg.solve_(an)
        jg.dcpowerflow.screenSummary_(an, np.ones(s.branch.number))
        an.time_kernel(0, 5)
        out[name + "_chain_ms"] = stats(an.time_kernel(0, a.reps), a.reps)
        if name == "pair":
            i = next(i for i, st in enumerate(an.status) if st == 0)
            out["islanding_lanes"] = int((np.asarray(an.status) == 3).sum())
            out["worst_angle_vs_rebuild"] = float(max(abs(an.voltage.angle[i] - P.pair_solve(t, pairs[i][0] - 1, pairs[i][1] - 1)[0])))
        an.close()
    out["pair_over_single"] = out["pair_chain_ms"]["median"] / out["single_chain_ms"]["median"]
    out["us_per_pair_lane"] = out["pair_chain_ms"]["median"] * 1e3 / a.lanes
    return out


def step_restate(a):
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    cand = jg.pairCandidates(s) - 1
    rating = P.rating_of(t)
    sample = np.sort(np.random.default_rng(1).choice(cand, a.sample, replace=False))
    t0 = time.perf_counter()
    Phi, f0, _ = P.sensitivities(t, sample)
    build = time.perf_counter() - t0
    t0 = time.perf_counter()
    n = 0
    for i in range(sample.size):
        for j in range(i + 1, sample.size):
            fr, _ = P.pair_flows(Phi, f0, sample, i, j)
            if fr is not None:
                P.loading(fr, rating)
            n += 1
    sec = time.perf_counter() - t0
    total = cand.size * (cand.size - 1) // 2
    return dict(sample_candidates=int(sample.size), sample_pairs=n, seconds_per_pair=sec / n, all_pairs=int(total), all_pairs_seconds_extrapolated=sec / n * total,
                sensitivities_seconds_per_candidate=build / sample.size, threads=1)


STEPS = {"pair": (step_pair, 600), "lanes": (step_lanes, 300), "restate": (step_restate, 600)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_pair_time.json"))
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--block", type=int, default=1024)
    p.add_argument("--sample", type=int, default=64)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    if a.step:
        print("DC_PAIR_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("pair", "lanes", "restate"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case,
               "--block", str(a.block), "--sample", str(a.sample)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "restate" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_PAIR_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_PAIR_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    result["screen_us_per_pair"] = 1e6 / result["pair"]["pairs_per_s_wall"]
    result["detail_over_screen_per_pair"] = result["lanes"]["us_per_pair_lane"] / result["screen_us_per_pair"]
    result["speedup_over_restatement"] = result["restate"]["all_pairs_seconds_extrapolated"] / result["pair"]["screen_wall_s"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
