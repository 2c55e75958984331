#!/usr/bin/env python3
"""Times the DC N-2 screen with the bridge pairs screened on the slack's island (islands="shed") beside the default screen, in ONE run: the 10k-bus grid,
HIP events after a warm-up, medians of REPS runs.

    python tools/dc_pair_shed_time.py [--out profiles/dc_pair_shed_time.json] [--reps 10] [--case case_ACTIVSg10k] [--block 1024]

The step that uses the GPU runs in a child process of its own under a time limit.  Per mode -- "skip": the default candidates (pairCandidates, no bridge),
k_pair_screen<false>; "shed": every in-service branch (shedCandidates), k_pair_screen<true> -- the build split, the screen over all pairs (wall clock over the
row blocks; the shed gather included in shed mode), k_pair_screen alone (jg_dc_pair_time_kernel 0, summed over the blocks per repetition) in pairs per
second with its spread, and the ratio of the two instances.
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


def stats(ms):
    ms = np.asarray(ms)
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(ms.size))


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
    mon = (np.flatnonzero((s.branch.layout.status == 1) & (rating > 0)) + 1).astype(np.int64)
    vp = lambda x: x.ctypes.data_as(_lib.VP)
    out = dict(monitored=int(mon.size))
    for mode, cand in (("skip", jg.pairCandidates(s)), ("shed", jg.shedCandidates(s))):
        nk = int(cand.size)
        builds = []
        for _ in range(3):                                              # the first is the warm-up
            info = np.zeros(8)
            t0 = time.perf_counter()
            _lib.check(L.jg_dc_pair_set_island_mode(an._h, 1 if mode == "shed" else 0))
            _lib.check(L.jg_dc_pair_build(an._h, nk, cand, int(mon.size), vp(mon), 0, info))
            builds.append((info[5], info[6], info[7], (time.perf_counter() - t0) * 1e3))
        b = np.median(np.array(builds[1:]), axis=0)
        rows, ld = int(info[0]), int(info[1])
        rec = np.zeros((1 << 16, 5))
        isl = np.zeros((1 << 16, 2), dtype=np.int64)
        blocks = [(k0, min(k0 + a.block, nk - 1)) for k0 in range(0, nk - 1, a.block)]

        def screen_all():
            tot = np.zeros(3, dtype=np.int64)
            worst = np.zeros(nk)
            shed = 0
            t0 = time.perf_counter()
            for k0, k1 in blocks:
                t6 = np.zeros(6, dtype=np.int64)
                _lib.check(L.jg_dc_pair_screen(an._h, k0, k1, 1.0, rec.shape[0], vp(rec), isl.shape[0], vp(isl), t6, vp(worst), None, None, None, None))
                tot += t6[:3]
            if mode == "shed":
                n = np.zeros(1, dtype=np.int64)
                q = [np.zeros(nk, dtype=np.int64) for _ in range(4)]
                _lib.check(L.jg_dc_pair_get_shed_table(an._h, 0, nk, n, *q))
                flow = np.zeros(int(n[0]))
                if n[0]:
                    _lib.check(L.jg_dc_pair_get_shed(an._h, 0, nk, flow))
                shed = int(n[0])
            return time.perf_counter() - t0, tot, shed
        screen_all()                                                    # warm-up
        walls = []
        for _ in range(3):
            sec, tot, shed = screen_all()
            walls.append(sec)
        kernel = []
        for k0, k1 in blocks:
            _lib.check(L.jg_dc_pair_screen(an._h, k0, k1, 1.0, 0, None, 0, None, np.zeros(6, dtype=np.int64), None, None, None, None, None))   # the block's rows in place
            ms = np.zeros(a.reps)
            _lib.check(L.jg_dc_pair_time_kernel(an._h, 0, k0, k1, 2, ms[:2].copy()))
            _lib.check(L.jg_dc_pair_time_kernel(an._h, 0, k0, k1, a.reps, ms))
            kernel.append(ms.copy())
        kernel = np.sum(np.array(kernel), axis=0)                       # per repetition, summed over the blocks
        pairs = int(tot[0])
        out[mode] = dict(candidates=nk, rows=rows, ld=ld, phi_bytes=int(info[2]), row_blocks=len(blocks), block_rows=a.block,
                         build_ms=dict(total=float(b[0]), sweep_pairs=float(b[1]), phi_kernel=float(b[2]), call_wall=float(b[3])),
                         pairs=pairs, violating=int(tot[1]), status3=int(tot[2]), shed=shed, screen_wall_s=stats(walls),
                         pairs_per_s_wall=pairs / float(np.median(walls)), screen_kernel_ms=stats(kernel),
                         pairs_per_s_kernel=pairs / (float(np.median(kernel)) * 1e-3),
                         pairs_per_s_kernel_spread=[pairs / (float(kernel.max()) * 1e-3), pairs / (float(kernel.min()) * 1e-3)],
                         pair_row_steps_per_s_kernel=float(pairs) * rows / (float(np.median(kernel)) * 1e-3))
    out["shed_over_skip_pairs_per_s"] = out["shed"]["pairs_per_s_kernel"] / out["skip"]["pairs_per_s_kernel"]
    out["shed_over_skip_pair_row_steps_per_s"] = out["shed"]["pair_row_steps_per_s_kernel"] / out["skip"]["pair_row_steps_per_s_kernel"]
    an.close()
    return out


STEPS = {"pair": (step_pair, 1100)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_pair_shed_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--block", type=int, default=1024)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    if a.step:
        print("DC_PAIR_SHED_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, reps=a.reps)
    for name in ("pair",):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--case", a.case, "--block", str(a.block)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1])       # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_PAIR_SHED_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_PAIR_SHED_TIME_JSON "):])
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
