#!/usr/bin/env python3
"""Times the DC generator-outage screen: the 10k-bus grid, all default generators x all default candidates, the default monitored list, HIP events, medians
of REPS runs after a warm-up.

    python tools/dc_generator_time.py [--out profiles/dc_generator_time.json] [--reps 5] [--case case_ACTIVSg10k]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  generator  per pickup ("slack", "participation"): the build split (Phi / the bus columns Psi: sweep pairs and flow kernel / k_gen_flows, HIP events inside
             jg_dc_generator_build, and the wall clock of the call), the screen over ALL candidates (k_series_screen on the generator screen's state and
             the summaries, jg_dc_generator_time_kernel summed over the row blocks; the wall clock of the whole screen, records included)
  series     the SAME cases handed to the series screen as hand-made injection rows, one per generator (what a user could do before): the build split
             (Phi / F0: one sweep pair per GENERATOR) and the same kernels through jg_dc_series_time_kernel
The comparison the run is for: the generator screen's build of its G-1 flows (distinct-bus sweeps + k_gen_flows) against the series route's (per-generator
sweeps) for the same cases.
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

BLOCK_BYTES = 256 << 20                                                 # SERIES_BLOCK_BYTES of dcpowerflow.py


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(ms.size))


def setup(a):
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
    return jg, _lib, L, s, an, cand, mon


def time_screen(_lib, L, an, which, nk, ld, cols, reps):
    """kernel times of the whole screen by jg_dc_<which>_time_kernel, summed over the row blocks, and the wall clock of the screen calls"""
    vp = lambda x: x.ctypes.data_as(_lib.VP)
    step = max(1, BLOCK_BYTES // (ld * 16))
    blocks = [(k0, min(k0 + step, nk)) for k0 in range(0, nk, step)]
    rec = np.zeros((1 << 16, 5))
    isl = np.zeros(step, dtype=np.int64)
    screen, timer = getattr(L, f"jg_dc_{which}_screen"), getattr(L, f"jg_dc_{which}_time_kernel")

    def screen_all():
        tot = np.zeros(3, dtype=np.int64)
        worst, wc, vc, base = np.zeros(nk), np.zeros(cols), np.zeros(cols, dtype=np.int64), np.zeros((cols, 3))
        t0 = time.perf_counter()
        for k0, k1 in blocks:
            t5 = np.zeros(5, dtype=np.int64)
            _lib.check(screen(an._h, k0, k1, 1.0, rec.shape[0], vp(rec), vp(isl), t5, vp(worst), vp(wc), vp(vc), vp(base) if k0 == 0 else None, None, None, None))
            tot += t5[:3]
        return time.perf_counter() - t0, tot
    screen_all()                                                        # warm-up
    walls = []
    for _ in range(reps):
        sec, tot = screen_all()
        walls.append(sec * 1e3)
    kernel = np.zeros(reps)
    summary = np.zeros(reps)
    for k0, k1 in blocks:
        _lib.check(screen(an._h, k0, k1, 1.0, 0, None, vp(isl), np.zeros(5, dtype=np.int64), None, None, None, None, None, None, None))      # the block's rows in place
        for kind, acc in ((0, kernel), (1, summary)):
            ms = np.zeros(reps)
            _lib.check(timer(an._h, kind, k0, k1, 1, np.zeros(1)))      # warm-up
            _lib.check(timer(an._h, kind, k0, k1, reps, ms))
            acc += ms
    return dict(row_blocks=len(blocks), block_rows=step, cases=int(tot[0]), violating=int(tot[1]), bridges=int(tot[2]), screen_wall_ms=stats(walls),
                screen_kernel_ms=stats(kernel), summary_kernels_ms=stats(summary))


def step_generator(a):
    jg, _lib, L, s, an, cand, mon = setup(a)
    from juliagrid.jl_amd.dcgenerator import GENERATOR_INFO, _build
    out = dict(candidates=int(cand.size), monitored=int(mon.size), runs={})
    for pickup in ("slack", "participation"):
        t0 = time.perf_counter()
        sh = jg.pickupShare(s, pickup=pickup)
        split_ms = (time.perf_counter() - t0) * 1e3
        G = int(sh.generators.size)
        builds = []
        for _ in range(a.reps + 1):                                     # the first is the warm-up
            t0 = time.perf_counter()
            info = _build(L, an, cand, mon, sh, 0, None)
            builds.append(np.r_[info, (time.perf_counter() - t0) * 1e3])
        b = np.array(builds[1:])
        col = {name: j for j, name in enumerate(GENERATOR_INFO)}
        flow = np.zeros(a.reps)
        _lib.check(L.jg_dc_generator_time_kernel(an._h, 2, 0, 0, 1, np.zeros(1)))
        _lib.check(L.jg_dc_generator_time_kernel(an._h, 2, 0, 0, a.reps, flow))
        run = dict(generators=G, ldg=(G + 63) // 64 * 64, generator_buses_swept=int(info[col["busesSwept"]]), entries_of_A=int(info[col["entries"]]),
                   rows=int(info[0]), phi_bytes=int(info[col["phiBytes"]]), psi_bytes=int(info[col["psiBytes"]]), f0_bytes=int(info[col["f0Bytes"]]),
                   host_split_ms=split_ms,
                   build_ms=dict(phi_total=stats(b[:, col["buildMs"]]), psi_sweep_pairs=stats(b[:, col["psiSweepMs"]]), psi_flow_kernel=stats(b[:, col["psiKernelMs"]]),
                                 k_gen_flows=stats(b[:, col["flowKernelMs"]]), k_gen_flows_alone=stats(flow),
                                 g1_flows_total=stats(b[:, col["psiBuildMs"]] + b[:, col["flowKernelMs"]]), call_wall=stats(b[:, -1])))
        run.update(time_screen(_lib, L, an, "generator", int(cand.size), run["ldg"], G, a.reps))
        out["runs"][pickup] = run
    _lib.check(L.jg_dc_generator_release(an._h))
    an.close()
    return out


def step_series(a):
    jg, _lib, L, s, an, cand, mon = setup(a)
    from juliagrid.jl_amd.dcpowerflow import _base_rhs
    sh = jg.pickupShare(s)                                              # slack pickup: one injection row per generator, by hand
    G = int(sh.generators.size)
    rhs = np.tile(_base_rhs(s), (G, 1))
    bus = s.generator.layout.bus[sh.generators - 1] - 1
    rhs[np.arange(G), bus] -= sh.lost
    builds = []
    for _ in range(a.reps + 1):
        info = np.zeros(12)
        t0 = time.perf_counter()
        _lib.check(L.jg_dc_series_build(an._h, int(cand.size), cand, int(mon.size), mon.ctypes.data_as(_lib.VP), G, rhs.reshape(-1), 0, info))
        builds.append(np.r_[info, (time.perf_counter() - t0) * 1e3])
    b = np.array(builds[1:])
    out = dict(profiles=G, ldt=(G + 63) // 64 * 64, rows=int(info[0]), f0_bytes=int(info[8]),
               build_ms=dict(phi_total=stats(b[:, 5]), f0_sweep_pairs=stats(b[:, 10]), f0_kernel=stats(b[:, 11]), g1_flows_total=stats(b[:, 9]), call_wall=stats(b[:, -1])))
    out.update(time_screen(_lib, L, an, "series", int(cand.size), out["ldt"], G, a.reps))
    _lib.check(L.jg_dc_series_release(an._h))
    an.close()
    return out


STEPS = {"generator": (step_generator, 600), "series": (step_series, 400)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_generator_time.json"))
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    if a.step:
        print("DC_GENERATOR_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, reps=a.reps)
    for name in ("generator", "series"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1])       # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_GENERATOR_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_GENERATOR_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    ser = result["series"]["build_ms"]["g1_flows_total"]["median"]
    for pickup, run in result["generator"]["runs"].items():
        run["series_route_g1_flows_ms"] = ser
        run["series_route_over_generator_screen_g1_flows"] = ser / run["build_ms"]["g1_flows_total"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
