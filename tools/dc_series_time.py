#!/usr/bin/env python3
"""Times the DC N-1 screen over a series of injection profiles: the 10k-bus grid, the default candidate and monitored lists, seeded profiles
(tests/dc_series_reference.py), HIP events after a warm-up, medians of REPS runs.

    python tools/dc_series_time.py [--out profiles/dc_series_time.json] [--reps 10] [--profiles 512 8760] [--case case_ACTIVSg10k] [--batches 6]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  series   per number of profiles T: the build split (Phi / F0 sweep pairs / F0 kernel, HIP events inside jg_dc_series_build, and the wall clock of the
           call with the host's transposes and uploads), the screen over ALL candidates (wall clock over the row blocks, records and summaries
           included), k_series_screen alone (jg_dc_series_time_kernel, summed over the blocks), the (case, row) steps per second, the counted f64
           operations (3 per step: one FMA, one multiply) and the F0 bytes the kernel design predicts
  lanes    the SAME cases by the route that exists without the screen: setInjection_ + setOutages_ + solve_ + screenSummary_, 512 cases per batch
           (one profile x 512 candidates); a sample of batches, wall clock of the whole route and HIP events of the device chain alone
           (jg_dc_time_kernel 0), both extrapolated to all cases per case
  restate  the same cases by the numpy restatement on one core (a sample of candidates x profiles, extrapolated; no GPU)
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

TILE, WAVES = 4, 4                                                      # DC_SERIES_TILE of csrc/jg_dc_series.hpp, DC_PAIR_WAVES of csrc/jg_dc_phi.hpp
BLOCK_BYTES = 256 << 20                                                 # SERIES_BLOCK_BYTES of dcpowerflow.py


def stats(ms):
    ms = np.asarray(ms)
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(ms.size))


def step_series(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    import dc_series_reference as S
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
    out = dict(candidates=nk, monitored=int(mon.size), runs={})
    for T in a.profiles:
        rhs = np.ascontiguousarray(S.profiles(t, T) - s.bus.shunt.conductance[None, :] - s.model.dc.shiftPower[None, :])
        builds = []
        for _ in range(3):                                              # the first is the warm-up
            info = np.zeros(12)
            t0 = time.perf_counter()
            _lib.check(L.jg_dc_series_build(an._h, nk, cand, int(mon.size), mon.ctypes.data_as(_lib.VP), T, rhs.reshape(-1), 0, info))
            builds.append((info[5], info[6], info[7], info[9], info[10], info[11], (time.perf_counter() - t0) * 1e3))
        del rhs
        b = np.median(np.array(builds[1:]), axis=0)
        rows, ldt = int(info[0]), (T + 63) // 64 * 64
        step = max(1, BLOCK_BYTES // (ldt * 16))
        blocks = [(k0, min(k0 + step, nk)) for k0 in range(0, nk, step)]
        rec = np.zeros((1 << 16, 5))
        isl = np.zeros(step, dtype=np.int64)
        vp = lambda x: x.ctypes.data_as(_lib.VP)

        def screen_all():
            tot = np.zeros(3, dtype=np.int64)
            worst, wp, vprof, base = np.zeros(nk), np.zeros(T), np.zeros(T, dtype=np.int64), np.zeros((T, 3))
            t0 = time.perf_counter()
            for k0, k1 in blocks:
                t5 = np.zeros(5, dtype=np.int64)
                _lib.check(L.jg_dc_series_screen(an._h, k0, k1, 1.0, rec.shape[0], vp(rec), vp(isl), t5, vp(worst), vp(wp), vp(vprof), vp(base) if k0 == 0 else None,
                                                 None, None, None))
                tot += t5[:3]
            return time.perf_counter() - t0, tot
        screen_all()                                                    # warm-up
        walls = []
        for _ in range(3):
            sec, tot = screen_all()
            walls.append(sec)
        kernel_ms = summary_ms = 0.0
        for k0, k1 in blocks:
            _lib.check(L.jg_dc_series_screen(an._h, k0, k1, 1.0, 0, None, vp(isl), np.zeros(5, dtype=np.int64), None, None, None, None, None, None, None))   # the block's rows in place
            ms = np.zeros(a.reps)
            _lib.check(L.jg_dc_series_time_kernel(an._h, 0, k0, k1, 2, ms[:2].copy()))
            _lib.check(L.jg_dc_series_time_kernel(an._h, 0, k0, k1, a.reps, ms))
            kernel_ms += float(np.median(ms))
            _lib.check(L.jg_dc_series_time_kernel(an._h, 1, k0, k1, a.reps, ms))
            summary_ms += float(np.median(ms))
        cases = int(tot[0])
        steps = float(cases) * rows
        # what the design predicts: per workgroup (WAVES x TILE candidates k, one chunk of 64 profiles) every row of F0 once, 512 bytes
        groups = sum(-(-(k1 - k0 // TILE * TILE) // (TILE * WAVES)) for k0, k1 in blocks) * (ldt // 64)
        wall = float(np.median(walls))
        out["runs"][str(T)] = dict(
            profiles=T, ldt=ldt, rows=rows, phi_bytes=int(info[2]), f0_bytes=int(info[8]), row_blocks=len(blocks), block_rows=step,
            build_ms=dict(phi_total=float(b[0]), phi_sweep_pairs=float(b[1]), phi_kernel=float(b[2]), f0_total=float(b[3]), f0_sweep_pairs=float(b[4]),
                          f0_kernel=float(b[5]), call_wall=float(b[6]), lane_batches=-(-ldt // 512)),
            cases=cases, violating=int(tot[1]), bridges=int(tot[2]), screen_wall_s=stats(walls), screen_kernel_s=kernel_ms * 1e-3, summary_kernels_s=summary_ms * 1e-3,
            cases_per_s_wall=cases / wall, ns_per_case_wall=wall / cases * 1e9, ns_per_case_wall_with_build=(wall + float(b[6]) * 1e-3) / cases * 1e9,
            case_row_steps=steps, steps_per_s_kernel=steps / (kernel_ms * 1e-3), f64_operations=3.0 * steps, f64_tflops_kernel=3.0 * steps / (kernel_ms * 1e-3) / 1e12,
            f0_bytes_predicted=float(groups) * rows * 512, f0_tbs_kernel=float(groups) * rows * 512 / (kernel_ms * 1e-3) / 1e12)
    an.close()
    return out


def step_lanes(a):
    import torch  # noqa: F401
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    import dc_series_reference as S
    from conftest import load_case
    D = jg.dcpowerflow
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = P.rating_of(t)
    cand = jg.pairCandidates(s)
    prof = S.profiles(t, a.batches)
    an = jg.dcPowerFlow(s, batch=a.lanes)
    rng = np.random.default_rng(3)
    walls, chains = [], []
    for b in range(a.batches + 1):                                      # the first is the warm-up; batch b: profile b x 512 seeded candidates
        labels = [int(x) for x in np.sort(rng.choice(cand, a.lanes, replace=False))]
        p = prof[b % a.batches]
        t0 = time.perf_counter()
        D.setInjection_(an, np.broadcast_to(p, (a.lanes, p.size)))
        D.setOutages_(an, labels)
        D.solve_(an)
        rec = D.screenSummary_(an, rating)
        walls.append(time.perf_counter() - t0)
        assert (rec[:, 4] == 0).all()
        chains.append(float(np.median(an.time_kernel(0, a.reps))))
    an.close()
    return dict(lanes=a.lanes, sampled_batches=a.batches, route_wall_ms_per_batch=stats(np.array(walls[1:]) * 1e3), device_chain_ms_per_batch=stats(chains[1:]),
                ns_per_case_wall=float(np.median(walls[1:])) / a.lanes * 1e9, ns_per_case_device_chain=float(np.median(chains[1:])) * 1e6 / a.lanes)


def step_restate(a):
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    import dc_series_reference as S
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    cand = jg.pairCandidates(s) - 1
    rating = P.rating_of(t)
    sample = np.sort(np.random.default_rng(1).choice(cand, a.sample, replace=False))
    prof = S.profiles(t, 4)
    t0 = time.perf_counter()
    Phi, _, _ = P.sensitivities(t, sample)
    F0 = S.base_flows(t, prof)
    build = time.perf_counter() - t0
    t0 = time.perf_counter()
    n = 0
    for i in range(sample.size):
        for tt in range(4):
            fr = S.series_flows(Phi, F0, sample, i, tt)
            if fr is not None:
                P.loading(fr, rating)
            n += 1
    sec = time.perf_counter() - t0
    return dict(sample_candidates=int(sample.size), sample_profiles=4, sample_cases=n, seconds_per_case=sec / n, build_seconds_of_the_sample=build, threads=1)


STEPS = {"series": (step_series, 900), "lanes": (step_lanes, 300), "restate": (step_restate, 600)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_series_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--batches", type=int, default=6)
    p.add_argument("--sample", type=int, default=64)
    p.add_argument("--profiles", type=int, nargs="+", default=[512, 8760])
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    if a.step:
        print("DC_SERIES_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("series", "lanes", "restate"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case,
               "--batches", str(a.batches), "--sample", str(a.sample), "--profiles"] + [str(x) for x in a.profiles]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "restate" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_SERIES_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_SERIES_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    lanes = result["lanes"]
    result["pair_screen_steps_per_s_design_3_9"] = 2.26e12
    for T, run in result["series"]["runs"].items():
        run["lane_route_ns_per_case"] = dict(wall=lanes["ns_per_case_wall"], device_chain=lanes["ns_per_case_device_chain"])
        run["lane_route_over_screen_per_case"] = dict(wall_over_wall=lanes["ns_per_case_wall"] / run["ns_per_case_wall"],
                                                      device_chain_over_wall_with_build=lanes["ns_per_case_device_chain"] / run["ns_per_case_wall_with_build"])
        run["lane_route_all_cases_s_extrapolated"] = dict(wall=lanes["ns_per_case_wall"] * run["cases"] * 1e-9, device_chain=lanes["ns_per_case_device_chain"] * run["cases"] * 1e-9)
        run["restatement_all_cases_s_extrapolated"] = result["restate"]["seconds_per_case"] * run["cases"]
        run["steps_per_s_over_pair_screen"] = run["steps_per_s_kernel"] / 2.26e12
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
