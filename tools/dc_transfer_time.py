#!/usr/bin/env python3
"""Times the DC transfer-capability screen: the 10k-bus grid, the default candidate and monitored lists, a seeded set of zone-to-zone directions, HIP
events after a warm-up, medians of REPS runs.

    python tools/dc_transfer_time.py [--out profiles/dc_transfer_time.json] [--reps 10] [--transfers 256] [--case case_ACTIVSg10k] [--batches 6]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  transfer per number of transfers T: the build split (Phi / G sweep pairs / G kernel, HIP events inside jg_dc_transfer_build, and the wall clock of the
           call with the host's transposes and uploads), the screen over ALL candidates (wall clock over the row blocks, summaries included),
           k_transfer_screen alone (jg_dc_transfer_time_kernel, summed over the blocks), the (case, row) steps per second and the counted f64 operations
           (per step and transfer: one FMA for g, a quarter of the FMA and multiply for the loading, |g| x rinv, two multiplies of the cross comparison)
  lanes    the SAME cases by the route that exists without the screen: TWO lanes per case (the injections P0 and P0 + d_t, the same outage) through
           setInjection_ + setOutages_ + solve_, 256 cases per batch; a sample of batches, wall clock of the route and HIP events of the device chain
           alone (jg_dc_time_kernel 0), both extrapolated to all cases per case.  The limits by the formula would still have to be taken on the host.
  restate  the same cases by the numpy restatement of tests/dc_transfer_reference.py on one core (a sample of candidates x 4 directions, extrapolated; no GPU)
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

TILE, WAVES = 4, 4                                                      # DC_TRANSFER_TILE of csrc/jg_dc_transfer.hpp, DC_PAIR_WAVES of csrc/jg_dc_phi.hpp
BLOCK_BYTES = 256 << 20                                                 # TRANSFER_BLOCK_BYTES of dcpowerflow.py
ZONES, ZONE_BUSES = 16, 8


def stats(ms):
    ms = np.asarray(ms)
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(ms.size))


def zone_directions(t, T, seed=9):
    """T seeded zone-to-zone directions: the buses in ZONES contiguous blocks of the bus order, +1 over ZONE_BUSES seeded buses of one zone, -1 over as
    many of another"""
    n = t["bus_type"].size
    rng = np.random.default_rng(seed)
    edges = np.linspace(0, n, ZONES + 1).astype(np.int64)
    D = np.zeros((T, n))
    for i in range(T):
        a, b = rng.choice(ZONES, 2, replace=False)
        for z, sign in ((a, 1.0), (b, -1.0)):
            D[i, rng.choice(np.arange(edges[z], edges[z + 1]), ZONE_BUSES, replace=False)] = sign / ZONE_BUSES
    return D


def step_transfer(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    from conftest import load_case
    from juliagrid.jl_amd import _lib
    from juliagrid.jl_amd.dcpowerflow import _base_rhs, _set_rating
    t = load_case(a.case)
    s = jg.powerSystem(t)
    rating = a.rating * P.rating_of(t)
    an = jg.dcPowerFlow(s)
    L = _lib.lib()
    an._rhs = np.ascontiguousarray(_base_rhs(s), dtype=np.float64)
    _lib.check(L.jg_dc_set_rhs(an._h, an._rhs))
    _set_rating(an, rating)
    cand = jg.pairCandidates(s)
    mon = (np.flatnonzero((s.branch.layout.status == 1) & (rating > 0)) + 1).astype(np.int64)
    nk = int(cand.size)
    out = dict(candidates=nk, monitored=int(mon.size), runs={})
    vp = lambda x: x.ctypes.data_as(_lib.VP)
    for T in a.transfers:
        D = np.ascontiguousarray(zone_directions(t, T))
        builds = []
        for _ in range(3):                                              # the first is the warm-up
            info = np.zeros(12)
            t0 = time.perf_counter()
            _lib.check(L.jg_dc_transfer_build(an._h, nk, cand, int(mon.size), vp(mon), T, D.reshape(-1), None, 0, info))
            builds.append((info[5], info[6], info[7], info[9], info[10], info[11], (time.perf_counter() - t0) * 1e3))
        b = np.median(np.array(builds[1:]), axis=0)
        rows, ldt = int(info[0]), (T + 63) // 64 * 64
        step = max(1, BLOCK_BYTES // (ldt * 12))
        blocks = [(k0, min(k0 + step, nk)) for k0 in range(0, nk, step)]
        isl = np.zeros(step, dtype=np.int64)

        def screen_all():
            tot = np.zeros(3, dtype=np.int64)
            worst, base = np.full(nk, np.inf), np.zeros((T, 3))
            cap, co, cb = np.full(T, np.inf), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
            t0 = time.perf_counter()
            for k0, k1 in blocks:
                t5 = np.zeros(5, dtype=np.int64)
                _lib.check(L.jg_dc_transfer_screen(an._h, k0, k1, a.cutoff, None, 0, None, vp(isl), t5, vp(worst), vp(cap), vp(co), vp(cb), vp(base) if k0 == 0 else None,
                                                   None, None))
                tot += t5[:3]
            return time.perf_counter() - t0, tot, cap, base
        screen_all()                                                    # warm-up
        walls = []
        for _ in range(3):
            sec, tot, cap, base = screen_all()
            walls.append(sec)
        kernel_ms = summary_ms = 0.0
        for k0, k1 in blocks:
            _lib.check(L.jg_dc_transfer_screen(an._h, k0, k1, a.cutoff, None, 0, None, vp(isl), np.zeros(5, dtype=np.int64), None, None, None, None, None, None, None))
            ms = np.zeros(a.reps)
            _lib.check(L.jg_dc_transfer_time_kernel(an._h, 0, k0, k1, 2, ms[:2].copy()))
            _lib.check(L.jg_dc_transfer_time_kernel(an._h, 0, k0, k1, a.reps, ms))
            kernel_ms += float(np.median(ms))
            _lib.check(L.jg_dc_transfer_time_kernel(an._h, 1, k0, k1, a.reps, ms))
            summary_ms += float(np.median(ms))
        cases = int(tot[0])
        steps = float(cases) * rows
        ops = 2.0 + 3.0 + 2.0 / TILE                                    # per (case, row): FMA g, |g| rinv, 2 cross multiplies; FMA + multiply of the loading per tile
        wall = float(np.median(walls))
        final = np.minimum(cap, base[:, 0])
        out["runs"][str(T)] = dict(
            transfers=T, ldt=ldt, rows=rows, phi_bytes=int(info[2]), g_bytes=int(info[8]), row_blocks=len(blocks), block_rows=step,
            build_ms=dict(phi_total=float(b[0]), phi_sweep_pairs=float(b[1]), phi_kernel=float(b[2]), g_total=float(b[3]), g_sweep_pairs=float(b[4]),
                          g_kernel=float(b[5]), call_wall=float(b[6]), lane_batches=-(-ldt // 512)),
            cases=cases, bridges=int(tot[2]), capability_finite=int(np.isfinite(final).sum()), capability_positive=int((final > 0).sum()),
            screen_wall_s=stats(walls), screen_kernel_s=kernel_ms * 1e-3, summary_kernels_s=summary_ms * 1e-3,
            cases_per_s_wall=cases / wall, ns_per_case_wall=wall / cases * 1e9, ns_per_case_kernel=kernel_ms * 1e6 / cases,
            ns_per_case_wall_with_build=(wall + float(b[6]) * 1e-3) / cases * 1e9,
            case_row_steps=steps, steps_per_s_kernel=steps / (kernel_ms * 1e-3), f64_operations=ops * steps, f64_tflops_kernel=ops * steps / (kernel_ms * 1e-3) / 1e12)
    an.close()
    return out


def step_lanes(a):
    import torch  # noqa: F401
    import juliagrid.jl_amd as jg
    import dc_transfer_reference as X
    from conftest import load_case
    D_ = jg.dcpowerflow
    t = load_case(a.case)
    s = jg.powerSystem(t)
    cand = jg.pairCandidates(s)
    P0, D = X.own_injection(t), zone_directions(t, a.batches)
    an = jg.dcPowerFlow(s, batch=a.lanes)
    rng = np.random.default_rng(3)
    half = a.lanes // 2
    walls, chains = [], []
    for b in range(a.batches + 1):                                      # the first is the warm-up; batch b: direction b x 256 seeded candidates, two lanes each
        labels = [int(x) for x in np.sort(rng.choice(cand, half, replace=False))]
        inj = np.concatenate([np.broadcast_to(P0, (half, P0.size)), np.broadcast_to(P0 + D[b % a.batches], (half, P0.size))])
        t0 = time.perf_counter()
        D_.setInjection_(an, inj)
        D_.setOutages_(an, labels + labels)
        D_.solve_(an)
        walls.append(time.perf_counter() - t0)
        assert (np.asarray(an.status) == 0).all()
        chains.append(float(np.median(an.time_kernel(0, a.reps))))
    an.close()
    return dict(lanes=a.lanes, cases_per_batch=half, sampled_batches=a.batches, route_wall_ms_per_batch=stats(np.array(walls[1:]) * 1e3),
                device_chain_ms_per_batch=stats(chains[1:]), ns_per_case_wall=float(np.median(walls[1:])) / half * 1e9,
                ns_per_case_device_chain=float(np.median(chains[1:])) * 1e6 / half)


def step_restate(a):
    import juliagrid.jl_amd as jg
    import dc_pair_reference as P
    import dc_transfer_reference as X
    from conftest import load_case
    t = load_case(a.case)
    s = jg.powerSystem(t)
    cand = jg.pairCandidates(s) - 1
    rating = a.rating * P.rating_of(t)
    sample = np.sort(np.random.default_rng(1).choice(cand, a.sample, replace=False))
    P0, D = X.own_injection(t), zone_directions(t, 4)
    t0 = time.perf_counter()
    n = 0
    for k in sample:
        f, g = X.flows_and_sensitivity(t, int(k), P0, D)
        for tt in range(4):
            X.limits(f, g[:, tt], rating, int(k), a.cutoff)
            n += 1
    sec = time.perf_counter() - t0
    return dict(sample_candidates=int(sample.size), sample_transfers=4, sample_cases=n, seconds_per_case=sec / n, threads=1)


STEPS = {"transfer": (step_transfer, 900), "lanes": (step_lanes, 300), "restate": (step_restate, 600)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_transfer_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--batches", type=int, default=6)
    p.add_argument("--sample", type=int, default=16)
    p.add_argument("--transfers", type=int, nargs="+", default=[256])
    p.add_argument("--rating", type=float, default=4.0, help="multiplier of the seeded ratings")
    p.add_argument("--cutoff", type=float, default=1e-6)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    if a.step:
        print("DC_TRANSFER_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps, cutoff=a.cutoff, rating_multiplier=a.rating)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("transfer", "lanes", "restate"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case, "--batches", str(a.batches),
               "--sample", str(a.sample), "--rating", str(a.rating), "--cutoff", str(a.cutoff), "--transfers"] + [str(x) for x in a.transfers]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "restate" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_TRANSFER_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_TRANSFER_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    lanes = result["lanes"]
    result["pair_screen_steps_per_s_design_3_9"] = 2.26e12
    result["series_screen_steps_per_s_design_3_11"] = 3.10e12
    for T, run in result["transfer"]["runs"].items():
        run["lane_route_ns_per_case"] = dict(wall=lanes["ns_per_case_wall"], device_chain=lanes["ns_per_case_device_chain"])
        run["lane_route_over_screen_per_case"] = dict(wall_over_wall=lanes["ns_per_case_wall"] / run["ns_per_case_wall"],
                                                      device_chain_over_wall_with_build=lanes["ns_per_case_device_chain"] / run["ns_per_case_wall_with_build"],
                                                      device_chain_over_kernel=lanes["ns_per_case_device_chain"] / run["ns_per_case_kernel"])
        run["a_case_costs_less_than_the_lane_route"] = bool(run["ns_per_case_wall_with_build"] < lanes["ns_per_case_device_chain"])
        run["lane_route_all_cases_s_extrapolated"] = dict(wall=lanes["ns_per_case_wall"] * run["cases"] * 1e-9, device_chain=lanes["ns_per_case_device_chain"] * run["cases"] * 1e-9)
        run["restatement_all_cases_s_extrapolated"] = result["restate"]["seconds_per_case"] * run["cases"]
        run["steps_per_s_over_pair_screen"] = run["steps_per_s_kernel"] / 2.26e12
        run["steps_per_s_over_series_screen"] = run["steps_per_s_kernel"] / 3.10e12
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
