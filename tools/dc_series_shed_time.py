#!/usr/bin/env python3
"""Times the DC series screen with the bridge candidates screened on the slack's island (islands="shed") beside the default screen, in ONE run: the 10k-bus
grid, seeded profiles (tests/dc_series_reference.py), HIP events after a warm-up, medians of REPS runs.

    python tools/dc_series_shed_time.py [--out profiles/dc_series_shed_time.json] [--reps 10] [--profiles 512 8760] [--case case_ACTIVSg10k] [--batches 6]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  series   per number of profiles T and per mode -- "skip": the default candidates (pairCandidates, no bridge), today's kernel instance; "shed": every
           in-service branch (shedCandidates), the shed instance -- the build split, the screen over all candidates (wall clock over the row blocks, the
           shed gather included in shed mode), k_series_screen alone (jg_dc_series_time_kernel, summed over the blocks) in (case, row) steps per second,
           and the ratio of the two instances
  lanes    the bridge cases by the route that exists without the screen: setInjection_ + setOutages_(..., islands="shed") + solve_ + screenSummary_, 512
           bridges per batch; a sample of batches, HIP events of the device chain alone (jg_dc_time_kernel 0), per case
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
    mon = (np.flatnonzero((s.branch.layout.status == 1) & (rating > 0)) + 1).astype(np.int64)
    vp = lambda x: x.ctypes.data_as(_lib.VP)
    out = dict(monitored=int(mon.size), runs={})
    for T in a.profiles:
        rhs = np.ascontiguousarray(S.profiles(t, T) - s.bus.shunt.conductance[None, :] - s.model.dc.shiftPower[None, :])
        run = {}
        for mode, cand in (("skip", jg.pairCandidates(s)), ("shed", jg.shedCandidates(s))):
            nk = int(cand.size)
            builds = []
            for _ in range(3):                                          # the first is the warm-up
                info = np.zeros(12)
                t0 = time.perf_counter()
                _lib.check(L.jg_dc_series_set_island_mode(an._h, 1 if mode == "shed" else 0))
                _lib.check(L.jg_dc_series_build(an._h, nk, cand, int(mon.size), vp(mon), T, rhs.reshape(-1), 0, info))
                builds.append((info[5], info[6], info[7], info[9], info[10], info[11], (time.perf_counter() - t0) * 1e3))
            b = np.median(np.array(builds[1:]), axis=0)
            rows, ldt = int(info[0]), (T + 63) // 64 * 64
            step = max(1, BLOCK_BYTES // (ldt * 16))
            blocks = [(k0, min(k0 + step, nk)) for k0 in range(0, nk, step)]
            rec = np.zeros((1 << 16, 5))
            isl = np.zeros(step, dtype=np.int64)

            def screen_all():
                tot = np.zeros(3, dtype=np.int64)
                worst, wp, vprof, base = np.zeros(nk), np.zeros(T), np.zeros(T, dtype=np.int64), np.zeros((T, 3))
                shed = 0
                t0 = time.perf_counter()
                for k0, k1 in blocks:
                    t5 = np.zeros(5, dtype=np.int64)
                    _lib.check(L.jg_dc_series_screen(an._h, k0, k1, 1.0, rec.shape[0], vp(rec), vp(isl), t5, vp(worst), vp(wp), vp(vprof), vp(base) if k0 == 0 else None,
                                                     None, None, None))
                    tot += t5[:3]
                    if mode == "shed":
                        n = np.zeros(1, dtype=np.int64)
                        q = [np.zeros(k1 - k0, dtype=np.int64) for _ in range(4)]
                        _lib.check(L.jg_dc_series_get_shed_table(an._h, k0, k1, n, *q))
                        flow = np.zeros((int(n[0]), T))
                        if n[0]:
                            _lib.check(L.jg_dc_series_get_shed(an._h, k0, k1, flow.reshape(-1)))
                        shed += int(n[0])
                return time.perf_counter() - t0, tot, shed
            screen_all()                                                # warm-up
            walls = []
            for _ in range(3):
                sec, tot, shed = screen_all()
                walls.append(sec)
            kernel = []
            for k0, k1 in blocks:
                _lib.check(L.jg_dc_series_screen(an._h, k0, k1, 1.0, 0, None, vp(isl), np.zeros(5, dtype=np.int64), None, None, None, None, None, None, None))   # the block's rows in place
                ms = np.zeros(a.reps)
                _lib.check(L.jg_dc_series_time_kernel(an._h, 0, k0, k1, 2, ms[:2].copy()))
                _lib.check(L.jg_dc_series_time_kernel(an._h, 0, k0, k1, a.reps, ms))
                kernel.append(ms.copy())
            kernel = np.sum(np.array(kernel), axis=0)                   # per repetition, summed over the blocks
            cases = int(tot[0])
            steps = float(cases) * rows
            wall = float(np.median(walls))
            run[mode] = dict(candidates=nk, rows=rows, ldt=ldt, phi_bytes=int(info[2]), f0_bytes=int(info[8]), row_blocks=len(blocks),
                             build_ms=dict(phi_total=float(b[0]), phi_sweep_pairs=float(b[1]), phi_kernel=float(b[2]), f0_total=float(b[3]), f0_sweep_pairs=float(b[4]),
                                           f0_kernel=float(b[5]), call_wall=float(b[6])),
                             cases=cases, violating=int(tot[1]), status3=int(tot[2]), shed=shed, screen_wall_s=stats(walls), ns_per_case_wall=wall / cases * 1e9,
                             screen_kernel_ms=stats(kernel), case_row_steps=steps, steps_per_s_kernel=steps / (float(np.median(kernel)) * 1e-3),
                             steps_per_s_kernel_spread=[steps / (float(kernel.max()) * 1e-3), steps / (float(kernel.min()) * 1e-3)])
        run["shed_over_skip_steps_per_s"] = run["shed"]["steps_per_s_kernel"] / run["skip"]["steps_per_s_kernel"]
        out["runs"][str(T)] = run
        del rhs
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
    bridges = np.setdiff1d(jg.shedCandidates(s), jg.pairCandidates(s))
    prof = S.profiles(t, a.batches)
    an = jg.dcPowerFlow(s, batch=a.lanes)
    rng = np.random.default_rng(3)
    chains = []
    for b in range(a.batches + 1):                                      # the first is the warm-up; batch b: profile b x 512 seeded bridges
        labels = [int(x) for x in np.sort(rng.choice(bridges, a.lanes, replace=False))]
        p = prof[b % a.batches]
        D.setInjection_(an, np.broadcast_to(p, (a.lanes, p.size)))
        D.setOutages_(an, labels, islands="shed")
        D.solve_(an)
        rec = D.screenSummary_(an, rating)
        assert (rec[:, 4] == 4).all()
        chains.append(float(np.median(an.time_kernel(0, a.reps))))
    an.close()
    return dict(lanes=a.lanes, bridges=int(bridges.size), sampled_batches=a.batches, device_chain_ms_per_batch=stats(chains[1:]),
                ns_per_case_device_chain=float(np.median(chains[1:])) * 1e6 / a.lanes)


STEPS = {"series": (step_series, 900), "lanes": (step_lanes, 300)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_series_shed_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--batches", type=int, default=6)
    p.add_argument("--profiles", type=int, nargs="+", default=[512, 8760])
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    if a.step:
        print("DC_SERIES_SHED_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps)
    for name in ("series", "lanes"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case,
               "--batches", str(a.batches), "--profiles"] + [str(x) for x in a.profiles]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1])       # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DC_SERIES_SHED_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DC_SERIES_SHED_TIME_JSON "):])
    try:
        import torch
        pr = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
        result["device"] = None if pr is None else dict(name=pr.name, arch=getattr(pr, "gcnArchName", None), compute_units=pr.multi_processor_count,
                                                        memory_GiB=round(pr.total_memory / 2 ** 30, 1))
    except ImportError:
        result["device"] = None
    result["series_screen_steps_per_s_design_3_11"] = 3.10e12
    for T, run in result["series"]["runs"].items():
        run["lane_route_over_screen_per_case"] = result["lanes"]["ns_per_case_device_chain"] / run["shed"]["ns_per_case_wall"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
