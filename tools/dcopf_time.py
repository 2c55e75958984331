#!/usr/bin/env python3
"""Times the batched DC optimal power flow (dcOptimalPowerFlow, csrc/jg_dcopf.hip) on the 10k-bus grid: synthetic quadratic costs and branch ratings
from a seeded draw, 512 lanes of demand scaled by seeded factors in [0.9, 1.05].

    python tools/dcopf_time.py [--out profiles/dcopf_time.json] [--reps 25] [--lanes 512] [--case case_ACTIVSg10k] [--sample 2]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  opf    set-up (host wall clock of dcOptimalPowerFlow), ms per iteration and per kernel (jg_dcopf_time: HIP events, median of REPS), iterations to
         1e-6 and to 1e-9 with the refactorisations and the wall clock of each solve
  host   the scipy.sparse restatement of the same iteration (splu of K, one right-hand side per iteration) on SAMPLE lanes on one core: ms per lane
         to 1e-6 (no GPU)
Nothing is compared against the code under test here; the tests do that (tests/test_dcopf_gpu.py).
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

SEED = 11


def build(a):
    """The grid with costs c2 in [5, 50], c1 in [1e3, 4e3] per per-unit power, pmin 0, ratings at 1.5 x the base DC flow (at least 0.5 p.u.)."""
    import importlib
    jg = importlib.import_module("juliagrid.jl_amd")
    from conftest import load_case
    t = dict(load_case(a.case))
    rng = np.random.default_rng(SEED)
    ng, nb = np.asarray(t["gen_bus"]).size, np.asarray(t["br_from"]).size
    c2, c1 = rng.uniform(5.0, 50.0, ng), rng.uniform(1e3, 4e3, ng)
    t.update(gen_pmin=np.zeros(ng), gen_cost_model=np.full(ng, 2, dtype=np.int8), gen_cost_ptr=np.arange(0, 3 * ng + 1, 3),
             gen_cost_data=np.stack([c2, c1, np.zeros(ng)], axis=1).reshape(-1))
    s = jg.powerSystem(t)
    jg.dcModel_(s)
    pf = jg.dcPowerFlow(s)
    jg.powerFlow_(pf, power=True)
    t["br_rating"] = np.maximum(1.5 * np.abs(np.asarray(pf.power.from_.active)), 0.5)
    s = jg.powerSystem(t)
    jg.dcModel_(s)
    demand = s.bus.demand.active[None, :] * rng.uniform(0.9, 1.05, size=a.lanes)[:, None]
    return jg, s, demand


def stats(ms, reps):
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), reps=int(reps))


def step_opf(a):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    jg, s, demand = build(a)
    opf = jg.dcoptimalpowerflow
    L, check = jg._lib.lib(), jg._lib.check
    out = dict(lanes=a.lanes)
    for tol in (1e-6, 1e-9):
        t0 = time.perf_counter()
        an = jg.dcOptimalPowerFlow(s, batch=a.lanes, tolerance=tol, iteration=a.iteration)
        setup = (time.perf_counter() - t0) * 1e3
        opf.setInjection_(an, demand)
        t0 = time.perf_counter()
        opf.solve_(an)
        wall = (time.perf_counter() - t0) * 1e3
        out[f"tolerance_{tol:g}"] = dict(setup_ms=setup, solve_wall_ms=wall, iterations_median=float(np.median(an.iterations)), iterations_max=int(np.max(an.iterations)),
                                         status_counts=np.bincount(np.asarray(an.status), minlength=6).tolist(), refactorisations=an.refactorisations,
                                         variables=an.model.n, rows=an.model.m)
    names = ("iteration", "rhs", "sweep_pair", "update", "residual_verdict", "assemble_refactorise")
    for k, name in enumerate(names):
        warm = np.zeros(3)
        check(L.jg_dcopf_time(an._h, k, 3, warm))
        ms = np.zeros(a.reps)
        check(L.jg_dcopf_time(an._h, k, a.reps, ms))
        out[name + "_ms"] = stats(ms, a.reps)
    return out


def step_host(a):
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    jg, s, demand = build(a)
    opf = jg.dcoptimalpowerflow
    md = opf.modelRows(s)
    A = sp.csr_matrix((md.val, md.col, md.rowptr), shape=(md.m, md.n))
    c = 1.0 / max(md.P.max(), np.abs(md.q).max())
    E = 1.0 / np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).reshape(-1))
    A = sp.diags(E) @ A
    P, q, rho, sigma, alpha, tol = c * md.P, c * md.q, 0.1, 1e-6, 1.6, 1e-6
    rv = np.where(md.equality == 1, 1e3 * rho, rho)
    bal = md.rows["balance"]
    per_lane, its = [], []
    for j in range(a.sample):
        l, u = md.l.copy(), md.u.copy()
        l[bal] = u[bal] = -(demand[j] + s.bus.shunt.conductance + s.model.dc.shiftPower)
        lo, up = np.where(np.isfinite(l), E * l, -1e30), np.where(np.isfinite(u), E * u, 1e30)
        t0 = time.perf_counter()
        lu = sla.splu((sp.diags(P + sigma) + A.T @ sp.diags(rv) @ A).tocsc())
        x, z, y = np.zeros(md.n), np.zeros(md.m), np.zeros(md.m)
        for k in range(1, a.iteration + 1):
            xt = lu.solve(sigma * x - q + A.T @ (rv * z - y))
            x = alpha * xt + (1 - alpha) * x
            zr = alpha * (A @ xt) + (1 - alpha) * z
            zn = np.clip(zr + y / rv, lo, up)
            y, z = y + rv * (zr - zn), zn
            if k % 25 == 0:
                ax, aty = A @ x, A.T @ y
                if (np.abs(ax - z).max() <= tol * (1 + max(np.abs(ax).max(), np.abs(z).max()))
                        and np.abs(P * x + q + aty).max() <= tol * (1 + max(np.abs(P * x).max(), np.abs(aty).max(), np.abs(q).max()))):
                    break
        per_lane.append((time.perf_counter() - t0) * 1e3)
        its.append(k)
    return dict(sample=a.sample, ms_per_lane=float(np.median(per_lane)), iterations=its, tolerance=tol, rho="fixed 0.1", threads=1)


STEPS = {"opf": (step_opf, 900), "host": (step_host, 900)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcopf_time.json"))
    p.add_argument("--reps", type=int, default=25)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--sample", type=int, default=2)
    p.add_argument("--iteration", type=int, default=20000)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--step", choices=sorted(STEPS))
    a = p.parse_args()
    if a.reps < 20:
        p.error("--reps: at least 20")
    if a.step:
        print("DCOPF_TIME_JSON " + json.dumps(STEPS[a.step][0](a), default=str))
        return
    result = dict(case=a.case, lanes=a.lanes, reps=a.reps)
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    for name in ("opf", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--lanes", str(a.lanes), "--sample", str(a.sample),
               "--iteration", str(a.iteration), "--case", a.case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1], env=env if name == "host" else None)   # a time limit of its own
        line = [l for l in r.stdout.splitlines() if l.startswith("DCOPF_TIME_JSON ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {name} failed (exit {r.returncode}): nothing further is started")
        result[name] = json.loads(line[0][len("DCOPF_TIME_JSON "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
