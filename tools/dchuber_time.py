#!/usr/bin/env python3
"""Times the batched DC Huber estimator (dcHuberStateEstimation, csrc/jg_dchuber.hip) on the measurement set of tools/dclav_time.py: the 10k-bus grid's
full set (injection + from + to wattmeters at 1e-2, bus PMUs at 1e-5), LANES realisations with seeded noise, three gross errors in every fourth lane.

    python tools/dchuber_time.py [--out profiles/dchuber_time.json] [--reps 10] [--lanes 512] [--case case_ACTIVSg10k] [--sample 1]

Every step that uses the GPU runs in a child process of its own under a time limit; the first step that fails ends the run.  Steps:
  huber  set-up (host wall clock of dcHuberStateEstimation), the handle's dims (bytes per lane among them), wall clock of a solve of the batch, the
         lanes' iteration counts and statuses, ms per iteration and per part (jg_dchuber_time_kernel: HIP events, median of REPS, every lane running)
  lav    the same figures of dcLavStateEstimation(weighted=True) on the same readings: its factorisation is the one the Huber iteration uses, so an
         iteration of either should cost the same
  host   the method of tests/dchuber_reference.py with scipy.sparse matrices and a sparse LU (the dense restatement does not fit a 45 412 x 10 000 H) on
         SAMPLE lanes on one core: seconds per lane and per iteration; `extrapolated` = that x LANES, stated as such
Nothing is compared against the code under test here; the tests do that (tests/test_dchuber_gpu.py).
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

SEED = 13
KERNELS = ("iteration", "assembly", "factorisation", "sweep_pair", "passes")


def build(a):
    import dc_reference as R
    import dcse_reference as S
    from conftest import load_case
    t = load_case(a.case)
    th, _ = R.solve(t)
    ms = S.full_set(t, th)
    z = S.model(t, ms).mean
    rng = np.random.default_rng(SEED)
    sigma = np.sqrt(np.r_[ms.w_variance, ms.p_variance])
    Z = z[None, :] + sigma[None, :] * rng.standard_normal((a.lanes, z.size))
    for s in range(0, a.lanes, 4):
        Z[s, rng.choice(ms.w_index.size, 3, replace=False)] += 5.0
    return t, ms, Z, sigma


def timed(an, mod, Z, setup, reps):
    mod.setReadings_(an, Z)
    t0 = time.perf_counter()
    mod.solve_(an)
    wall = time.perf_counter() - t0
    it = np.atleast_1d(an.iterations)
    out = dict(setup_s=setup, dims=an.dims(), solve_wall_s=wall, iterations=dict(min=int(it.min()), median=float(np.median(it)), max=int(it.max())),
               status={str(k): int(v) for k, v in zip(*np.unique(np.atleast_1d(an.status), return_counts=True))}, ms={})
    for k, name in enumerate(KERNELS):
        ms_k = an.time_kernel(k, reps)
        out["ms"][name] = dict(median=float(np.median(ms_k)), min=float(ms_k.min()), max=float(ms_k.max()), reps=int(reps))
    an.close()
    return out


def step_device(a, which):
    import torch  # noqa: F401  (one HIP runtime for the process: tests/conftest.py)
    import juliagrid.jl_amd as jg
    from test_dcse_host import monitoring_of
    t, ms, Z, _ = build(a)
    mon = monitoring_of(jg, t, ms)
    t0 = time.perf_counter()
    an = jg.dcHuberStateEstimation(mon, batch=a.lanes) if which == "huber" else jg.dcLavStateEstimation(mon, batch=a.lanes, weighted=True)
    return timed(an, jg.dchuberstateestimation if which == "huber" else jg.dclavstateestimation, Z, time.perf_counter() - t0, a.reps)


def sparse_huber(H, z, kappa, slack, iteration=50, tolerance=1e-8):
    """tests/dchuber_reference.huber_ipm with H in CSR and the gain through a sparse LU; every row in service.  -> iterations, status"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    m, n = H.shape
    Ht = H.T.tocsr()
    fix = sp.csr_matrix(([1.0], ([slack], [slack])), shape=(n, n))
    hnorm, k = float(abs(H).sum(axis=0).max()), np.full(m, float(kappa))

    def solve(q, rhs):
        x = sla.splu((Ht @ sp.diags(q) @ H + fix).tocsc()).solve(rhs)
        x[slack] = 0.0
        return x

    def boundary(x, dx):
        neg = dx < 0.0
        return float(np.min(-x[neg] / dx[neg])) if neg.any() else np.inf

    theta = solve(np.ones(m), Ht @ z)
    r0 = z - H @ theta
    y = np.clip(r0, -0.5 * k, 0.5 * k)
    r1 = r0 - y
    s = max(np.abs(r1).sum() / m, 1e-8)
    u, v = np.maximum(r1, 0.0) + s, np.maximum(-r1, 0.0) + s
    for it in range(iteration + 1):
        r = z - H @ theta
        rp, rd = r - y - u + v, -(Ht @ y)
        gap, obj = float((u * (k - y) + v * (k + y)).sum()), float((0.5 * y * y + k * (u + v)).sum())
        if np.abs(rp).max() <= tolerance * (1.0 + np.abs(z).max()) and np.abs(rd).max() <= tolerance * hnorm * k.max() and gap <= tolerance * (1.0 + obj):
            return it, 0
        if it == iteration:
            break
        q = 1.0 / (1.0 + u / (k - y) + v / (k + y))
        lu = sla.splu((Ht @ sp.diags(q) @ H + fix).tocsc())

        def step(t):
            d = lu.solve(Ht @ t - rd)
            d[slack] = 0.0
            return d
        dth = step(q * (r - y))
        dya = q * (r - y - H @ dth)
        dua, dva = -u + u * dya / (k - y), -v - v * dya / (k + y)
        aa = min(1.0, boundary(u, dua), boundary(v, dva), boundary(k - y, -dya), boundary(k + y, dya))
        smu = (float(((u + aa * dua) * (k - y - aa * dya) + (v + aa * dva) * (k + y + aa * dya)).sum()) / gap) ** 3 * gap / (2.0 * m)
        cu, cv = smu - u * (k - y) + dua * dya, smu - v * (k + y) - dva * dya
        c = cu / (k - y) - cv / (k + y)
        dth = step(q * (rp - c))
        dy = q * (rp - c - H @ dth)
        du, dv = (cu + u * dy) / (k - y), (cv - v * dy) / (k + y)
        al = min(1.0, 0.995 * min(boundary(u, du), boundary(v, dv), boundary(k - y, -dy), boundary(k + y, dy)))
        theta, u, v, y = theta + al * dth, u + al * du, v + al * dv, y + al * dy
    return iteration, 5


def step_host(a):
    import dcse_reference as S
    t, ms, Z, sigma = build(a)
    H, w, _, slack = S.matrices(t, ms)
    import scipy.sparse as sp
    Hs = (sp.diags(np.sqrt(w)) @ H).tocsr()
    secs, its = [], []
    for s in range(a.sample):
        t0 = time.perf_counter()
        it, status = sparse_huber(Hs, Z[s] / sigma, 1.345, slack)
        secs.append(time.perf_counter() - t0)
        its.append(it)
        assert status == 0
    per = float(np.median(secs))
    return dict(restatement_s_per_lane=per, iterations=its, s_per_iteration=per / max(float(np.median(its)), 1.0), sample=a.sample,
                extrapolated_s_for_batch=per * a.lanes,
                note="the method with scipy.sparse and a sparse LU per iteration on one core; the batch figure is the sample's median x lanes, not a run")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dchuber_time.json"))
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--lanes", type=int, default=512)
    p.add_argument("--case", default="case_ACTIVSg10k")
    p.add_argument("--sample", type=int, default=1)
    p.add_argument("--step", default=None)
    a = p.parse_args()
    steps = {"huber": lambda a: step_device(a, "huber"), "lav": lambda a: step_device(a, "lav"), "host": step_host}
    if a.step:
        print("__RESULT__" + json.dumps(steps[a.step](a)))
        return
    result = dict(case=a.case, lanes=a.lanes, seed=SEED)
    for step, limit in (("huber", 600), ("lav", 600), ("host", 1200)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--lanes", str(a.lanes), "--case", a.case, "--sample", str(a.sample)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        line = [l for l in r.stdout.splitlines() if l.startswith("__RESULT__")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"step {step} failed with code {r.returncode}: the run ends here")
        result[step] = json.loads(line[0][len("__RESULT__"):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
