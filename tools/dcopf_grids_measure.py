"""Measures, on the CPU, the figures of tests/dcopf_grids.py's MEASURED (its bounds() are ten times these), per dressed grid at rho = 0.1, not adapted:
  move         the restatement between tolerance 1e-9 and 1e-10 over lanes 0, 63 and 64: angles, outputs and helpers, nodal prices, objective (relative)
  certificate  the restatement's KKT certificate, the worst over all 65 lanes of the device test
  polish       lane 0's restatement from the polished point (as move)
Prints the entries to paste into tests/dcopf_grids.py.

    python tools/dcopf_grids_measure.py [grid ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dcopf_grids as Q                                                  # noqa: E402
import dcopf_reference as R                                              # noqa: E402


def measure(name):
    s, _ = Q.grid(name)
    move, cert = np.zeros(4), np.zeros(4)
    for j in Q.REFERENCE_LANES:
        md, a = Q.solved(name, j)
        _, b = Q.solved(name, j, tolerance=1e-10)
        assert a.status == 0 and b.status == 0, (name, j, a.status, b.status)
        move = np.maximum(move, np.r_[Q.distance(md, a.x, a.y, b.x, b.y), abs(a.objective - b.objective) / abs(b.objective)])
    for j in range(Q.LANES):                                             # the device test holds every lane to the certificate
        md, a = Q.solved(name, j)
        assert a.status == 0, (name, j, a.status)
        th, gp, h = R.parts(md, s, a.x)
        cert = np.maximum(cert, R.kkt(md, md.l, md.u, th, gp, h, R.duals(md, s, a.y)))
    md, a = Q.solved(name)
    p = Q.polished(name)
    return dict(move=move, certificate=cert, polish=np.r_[Q.distance(md, a.x, a.y, p.x, p.y), abs(a.objective - p.objective) / abs(p.objective)])


if __name__ == "__main__":
    for name in sys.argv[1:] or list(Q.GRIDS):
        out = measure(name)
        print(f'    "{name}": dict(' + ", ".join(f"{k}=({', '.join(f'{x:.2e}' for x in v)})" for k, v in out.items()) + "),", flush=True)
