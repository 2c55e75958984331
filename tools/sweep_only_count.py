"""What the sweep-only flag (jg_symbolic.hpp: top_dead) keeps the top tasks from storing, counted on the plan of a batched Newton-Raphson handle.

    python tools/sweep_only_count.py [case] [lanes]

Prints, per scenario and factorisation, the 16-byte units the Jordan tasks store with and without the flag, and the bytes of a batch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_case  # noqa: E402
import juliagrid.jl_amd as jg  # noqa: E402

case = sys.argv[1] if len(sys.argv) > 1 else "case_ACTIVSg10k"
lanes = int(sys.argv[2]) if len(sys.argv) > 2 else 512
s = jg.powerSystem(load_case(case))
jg.acModel_(s)
Y = s.model.ac.nodalMatrix
big = Y.n >= 4000
# the policy Engine::create completes for a batch of 256 lanes and more (jg_engine.hip)
policy = 1 | 4 | 1 << 49 | 8 | 1 << 50 | ((47 << 16 | 127 << 24 | 12 << 4) if big else (47 << 16 | (280 // 8) << 24 | 4 << 4))
plan = jg._lib.Plan(Y.n, Y.colptr - 1, Y.rowval - 1, policy=policy)
hdr, data, launches, task_of, info = plan.top_tables()
ok, dead, store = (int(v) for v in plan.get(102))
m, e = hdr[:, 0].astype(np.int64), hdr[:, 1].astype(np.int64)
print(f"{case}: n {Y.n}, tasks {hdr.shape[0]}, task pivots {int((task_of >= 0).sum())}, launches {launches.shape[0]}, Jordan blocks {int(info[7])}")
print(f"flag granted {ok}; 16-byte units per scenario and factorisation: stored without the flag {store}, kept back {dead} ({100.0 * dead / max(store, 1):.1f} %)")
print(f"  of the stored units: diagonal blocks {int(2 * m.sum())}, Jordan rows {int(2 * (m * e).sum())}, y' {int(m.sum())}, update matrices | vectors {int(2 * (e * (e + 1)).sum())}, dead entries {dead}")
print(f"bytes per factorisation of {lanes} lanes: stored {store * 16 * lanes / 1e6:.1f} MB -> {(store - dead) * 16 * lanes / 1e6:.1f} MB (-{dead * 16 * lanes / 1e6:.1f} MB)")
