"""What the sweep-only flag (jg_symbolic.hpp: top_dead) keeps the top tasks from storing, counted on the plan of a batched Newton-Raphson handle.

    python tools/sweep_only_count.py [case] [lanes]

Prints, per scenario and factorisation, the 16-byte units the Jordan tasks store with and without the flag, and the bytes of a batch; then what a handle
without the bus-order increment (jg_nr_set_keep_increment(h, 0)) no longer writes per backward sweep and per shared-factor first step."""
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
# the bus-order increment: every solved row is stored once more, 16 bytes, in bus order -- by the backward sweep of a refactorising iteration and by the backward
# rows + the dense top's epilogue of a shared-factor first step alike (one store per pivot and active scenario); a lane compaction carries the same rows.
# Counted from the tables: the rows of the Jordan sweep's records and chain tasks, the backward records and top pivots of the shared-factor plan.
seg, rec = plan.replay_tables("bwdj")
chain = plan.get("bwd_chain")
rows = set()
for base, nchunks, wpi, rpw, *_ in seg:
    if wpi <= 0:
        for t in range(nchunks):
            nb, _, off, _ = (int(v) for v in rec[base + t][:4])
            rows.update(int(v) for v in chain[off:off + 3 * nb:3])
    else:
        rows.update(int(r[0]) for r in rec[base: base + nchunks * 16 * rpw] if r[0] >= 0)
cinfo, ctop, _, (cseg, crec) = plan.comp_tables(512)
crow = set(int(r[0]) for r in crec if r[0] >= 0)
unit = 16 * lanes
print(f"without the bus-order increment (A), {lanes} lanes, all active: backward sweep {len(rows)} rows = {len(rows) * unit / 1e6:.2f} MB less written; shared-factor step "
      f"{len(crow)} backward rows + {ctop.size} top pivots = {len(crow) * unit / 1e6:.2f} + {ctop.size * unit / 1e6:.2f} = {(len(crow) + ctop.size) * unit / 1e6:.2f} MB less; "
      f"a compaction moves {16 * Y.n} B less per lane that changes place (read and written)")


def comp_get(which):
    L = jg._lib.plan_lib()
    m = L.jg_plan_comp_export(plan.h, 512, which, None, 0)
    out = np.zeros(max(m, 1), dtype=np.int32)
    L.jg_plan_comp_export(plan.h, 512, which, out.ctypes.data, m)
    return out[:m]


ok, dead_rows = (int(v) for v in plan.get(104))
cdead, cdead_top = (int(v) for v in comp_get(7))
print(f"pivot-order stores nobody reads back (B), flag granted {ok}: backward sweep {dead_rows} of {Y.n} rows = {dead_rows * unit / 1e6:.2f} MB less written; shared-factor step "
      f"{cdead} rows ({cdead_top} of them top pivots) = {cdead * unit / 1e6:.2f} MB less")
print(f"A + B: {(len(rows) + dead_rows) * unit / 1e6:.2f} MB per backward sweep, {(len(crow) + ctop.size + cdead) * unit / 1e6:.2f} MB per shared-factor step")
