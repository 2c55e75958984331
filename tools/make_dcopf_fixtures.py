#!/usr/bin/env python3
"""Writes the fixtures of the DC optimal power flow tests from a checkout of the reference.

    python tools/make_dcopf_fixtures.py <path to the reference checkout>

tests/golden/results_dcopf_<case>.npz: /case{14,30}test/dcOptimalPowerFlow/{voltage, from, injection, supply, generator} of test/data/results.h5
(MATPOWER's solution), read with the project's own HDF5 reader (juliagrid.jl_amd/hdf5.py).
tests/golden/cases/<case>_opf.npz: what the optimal power flow reads beyond the existing case fixtures -- the cost tables, pmin, the branch
ratings and the angle-difference limits of test/data/<case>.m, in the units of system.py's tables.  Data only, a few kB; the existing case
fixtures stay as they are.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPF_KEYS = ("gen_pmin", "gen_pmax", "br_rating", "br_angmin", "br_angmax", "gen_cost_model", "gen_cost_ptr", "gen_cost_data")


def main(reference):
    import importlib
    hdf5 = importlib.import_module("juliagrid.jl_amd.hdf5")
    system = importlib.import_module("juliagrid.jl_amd.system")
    f = hdf5.H5File(os.path.join(reference, "test", "data", "results.h5"))
    for case in ("case14test", "case30test"):
        out = {}
        for name in ("voltage", "from", "injection", "supply", "generator"):
            out[name] = np.asarray(f.read(f"/{case}/dcOptimalPowerFlow/{name}"), dtype=np.float64).reshape(-1)
        path = os.path.join(ROOT, "tests", "golden", f"results_dcopf_{case}.npz")
        np.savez(path, **out)
        print(path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
        t = system._matpower_tables(os.path.join(reference, "test", "data", case + ".m"))
        path = os.path.join(ROOT, "tests", "golden", "cases", case + "_opf.npz")
        np.savez(path, **{k: t[k] for k in OPF_KEYS})
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
