#!/usr/bin/env python3
"""Writes tests/golden/results_gs_<case>.npz from the Gauss-Seidel vectors of the reference's test/data/results.h5.

    python tools/make_gs_fixtures.py <path to the reference checkout>

Data only: /case{14,30}test/gaussSeidel/{iteration, voltageMagnitude, voltageAngle}, a few hundred bytes per case (the MATPOWER results the
reference's own test holds its gaussSeidel against, test/powerFlow/analysis.jl:145-171).  The file is read with the project's own HDF5 reader
(juliagrid.jl_amd/hdf5.py).  tests/gs_reference.py is pinned to these vectors (tests/test_gs_host.py).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(reference):
    from juliagrid.jl_amd.hdf5 import H5File
    f = H5File(os.path.join(reference, "test", "data", "results.h5"))
    for case in ("case14test", "case30test"):
        out = {"iteration": np.asarray(f.read(f"/{case}/gaussSeidel/iteration")).reshape(-1).astype(np.int64)}
        for name in ("voltageMagnitude", "voltageAngle"):
            out[name] = np.asarray(f.read(f"/{case}/gaussSeidel/{name}"), dtype=np.float64).reshape(-1)
        path = os.path.join(ROOT, "tests", "golden", f"results_gs_{case}.npz")
        np.savez(path, **out)
        print(path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
