"""The polar power-flow equations the Newton-Raphson kernels call (csrc/jg_pf.hpp), checked on the host.

The assembly, the refinement residual and the shared-factor first step must agree on the Jacobian to the bit, so its formulas are stated once, in a header of
arithmetic on register values.  tools/pf_check.cpp includes that header and, on small grids it generates itself (complete grids of 3 .. 6 buses under every mix of
PQ / PV / slack, a row of one entry, a row of 19), compares the mismatch with V conj(Y V) - S in complex arithmetic (1e-12 of the row's scale), every existing
Jacobian entry with a central difference of that restatement (1e-7), masked entries and identity rows exactly, the edit patch bit for bit, the dG / dB form of
the first-step correction with the difference of two assemblies (1e-12) and the branch-end currents and powers with I = Y_branch V (1e-12).  Built with
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_header_states_the_power_flow_equations(tmp_path):
    from juliagrid.jl_amd import build as B
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B.hipcc()))), "include")      # jg_engine.hpp includes hip/hip_runtime.h (host half only here)
    exe = str(tmp_path / "pf_check")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                        "-I", include, "-o", exe, os.path.join(ROOT, "tools", "pf_check.cpp")], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out[-2000:])
    assert r.returncode == 0, out[-3000:]
    assert " 0 failures" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
