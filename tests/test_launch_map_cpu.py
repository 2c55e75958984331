"""The workgroup -> (lane group, chunk) mapping of every level launch (csrc/jg_engine.hpp: map_slot, grid_blocks), walked exhaustively on the host.

The GPU tests sample a few (handle group count, active group count, chunks per group) triples; the arithmetic has its edges elsewhere -- `chunk = (total + 7) >> 3`
with `total` just above a multiple of 8, a grid sized for the pinned class serving a count of the balanced one after compaction and the other way round.
tools/map_check.cpp includes the header the kernels include and loops over handle counts 1..72, every active count up to the handle's and twelve chunk counts: every
pair exactly once, nothing outside, slot == id % gact for pinned counts, one contiguous run per XCD for balanced counts.  Built with AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_every_pair_of_every_launch_is_served_exactly_once(tmp_path):
    from juliagrid.jl_amd import build as B
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B.hipcc()))), "include")      # jg_engine.hpp includes hip/hip_runtime.h (host half only here)
    exe = str(tmp_path / "map_check")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                        "-I", include, "-o", exe, os.path.join(ROOT, "tools", "map_check.cpp")], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, (c.stdout + c.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out[-2000:])
    assert r.returncode == 0, out[-3000:]
    assert " 0 failures" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
