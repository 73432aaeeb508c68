"""Host model of the refined stream of a kept bucket partition (enoki_amd/csrc/ek_refine.h) under AddressSanitizer + UBSan, no GPU
needed: tests/cpp/partition_refine_host.cpp is a stand-alone program (its own main) over the header the kernels include.  It lays
pieces out into buffers of exactly the size the host's bound gives and checks the slot mapping (a bijection onto the piece's tiles,
lane-transposed, a group inside one slot) and the bound for the piece shapes where it can go wrong: empty, one element, runs of
1, 3, 4, 5 and 4 R 64 +- 1, one entry holding everything, every entry holding one.  Built for every R the kernels may be built
with.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "partition_refine_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("R", [4, 8, 16])
def test_layout_and_bound_under_sanitizers(tmp_path, R):
    exe = os.path.join(str(tmp_path), f"partition_refine_host_{R}")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", f"-DEK_REFINE_R={R}", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert f"R = {R}," in out.stdout and "checks passed" in out.stdout
