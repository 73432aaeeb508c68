"""The binding layer of block_search_sorted (include/enoki/array.h, hip.h, autodiff.h) on the host stand-in of the C ABI, no GPU
needed.

tests/cpp/block_search_sorted_host.cpp is a stand-alone program (its own main) that defines ek_hip_search_sorted_blocks as a host loop
on top of tests/cpp/host_abi_stub.h: unevaluated operands are evaluated once, blocked and indexed needles reach the entry as called,
the length checks of the binding layer hold before any call, a DiffArray call records no node, nothing stays allocated.  It is built
plain and under AddressSanitizer + UBSan; nothing is loaded into python.  A table and needles of different element types must not
compile."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "block_search_sorted_host.cpp")
BASE = ["g++", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.mark.parametrize("flavour", ["plain", "sanitized"])
def test_binding_layer_on_the_host_stand_in(tmp_path, flavour):
    exe = os.path.join(str(tmp_path), "block_search_sorted_host_" + flavour)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if flavour == "sanitized" else ["-O1"]
    r = subprocess.run(BASE + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("ENOKI_HIP_DEFER", "ENOKI_HIP_DEFER_GATHER", "ENOKI_HIP_DEFER_MIN"):
        env.pop(k, None)
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert "operands evaluated once" in out.stdout and "length checks hold" in out.stdout
    assert "no tape node" in out.stdout and "no block left allocated" in out.stdout


def test_mismatched_element_types_do_not_compile():
    cmd = BASE + ["-fsyntax-only", SRC]
    ok = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert ok.returncode == 0, ok.stderr[-3000:]
    bad = subprocess.run(cmd + ["-DEXPECT_FAIL"], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "block_search_sorted(): table and needles must have the same element type" in bad.stderr, bad.stderr[-3000:]
