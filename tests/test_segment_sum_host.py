"""The binding layer of segment_sum / segment_prod / segment_min / segment_max / segment_repeat (include/enoki/array.h, hip.h,
autodiff.h and the tape nodes of enoki_amd/src/autodiff_impl.h) on the host stand-in of the C ABI, no GPU needed.

tests/cpp/segment_sum_host.cpp is a stand-alone program (its own main) that defines ek_hip_reduce_segments and ek_hip_repeat_segments
as host loops on top of tests/cpp/host_abi_stub.h: the clamp rule of enoki_amd/csrc/ek_block.h keeps every segment inside the array
for starts above n and decreasing starts, an unevaluated operand is evaluated once, values that do not match the starts throw before
the C ABI is reached, segment_sum and segment_repeat record one node each whose forward and backward sweeps are each other's
transpose (size-1 seeds included), segment_max of a tracked array throws, the node releases the starts it keeps, nothing stays
allocated.  It is built plain and under AddressSanitizer + UBSan; nothing is loaded into python.  With -DBARE_TYPE the same file is
a second tiny program: a flat array type without the members compiles and throws."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "segment_sum_host.cpp")
BASE = ["g++", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build_and_run(tmp_path, name, flags):
    exe = os.path.join(str(tmp_path), name)
    r = subprocess.run(BASE + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("ENOKI_HIP_DEFER", "ENOKI_HIP_DEFER_GATHER", "ENOKI_HIP_DEFER_MIN"):
        env.pop(k, None)
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return out.stdout


@pytest.mark.parametrize("flavour", ["plain", "sanitized"])
def test_binding_layer_on_the_host_stand_in(tmp_path, flavour):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if flavour == "sanitized" else ["-O1"]
    out = build_and_run(tmp_path, "segment_sum_host_" + flavour, flags)
    assert "clamp rule holds" in out and "operands evaluated once" in out and "bad shapes refused" in out
    assert "tape nodes transpose" in out and "starts released" in out and "no block left allocated" in out


@pytest.mark.parametrize("flavour", ["plain", "sanitized"])
def test_a_type_without_the_members_compiles_and_throws(tmp_path, flavour):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if flavour == "sanitized" else ["-O1"]
    out = build_and_run(tmp_path, "segment_sum_bare_" + flavour, flags + ["-DBARE_TYPE"])
    assert "a type without the members compiles and throws" in out
