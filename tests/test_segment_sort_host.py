"""The binding layer of segment_sort / segment_argsort (include/enoki/array.h, hip.h, autodiff.h and the block_sort tape node of
enoki_amd/src/autodiff_impl.h, which segment_sort reuses) on the host stand-in of the C ABI, no GPU needed.

tests/cpp/segment_sort_host.cpp is a stand-alone program (its own main) that defines ek_hip_sort_segments as std::stable_sort per
clamped segment on top of tests/cpp/host_abi_stub.h: unevaluated operands are evaluated once, no entries make no call, starts that
are no UInt32 array are refused before the C ABI is reached, one call serves values and permutation, segment_sort records one node
and segment_argsort none, the forward and backward sweeps are each other's transpose (size-1 seeds included), the node releases the
permutation it keeps, nothing stays allocated.  It is built plain and under AddressSanitizer + UBSan; nothing is loaded into
python.  With -DBARE_TYPE the same file is a second tiny program: a flat array type without the members compiles and throws."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "segment_sort_host.cpp")
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
    out = build_and_run(tmp_path, "segment_sort_host_" + flavour, flags)
    assert "operands evaluated once" in out and "no entries make no call" in out and "a wrong starts type refused" in out
    assert "one tape node for segment_sort and none for segment_argsort" in out and "sweeps transpose" in out
    assert "permutation released" in out and "no block left allocated" in out


@pytest.mark.parametrize("flavour", ["plain", "sanitized"])
def test_a_type_without_the_members_compiles_and_throws(tmp_path, flavour):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if flavour == "sanitized" else ["-O1"]
    out = build_and_run(tmp_path, "segment_sort_bare_" + flavour, flags + ["-DBARE_TYPE"])
    assert "a type without the members compiles and throws" in out
