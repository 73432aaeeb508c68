"""Host logic of the kind-2 node with a host-scalar addend that REQUIRES A GRADIENT under AddressSanitizer + LeakSanitizer + UBSan,
no GPU needed.

tests/cpp/trainable_addend_host.cpp is a stand-alone program (its own main) over include/enoki/hip.h, include/enoki/autodiff.h and
the host stand-in of the C ABI (tests/cpp/host_abi_stub.h).  The stand-in defines neither ek_hip_bucketed_pair_create_scalar nor
ek_hip_bucketed_addend_adjoint, so the plain build proves the fallback: the weak references are null, DiffArray's guard arms and the
programs run in element order with the eager bits.  The second build defines both entries on top of the stand-in: the node forms,
the gradient of the scalar is one call of the new entry, same bits.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "trainable_addend_host.cpp")


def build(tmp, name, defines):
    exe = os.path.join(str(tmp), name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{os.path.join(ROOT, 'include')}"] + defines + [SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("ENOKI_HIP_DEFER", "ENOKI_HIP_DEFER_GATHER", "ENOKI_HIP_DEFER_MIN"):
        env.pop(k, None)
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("entries", ["absent", "present"])
def test_trainable_addend_node_under_sanitizers(tmp_path, entries):
    exe = build(tmp_path, "trainable_addend_host_" + entries, ["-DTRAINABLE_ENTRIES_PRESENT"] if entries == "present" else [])
    text = run(exe)
    assert "agree with eager evaluation" in text and "no block left allocated" in text
    assert ("entries absent: element-order fallback" if entries == "absent" else "entries present: the gradient of the scalar") in text
