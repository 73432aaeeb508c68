"""Host logic of the gradient-table hand-over (include/enoki/hip.h: HIPArray::scatter_add_bucketed_ asks ek_hip_bucketed_take_tables
before it adopts uninitialised storage, HIPBuffer::adopt_pointer) under AddressSanitizer + LeakSanitizer + UBSan, no GPU needed.

tests/cpp/direct_tables_host.cpp is a stand-alone program (its own main) over include/enoki/hip.h and the host stand-in of the C ABI
(tests/cpp/host_abi_stub.h).  The stand-in does not define the entry, so the plain build proves the fallback: hip.h's weak reference
is null and every step folds as before.  The second build defines the entry in the program's own translation unit, on malloc'd
memory, and asserts that tables are handed over exactly when every target is fresh and every factor is 1, that a refusal leaves
adopt_uninitialized() + fold, and that every handed-over block is freed exactly once in every drop order.  Nothing is loaded into
python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "direct_tables_host.cpp")


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
    assert "ERROR: AddressSanitizer" not in out.stderr and "ERROR: LeakSanitizer" not in out.stderr and "runtime error" not in out.stderr, \
        out.stderr[-3000:]
    return out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("entry", ["absent", "present"])
def test_direct_tables_under_sanitizers(tmp_path, entry):
    exe = build(tmp_path, "direct_tables_host_" + entry, ["-DTAKE_TABLES_PRESENT"] if entry == "present" else [])
    text = run(exe)
    assert "32 programs agree with eager evaluation" in text and "no block left allocated" in text
    if entry == "absent":
        assert "entry absent: every step folds" in text and " 0 tables handed over" in text
    else:
        # Plain and Masked hand over 2 tables per step, Product 1, two backward() calls 4, one array for both tables 1: 3 steps, 4 drop orders
        assert "entry present: tables taken over" in text and f" {(2 + 2 + 1 + 4 + 1) * 3 * 4} tables handed over" in text
