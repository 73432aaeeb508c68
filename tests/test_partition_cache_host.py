"""Host logic of the partition cache (include/enoki/hip.h, HIPBuffer::PartitionEntry: the bucket partition of a kind-2 node stays on its
index array while index, x and mask cannot change) under AddressSanitizer + LeakSanitizer + UBSan, no GPU needed.

tests/cpp/partition_cache_host.cpp is a stand-alone program (its own main) over include/enoki/hip.h and the host stand-in of the C
ABI (tests/cpp/host_abi_stub.h).  The stand-in defines none of the partition entries, so the plain build proves the fallback: hip.h's
weak references are null and every step partitions for itself.  The second build defines the entries in the program's own
translation unit -- a partition is a copy of (index, x, mask), so a hit on a stale entry shows as a wrong value -- and sends the same
programs through them: directed scenarios, the handles dropped in every order, and seeded walks over interleavings of steps, writes,
exports, pointer hand-outs and the switch.  The program counts partitions built and asserts the number scenario by scenario.
Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "partition_cache_host.cpp")


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
def test_partition_cache_under_sanitizers(tmp_path, entries):
    exe = build(tmp_path, "partition_cache_host_" + entries, ["-DPARTITION_ENTRIES_PRESENT"] if entries == "present" else [])
    text = run(exe)
    assert "agree with eager evaluation" in text and "no block left allocated" in text
    assert ("entries absent: one partition per step" if entries == "absent" else "entries present: partitions kept") in text
    if entries == "absent":
        assert " 0 objects made on a kept one" in text
