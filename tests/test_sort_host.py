"""The binding layer of sort / argsort (include/enoki/array.h, hip.h, autodiff.h and the tape node of
enoki_amd/src/autodiff_impl.h) on the host stand-in of the C ABI, no GPU needed.

tests/cpp/sort_host.cpp is a stand-alone program (its own main) that defines ek_hip_sort as std::stable_sort on top of
tests/cpp/host_abi_stub.h: an unevaluated operand is evaluated once, one call serves values and permutation (and an output that was
not requested is not passed), a tracked sort records exactly one node and argsort none, backward scatters and forward gathers through
the permutation, more than 2^32 - 1 entries are refused before the C ABI, an unqualified sort(first, last, cmp) over a std::vector
of arrays still means std::sort, nothing stays allocated.  It is built plain and under AddressSanitizer + UBSan and run as a child
process; nothing is loaded into python.  With -DNO_ENTRY the C ABI lacks the entry and the members say so; with -DBARE_TYPE the same
file is a tiny program in which a flat array type without the members compiles and throws."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sort_host.cpp")
BASE = ["g++", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}"]
FLAVOURS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]}

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


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_binding_layer_on_the_host_stand_in(tmp_path, flavour):
    out = build_and_run(tmp_path, "sort_host_" + flavour, FLAVOURS[flavour])
    assert "operands evaluated once" in out and "one call serves values and permutation" in out
    assert "an output that was not requested is not passed" in out
    assert "one tape node for sort and none for argsort" in out and "gradients permuted" in out
    assert "too many entries refused" in out and "std::sort still compiles" in out
    assert "no block left allocated" in out


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_without_the_entry_the_members_throw(tmp_path, flavour):
    out = build_and_run(tmp_path, "sort_noentry_" + flavour, FLAVOURS[flavour] + ["-DNO_ENTRY"])
    assert "without the entry the members throw and name it" in out


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_a_type_without_the_members_compiles_and_throws(tmp_path, flavour):
    out = build_and_run(tmp_path, "sort_bare_" + flavour, FLAVOURS[flavour] + ["-DBARE_TYPE"])
    assert "a type without the members compiles and throws" in out
