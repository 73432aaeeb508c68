"""Reference counts and reader lists of HIPArray's unevaluated nodes when ONE buffer fills several source slots, under
AddressSanitizer + LeakSanitizer + UBSan, no GPU needed.

tests/cpp/aliased_sources_host.cpp is a stand-alone program (its own main) over include/enoki/hip.h and the host stand-in of the C
ABI (tests/cpp/host_abi_stub.h): `fmadd(gather(A, i), A, gather(A, i))`, `gather(A, i) * A`, the two scalar-addend forms,
`fmadd(a, a, a)`, `a * a + a`, each also under a map.  Built once, run at 64 Ki elements with the binding's own thresholds and at
16 elements with every threshold at 1.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "aliased_sources_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("aliased_sources")), "aliased_sources_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{os.path.join(ROOT, 'include')}", SRC, "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("args, elements", [([], 1 << 16), (["--tiny"], 16)])
def test_aliased_sources_under_sanitizers(exe, args, elements):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in ("ENOKI_HIP_DEFER", "ENOKI_HIP_DEFER_GATHER", "ENOKI_HIP_DEFER_MIN"):
        env.pop(k, None)
    out = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert f"{elements} elements, 7 node shapes agree with eager evaluation, no block left allocated" in out.stdout
