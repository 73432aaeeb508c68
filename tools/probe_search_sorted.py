"""search_sorted next to the spelling it replaces, on the same inputs, in one process.  GPU box:

    python tools/probe_search_sorted.py [n_log2 [seconds]] > profiles/probe_search_sorted_rNN.txt

    (a) binary_search(0, K, lambda i: gather(T, min(i, K - 1)) < needles)     log2(K) + 1 rounds of min / gather+compare / select / select
        (enoki_amd.hip.binary_search runs the C++ loop of include/enoki/array.h; the predicate is called back once per round, which
        the device never waits for at this size)
    (b) search_sorted(T, needles)                                             one kernel (csrc/search.hip)

n = 2^n_log2 (default 26) uniform float32 needles in [0, 1); tables of K = 1 Ki, 64 Ki, 1 Mi, 16 Mi sorted entries, uniform in [0, 1)
and the CDF of Zipf weights 1 / (k + 1).  Per shape: the two results are compared (exact equality) BEFORE anything is timed, then
one warm-up call and `reps` calls each, every call between its own pair of HIP events on the library stream; the line gives the
minimum and the median, needles per second at the minimum and the minimum's share of the floor of 8 B per needle at 8 TB/s.
The process ends itself after `seconds` (default 900)."""
import os
import platform
import signal
import statistics
import sys

import numpy as np
import torch  # first: torch ships its own HIP runtime, which must initialise before the library's (tests/conftest.py)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enoki_amd import capi, hiprt  # noqa: E402
import enoki_amd.hip as ek  # noqa: E402

n_log2 = int(sys.argv[1]) if len(sys.argv) > 1 else 26
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 900)
capi.init(); st = capi.stream()
n = 1 << n_log2
FLOOR_BYTES, PEAK = 8, 8e12


def device_name():
    p = torch.cuda.get_device_properties(capi.lib.ek_hip_device())
    return f"{p.name or 'unnamed device'} ({p.gcnArchName}, {p.multi_processor_count} CUs, {p.total_memory >> 30} GiB)"


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = hiprt.Event(), hiprt.Event()
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_ms(e1))
    return min(ms), statistics.median(ms)


def tables(K, rng):
    uniform = np.sort(rng.random(K, dtype=np.float32))
    w = 1.0 / np.arange(1, K + 1, dtype=np.float64)
    zipf = (np.cumsum(w) / w.sum()).astype(np.float32)
    return (("uniform", uniform), ("zipf cdf", zipf))


print(f"# probe_search_sorted on {platform.node()}: {device_name()}; n = 2^{n_log2} float32 needles, floor = {FLOOR_BYTES} B/needle at 8 TB/s "
      f"= {n * FLOOR_BYTES / PEAK * 1e3:.4f} ms", flush=True)
print(f"# {'table':9s} {'K':>9s} {'plan (resident, stride, global steps)':>38s}  {'variant':16s} {'min ms':>9s} {'median ms':>9s} "
      f"{'G needles/s':>11s} {'of floor':>8s}", flush=True)
rng = np.random.default_rng(1)
needles = ek.Float32(rng.random(n, dtype=np.float32))
for K in (1 << 10, 1 << 16, 1 << 20, 1 << 24):
    for tname, host in tables(K, rng):
        T, last = ek.Float32(host), ek.UInt32(np.array([K - 1], np.uint32))
        loop = lambda: ek.binary_search(0, K, lambda i: ek.gather(T, ek.min(i, last)) < needles)
        one = lambda: ek.search_sorted(T, needles)
        a, b = loop().numpy(), one().numpy()
        if not np.array_equal(a, b):
            sys.exit(f"FAILED: K = {K} ({tname}): {int((a != b).sum())} of {n} results differ")
        del a, b
        l0 = ek.hip_launch_count(); loop(); la = ek.hip_launch_count() - l0
        plan = capi.search_sorted_plan(np.float32, K)
        rows = (("(a) loop", loop, 5, la), ("(b) search_sorted", one, 20, 1))
        res = {}
        for vname, fn, reps, launches in rows:
            lo, med = timed(fn, reps)
            res[vname] = lo
            print(f"  {tname:9s} {K:9d} {str(plan):>38s}  {vname:16s} {lo:9.4f} {med:9.4f} {n / lo / 1e6:11.2f} "
                  f"{n * FLOOR_BYTES / PEAK * 1e3 / lo:8.3f}   ({launches} launches, {reps} timed calls)", flush=True)
        print(f"  {tname:9s} {K:9d} (a) / (b) = {res['(a) loop'] / res['(b) search_sorted']:.1f}", flush=True)
