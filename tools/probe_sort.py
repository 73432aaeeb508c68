"""ek_hip_sort on its radix route next to its forwarded route (block_sort of one row) and to torch.sort, in one process.  GPU box:

    python tools/probe_sort.py [seconds] > profiles/probe_sort_rNN.txt

Per element class (float32 for 4-byte types, float64 for 8-byte types) and per n = 4 Ki, 16 Ki, .. 64 Mi, values plus index:
    (r) ek_hip_sort, tuning "sort_radix" = 2          csrc/sort.hip: 4 or 8 radix passes
    (f) ek_hip_sort, tuning "sort_radix" = 0          forwarded to ek_hip_sort_blocks(x, block = n): the route before this file
    (t) torch.sort(x, stable=True)                    the yardstick, outside the code under test: the SAME device buffer, zero-copy
                                                      (a torch tensor owns it, the library sorts it through its pointer)
and uint32 at 64 Mi (ray ids below 2^20: the upper passes see one digit).  Before anything is timed, the values and the permutation
of (r) are compared with numpy.argsort(kind="stable") on the host, exactly (values as bit patterns).  The input has ties (a quarter of
the entries are drawn from 1000 values), zeros of both signs and NaNs of both signs.  Then warm-up calls and 20 calls each into
preallocated outputs, every call between its own pair of events (HIP events on the library stream for (r) and (f); torch events on
torch's stream for (t)); the line gives the minimum and the median.  The crossover of a class is the smallest measured n from which
(r) is faster than (f) at that and every larger measured n, never below block_sort's chunk + 1: what kRadixAuto4 / kRadixAuto8 of
sort.hip should hold.  The process ends itself after `seconds` (default 900)."""
import ctypes
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

signal.alarm(int(sys.argv[1]) if len(sys.argv) > 1 else 900)
capi.init(); st = capi.stream()
SZ = ctypes.c_size_t
SIZES = [1 << k for k in (12, 14, 16, 18, 20, 22, 24, 26)]
REPS = 20
p = lambda b: ctypes.c_void_p(b.ptr)


def device():
    pr = torch.cuda.get_device_properties(capi.lib.ek_hip_device())
    return pr, f"{pr.name or 'unnamed device'} ({pr.gcnArchName}, {pr.multi_processor_count} CUs, {pr.total_memory >> 30} GiB)"


def timed(fn, reps, warm=2):
    for _ in range(warm):
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


def timed_torch(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), statistics.median(ms)


def host_data(dt, n, rng):
    dt = np.dtype(dt)
    if dt.kind != "f":
        return rng.integers(0, 1 << 20, n).astype(dt)
    host = rng.standard_normal(n).astype(dt)
    ties = rng.random(n) < 0.25
    host[ties] = (rng.integers(-500, 500, int(ties.sum())) / 64).astype(dt)
    host[rng.integers(0, n, max(1, n >> 10))] = -0.0
    host[rng.integers(0, n, max(1, n >> 12))] = np.nan
    host[rng.integers(0, n, max(1, n >> 12))] = -np.nan
    return host


props, dev_name = device()
cu = props.multi_processor_count
print(f"# probe_sort on {platform.node()}: {dev_name}; values + index, min / median of {REPS} calls", flush=True)
print(f"# {'type':>8s} {'n':>9s} {'radix plan (route, passes, tile, tiles/wg, wgs, launches, scratch)':>68s}  {'(r) radix ms':>16s} {'(f) forwarded ms':>16s} "
      f"{'(t) torch.sort ms':>17s} {'r / f':>6s} {'r / t':>6s}", flush=True)
crossover = {}
for dt, sizes in ((np.float32, SIZES), (np.float64, SIZES), (np.uint32, SIZES[-1:])):
    dt = np.dtype(dt)
    rng = np.random.default_rng(1)
    chunk = capi.sort_blocks_plan(dt, 4, 2)[2]
    faster = []
    for n in sizes:
        host = host_data(dt, n, rng)
        xt = torch.from_numpy(host.view(np.int32) if dt == np.uint32 else host).cuda()          # torch owns the buffer ...
        torch.cuda.synchronize()
        x = capi.Buf(dt, n, own=False, ptr=xt.data_ptr())                                       # ... and the library reads the same bytes
        outv, outi = capi.Buf(dt, n), capi.Buf(np.uint32, n)
        call = lambda: capi.check(capi.lib.ek_hip_sort(x.ek, p(outv), p(outi), p(x), SZ(n), 0))
        capi.set_tuning("sort_radix", 2)
        plan = capi.sort_plan(dt, n, True, cu)
        call()
        want = np.argsort(host, kind="stable")
        bit = np.uint32 if dt.itemsize == 4 else np.uint64
        if not np.array_equal(outi.numpy(), want):
            sys.exit(f"FAILED: {dt.name}, n = {n}: the permutation is not numpy's stable argsort")
        if not np.array_equal(outv.numpy().view(bit), host[want].view(bit)):
            sys.exit(f"FAILED: {dt.name}, n = {n}: the values are not the entries in that order")
        del want
        r_lo, r_med = timed(call, REPS)
        capi.set_tuning("sort_radix", 0)
        f_lo, f_med = timed(call, REPS)
        capi.set_tuning("sort_radix", 1)
        view = xt.view(torch.int32) if dt == np.uint32 else xt           # (ids below 2^20: the same order signed or unsigned)
        t_lo, t_med = timed_torch(lambda: torch.sort(view, stable=True), REPS)
        torch.cuda.synchronize()
        print(f"  {dt.name:>8s} {n:9d} {str(plan):>68s}  {r_lo:7.4f} /{r_med:7.4f} {f_lo:7.4f} /{f_med:7.4f} {t_lo:8.4f} /{t_med:7.4f} "
              f"{r_lo / f_lo:6.2f} {r_lo / t_lo:6.2f}", flush=True)
        faster.append((n, r_lo < f_lo))
        del x, outv, outi, xt, view
        torch.cuda.empty_cache()
    if len(sizes) > 1:
        t = None
        for n, won in reversed(faster):
            if not won:
                break
            t = n
        crossover[dt.itemsize] = None if t is None else max(t, chunk + 1)
for size, t in crossover.items():
    print(f"# crossover of the {size}-byte class: " + (f"{t} entries" if t else "none: the forwarded route won at 64 Mi"), flush=True)
print("# done", flush=True)
