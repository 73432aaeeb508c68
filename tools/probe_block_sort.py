"""sort_blocks next to torch.sort on the same buffer, in one process.  GPU box:

    python tools/probe_block_sort.py [n_log2 [seconds]] > profiles/probe_block_sort_rNN.txt

Per row length B over n = 2^n_log2 (default 26) float32 entries (the largest whole number of rows where B does not divide n):
    (v) sort_blocks(x, B), values only                    csrc/block_sort.hip
    (b) sort_blocks(x, B), values and the flat index
    (t) torch.sort(x.view(R, B), dim=1, stable=True)      the yardstick, outside the code under test: the SAME device buffer,
                                                          zero-copy (a torch tensor owns it, the library sorts it through its pointer)
    (c) memcpy_device(out, x)                             the 8 bytes per entry of (v) without any work
Before anything is timed, the values and the flat index of (b) and the values of (v) are compared with numpy.argsort(kind="stable")
per row on the host, exactly (values as bit patterns).  The input has ties (a quarter of the entries are drawn from 1000 values),
zeros of both signs and NaNs of both signs.  Then warm-up calls and `reps` calls each into preallocated outputs, every call between
its own pair of events (HIP events on the library stream for (v), (b), (c); torch events on torch's stream for (t)); the line gives
the minimum and the median, the minimum's share of the floor of 8 (12 with the index) bytes per entry at 8 TB/s, and the minimum as a
multiple of torch.sort's.  The process ends itself after `seconds` (default 900)."""
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

n_log2 = int(sys.argv[1]) if len(sys.argv) > 1 else 26
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 900)
capi.init(); st = capi.stream()
n = 1 << n_log2
PEAK = 8e12
SZ = ctypes.c_size_t
chunk = capi.sort_blocks_plan(np.float32, 4, 2)[2]
BLOCKS = sorted({b for b in (2, 16, 64, 128, 192, 1024, 1025, 2048, 2049, chunk, chunk + 1, 1 << 16, 1 << 20, n) if b <= n})


def device():
    p = torch.cuda.get_device_properties(capi.lib.ek_hip_device())
    return p, f"{p.name or 'unnamed device'} ({p.gcnArchName}, {p.multi_processor_count} CUs, {p.total_memory >> 30} GiB)"


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


props, dev_name = device()
cu = props.multi_processor_count
rng = np.random.default_rng(1)
host = rng.standard_normal(n).astype(np.float32)
ties = rng.random(n) < 0.25
host[ties] = (rng.integers(-500, 500, int(ties.sum())) / 64).astype(np.float32)
host[rng.integers(0, n, n >> 10)] = -0.0
host[rng.integers(0, n, n >> 12)] = np.nan
host[rng.integers(0, n, n >> 12)] = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
xt = torch.from_numpy(host).cuda()                       # torch owns the buffer ...
torch.cuda.synchronize()
x = capi.Buf(np.float32, n, own=False, ptr=xt.data_ptr())     # ... and the library reads the same bytes
outv, outi = capi.Buf(np.float32, n), capi.Buf(np.uint32, n)
p = lambda b: ctypes.c_void_p(b.ptr)
print(f"# probe_block_sort on {platform.node()}: {dev_name}; n = 2^{n_log2} float32 entries; chunk = {chunk}", flush=True)
print(f"# {'B':>9s} {'plan (route, tile_rows, chunk, passes, wgs)':>44s}  {'variant':28s} {'min ms':>9s} {'median ms':>9s} {'of floor':>8s} {'x torch':>8s}", flush=True)
c_lo, c_med = timed(lambda: capi.check(capi.lib.ek_hip_memcpy_device(p(outv), p(x), SZ(n * 4))), 20)
print(f"  {'-':>9s} {'':>44s}  {'(c) memcpy_device':28s} {c_lo:9.4f} {c_med:9.4f} {n * 8 / PEAK * 1e3 / c_lo:8.3f}", flush=True)
for B in BLOCKS:
    m = n // B
    nn = m * B
    plan = capi.sort_blocks_plan(np.float32, nn, B, True, cu)
    both = lambda: capi.check(capi.lib.ek_hip_sort_blocks(capi.F32, p(outv), p(outi), p(x), SZ(nn), SZ(B), capi.SORT_FLAT_INDEX))
    vals = lambda: capi.check(capi.lib.ek_hip_sort_blocks(capi.F32, p(outv), None, p(x), SZ(nn), SZ(B), 0))
    x2 = host[:nn].reshape(m, B)
    want = np.argsort(x2, axis=1, kind="stable")
    want_v = np.take_along_axis(x2, want, axis=1).reshape(-1).view(np.uint32)
    want += np.arange(m, dtype=want.dtype)[:, None] * B
    both()
    if not np.array_equal(outi.numpy()[:nn], want.reshape(-1)):
        sys.exit(f"FAILED: B = {B}: the flat index is not numpy's stable argsort")
    if not np.array_equal(outv.numpy()[:nn].view(np.uint32), want_v):
        sys.exit(f"FAILED: B = {B}: the values of the two-output call are not the entries in that order")
    capi.check(capi.lib.ek_hip_memset(p(outv), 0, SZ(nn * 4)))
    vals()
    if not np.array_equal(outv.numpy()[:nn].view(np.uint32), want_v):
        sys.exit(f"FAILED: B = {B}: the values of the values-only call are not the entries in that order")
    del want, want_v
    view = xt[:nn].view(m, B)
    # one call first to size the repetitions: about two seconds per variant at the most
    e0, e1 = hiprt.Event(), hiprt.Event()
    e0.record(st); both(); e1.record(st); e1.synchronize()
    reps = int(max(3, min(20, 2000 / max(e0.elapsed_ms(e1), 0.01))))
    t_lo, t_med = timed_torch(lambda: torch.sort(view, dim=1, stable=True), reps)
    print(f"  {B:9d} {str(plan):>44s}  {'(t) torch.sort stable':28s} {t_lo:9.4f} {t_med:9.4f} {nn * 16 / PEAK * 1e3 / t_lo:8.3f} {1.0:8.2f}", flush=True)
    torch.cuda.synchronize()
    for vname, fn, bytes_per in (("(v) sort_blocks values", vals, 8), ("(b) sort_blocks values+flat", both, 12)):
        lo, med = timed(fn, reps)
        print(f"  {B:9d} {str(plan):>44s}  {vname:28s} {lo:9.4f} {med:9.4f} {nn * bytes_per / PEAK * 1e3 / lo:8.3f} {lo / t_lo:8.2f}", flush=True)
print("# done", flush=True)
