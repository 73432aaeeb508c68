"""psum_blocks next to the whole-array prefix sum and a device copy, on the same input, in one process.  GPU box:

    python tools/probe_block_psum.py [n_log2 [seconds]] > profiles/probe_block_psum_rNN.txt

Per block size B over n = 2^n_log2 (default 26) float32 entries (the largest whole number of blocks where B does not divide n):
    (a) psum_blocks(x, B)            csrc/block_scan.hip; all four flag combinations at B = 64, 4096 and 1 Mi, inclusive elsewhere
    (p) psum(x)                      the one-pass look-back scan of the whole array (csrc/scan.hip), the yardstick
    (c) memcpy_device(out, x)        the 8 bytes per entry of (a) and (p) without any arithmetic
Before anything is timed every (a) is compared with float64 prefix sums on the host: an output with t terms is held to the
order-independent bound gamma_(t-1) * sum |x_i| + t * 2^-53 * sum |x_i| (the second part is the reference's own rounding); where
(t - 1) u >= 1/2 that bound is void and the largest error is only reported, as a multiple of u * sum |x_i|.  Exclusive results are
compared with the inclusive ones moved by one entry, bit for bit.  Then three warm-up calls and `reps` calls each into a preallocated
output, every call between its own pair of HIP events on the library stream; the line gives the minimum and the median, the
minimum's share of the floor of 8 bytes per entry at 8 TB/s, and the minimum as a multiple of psum's and of the copy's.  The process
ends itself after `seconds` (default 900)."""
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
PEAK, U = 8e12, 2.0 ** -24
BLOCKS = [b for b in (2, 3, 16, 64, 100, 256, 1000, 1024, 1025, 4096, 1 << 16, 1 << 20, 1 << 25, n) if b <= n]
ALL_FLAGS = (64, 4096, 1 << 20)
SZ = ctypes.c_size_t


def device():
    p = torch.cuda.get_device_properties(capi.lib.ek_hip_device())
    return p, f"{p.name or 'unnamed device'} ({p.gcnArchName}, {p.multi_processor_count} CUs, {p.total_memory >> 30} GiB)"


def timed(fn, reps=20, warm=3):
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


def scan_rows(a2, excl, rev):
    if rev:
        a2 = a2[:, ::-1]
    c = np.cumsum(a2, axis=1, dtype=np.float64)
    if excl:
        c = np.concatenate([np.zeros((a2.shape[0], 1)), c[:, :-1]], axis=1)
    return c[:, ::-1] if rev else c


def verify(B, nn, host, mass_in, got, excl, rev):
    m = nn // B
    truth = scan_rows(host[:nn].reshape(m, B), excl, rev)
    mass = scan_rows(mass_in[:nn].reshape(m, B), excl, rev)
    err = np.abs(got.reshape(m, B).astype(np.float64) - truth)
    t = np.arange(B, dtype=np.float64) if excl else np.arange(1, B + 1, dtype=np.float64)
    if rev:
        t = t[::-1]
    k = np.maximum(t - 1, 0)
    valid = k * U < 0.5
    bound = (np.where(valid, k * U / (1 - np.minimum(k * U, 0.5)), 0) + t * 2.0 ** -53) * mass
    if not np.all(err[:, valid] <= bound[:, valid]):
        sys.exit(f"FAILED: B = {B}, exclusive = {excl}, reverse = {rev}: a prefix sum leaves the bound")
    worst = float(np.max(err / np.maximum(U * mass, 1e-300)))
    return worst, int(valid.sum())


props, dev_name = device()
cu = props.multi_processor_count
rng = np.random.default_rng(1)
host = rng.standard_normal(n).astype(np.float32)
mass_in = np.abs(host)
x = capi.Buf.from_numpy(host)
out = capi.Buf(np.float32, n)
p = lambda b: ctypes.c_void_p(b.ptr)
print(f"# probe_block_psum on {platform.node()}: {dev_name}; n = 2^{n_log2} float32 entries", flush=True)
print(f"# {'B':>9s} {'plan (regime, splits, workgroups)':>34s}  {'variant':34s} {'min ms':>9s} {'median ms':>9s} {'of floor':>8s} {'x psum':>7s} {'x copy':>7s}", flush=True)
floor_n = n * 8 / PEAK * 1e3
c_lo, c_med = timed(lambda: capi.check(capi.lib.ek_hip_memcpy_device(p(out), p(x), SZ(n * 4))))
print(f"  {'-':>9s} {'':>34s}  {'(c) memcpy_device':34s} {c_lo:9.4f} {c_med:9.4f} {floor_n / c_lo:8.3f} {'':>7s} {1.0:7.2f}", flush=True)
p_lo, p_med = timed(lambda: capi.check(capi.lib.ek_hip_psum(capi.F32, p(out), p(x), SZ(n))))
print(f"  {'-':>9s} {'':>34s}  {'(p) psum':34s} {p_lo:9.4f} {p_med:9.4f} {floor_n / p_lo:8.3f} {1.0:7.2f} {p_lo / c_lo:7.2f}", flush=True)
for B in BLOCKS:
    m = n // B
    nn = m * B
    plan = capi.psum_blocks_plan(np.float32, nn, B, cu)
    floor = nn * 8 / PEAK * 1e3
    combos = [(False, False), (True, False), (False, True), (True, True)] if B in ALL_FLAGS else [(False, False)]
    kept = {}
    for excl, rev in combos:
        flags = (1 if excl else 0) | (2 if rev else 0)
        call = lambda: capi.check(capi.lib.ek_hip_psum_blocks(capi.F32, p(out), p(x), SZ(nn), SZ(B), flags))
        call()
        got = out.numpy()[:nn]
        worst, held = verify(B, nn, host, mass_in, got, excl, rev)
        kept[excl, rev] = got if B in ALL_FLAGS else None
        lo, med = timed(call)
        vname = f"(a) psum_blocks{' exclusive' if excl else ''}{' reverse' if rev else ''}"
        print(f"  {B:9d} {str(plan):>34s}  {vname:34s} {lo:9.4f} {med:9.4f} {floor / lo:8.3f} {lo / p_lo * n / nn:7.2f} {lo / c_lo * n / nn:7.2f}"
              f"   # worst error {worst:.3g} u sum|x|; {held} of {B} positions under the gamma bound", flush=True)
    if B in ALL_FLAGS:
        for rev in (False, True):
            inc, exc = kept[False, rev].view(np.uint32).reshape(m, B), kept[True, rev].view(np.uint32).reshape(m, B)
            same = (np.array_equal(exc[:, 1:], inc[:, :-1]) and not exc[:, 0].any()) if not rev else \
                   (np.array_equal(exc[:, :-1], inc[:, 1:]) and not exc[:, -1].any())
            if not same:
                sys.exit(f"FAILED: B = {B}, reverse = {rev}: the exclusive result is not the inclusive one moved by one entry")
    del kept
print("# done", flush=True)
