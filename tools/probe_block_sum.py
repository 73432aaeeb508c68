"""reduce_blocks / repeat next to the spellings they replace and next to hsum, on the same input, in one process.  GPU box:

    python tools/probe_block_sum.py [n_log2 [seconds]] > profiles/probe_block_sum_rNN.txt

Per block size B over n = 2^n_log2 (default 26) float32 entries:
    (a) reduce_blocks(hsum, x, B)                      csrc/block_reduce.hip
    (b) scatter_add(zero(n / B), x, arange(n) // B)    the old spelling; the index array is built OUTSIDE the timed region (which
                                                       favours it), the zero fill of the target is inside (it is part of the call)
    (c) repeat(v, B)                                   v = the n / B block sums
    (d) gather(v, arange(n) // B)                      the old spelling, index prebuilt
    (e) hsum(x)                                        the one-pass yardstick
Before anything is timed (a) and (b) are both compared with a float64 sum on the host under the order-independent bound
gamma_(B-1) * sum |x_i| (where (B - 1) u >= 1/2 that bound is void: see below) and (c) with (d) exactly.  Then
one warm-up call and `reps` calls each, every call between its own pair of HIP events on the library stream; the line gives the
minimum and the median, the minimum's share of the floor of 4 (1 + 1 / B) bytes per entry at 8 TB/s, and the minimum as a multiple
of hsum's.  The process ends itself after `seconds` (default 900)."""
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
PEAK, U, CHAIN = 8e12, 2.0 ** -24, 4096
BLOCKS = [b for b in (2, 3, 4, 16, 64, 100, 256, 1000, 4096, 1 << 16, 1 << 20, 1 << 25) if b <= n // 2]


def device():
    p = torch.cuda.get_device_properties(capi.lib.ek_hip_device())
    return p, f"{p.name or 'unnamed device'} ({p.gcnArchName}, {p.multi_processor_count} CUs, {p.total_memory >> 30} GiB)"


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


props, dev_name = device()
cu = props.multi_processor_count
rng = np.random.default_rng(1)
host = rng.standard_normal(n).astype(np.float32)
x = capi.Buf.from_numpy(host)
print(f"# probe_block_sum on {platform.node()}: {dev_name}; n = 2^{n_log2} float32 entries", flush=True)
print(f"# {'B':>9s} {'plan (regime, splits, workgroups)':>34s}  {'variant':28s} {'min ms':>9s} {'median ms':>9s} {'of floor':>8s} {'x hsum':>7s}", flush=True)
h_lo, h_med = timed(lambda: capi.reduce("hsum", x), 20)
print(f"  {'-':>9s} {'':>34s}  {'(e) hsum':28s} {h_lo:9.4f} {h_med:9.4f} {n * 4 / PEAK * 1e3 / h_lo:8.3f} {1.0:7.2f}", flush=True)
for B in BLOCKS:
    m = n // B
    nn = m * B                                        # (B = 3, 100, 1000: the largest whole number of blocks)
    xs = x.view(0, nn)
    index = capi.Buf.from_numpy((np.arange(nn, dtype=np.uint64) // B).astype(np.uint32))

    def old_sum():
        target = capi.fill(np.float32, 0.0, m)
        capi.scatter_add(target, xs, index)
        return target

    new_sum = lambda: capi.reduce_blocks("hsum", xs, B)
    a, b = new_sum().numpy().astype(np.float64), old_sum().numpy().astype(np.float64)
    h2 = host[:nn].reshape(m, B)
    truth, mass = h2.sum(axis=1, dtype=np.float64), np.abs(h2).sum(axis=1, dtype=np.float64)
    k = B - 1
    if k * U < 0.5:
        bound = k * U / (1 - k * U) * mass
        if not (np.all(np.abs(a - truth) <= bound) and np.all(np.abs(b - truth) <= bound)):
            sys.exit(f"FAILED: B = {B}: a block sum leaves the bound")
    else:
        # (B - 1) u >= 1/2: the order-independent bound is void.  No chain of additions behind an output of block_reduce.hip is
        # longer than 4096 (a lane adds piece / 4096 + 8 entries in sequence, a piece has at most n / 1024 entries; then trees):
        # (a) is held to gamma_4096; the old spelling adds a bin's entries in an order of its own and is only reported
        bound = CHAIN * U / (1 - CHAIN * U) * mass
        if not np.all(np.abs(a - truth) <= bound):
            sys.exit(f"FAILED: B = {B}: a block sum leaves the bound")
        print(f"# B = {B}: (B - 1) u >= 1/2, (a) within gamma_{CHAIN} sum|x|; (b) is {float((np.abs(b - truth) / bound).max()):.3g} of that bound away", flush=True)
    v = new_sum()
    new_rep = lambda: capi.repeat(v, B)
    old_rep = lambda: capi.gather(v, index)
    if not np.array_equal(new_rep().numpy(), old_rep().numpy()):
        sys.exit(f"FAILED: B = {B}: repeat and gather differ")
    plan = capi.reduce_blocks_plan(np.float32, nn, B, cu)
    floor = nn * 4 * (1 + 1 / B) / PEAK * 1e3
    res = {}
    for vname, fn, reps in (("(a) reduce_blocks(hsum)", new_sum, 20), ("(b) scatter_add, arange // B", old_sum, 5),
                            ("(c) repeat", new_rep, 20), ("(d) gather, arange // B", old_rep, 5)):
        lo, med = timed(fn, reps)
        res[vname[:3]] = lo
        print(f"  {B:9d} {str(plan):>34s}  {vname:28s} {lo:9.4f} {med:9.4f} {floor / lo:8.3f} {lo / h_lo:7.2f}", flush=True)
    print(f"  {B:9d} (b) / (a) = {res['(b)'] / res['(a)']:.1f}   (d) / (c) = {res['(d)'] / res['(c)']:.1f}", flush=True)
    del index, v
