"""reduce_segments / repeat_segments next to the spellings they replace and, at uniform lengths, next to reduce_blocks / repeat, on
the same input, in one process.  GPU box:

    python tools/probe_segment_sum.py [n_log2 [seconds]] > profiles/probe_segment_sum_rNN.txt

Per shape over about n = 2^n_log2 (default 26) float32 entries in m ragged segments:
    (a) reduce_segments(hsum, x, starts)               csrc/block_segments.hip
    (b) scatter_add(zero(m), x, seg_id)                the old spelling; seg_id = search_sorted(starts, arange(n), right) - 1 is
                                                       built OUTSIDE the timed region (which favours it: it costs three more
                                                       kernels), the zero fill of the target is inside (it is part of the call)
    (c) repeat_segments(v, starts, n)                  v = the m segment sums
    (d) gather(v, seg_id)                              the old spelling, index prebuilt
    (e), (f) reduce_blocks(hsum, x, B), repeat(v, B)   uniform lengths only
Shapes: uniform lengths 16 / 64 / 1024 / 64 Ki; geometric lengths of mean 16 and 256; "culled rays": n / 64 rays of 64 samples of
which 0, 10, 50, 90 and 100 % are kept; one segment of n / 2 entries among n / 2 single entries.
Before anything is timed (a) and (b) are both compared with a float64 sum per segment on the host under the order-independent bound
gamma_(L-1) * sum |x_i| (where (L - 1) u >= 1/2 that bound is void and gamma_CHAIN stands in for (a), CHAIN being the longest chain
of additions behind an output; (b) is then only reported) and (c) with (d) exactly.  Then one warm-up call and `reps` calls each, every call
between its own pair of HIP events on the library stream; the line gives the minimum and the median and the minimum's share of the
floor of 4 (n + m) + 4 m bytes at 8 TB/s.  The process ends itself after `seconds` (default 900)."""
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
N = 1 << n_log2
PEAK, U = 8e12, 2.0 ** -24
# the longest chain of additions behind an output: a workgroup that streams a segment of L entries adds them in 1024 accumulators
# (256 lanes x 4), L / 1024 in a row each, then folds; the grouped route adds at most 2048 staged entries per lane and 6 shuffle
# steps on top for the segment's last chunk
CHAIN = N // 1024 + 2048 + 6 + 16


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


def shapes(rng):
    """(label, lengths, uniform B or 0)"""
    for B in (16, 64, 1024, 1 << 16):
        if B <= N // 2:
            yield f"uniform {B}", np.full(N // B, B, np.int64), B
    for mean in (16, 256):
        yield f"geometric, mean {mean}", rng.geometric(1.0 / mean, N // mean).astype(np.int64), 0
    rays = N // 64
    for keep in (0.0, 0.1, 0.5, 0.9, 1.0):
        yield f"culled rays, {int(keep * 100)} % kept", rng.binomial(64, keep, rays).astype(np.int64), 0
    half = N // 2
    yield "one long among singles", np.concatenate([np.ones(half // 2, np.int64), [half], np.ones(half - half // 2, np.int64)]), 0


props, dev_name = device()
cu = props.multi_processor_count
rng = np.random.default_rng(1)
print(f"# probe_segment_sum on {platform.node()}: {dev_name}; about 2^{n_log2} float32 entries", flush=True)
print(f"# {'shape':28s} {'n':>10s} {'m':>9s} {'plan (route, lanes, splits, workgroups)':>40s}  {'variant':30s} {'min ms':>9s} {'median ms':>9s} {'of floor':>8s}",
      flush=True)
for label, lengths, B in shapes(rng):
    m = lengths.size
    ends = np.cumsum(lengths)
    n = int(ends[-1])
    if n == 0 or n >= 1 << 32:
        print(f"# {label}: n = {n}: skipped", flush=True)
        continue
    hstarts = (ends - lengths).astype(np.uint32)
    host = rng.standard_normal(n).astype(np.float32)
    x, starts = capi.Buf.from_numpy(host), capi.Buf.from_numpy(hstarts)
    seg_id = capi.Buf.from_numpy(np.repeat(np.arange(m, dtype=np.uint32), lengths))

    def old_sum():
        target = capi.fill(np.float32, 0.0, m)
        capi.scatter_add(target, x, seg_id)
        return target

    new_sum = lambda: capi.reduce_segments("hsum", x, starts)
    a, b = new_sum().numpy().astype(np.float64), old_sum().numpy().astype(np.float64)
    ne = np.flatnonzero(lengths > 0)
    truth, mass = np.zeros(m), np.zeros(m)
    truth[ne] = np.add.reduceat(host.astype(np.float64), hstarts[ne].astype(np.int64))
    mass[ne] = np.add.reduceat(np.abs(host.astype(np.float64)), hstarts[ne].astype(np.int64))
    k = np.maximum(lengths - 1, 0).astype(np.float64)
    void = k * U >= 0.5
    ku = np.where(void, CHAIN * U, k * U)
    bound = ku / (1 - ku) * mass
    if not np.all(np.abs(a - truth) <= bound):
        sys.exit(f"FAILED: {label}: a segment sum leaves the bound")
    if not np.all((np.abs(b - truth) <= bound) | void):
        sys.exit(f"FAILED: {label}: a scatter_add sum leaves the bound")
    if void.any():
        print(f"# {label}: {int(void.sum())} segment(s) with (L - 1) u >= 1/2: (a) within gamma_{CHAIN} sum|x|; (b) is "
              f"{float((np.abs(b - truth)[void] / bound[void]).max()):.3g} of that bound away", flush=True)
    v = new_sum()
    new_rep = lambda: capi.repeat_segments(v, starts, n)
    old_rep = lambda: capi.gather(v, seg_id)
    if not np.array_equal(new_rep().numpy(), old_rep().numpy()):
        sys.exit(f"FAILED: {label}: repeat_segments and gather differ")
    plan = capi.reduce_segments_plan(np.float32, n, m, cu)
    floor = (4 * (n + m) + 4 * m) / PEAK * 1e3
    variants = [("(a) reduce_segments(hsum)", new_sum, 20), ("(b) scatter_add, seg_id", old_sum, 5),
                ("(c) repeat_segments", new_rep, 20), ("(d) gather, seg_id", old_rep, 5)]
    if B:
        vb = capi.reduce_blocks("hsum", x, B)
        if not np.all(np.abs(vb.numpy().astype(np.float64) - truth) <= bound):
            sys.exit(f"FAILED: {label}: a block sum leaves the bound")
        variants += [("(e) reduce_blocks(hsum)", lambda: capi.reduce_blocks("hsum", x, B), 20), ("(f) repeat", lambda: capi.repeat(vb, B), 20)]
    res = {}
    for vname, fn, reps in variants:
        lo, med = timed(fn, reps)
        res[vname[:3]] = lo
        print(f"  {label:28s} {n:10d} {m:9d} {str(plan):>40s}  {vname:30s} {lo:9.4f} {med:9.4f} {floor / lo:8.3f}", flush=True)
    line = f"  {label:28s} (b) / (a) = {res['(b)'] / res['(a)']:.2f}   (d) / (c) = {res['(d)'] / res['(c)']:.2f}"
    if B:
        line += f"   (a) / (e) = {res['(a)'] / res['(e)']:.2f}   (c) / (f) = {res['(c)'] / res['(f)']:.2f}"
    print(line, flush=True)
    del x, starts, seg_id, v
