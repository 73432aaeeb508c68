"""psum_segments next to the spelling it replaces, next to psum_blocks at uniform lengths, and next to the whole-array psum and a
device copy of the same input, in one process.  GPU box:

    python tools/probe_segment_psum.py [n_log2 [seconds]] > profiles/probe_segment_psum_rNN.txt

Per shape over about n = 2^n_log2 (default 26) float32 entries in m ragged segments:
    (a) psum_segments(x, starts)                        csrc/segment_scan.hip
    (b) P - repeat_segments(gather(P - x, starts), starts, n) with P = psum(x): the old spelling, five kernels, nothing prebuilt
        but the starts clipped to n - 1 for the gather (segments that are empty at n)
    (c) psum_blocks(x, B)                               uniform lengths only
    (d) psum(x)                                         the whole-array look-back scan
    (e) a device copy                                   the 8 B / entry floor
Shapes: uniform lengths 16 / 64 / 1024 / 64 Ki; geometric lengths of mean 16 and 256; "culled rays": n / 64 rays of 64 samples of
which 10, 50 and 90 % are kept; one segment of n / 2 entries among n / 2 single entries.  At uniform 64 all four flag modes.
Before anything is timed (a) is compared, in all four modes, with float64 prefix sums per segment on the host under the bound
gamma_min(k, CHAIN) * sum |x_i| over the k + 1 terms of a prefix -- any order of k additions, and no output of this kernel has more
than CHAIN additions in a row behind it (16 in a lane's run, 6 shuffle steps, 4 wave totals, the tiles of a workgroup, and the same
again for the totals and carries of the earlier launches) -- and exclusive against inclusive bit for bit; (b) is only reported (its
error is relative to the running sum of the whole array, not to the segment's).  Then one warm-up call and `reps` calls each, every
call between its own pair of HIP events on the library stream; the line gives the minimum and the median and the minimum's share of
the floor of 8 n + 4 m bytes at 8 TB/s.  The process ends itself after `seconds` (default 900)."""
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
N = 1 << n_log2
PEAK, U = 8e12, 2.0 ** -24
MODES = [(False, False), (True, False), (False, True), (True, True)]


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
    for keep in (0.1, 0.5, 0.9):
        yield f"culled rays, {int(keep * 100)} % kept", rng.binomial(64, keep, rays).astype(np.int64), 0
    half = N // 2
    yield "one long among singles", np.concatenate([np.ones(half // 2, np.int64), [half], np.ones(half - half // 2, np.int64)]), 0


def host_prefix(v, lengths, hstarts, excl, rev):
    """float64 prefix sums per segment of consecutive segments that cover v (vectorised: a running sum minus its value at the start)"""
    if rev:
        return host_prefix(v[::-1], lengths[::-1], None, excl, False)[::-1]
    c = np.cumsum(v)
    ne = lengths > 0
    starts = np.cumsum(lengths) - lengths
    before = np.where(starts[ne] > 0, c[np.maximum(starts[ne], 1) - 1], 0.0)
    out = c - np.repeat(before, lengths[ne])
    return out - v if excl else out


def check(label, host, lengths, hstarts, x, starts):
    n = host.size
    pos = np.arange(n) - np.repeat((np.cumsum(lengths) - lengths), lengths)                  # position inside the segment
    left = np.repeat(lengths, lengths) - 1 - pos
    h64, a64 = host.astype(np.float64), np.abs(host.astype(np.float64))
    chain = 2 * (16 + 6 + 4) + capi.psum_segments_plan(np.float32, n, lengths.size, cu)[1] + (65536 * 4 // 1024) + 16
    got = {}
    for excl, rev in MODES:
        got[excl, rev] = g = capi.psum_segments(x, starts, excl, rev).numpy()
        k = np.maximum((left if rev else pos) - (1 if excl else 0), 0).astype(np.float64)
        ku = np.minimum(k, chain) * U
        bound = ku / (1 - ku) * host_prefix(a64, lengths, hstarts, excl, rev) + 1e-9         # (+ the host's own float64 cancellation)
        err = np.abs(g.astype(np.float64) - host_prefix(h64, lengths, hstarts, excl, rev))
        if not np.all(err <= bound):
            sys.exit(f"FAILED: {label}: excl={excl} rev={rev}: a prefix sum leaves the bound ({float((err - bound).max()):.3g})")
    inner = pos > 0
    if not np.array_equal(got[True, False][inner], got[False, False][np.flatnonzero(inner) - 1]) or np.any(got[True, False][~inner] != 0):
        sys.exit(f"FAILED: {label}: exclusive is not inclusive moved by one")
    inner = left > 0
    if not np.array_equal(got[True, True][inner], got[False, True][np.flatnonzero(inner) + 1]) or np.any(got[True, True][~inner] != 0):
        sys.exit(f"FAILED: {label}: reverse exclusive is not reverse inclusive moved by one")
    return got[False, False], chain


props, dev_name = device()
cu = props.multi_processor_count
rng = np.random.default_rng(1)
print(f"# probe_segment_psum on {platform.node()}: {dev_name}; about 2^{n_log2} float32 entries", flush=True)
print(f"# {'shape':28s} {'n':>10s} {'m':>9s} {'plan (tile, tiles/wg, workgroups, launches)':>44s}  {'variant':34s} {'min ms':>9s} {'median ms':>9s} {'of floor':>8s}",
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
    clipped = capi.Buf.from_numpy(np.minimum(hstarts, n - 1))
    incl, chain = check(label, host, lengths, hstarts, x, starts)

    def old():
        P = capi.psum(x)
        return capi.binary("sub", P, capi.repeat_segments(capi.gather(capi.binary("sub", P, x), clipped), starts, n))

    b = old().numpy().astype(np.float64)
    print(f"# {label}: checked in all four modes (chain bound {chain}); the old spelling is at most "
          f"{float(np.abs(b - incl.astype(np.float64)).max()):.3g} away from (a)", flush=True)
    copy_to = capi.Buf(np.float32, n)
    plan = capi.psum_segments_plan(np.float32, n, m, cu)
    floor = (8 * n + 4 * m) / PEAK * 1e3
    variants = [("(a) psum_segments", lambda: capi.psum_segments(x, starts), 20), ("(b) psum - repeat(gather(psum))", old, 5)]
    if B:
        variants.append(("(c) psum_blocks", lambda: capi.psum_blocks(x, B), 20))
    variants += [("(d) psum", lambda: capi.psum(x), 10),
                 ("(e) device copy", lambda: capi.check(capi.lib.ek_hip_memcpy_device(ctypes.c_void_p(copy_to.ptr), ctypes.c_void_p(x.ptr),
                                                                                      ctypes.c_size_t(4 * n))), 20)]
    if B == 64:
        variants += [(f"(a) excl={int(e)} rev={int(r)}", (lambda e=e, r=r: capi.psum_segments(x, starts, e, r)), 20) for e, r in MODES[1:]]
    res = {}
    for vname, fn, reps in variants:
        lo, med = timed(fn, reps)
        res.setdefault(vname[:3], lo)
        print(f"  {label:28s} {n:10d} {m:9d} {str(plan):>44s}  {vname:34s} {lo:9.4f} {med:9.4f} {floor / lo:8.3f}", flush=True)
    line = f"  {label:28s} (b) / (a) = {res['(b)'] / res['(a)']:.2f}   (a) / (d) = {res['(a)'] / res['(d)']:.2f}   (a) / (e) = {res['(a)'] / res['(e)']:.2f}"
    if B:
        line += f"   (a) / (c) = {res['(a)'] / res['(c)']:.2f}"
    print(line, flush=True)
    del x, starts, clipped, copy_to
