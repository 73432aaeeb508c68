"""segment_search_sorted next to the loop spelling it replaces and, at uniform lengths, next to block_search_sorted on the same
buffers, in one process.  GPU box:

    python tools/probe_segment_search_sorted.py [n_log2 [seconds]] > profiles/probe_segment_search_sorted_rNN.txt

Per shape over about n = 2^n_log2 (default 26) float32 needles:
    (a) segment_search_sorted(T, table_starts, needles, needle_starts | rows)                csrc/segment_search.hip
    (b) the loop, its row array prebuilt: lo = gather(table_starts, row), len = gather(table_starts shifted by one, row) - lo, then
        binary_search(0, longest, lambda i: (i < len) & (gather(T, min(lo + i, nt - 1)) < needles)) -- log2(longest) + 1 rounds of
        min / add / gather+compare / select / select over n-element arrays.  `longest` is handed to it from the host here; a
        program that has the lengths on the device only would have to read it back first.
    (c) the loop with nothing prebuilt: row = segment_repeat(arange(m), needle_starts, n) first (with `rows` the row array is the
        input itself, so (c) is left out)
    (d) block_search_sorted(T, needles, B)                                                    uniform lengths only
Shapes: uniform 64 x 64 and 1 Ki x 1 Ki (entries x needles per segment); geometric lengths of mean 16 and 256 with as many needles
as entries per segment; "culled rays": n / 64 rays of 64 samples of which 10, 50 and 90 % are kept, a geometric number of new samples
(mean 64) per ray; 64 segments of n / 64 entries; one segment of n / 2 entries among n / 2 single entries, as many needles as
entries; 2048 segments of mean 4096 entries with a row per needle drawn from the marginal.  Every segment is a running sum of
positive weights formed in float64 on the host and rounded once (rounding is monotone, so every segment IS sorted), every needle a
random fraction of its segment's total.  Before anything is timed (a) is compared with (b) and (c), element by element.  Then one
warm-up call and `reps` calls each, every call between its own pair of HIP events on the library stream; a line gives the minimum,
the median and the maximum and the minimum's share of the floor -- the table once + 8 B per needle + 8 B per segment (12 B per
needle with rows) at 8 TB/s.  The process ends itself after `seconds` (default 900)."""
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
N = 1 << n_log2
PEAK = 8e12
props = torch.cuda.get_device_properties(capi.lib.ek_hip_device())
CU = props.multi_processor_count


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
    return min(ms), statistics.median(ms), max(ms)


def shapes(rng):
    """(label, entries per segment, needles per segment or None for a row per needle, uniform B or 0)"""
    for B in (64, 1024):
        yield f"uniform {B} x {B}", np.full(N // B, B, np.int64), np.full(N // B, B, np.int64), B
    for mean in (16, 256):
        lengths = rng.geometric(1.0 / mean, N // mean).astype(np.int64)
        yield f"geometric, mean {mean}", lengths, lengths, 0
    rays = N // 64
    for keep in (0.1, 0.5, 0.9):
        yield f"culled rays, {int(keep * 100)} % kept", rng.binomial(64, keep, rays).astype(np.int64), rng.geometric(1.0 / 64, rays).astype(np.int64) - 1, 0
    yield f"64 segments of {N // 64}", np.full(64, N // 64, np.int64), np.full(64, N // 64, np.int64), 0
    half = N // 2
    lengths = np.concatenate([np.ones(half // 2, np.int64), [half], np.ones(half - half // 2, np.int64)])
    yield "one long among singles", lengths, lengths, 0
    yield "2048 of mean 4096, rows", rng.integers(0, 8193, 2048).astype(np.int64), None, 0


def compare(label, what, a, b):
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        sys.exit(f"FAILED: {label}: {what}: {bad.size} of {a.size} results differ, first at {bad[:5]}: (a) {a[bad[:5]]}, other {b[bad[:5]]}")


print(f"# probe_segment_search_sorted on {platform.node()}: {props.name or 'unnamed device'} ({props.gcnArchName}, {CU} CUs, "
      f"{props.total_memory >> 30} GiB); about 2^{n_log2} float32 needles; floor = table bytes + 8 B / needle + 8 B / segment (12 B / needle "
      f"with rows) at 8 TB/s", flush=True)
print(f"# {'shape':26s} {'nt':>10s} {'m':>9s} {'n':>10s} {'longest':>9s}  {'plan (route, tile, tiles/wg, wgs, lds, window)':>46s}  {'variant':34s} "
      f"{'min ms':>9s} {'median ms':>9s} {'max ms':>9s} {'of floor':>8s}", flush=True)
rng = np.random.default_rng(1)
for label, lengths, counts, B in shapes(rng):
    m = lengths.size
    ends = np.cumsum(lengths)
    nt, longest = int(ends[-1]), int(lengths.max())
    hts = (ends - lengths).astype(np.uint32)
    # every segment a running sum of positive weights from its own start, in float64, rounded once
    c = np.cumsum(rng.random(nt, dtype=np.float32) + np.float32(0.01), dtype=np.float64)
    before = np.where(hts > 0, c[np.maximum(hts.astype(np.int64), 1) - 1], 0.0)
    total = np.where(lengths > 0, c[np.maximum(ends, 1) - 1] - before, 0.0)
    host_table = (c - np.repeat(before, lengths)).astype(np.float32)
    del c
    if counts is not None:
        n = int(counts.sum())
        hns = (np.cumsum(counts) - counts).astype(np.uint32)
        hrow = np.repeat(np.arange(m, dtype=np.uint32), counts)
    else:
        n = N
        hrow = np.minimum(np.searchsorted(ends / ends[-1], rng.random(n), side="right"), m - 1).astype(np.uint32)
    host_needles = (rng.random(n) * total[hrow]).astype(np.float32)
    if max(nt, n) >= 1 << 32:
        print(f"# {label}: too large: skipped", flush=True)
        continue
    T, needles, ts = ek.Float32(host_table), ek.Float32(host_needles), ek.UInt32(hts)
    ts_next = ek.UInt32(np.concatenate([hts[1:], [nt]]).astype(np.uint32))
    row = ek.UInt32(hrow)
    ns = ek.UInt32(hns) if counts is not None else None
    last = ek.UInt32(np.array([nt - 1], np.uint32))
    del host_table, host_needles

    def loop(r):
        lo = ek.gather(ts, r)
        ln = ek.gather(ts_next, r) - lo
        return ek.binary_search(0, longest, lambda i: (i < ln) & (ek.gather(T, ek.min(lo + i, last)) < needles))

    prebuilt = lambda: loop(row)
    scratch = lambda: loop(ek.segment_repeat(ek.UInt32.arange(m), ns, n))
    if counts is not None:
        one = lambda: ek.segment_search_sorted(T, ts, needles, needle_starts=ns)
    else:
        one = lambda: ek.segment_search_sorted(T, ts, needles, rows=row)
    got = one().numpy()
    compare(label, "(b) the loop, row array prebuilt", got, prebuilt().numpy())
    l0 = ek.hip_launch_count(); prebuilt(); lb = ek.hip_launch_count() - l0
    variants = [("(a) segment_search_sorted", one, 20, 1), ("(b) loop, row array prebuilt", prebuilt, 5, lb)]
    if counts is not None:
        compare(label, "(c) the loop, nothing prebuilt", got, scratch().numpy())
        l0 = ek.hip_launch_count(); scratch(); lc = ek.hip_launch_count() - l0
        variants.append(("(c) loop, nothing prebuilt", scratch, 5, lc))
    if B:
        blocks = lambda: ek.block_search_sorted(T, needles, B)
        compare(label, "(d) block_search_sorted", got, blocks().numpy())
        variants.append(("(d) block_search_sorted", blocks, 20, 1))
    del got
    print(f"# {label}: (a) equals {', '.join(v[0][:3] for v in variants[1:])} element by element", flush=True)
    plan = capi.search_sorted_segments_plan(np.float32, nt, m, n, counts is None, CU)
    floor = (4 * nt + (8 if counts is not None else 12) * n + 8 * m) / PEAK * 1e3
    res = {}
    for vname, fn, reps, launches in variants:
        lo, med, hi = timed(fn, reps)
        res[vname[:3]] = (lo, med, hi)
        print(f"  {label:26s} {nt:10d} {m:9d} {n:10d} {longest:9d}  {str(plan):>46s}  {vname:34s} {lo:9.4f} {med:9.4f} {hi:9.4f} {floor / lo:8.3f}"
              f"   ({launches} launches, {reps} timed calls)", flush=True)
    line = f"  {label:26s} floor {floor:.4f} ms; (b) / (a) = {res['(b)'][0] / res['(a)'][0]:.2f} (slowest (a) against fastest (b): {res['(b)'][0] / res['(a)'][2]:.2f})"
    if "(c)" in res:
        line += f"   (c) / (a) = {res['(c)'][0] / res['(a)'][0]:.2f}"
    if "(d)" in res:
        line += f"   (a) / (d) = {res['(a)'][0] / res['(d)'][0]:.2f}"
    print(line, flush=True)
    del T, needles, ts, ts_next, row, ns, last
