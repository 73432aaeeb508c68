"""sort_segments next to what it replaces and, at uniform lengths, next to sort_blocks, on the same input, in one process.  GPU box:

    python tools/probe_segment_sort.py [n_log2 [seconds]] > profiles/probe_segment_sort_rNN.txt

Per shape over about n = 2^n_log2 (default 26) float32 entries WITH TIES (integers 0 .. 1023) in m ragged segments, values and flat
permutation asked for:
    (new) sort_segments(x, starts, flat)               csrc/segment_sort.hip
    (a)   sort_blocks(x, B, flat)                      uniform lengths only
    (b)   two stable torch.sort calls -- by key, then by a segment-id array that is built OUTSIDE the timed region -- and the three
          gathers between and behind them (seg_id[p1], p1[p2], x[perm]): the spelling that leaves the library
Shapes: uniform 8 / 64 / 100 / 1024 / 64 Ki; geometric lengths of mean 64; one segment of n / 2 entries among n / 2 single entries.
Before anything is timed the flat permutation of (new) is compared exactly with (b)'s and, for uniform shapes, with (a)'s, and the
values with a gather through it.  Then one warm-up call and `reps` calls each, every call between its own pair of events on the
stream it runs on (the library's for (new) and (a), torch's for (b)); the line gives the minimum and the median.  One more call of
(new) runs under the library's launch profiler: the time of the tile launch alone, of the pass count and of all merge launches, so
that a shape whose merges all return at once shows the price of the launches it does not need.  A row is marked ** where (new) is
slower than (b) or more than twice (a).  The process ends itself after `seconds` (default 900)."""
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


def timed_torch(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), statistics.median(ms)


def shapes(rng):
    """(label, lengths, uniform B or 0)"""
    for B in (8, 64, 100, 1024, 1 << 16):
        if B <= N // 2:
            yield f"uniform {B}", np.full(N // B, B, np.int64), B
    yield "geometric, mean 64", rng.geometric(1.0 / 64, N // 64).astype(np.int64), 0
    half = N // 2
    yield "one long among singles", np.concatenate([np.ones(half // 2, np.int64), [half], np.ones(half - half // 2, np.int64)]), 0


props, dev_name = device()
cu = props.multi_processor_count
rng = np.random.default_rng(1)
print(f"# probe_segment_sort on {platform.node()}: {dev_name}; about 2^{n_log2} float32 entries with ties, values and flat permutation", flush=True)
print(f"# plan: (tile, tiles, tiles_per_workgroup, workgroups, merges, merge_workgroups, launches, scratch_bytes)", flush=True)
print(f"# {'shape':24s} {'n':>10s} {'m':>9s}  {'variant':34s} {'min ms':>9s} {'median ms':>9s}", flush=True)
for label, lengths, B in shapes(rng):
    m = lengths.size
    ends = np.cumsum(lengths)
    n = int(ends[-1])
    if n == 0 or n >= 1 << 32:
        print(f"# {label}: n = {n}: skipped", flush=True)
        continue
    hstarts = (ends - lengths).astype(np.uint32)
    host = rng.integers(0, 1024, n).astype(np.float32)
    x, starts = capi.Buf.from_numpy(host), capi.Buf.from_numpy(hstarts)
    tx = torch.from_numpy(host).cuda()
    tseg = torch.from_numpy(np.repeat(np.arange(m, dtype=np.int32), lengths)).cuda()
    ov, oi = capi.Buf(np.float32, n), capi.Buf(np.uint32, n)

    new = lambda: capi.sort_segments(x, starts, False, True, True, True, ov, oi)
    blocks = lambda: capi.sort_blocks(x, B, False, True, True, True, ov, oi)

    def old():
        _, p1 = torch.sort(tx, stable=True)
        _, p2 = torch.sort(tseg[p1], stable=True)
        perm = p1[p2]
        return tx[perm], perm

    # ---- correctness first
    new()
    got_v, got_i = ov.numpy(), oi.numpy()
    want_v, want_i = old()
    want_i = want_i.cpu().numpy().astype(np.uint32)
    if not np.array_equal(got_i, want_i):
        sys.exit(f"FAILED: {label}: the permutation differs from two stable sorts at {np.flatnonzero(got_i != want_i)[:4]}")
    if not np.array_equal(got_v.view(np.uint32), host[want_i].view(np.uint32)) or not np.array_equal(got_v, want_v.cpu().numpy()):
        sys.exit(f"FAILED: {label}: the values are not the gather through the permutation")
    del want_v
    if B:
        blocks()
        if not np.array_equal(oi.numpy(), want_i) or not np.array_equal(ov.numpy().view(np.uint32), got_v.view(np.uint32)):
            sys.exit(f"FAILED: {label}: sort_blocks differs")
    plan = capi.sort_segments_plan(np.float32, n, m, True, cu)
    print(f"# {label}: correct; plan {plan}", flush=True)
    # ---- times
    res = {}
    res["new"] = timed(new, 10)
    if B:
        res["a"] = timed(blocks, 10)
    torch.cuda.synchronize()
    res["b"] = timed_torch(old, 3)
    slow = res["new"][0] > res["b"][0] or (B and res["new"][0] > 2 * res["a"][0])
    mark = "**" if slow else "  "
    print(f"{mark}{label:24s} {n:10d} {m:9d}  {'(new) sort_segments':34s} {res['new'][0]:9.4f} {res['new'][1]:9.4f}", flush=True)
    if B:
        print(f"  {label:24s} {n:10d} {m:9d}  {'(a) sort_blocks':34s} {res['a'][0]:9.4f} {res['a'][1]:9.4f}", flush=True)
    print(f"  {label:24s} {n:10d} {m:9d}  {'(b) 2 x torch.sort + 3 gathers':34s} {res['b'][0]:9.4f} {res['b'][1]:9.4f}", flush=True)
    line = f"  {label:24s} (b) / (new) = {res['b'][0] / res['new'][0]:.2f}"
    if B:
        line += f"   (new) / (a) = {res['new'][0] / res['a'][0]:.2f}"
    # ---- one call under the launch profiler: the tile launch alone against the whole call
    capi.profile_begin()
    new()
    prof = {p["kernel"]: (p["launches"], p["total_ms"]) for p in capi.profile_end()}
    parts = ", ".join(f"{k} x{v[0]} {v[1]:.4f} ms" for k, v in prof.items())
    print(line + f"   profiled call: {parts}", flush=True)
    del x, starts, tx, tseg, ov, oi
    torch.cuda.empty_cache()
