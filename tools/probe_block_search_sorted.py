"""block_search_sorted next to the spelling it replaces, on the same inputs, in one process.  GPU box:

    python tools/probe_block_search_sorted.py [n_log2 [seconds]] > profiles/probe_block_search_sorted_rNN.txt

    (a) binary_search(0, B, lambda i: gather(T, row * B + min(i, B - 1)) < needles)   log2(B) + 1 rounds of min / multiply-add /
        gather+compare / select / select, with the index array `row` built beforehand (not timed)
    (b) block_search_sorted(T, needles, B [, rows=row])                               one kernel (csrc/block_search.hip)

n = 2^n_log2 (default 26) float32 needles.  Shapes: R x B tables of per-row CDFs of uniform weights (summed in float64 on the host,
so that every row is sorted) with M = n / R needles per row -- 64 x 64 per ray, 1 Ki x 1 Ki, 64 rows of 1 Mi entries (sampled rows);
indexed needles over 2048 x 4096 conditional CDFs built with block_psum (checked to be sorted first), the rows drawn by
search_sorted from the marginal CDF; and one row of 1 Mi entries against search_sorted itself.  Per shape the two
results are compared (exact equality) BEFORE anything is timed, then one warm-up call and `reps` calls each, every call between its
own pair of HIP events on the library stream; the line gives the minimum and the median, the minimum's share of the floor (the table
once plus 8 B per needle, 12 B with a row per needle, at 8 TB/s) and (a) / (b).  The process ends itself after `seconds` (default
900)."""
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
PEAK = 8e12
CU = torch.cuda.get_device_properties(capi.lib.ek_hip_device()).multi_processor_count


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
    return min(ms), statistics.median(ms), max(ms)


def report(label, R, B, n, indexed, variants, floor_ms):
    plan = capi.search_sorted_blocks_plan(np.float32, R, B, n, indexed, CU)
    res = {}
    for vname, fn, reps, launches in variants:
        lo, med, hi = timed(fn, reps)
        res[vname] = (lo, med, hi)
        print(f"  {label:22s} {R:8d} {B:8d} {n // R if not indexed else 0:8d}  {capi.BLOCK_SEARCH_ROUTES[plan[0]]:14s} {str(plan[1:]):>22s}  "
              f"{vname:24s} {lo:9.4f} {med:9.4f} {hi:9.4f} {floor_ms / lo:8.3f}   ({launches} launches, {reps} timed calls)", flush=True)
    return res


print(f"# probe_block_search_sorted on {platform.node()}: {device_name()}; n = 2^{n_log2} float32 needles; floor = table bytes + 8 B/needle "
      f"(12 B with a row per needle) at 8 TB/s", flush=True)
print(f"# {'shape':22s} {'R':>8s} {'B':>8s} {'M':>8s}  {'route':14s} {'(t, s, res, stride, gs)':>22s}  {'variant':24s} {'min ms':>9s} "
      f"{'median ms':>9s} {'max ms':>9s} {'of floor':>8s}", flush=True)
rng = np.random.default_rng(1)
u = rng.random(n, dtype=np.float32)


def cdf_rows(R, B, pdf=None):
    """per-row running sums of uniform weights, every row ending near 1, summed in float64 on the host and rounded once: rounding
    is monotone, so every row IS sorted (a float32 running sum in a fixed tree order need not be, entry by entry)"""
    pdf = rng.random(R * B, dtype=np.float32) * np.float32(2.0 / B) if pdf is None else pdf
    return np.cumsum(pdf.reshape(R, B), axis=1, dtype=np.float64).astype(np.float32).reshape(-1)


def rows_sorted(host, B):
    return bool(np.all(np.diff(host.reshape(-1, B), axis=1) >= 0))


def loop_for(T, B, row, needles):
    last, width = ek.UInt32(np.array([B - 1], np.uint32)), ek.UInt32(np.array([B], np.uint32))
    return lambda: ek.binary_search(0, B, lambda i: ek.gather(T, row * width + ek.min(i, last)) < needles)


def compare(label, fa, fb):
    a, b = fa().numpy(), fb().numpy()
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        sys.exit(f"FAILED: {label}: {bad.size} of {a.size} results differ, first at {bad[:5]}: (a) {a[bad[:5]]}, (b) {b[bad[:5]]}")


# ---- blocked needles -------------------------------------------------------------------------------------------------------
for label, R, B in (("64 x 64 per ray", n >> 6, 64), ("1 Ki x 1 Ki", n >> 10, 1 << 10), ("64 rows of 1 Mi", 64, 1 << 20)):
    M = n // R
    T = ek.Float32(cdf_rows(R, B))
    needles = ek.Float32(u)
    row = ek.UInt32((np.arange(n, dtype=np.uint32) // np.uint32(M)).astype(np.uint32))
    loop = loop_for(T, B, row, needles)
    one = lambda: ek.block_search_sorted(T, needles, B)
    compare(label, loop, one)
    l0 = ek.hip_launch_count(); loop(); la = ek.hip_launch_count() - l0
    floor_ms = (4 * R * B + 8 * n) / PEAK * 1e3
    res = report(label, R, B, n, False, (("(a) loop", loop, 5, la), ("(b) block_search_sorted", one, 20, 1)), floor_ms)
    print(f"  {label:22s} floor {floor_ms:.4f} ms; (a) / (b) = {res['(a) loop'][0] / res['(b) block_search_sorted'][0]:.1f}", flush=True)
    del T, needles, row, loop, one

# ---- a row per needle: a 2-D distribution, the row from the marginal, the column from the row's conditional CDF --------------
R, B = 2048, 4096
label = "2048 x 4096 indexed"
host_pdf = rng.random(R * B, dtype=np.float32)
pdf = ek.Float32(host_pdf)
T = ek.block_psum(pdf, B)                                        # conditional CDFs, unnormalised: row r ends at its total
if rows_sorted(T.numpy(), B):
    print(f"  {label:22s} the rows block_psum wrote are sorted", flush=True)
else:                                                            # (both spellings need sorted rows to agree)
    print(f"  {label:22s} block_psum wrote rows that are not sorted entry by entry: the CDFs are summed on the host instead", flush=True)
    T = ek.Float32(cdf_rows(R, B, host_pdf))
totals = ek.block_sum(pdf, B)
marginal = ek.psum(totals)
total = float(marginal.numpy()[-1])
row = ek.search_sorted(marginal, ek.Float32(rng.random(n, dtype=np.float32) * np.float32(total)))
needles = ek.Float32(u) * ek.gather(totals, ek.min(row, ek.UInt32(np.array([R - 1], np.uint32))))
needles.numpy()                                                  # evaluated before anything is timed
loop = loop_for(T, B, ek.min(row, ek.UInt32(np.array([R - 1], np.uint32))), needles)
one = lambda: ek.block_search_sorted(T, needles, B, rows=row)
compare(label, loop, one)
l0 = ek.hip_launch_count(); loop(); la = ek.hip_launch_count() - l0
floor_ms = (4 * R * B + 12 * n) / PEAK * 1e3
res = report(label, R, B, n, True, (("(a) loop", loop, 5, la), ("(b) block_search_sorted", one, 20, 1)), floor_ms)
print(f"  {label:22s} floor {floor_ms:.4f} ms; (a) / (b) = {res['(a) loop'][0] / res['(b) block_search_sorted'][0]:.1f}", flush=True)
del T, pdf, totals, marginal, row, needles, loop, one

# ---- one row: forwarded to search_sorted -------------------------------------------------------------------------------------
R, B = 1, 1 << 20
label = "one row of 1 Mi"
T = ek.Float32(cdf_rows(R, B))
needles = ek.Float32(u)
direct = lambda: ek.search_sorted(T, needles)
one = lambda: ek.block_search_sorted(T, needles, B)
compare(label, direct, one)
floor_ms = (4 * R * B + 8 * n) / PEAK * 1e3
res = report(label, R, B, n, False, (("(a) search_sorted", direct, 20, 1), ("(b) block_search_sorted", one, 20, 1)), floor_ms)
a, b = res["(a) search_sorted"], res["(b) block_search_sorted"]
print(f"  {label:22s} floor {floor_ms:.4f} ms; (b) / (a) at the minimum = {b[0] / a[0]:.3f}; spread of (a)'s own 20 calls: "
      f"max / min = {a[2] / a[0]:.3f}", flush=True)
