"""ek_hip_reduce_segments through the C ABI (csrc/block_segments.hip): out[j] = op over in[lo_j : hi_j] with
lo_j = min(starts[j], n), hi_j = max(lo_j, min(starts[j + 1], n)) and starts[m] := n.

Expected values are numpy's (ufunc.reduceat over the non-empty segments, which are consecutive for non-decreasing starts; the
identity for the empty ones).  Integers (wrapping), hmin / hmax (minNum / maxNum, -0 < +0), float sums of small-integer data and
float products over {+-1, +-2, +-0.5} (only the first 100 entries of a segment differ from +-1, so that no partial product leaves
the exponent range in any order) are exact in every summation order and compared bit for bit.  Float sums of random data are
compared with a float64 (f32) or math.fsum (f64) sum under the order-independent bound  gamma_(L-1) * sum |x_i|  per segment of L
entries, gamma_k = k u / (1 - k u), u = 2^-24 or 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any
order of L - 1 additions): derived, not measured.  The shapes at which the route changes are asked from ek_hip_reduce_segments_plan.
Bad starts are only ever tried on views into larger buffers of the test's own, and no bad value exceeds the enclosing allocation."""
import ctypes
import math

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
OPS = ["hsum", "hprod", "hmin", "hmax"]
SZ = ctypes.c_size_t
CAP = 2 << 20
GROUPED, SEGMENT, SPLIT = 1, 2, 3
BASE = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, n, m):
    return capi.reduce_segments_plan(dt, n, m, cu_count())


# ---- shapes ----------------------------------------------------------------------------------------------------------
def starts_of(lengths, gap=0):
    """(starts, n) of consecutive segments of these lengths, the first behind `gap` entries that belong to no segment"""
    lengths = np.asarray(lengths, np.int64)
    ends = gap + np.cumsum(lengths)
    return (ends - lengths).astype(np.uint32), int(ends[-1]) if lengths.size else gap


def length_mixes():
    """(label, lengths, gap): every length of BASE in front of, between and behind the others; one long segment among single
    entries (with a mean of at most 1024 entries: several chunks in one workgroup of the grouped route; with fewer single entries:
    a workgroup of its own); nothing but empty segments; one segment; entries in front of the first start; trailing starts equal to n"""
    mixes = [(f"rot{r}", BASE[r:] + BASE[:r], 0) for r in range(len(BASE))]
    mixes += [("long_between", [1] * 15 + [20000] + [1] * 17, 0), ("long_between_own_workgroup", [1] * 5 + [20000] + [1] * 7, 0), ("long_first", [20000] + [1] * 300, 0), ("long_last", [1] * 300 + [20000], 0)]
    mixes += [("all_empty", [0] * 37, 0), ("all_empty_behind_entries", [0] * 300, 11)]
    mixes += [(f"one_{L}", [L], 0) for L in (0, 1, 5000)] + [("one_behind_a_gap", [777], 5)]
    mixes += [("gap", BASE, 7), ("trailing_at_n", BASE[1:] + [0] * 9, 0), ("many_short", [3, 0, 1, 2] * 3000, 1)]
    return mixes


def bounds(starts, n):
    """(lo, hi) of every segment: the clamped definition"""
    s = np.minimum(starts.astype(np.int64), n)
    nxt = np.concatenate([s[1:], [n]])
    return s, np.maximum(s, nxt)


# ---- data and expected values ----------------------------------------------------------------------------------------
def exact_data(dt, op, n, lo, seed):
    """inputs whose reduction is exact in every order (see the module docstring); lo: the segments' first entries, ascending"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        return v | dt.type(1) if op == "hprod" else v               # odd factors: the wrapped product keeps information
    if op == "hsum":
        return rng.integers(-8, 9, n).astype(dt)
    if op == "hprod":
        v = rng.choice(np.array([1.0, -1.0], dt), n)
        if n and lo.size:
            seg = np.searchsorted(lo, np.arange(n), side="right") - 1
            early = (seg >= 0) & (np.arange(n) - lo[np.maximum(seg, 0)] < 100)
            v[early] = rng.choice(np.array([2.0, -2.0, 0.5, -0.5, 1.0, -1.0], dt), int(early.sum()))
        return v
    v = (rng.standard_normal(n) * 100).astype(dt)
    for value in (np.nan, -0.0, 0.0, np.inf, -np.inf):
        if n:
            v[rng.integers(0, n, max(1, n // 16))] = value
    return v


def identity(dt, op):
    dt = np.dtype(dt)
    if op == "hsum":
        return dt.type(0)
    if op == "hprod":
        return dt.type(1)
    if dt.kind == "f":
        return dt.type(np.nan)
    return np.iinfo(dt).max if op == "hmin" else np.iinfo(dt).min


def expected(x, op, lo, hi):
    """numpy's reduction of every segment [lo, hi); the non-empty ones are consecutive"""
    out = np.full(lo.size, identity(x.dtype, op), x.dtype)
    ne = np.flatnonzero(hi > lo)
    if ne.size == 0:
        return out
    assert np.array_equal(hi[ne[:-1]], lo[ne[1:]])
    xs, at = x[:hi[ne[-1]]], lo[ne]
    with np.errstate(all="ignore"):
        if op == "hsum":
            out[ne] = np.add.reduceat(xs, at, dtype=x.dtype)
        elif op == "hprod":
            out[ne] = np.multiply.reduceat(xs, at, dtype=x.dtype)
        elif x.dtype.kind != "f":
            out[ne] = (np.minimum if op == "hmin" else np.maximum).reduceat(xs, at)
        else:
            # minNum / maxNum with -0 < +0 (numpy's fmin / fmax leave the sign of a zero result open)
            r = (np.fmin if op == "hmin" else np.fmax).reduceat(xs, at)
            zero = r == 0
            if zero.any():
                neg = np.logical_or.reduceat((xs == 0) & np.signbit(xs), at)
                pos = np.logical_or.reduceat((xs == 0) & ~np.signbit(xs), at)
                r[zero] = np.where(neg[zero], -0.0, 0.0) if op == "hmin" else np.where(pos[zero], 0.0, -0.0)
            out[ne] = r
    return out


def true_sums_and_bounds(x, lo, hi):
    """per segment the sum in higher precision and gamma_(L-1) * sum |x|"""
    u = 2.0 ** -24 if x.dtype == np.float32 else 2.0 ** -53
    true, mag = np.zeros(lo.size), np.zeros(lo.size)
    for j in np.flatnonzero(hi > lo):
        seg = x[lo[j]:hi[j]]
        true[j] = seg.astype(np.float64).sum() if x.dtype == np.float32 else math.fsum(seg)
        mag[j] = np.abs(seg.astype(np.float64)).sum()
    k = np.maximum(hi - lo - 1, 0)
    return true, k * u / (1 - k * u) * mag


def run(capi, op, x, starts, in_offset=0, out_offset=0):
    """reduce_segments on device copies of x and starts; the offsets make `in` / `out` views that are only element-aligned"""
    dt = x.dtype
    base = capi.Buf.from_numpy(np.concatenate([np.zeros(in_offset, dt), x]))       # (owns the memory the view looks into)
    src = base.view(in_offset, x.size)
    st = capi.Buf.from_numpy(starts.astype(np.uint32))
    if not out_offset:
        return capi.reduce_segments(op, src, st).numpy()
    pad, mark = 4, dt.type(123)
    out = capi.Buf.from_numpy(np.full(starts.size + 2 * pad, mark, dt))
    capi.check(capi.lib.ek_hip_reduce_segments(capi.REDUCE[op], src.ek, ctypes.c_void_p(out.ptr + out_offset * dt.itemsize),
                                               ctypes.c_void_p(src.ptr if x.size else None), SZ(x.size), ctypes.c_void_p(st.ptr), SZ(starts.size)))
    got = out.numpy()
    assert np.all(got[:out_offset] == mark) and np.all(got[out_offset + starts.size:] == mark), "written outside out"
    return got[out_offset:out_offset + starts.size]


def check_exact(capi, dt, op, lengths, gap, seed, in_offset=0, out_offset=0, label=""):
    starts, n = starts_of(lengths, gap)
    lo, hi = bounds(starts, n)
    x = exact_data(dt, op, n, lo, seed)
    got = run(capi, op, x, starts, in_offset, out_offset)
    want = expected(x, op, lo, hi)
    assert bits_equal(got, want), (name(dt), op, label, n, starts.size, in_offset, out_offset, plan(capi, dt, n, starts.size),
                                   np.flatnonzero(~((got == want) | ((got != got) & (want != want))))[:8])


def random_lengths(rng, n, m):
    """m lengths that sum to n, a few of them empty"""
    cuts = np.sort(rng.integers(0, n + 1, m - 1))
    return np.diff(np.concatenate([[0], cuts, [n]]))


# ---- 1. the length mixes, all types and ops ------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_length_mixes(capi, dt, op):
    for k, (label, lengths, gap) in enumerate(length_mixes()):
        check_exact(capi, dt, op, lengths, gap, 100 * k + 1, label=label)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_uniform_lengths_against_reduce_blocks(capi, dt, op):
    for B, m in ((1, 300), (3, 1000), (64, 257), (100, 65), (1024, 9), (1025, 9), (4099, 5), (300000, 2)):
        starts = (np.arange(m, dtype=np.int64) * B).astype(np.uint32)
        x = exact_data(dt, op, m * B, starts.astype(np.int64), B + m)
        buf = capi.Buf.from_numpy(x)
        got = capi.reduce_segments(op, buf, capi.Buf.from_numpy(starts)).numpy()
        assert bits_equal(got, capi.reduce_blocks(op, buf, B).numpy()), (name(dt), op, B, m)


# ---- 2. the edges of the three routes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_edges_of_every_route(capi, dt, op):
    rng = np.random.default_rng(17)
    cu = cu_count()
    assert cu >= 2                                               # (m = 3 segments are fewer than 2 x #CU)
    for m in (3, 64):
        # grouped up to a mean of 1024 entries, one workgroup per segment beyond
        assert plan(capi, dt, 1024 * m, m)[0] == GROUPED and plan(capi, dt, 1024 * m + 1, m)[0] == SEGMENT
        for n in (1024 * m - 1, 1024 * m, 1024 * m + 1, 1024 * m + 2):
            check_exact(capi, dt, op, random_lengths(rng, n, m), 0, n, label=f"grouped_edge_{n}_{m}")
    # split from a mean (rounded up) of 16 Ki entries for fewer than 2 x #CU segments
    for m in (2, 3):
        assert plan(capi, dt, 16383 * m, m)[0] == SEGMENT and plan(capi, dt, 16383 * m + 1, m)[0] == SPLIT
        for n in (16383 * m - 1, 16383 * m, 16383 * m + 1, 16384 * m):
            check_exact(capi, dt, op, random_lengths(rng, n, m), 0, n, label=f"split_edge_{n}_{m}")
    # the split route with one segment 100 x the other, in front of, between and behind
    for lengths in ([5000, 500000], [500000, 5000], [4000, 400000, 4000], [400000, 4000, 0], [0, 0, 300007]):
        n, m = sum(lengths), len(lengths)
        route, _, splits, _ = plan(capi, dt, n, m)
        assert route == SPLIT and splits >= 2
        check_exact(capi, dt, op, lengths, 0, n, label=f"split_{lengths}")
        check_exact(capi, dt, op, lengths, 3, n + 1, label=f"split_gap_{lengths}")


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_float_sums_of_random_data_within_the_gamma_bound(capi, dt):
    rng = np.random.default_rng(7)
    shapes = [(lengths, gap) for _, lengths, gap in length_mixes()[::3]]
    shapes += [(random_lengths(rng, 1024 * 3 + 1, 3), 0), (random_lengths(rng, 70000, 1000), 0), ([5000, 500000], 0), ([400000, 4000, 4000], 2)]
    for lengths, gap in shapes:
        starts, n = starts_of(lengths, gap)
        lo, hi = bounds(starts, n)
        x = (rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n))).astype(dt)
        got = run(capi, "hsum", x, starts).astype(np.float64)
        true, bound = true_sums_and_bounds(x, lo, hi)
        err = np.abs(got - true)
        print(name(dt), n, starts.size, plan(capi, dt, n, starts.size), "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (name(dt), n, starts.size, float((err - bound).max()))
        assert np.all(got[hi == lo] == 0) and not np.any(np.signbit(got[hi == lo]))


# ---- 3. misaligned views ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_misaligned_views(capi, dt):
    offsets = (1, 2, 3) if np.dtype(dt).itemsize == 4 else (1,)
    shapes = [(BASE, 0), (BASE[::-1], 5), ([1] * 15 + [20000] + [1] * 17, 0), ([1500, 0, 3000, 1], 0), ([5000, 500000], 1)]
    for offset in offsets:
        for op in OPS:
            for k, (lengths, gap) in enumerate(shapes):
                check_exact(capi, dt, op, lengths, gap, 31 * k + offset, in_offset=offset, label="in")
                check_exact(capi, dt, op, lengths, gap, 31 * k + offset, out_offset=offset, label="out")
                check_exact(capi, dt, op, lengths, gap, 31 * k + offset, in_offset=offset, out_offset=(offset % 3) + 1 if len(offsets) > 1 else 1,
                            label="both")
    # the result of a sum does not leave the gamma bound at any alignment either
    if np.dtype(dt).kind == "f":
        rng = np.random.default_rng(3)
        for lengths, gap in shapes:
            starts, n = starts_of(lengths, gap)
            lo, hi = bounds(starts, n)
            x = rng.standard_normal(n).astype(dt)
            got = run(capi, "hsum", x, starts, in_offset=1).astype(np.float64)
            true, bound = true_sums_and_bounds(x, lo, hi)
            assert np.all(np.abs(got - true) <= bound), (name(dt), lengths[:4], gap)


# ---- 4. nothing leaks between neighbouring segments ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_no_leakage_between_neighbours(capi, dt):
    shapes = [[3, 1, 0, 64, 65, 2, 7], [1, 1, 20000, 1, 1], [1] * 12 + [20000] + [1] * 12, [1500, 3000, 1100, 2000], [5000, 500000, 5000]]
    for lengths in shapes:
        starts, n = starts_of(lengths, 2)
        lo, hi = bounds(starts, n)
        st = capi.Buf.from_numpy(starts)
        for j in np.flatnonzero(hi > lo):
            for at in (lo[j], hi[j] - 1):
                for special in (np.nan, np.inf, -np.inf, 1e30):
                    x = np.zeros(n, dt)
                    x[at] = special
                    got = capi.reduce_segments("hsum", capi.Buf.from_numpy(x), st).numpy()
                    want = np.zeros(starts.size, dt)
                    want[j] = special
                    assert bits_equal(got, want), (name(dt), lengths, j, at, special, got[max(0, j - 1):j + 2])
        # ... and a value in front of the first start reaches no segment
        x = np.zeros(n, dt)
        x[:2] = np.nan
        assert bits_equal(capi.reduce_segments("hsum", capi.Buf.from_numpy(x), st).numpy(), np.zeros(starts.size, dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_min_num_max_num_and_empty_segments(capi, dt):
    for L in (2, 5, 64, 1500, 40000):
        lengths = [L, 0, L, L, 0, L]
        starts, n = starts_of(lengths)
        x = np.full(n, np.nan, dt)
        x[:L] = 3.0
        x[L // 2] = np.nan                           # a NaN inside a segment is ignored
        x[2 * L], x[3 * L - 1] = -0.0, 0.0           # segment 2 stays all NaN; segment 3 is {-0, +0} and NaN
        x[3 * L:] = 0.0
        x[n - 1] = -0.0
        buf, st = capi.Buf.from_numpy(x), capi.Buf.from_numpy(starts)
        lo, hi = capi.reduce_segments("hmin", buf, st).numpy(), capi.reduce_segments("hmax", buf, st).numpy()
        assert lo[0] == 3 and hi[0] == 3, (L, lo, hi)
        for j in (1, 2, 4):                          # empty, all NaN, empty
            assert np.isnan(lo[j]) and np.isnan(hi[j]), (L, j, lo, hi)
        for j in (3, 5):
            assert lo[j] == 0 and np.signbit(lo[j]) and hi[j] == 0 and not np.signbit(hi[j]), (L, j, lo, hi)


# ---- 5. run-to-run identity ------------------------------------------------------------------------------------------------
def test_run_to_run_identity(capi):
    rng = np.random.default_rng(11)
    for lengths in (random_lengths(rng, 300000, 40000), [1] * 5 + [20000] + [1] * 7, random_lengths(rng, 1 << 20, 257), [5000, 500000, 7]):
        starts, n = starts_of(lengths)
        buf, st = capi.Buf.from_numpy(rng.standard_normal(n).astype(np.float32)), capi.Buf.from_numpy(starts)
        runs = [capi.reduce_segments("hsum", buf, st).numpy() for _ in range(3)]
        assert bits_equal(runs[0], runs[1]) and bits_equal(runs[0], runs[2]), (n, starts.size)


# ---- 6. inside a step graph, replayed with new entries AND new starts --------------------------------------------------------
def test_inside_a_step_graph(capi):
    lib = capi.lib
    rng = np.random.default_rng(13)
    shapes = [(100000, 3001), (1 << 20, 300), (600000, 3)]
    routes = [plan(capi, np.float32, n, m)[0] for n, m in shapes]
    assert routes == [GROUPED, SEGMENT, SPLIT]
    def hosts():
        return [(rng.standard_normal(n).astype(np.float32), starts_of(random_lengths(rng, n - 5, m), 5)[0]) for n, m in shapes]
    h1, h2 = hosts(), hosts()
    xs = [capi.Buf.from_numpy(x) for x, _ in h1]
    sts = [capi.Buf.from_numpy(s) for _, s in h1]
    held = []
    capi.check(lib.ek_hip_graph_begin())
    try:
        held = [capi.reduce_segments("hsum", x, s) for x, s in zip(xs, sts)]
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        for hs in (h1, h2, h1):
            for x, s, (hx, hst) in zip(xs, sts, hs):
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(x.ptr), hx.ctypes.data_as(ctypes.c_void_p), SZ(hx.nbytes)))
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(s.ptr), hst.ctypes.data_as(ctypes.c_void_p), SZ(hst.nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            replayed = [b.numpy() for b in held]
            eager = [capi.reduce_segments("hsum", x, s).numpy() for x, s in zip(xs, sts)]
            for a, b, (hx, hst) in zip(replayed, eager, hs):
                assert bits_equal(a, b)
                lo, hi = bounds(hst, hx.size)
                true, bound = true_sums_and_bounds(hx, lo, hi)
                assert np.all(np.abs(a.astype(np.float64) - true) <= bound)
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------
def test_arguments(capi):
    lib = capi.lib
    x = capi.Buf.from_numpy(np.arange(12, dtype=np.float32))
    st = capi.Buf.from_numpy(np.array([0, 3, 3, 10], np.uint32))
    out = capi.Buf.from_numpy(np.full(4, 7, np.float32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    rs = lib.ek_hip_reduce_segments
    l0 = lib.ek_hip_launch_count()
    assert rs(4, capi.F32, p(out), p(x), SZ(12), p(st), SZ(4)) == -1 and rs(-1, capi.F32, p(out), p(x), SZ(12), p(st), SZ(4)) == -1
    assert b"ek_hip_reduce_segments" in lib.ek_hip_last_error()
    assert rs(0, capi.F32, None, p(x), SZ(12), p(st), SZ(4)) == -1 and rs(0, capi.F32, p(out), None, SZ(12), p(st), SZ(4)) == -1
    assert rs(0, capi.F32, p(out), p(x), SZ(12), None, SZ(4)) == -1
    for bad in (ctypes.c_void_p(out.ptr + 1), ctypes.c_void_p(out.ptr + 2)):
        assert rs(0, capi.F32, bad, p(x), SZ(12), p(st), SZ(4)) == -1
    assert rs(0, capi.F32, p(out), ctypes.c_void_p(x.ptr + 2), SZ(8), p(st), SZ(4)) == -1
    assert rs(0, capi.F32, p(out), p(x), SZ(12), ctypes.c_void_p(st.ptr + 2), SZ(3)) == -1
    assert rs(0, capi.BOOL, p(out), p(x), SZ(12), p(st), SZ(4)) == -2 and rs(0, 99, p(out), p(x), SZ(12), p(st), SZ(4)) == -2
    assert rs(0, capi.F32, p(out), p(x), SZ(1 << 32), p(st), SZ(4)) == -2 and b"2^32" in lib.ek_hip_last_error()
    assert rs(0, capi.F32, p(out), p(x), SZ(12), p(st), SZ(1 << 32)) == -2
    assert rs(0, capi.F32, None, None, SZ(0), None, SZ(0)) == 0 and rs(0, capi.F32, None, p(x), SZ(12), None, SZ(0)) == 0    # no segment
    assert lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), np.full(4, 7, np.float32))
    # the calls after refused ones work; n == 0 fills with the identity, whatever the starts
    assert rs(0, capi.F32, p(out), p(x), SZ(12), p(st), SZ(4)) == 0 and np.array_equal(out.numpy(), [3, 0, 42, 21])
    for op, dt, want in (("hsum", np.float32, 0), ("hprod", np.int64, 1), ("hmax", np.int32, -(1 << 31)), ("hmin", np.uint64, (1 << 64) - 1)):
        got = capi.reduce_segments(op, capi.Buf(dt, 0), st).numpy()
        assert got.dtype == dt and np.all(got == np.array(want, dt)), (op, got)
    assert np.all(np.isnan(capi.reduce_segments("hmin", capi.Buf(np.float64, 0), st).numpy()))


# ---- 8. bad starts: inside the test's own memory ------------------------------------------------------------------------------
def bad_starts_run(capi, dt, op, x, starts, pad=256):
    """x and out are views into larger buffers: `pad` sentinel entries on both sides of each"""
    dt = np.dtype(dt)
    poison = dt.type(1e30) if dt.kind == "f" else dt.type(0x5A5A5A5A)
    mark = dt.type(np.nan) if dt.kind == "f" else dt.type(0x3C3C3C3C)
    assert int(starts.max()) <= x.size + pad                      # no bad value leaves the enclosing allocation
    src = capi.Buf.from_numpy(np.concatenate([np.full(pad, poison, dt), x, np.full(pad, poison, dt)]))
    out = capi.Buf.from_numpy(np.full(starts.size + 2 * pad, mark, dt))
    st = capi.Buf.from_numpy(starts.astype(np.uint32))
    capi.check(capi.lib.ek_hip_reduce_segments(capi.REDUCE[op], src.ek, ctypes.c_void_p(out.ptr + pad * dt.itemsize),
                                               ctypes.c_void_p(src.ptr + pad * dt.itemsize), SZ(x.size), ctypes.c_void_p(st.ptr), SZ(starts.size)))
    got = out.numpy()
    assert bits_equal(got[:pad], np.full(pad, mark, dt)) and bits_equal(got[pad + starts.size:], np.full(pad, mark, dt)), "written outside out"
    assert bits_equal(src.numpy()[:pad], np.full(pad, poison, dt)), "the input changed"
    return got[pad:pad + starts.size]


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_starts_above_n_are_clamped(capi, dt):
    rng = np.random.default_rng(23)
    for n, lengths in ((3000, [5, 0, 700, 64, 1, 2000]), (50000, [1] * 40 + [30000] + [7] * 100), (200000, [100, 150000]), (40000, [39000, 500])):
        starts, used = starts_of(lengths, 3)
        assert used < n
        # the last few starts lie behind the end of the array: at n, just above it, and up to the end of the enclosing buffer
        above = np.array([n, n, n + 1, n + 1, n + 7, n + 200, n + 256], np.uint32)
        bad = np.concatenate([starts, above])
        lo, hi = bounds(bad, n)
        for op in OPS:
            x = exact_data(dt, op, n, lo, n)
            got = bad_starts_run(capi, dt, op, x, bad)
            assert bits_equal(got, expected(x, op, lo, hi)), (name(dt), op, n, plan(capi, dt, n, bad.size))
    # every start above n: every segment is empty
    bad = np.array([1001, 1001, 1100, 1256], np.uint32)
    assert bits_equal(bad_starts_run(capi, dt, "hsum", exact_data(dt, "hsum", 1000, np.zeros(0, np.int64), 1), bad), np.zeros(4, dt))


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_decreasing_starts_stay_inside(capi, dt):
    rng = np.random.default_rng(29)
    cases = []
    for n, m in ((5000, 40), (5000, 3), (100000, 2500), (300000, 4), (600000, 3)):
        cases.append((n, rng.integers(0, n + 256, m).astype(np.uint32)))                       # no order at all
        s = np.sort(rng.integers(0, n, m)).astype(np.uint32)
        cases.append((n, s[::-1].copy()))                                                      # strictly the wrong way round
        s[m // 2] = n + 200                                                                    # one value out of line
        cases.append((n, s))
    for n, bad in cases:
        x = rng.integers(-8, 9, n).astype(dt)
        got = bad_starts_run(capi, dt, "hsum", x, bad)
        # every entry was written (the float mark is NaN, the integer mark is no possible sum) and holds a sum of entries of x only
        if np.dtype(dt).kind == "f":
            assert np.all(np.isfinite(got)), (name(dt), n, bad.size)
        assert np.all(np.abs(got.astype(np.float64)) <= 8.0 * n), (name(dt), n, bad.size, plan(capi, dt, n, bad.size))
        # a segment whose own two starts are in order holds its sum wherever the disorder is, as long as its workgroup reads it:
        # not promised, so not asserted; what IS promised is checked above and in bad_starts_run
