"""ek_hip_psum_segments through the C ABI (csrc/segment_scan.hip): prefix sums inside the ragged segments [lo_j, hi_j) with
lo_j = min(starts[j], n), hi_j = max(lo_j, min(starts[j + 1], n)) and starts[m] := n; +0 in front of min(starts[0], n).

Expected values are numpy's: np.cumsum per clamped segment (reversed for `reverse`, shifted for `exclusive`), +0 outside.  Integers
(wrapping) and floats of small-integer data are exact in every order and compared bit for bit.  Random float data are compared with
float64 (f32) or long double (f64) prefix sums under the order-independent bound  gamma_k * sum |x_i|  over the k + 1 terms of that
prefix, gamma_k = k u / (1 - k u), u = 2^-24 or 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any order
of k additions): derived, not measured.  Tile, tiles per workgroup and the grid cap are asked from ek_hip_psum_segments_plan.  Bad
starts are only ever tried on views into larger buffers of the test's own, and no bad value exceeds the enclosing allocation."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
MODES = [(False, False), (True, False), (False, True), (True, True)]          # (exclusive, reverse)
SZ = ctypes.c_size_t
BASE = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def name(dt):
    return np.dtype(dt).name


@functools.lru_cache(None)
def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, n, m):
    return capi.psum_segments_plan(dt, n, m, cu_count())


def tile_of(capi, dt):
    return plan(capi, dt, 1, 1)[0]


def grid_cap(capi, dt):
    """the largest number of workgroups: asked with more tiles than any cap"""
    return plan(capi, dt, (1 << 32) - 1, 1)[2]


# ---- shapes ----------------------------------------------------------------------------------------------------------
def starts_of(lengths, gap=0):
    """(starts, n) of consecutive segments of these lengths, the first behind `gap` entries that belong to no segment"""
    lengths = np.asarray(lengths, np.int64)
    ends = gap + np.cumsum(lengths)
    return (ends - lengths).astype(np.uint32), int(ends[-1]) if lengths.size else gap


def bounds(starts, n):
    s = np.minimum(starts.astype(np.int64), n)
    nxt = np.concatenate([s[1:], [n]])
    return s, np.maximum(s, nxt)


def length_mixes():
    """the lengths of test_segment_reduce_gpu.py"""
    mixes = [(f"rot{r}", BASE[r:] + BASE[:r], 0) for r in range(0, len(BASE), 3)]
    mixes += [("long_between", [1] * 15 + [20000] + [1] * 17, 0), ("long_first", [20000] + [1] * 300, 0), ("long_last", [1] * 300 + [20000], 0)]
    mixes += [("all_empty", [0] * 37, 0), ("all_empty_behind_entries", [0] * 300, 11)]
    mixes += [(f"one_{L}", [L], 0) for L in (1, 5000)] + [("one_behind_a_gap", [777], 5)]
    mixes += [("gap", BASE, 7), ("trailing_at_n", BASE[1:] + [0] * 9, 0), ("many_short", [3, 0, 1, 2] * 3000, 1)]
    return mixes


def tile_mixes(T):
    """the shapes at which THIS kernel can go wrong, for a tile of T entries (every workgroup owns one tile at these sizes)"""
    return [("head_at_tile_first", [T, T, 3], 0), ("head_at_tile_last", [T - 1, 1, T - 1, 1, 5], 0), ("head_at_tile_plus_1", [T + 1, T, 5], 0),
            ("head_at_tile_minus_1", [T - 1, T, 5], 0), ("one_tile_behind_a_gap", [T], T), ("spans_three_tiles", [5, 3 * T + 11, 6], 0),
            ("spans_with_singles", [1] * 9 + [3 * T + 5] + [1] * 9, 0), ("spans_ten_tiles", [1] * 3 + [10 * T + 3] + [1] * 3, 2),
            ("equal_starts_inside_a_tile", [100] + [0] * 10000 + [T], 0), ("equal_starts_at_a_tile_boundary", [T] + [0] * 10000 + [T + 3], 0),
            ("gap_past_the_first_tile", [5, T, 3], T + 17), ("whole_array", [2 * T + 77], 0), ("whole_small", [7], 0)]


def all_mixes(T):
    return length_mixes() + tile_mixes(T)


def seams_shape(capi, dt):
    """2 x grid cap + 1 tiles: every workgroup owns three tiles (the last fewer) and carries between them; one segment crosses a
    seam between two tiles of a workgroup, one a seam between two workgroups, one spans several workgroups"""
    T, cap = tile_of(capi, dt), grid_cap(capi, dt)
    n = (2 * cap + 1) * T
    per = plan(capi, dt, n, 1)[1]
    assert per == 3 and plan(capi, dt, n, 1)[3] == 3
    cuts = [0, 5, T - 3, T + 9, 3 * T - 5, 3 * T + 5, 7 * T, 7 * T + 1, 19 * T + 100, n - 2 * T - 1, n - 1]
    return np.array(cuts, np.uint32), n


# ---- data and expected values ----------------------------------------------------------------------------------------
def exact_data(dt, n, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    return rng.integers(-8, 9, n).astype(dt)


def reference(x, starts, excl, rev, acc=None):
    """np.cumsum per clamped segment, +0 outside; acc: the type the sums are formed in"""
    n = x.size
    out = np.zeros(n, acc or x.dtype)
    lo, hi = bounds(starts, n)
    with np.errstate(all="ignore"):
        for j in np.flatnonzero(hi > lo):
            seg = x[lo[j]:hi[j]].astype(out.dtype)
            c = np.cumsum(seg[::-1] if rev else seg, dtype=out.dtype)
            if excl:
                c = np.concatenate([np.zeros(1, out.dtype), c[:-1]])
            out[lo[j]:hi[j]] = c[::-1] if rev else c
    return out


def gamma_bound(x, starts, excl, rev):
    """gamma_k * sum |x| over the k + 1 terms of every prefix (0 where it has at most one term)"""
    u = 2.0 ** -24 if x.dtype == np.float32 else 2.0 ** -53
    terms = reference(np.ones(x.size, np.float64), starts, excl, rev)
    mag = reference(np.abs(x.astype(np.float64)), starts, excl, rev)
    k = np.maximum(terms - 1, 0)
    return k * u / (1 - k * u) * mag


def run(capi, x, starts, excl=False, rev=False, in_offset=0, out_offset=0, inplace=False):
    """psum_segments on device copies; the offsets make `in` / `out` views that are only element-aligned; the entries around
    `out` must keep their mark"""
    dt, n, pad = x.dtype, x.size, 8
    mark = dt.type(123)
    st = capi.Buf.from_numpy(starts.astype(np.uint32))
    if inplace:
        buf = capi.Buf.from_numpy(np.concatenate([np.full(pad + in_offset, mark, dt), x, np.full(pad, mark, dt)]))
        src = dst = buf.ptr + (pad + in_offset) * dt.itemsize
        out, out_offset = buf, in_offset
    else:
        base = capi.Buf.from_numpy(np.concatenate([np.zeros(in_offset, dt), x]))       # (owns the memory the view looks into)
        src = base.ptr + in_offset * dt.itemsize
        out = capi.Buf.from_numpy(np.full(n + 2 * pad + out_offset, mark, dt))
        dst = out.ptr + (pad + out_offset) * dt.itemsize
    flags = (capi.SCAN_EXCLUSIVE if excl else 0) | (capi.SCAN_REVERSE if rev else 0)
    capi.check(capi.lib.ek_hip_psum_segments(capi.NP2EK[np.dtype(dt)], ctypes.c_void_p(dst if n else None), ctypes.c_void_p(src if n else None), SZ(n),
                                             ctypes.c_void_p(st.ptr if starts.size else None), SZ(starts.size), flags))
    got = out.numpy()
    a = pad + out_offset
    assert np.all(got[:a] == mark) and np.all(got[a + n:] == mark), "written outside out"
    return got[a:a + n]


def check_exact(capi, dt, starts, n, seed, label="", **kw):
    x = exact_data(dt, n, seed)
    for excl, rev in MODES:
        got = run(capi, x, starts, excl, rev, **kw)
        want = reference(x, starts, excl, rev)
        assert bits_equal(got, want), (name(dt), label, n, starts.size, excl, rev, kw, plan(capi, dt, n, starts.size),
                                       np.flatnonzero(~((got == want) | ((got != got) & (want != want))))[:8])


# ---- 1. every shape, all types, all four modes ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_length_mixes(capi, dt):
    for k, (label, lengths, gap) in enumerate(all_mixes(tile_of(capi, dt))):
        starts, n = starts_of(lengths, gap)
        check_exact(capi, dt, starts, n, 100 * k + 1, label=label)
    # no segment at all: +0 everywhere; no entry: nothing happens
    x = exact_data(dt, 5000, 3)
    for excl, rev in MODES:
        assert bits_equal(run(capi, x, np.zeros(0, np.uint32), excl, rev), np.zeros(5000, dt))
        assert run(capi, x[:0], np.array([0, 0], np.uint32), excl, rev).size == 0


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_several_tiles_per_workgroup(capi, dt):
    starts, n = seams_shape(capi, dt)
    check_exact(capi, dt, starts, n, 5, label="seams")


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_misaligned_views_and_in_place(capi, dt):
    T = tile_of(capi, dt)
    shapes = [(BASE, 5), ([1] * 9 + [3 * T + 5] + [1] * 9, 0), ([T + 1, T, 5], 1)]
    for k, (lengths, gap) in enumerate(shapes):
        starts, n = starts_of(lengths, gap)
        x = exact_data(dt, n, 31 * k)
        for excl, rev in MODES:
            want = reference(x, starts, excl, rev)
            for i in range(4):
                for o in range(4):
                    assert bits_equal(run(capi, x, starts, excl, rev, in_offset=i, out_offset=o), want), (name(dt), k, excl, rev, i, o)
                assert bits_equal(run(capi, x, starts, excl, rev, in_offset=i, inplace=True), want), (name(dt), k, excl, rev, i, "in place")
    starts, n = seams_shape(capi, dt)
    x = exact_data(dt, n, 77)
    for excl, rev in MODES:
        assert bits_equal(run(capi, x, starts, excl, rev, in_offset=1, inplace=True), reference(x, starts, excl, rev)), (name(dt), excl, rev)


# ---- 2. random float data: the gamma bound; exclusive IS the neighbouring inclusive entry ----------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_random_floats_within_the_gamma_bound_and_moved_not_recomputed(capi, dt):
    rng = np.random.default_rng(7)
    T = tile_of(capi, dt)
    shapes = [starts_of(lengths, gap) for _, lengths, gap in all_mixes(T)[::2]] + [seams_shape(capi, dt)]
    for starts, n in shapes:
        x = (rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n))).astype(dt)
        lo, hi = bounds(starts, n)
        first = np.zeros(n, bool)
        last = np.zeros(n, bool)
        ne = hi > lo
        first[lo[ne]] = True
        last[hi[ne] - 1] = True
        outside = np.arange(n) < (min(int(starts[0]), n) if starts.size else n)
        got = {}
        for excl, rev in MODES:
            got[excl, rev] = g = run(capi, x, starts, excl, rev)
            true = reference(x, starts, excl, rev, acc=np.float64 if dt == np.float32 else np.longdouble)
            bound = gamma_bound(x, starts, excl, rev)
            err = np.abs(g.astype(true.dtype) - true).astype(np.float64)
            print(name(dt), n, starts.size, excl, rev, "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()) if n else 0)
            assert np.all(err <= bound), (name(dt), n, starts.size, excl, rev, float((err - bound).max()))
            assert np.all(g[outside] == 0) and not np.any(np.signbit(g[outside]))
        # forward: exclusive entry i is inclusive entry i - 1; reverse: inclusive entry i + 1; the segment's first / last entry: +0
        inner = ~first & ~outside
        assert bits_equal(got[True, False][inner], got[False, False][np.flatnonzero(inner) - 1]), (name(dt), n, starts.size)
        inner = ~last & ~outside
        assert bits_equal(got[True, True][inner], got[False, True][np.flatnonzero(inner) + 1]), (name(dt), n, starts.size)
        for g, ends in ((got[True, False], first), (got[True, True], last)):
            assert np.all(g[ends] == 0) and not np.any(np.signbit(g[ends]))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_single_term_entries_keep_negative_zero(capi, dt):
    T = tile_of(capi, dt)
    for lengths, gap in (([1] * 300, 0), ([T - 1, 1, T - 1, 1, 5], 0), ([3, 1, T, 2, 2 * T + 1, 1], 2)):
        starts, n = starts_of(lengths, gap)
        lo, hi = bounds(starts, n)
        x = np.full(n, 1.0, dt)
        x[lo] = -0.0
        x[hi - 1] = -0.0
        fwd, bwd = run(capi, x, starts), run(capi, x, starts, rev=True)
        assert np.all(fwd[lo] == 0) and np.all(np.signbit(fwd[lo])) and np.all(bwd[hi - 1] == 0) and np.all(np.signbit(bwd[hi - 1]))
        assert bits_equal(fwd, reference(x, starts, False, False)) and bits_equal(bwd, reference(x, starts, False, True))


# ---- 3. nothing leaks between neighbouring segments --------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_no_leakage_between_neighbours(capi, dt):
    T = tile_of(capi, dt)
    shapes = [[3, 1, 0, 64, 65, 2, 7], [1, 1, 3 * T + 5, 1, 1], [T, T - 1, 1, T + 1]]
    for lengths in shapes:
        starts, n = starts_of(lengths, 2)
        lo, hi = bounds(starts, n)
        for j in np.flatnonzero(hi > lo):
            for at in {int(lo[j]), int(hi[j] - 1)}:
                for special in (np.nan, np.inf, 1e30):
                    x = np.zeros(n, dt)
                    x[at] = special
                    for excl, rev in MODES:
                        got, want = run(capi, x, starts, excl, rev), reference(x, starts, excl, rev)
                        assert bits_equal(got, want), (name(dt), lengths, j, at, special, excl, rev)
                        touched = got != 0
                        assert not np.any(touched[:lo[j]]) and not np.any(touched[hi[j]:])
        # ... and a value in front of the first start reaches nothing
        x = np.zeros(n, dt)
        x[:2] = np.nan
        for excl, rev in MODES:
            assert bits_equal(run(capi, x, starts, excl, rev), np.zeros(n, dt))
    # the same with the gap reaching past the first tile and over a workgroup's whole range
    starts, n = starts_of([5, T, 3], 2 * T + 17)
    x = np.zeros(n, dt)
    x[:2 * T + 17] = np.nan
    for excl, rev in MODES:
        assert bits_equal(run(capi, x, starts, excl, rev), np.zeros(n, dt))


# ---- 4. agreement with the block scan and the segment sum --------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_against_psum_blocks_and_reduce_segments(capi, dt):
    T = tile_of(capi, dt)
    for B, m in ((1, 300), (3, 1000), (64, 257), (1025, 9), (T, 5)):
        starts = (np.arange(m, dtype=np.int64) * B).astype(np.uint32)
        buf, st = capi.Buf.from_numpy(exact_data(dt, m * B, B + m)), capi.Buf.from_numpy(starts)
        for excl, rev in MODES:
            assert bits_equal(capi.psum_segments(buf, st, excl, rev).numpy(), capi.psum_blocks(buf, B, excl, rev).numpy()), (name(dt), B, m, excl, rev)
    for _, lengths, gap in all_mixes(T)[::3]:
        starts, n = starts_of(lengths, gap)
        lo, hi = bounds(starts, n)
        ne = hi > lo
        buf, st = capi.Buf.from_numpy(exact_data(dt, n, n)), capi.Buf.from_numpy(starts)
        sums = capi.reduce_segments("hsum", buf, st).numpy()
        assert bits_equal(capi.psum_segments(buf, st).numpy()[hi[ne] - 1], sums[ne])
        assert bits_equal(capi.psum_segments(buf, st, reverse=True).numpy()[lo[ne]], sums[ne])


# ---- 5. run-to-run identity ------------------------------------------------------------------------------------------------
def test_run_to_run_identity(capi):
    rng = np.random.default_rng(11)
    T = tile_of(capi, np.float32)
    for starts, n in (starts_of([3, 0, 1, 2] * 3000, 1), starts_of([1] * 9 + [10 * T + 5] + [1] * 9), seams_shape(capi, np.float32)):
        buf, st = capi.Buf.from_numpy(rng.standard_normal(n).astype(np.float32)), capi.Buf.from_numpy(starts)
        for excl, rev in MODES:
            runs = [capi.psum_segments(buf, st, excl, rev).numpy() for _ in range(3)]
            assert bits_equal(runs[0], runs[1]) and bits_equal(runs[0], runs[2]), (n, starts.size, excl, rev)


# ---- 6. inside a step graph, replayed with new entries AND new starts --------------------------------------------------------
def test_inside_a_step_graph(capi):
    lib = capi.lib
    rng = np.random.default_rng(13)
    T = tile_of(capi, np.float32)
    shapes = [(3000, 301), (20 * T + 7, 30), (20 * T + 7, 3)]
    assert [plan(capi, np.float32, n, m)[3] for n, m in shapes] == [1, 3, 3]

    def random_starts(n, m):
        return np.sort(rng.integers(5, n + 1, m)).astype(np.uint32)

    def hosts():
        return [(rng.standard_normal(n).astype(np.float32), random_starts(n, m)) for n, m in shapes]
    h1, h2 = hosts(), hosts()
    xs = [capi.Buf.from_numpy(x) for x, _ in h1]
    sts = [capi.Buf.from_numpy(s) for _, s in h1]
    modes = [(False, False), (True, False), (True, True)]
    held = []
    capi.check(lib.ek_hip_graph_begin())
    try:
        held = [capi.psum_segments(x, s, *mode) for x, s, mode in zip(xs, sts, modes)]
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
            eager = [capi.psum_segments(x, s, *mode).numpy() for x, s, mode in zip(xs, sts, modes)]
            for a, b, (hx, hst), mode in zip(replayed, eager, hs, modes):
                assert bits_equal(a, b)
                err = np.abs(a.astype(np.float64) - reference(hx, hst, *mode, acc=np.float64))
                assert np.all(err <= gamma_bound(hx, hst, *mode))
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------
def test_arguments(capi):
    lib = capi.lib
    x = capi.Buf.from_numpy(np.arange(12, dtype=np.float32))
    st = capi.Buf.from_numpy(np.array([0, 3, 3, 10], np.uint32))
    out = capi.Buf.from_numpy(np.full(12, 7, np.float32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    ps = lib.ek_hip_psum_segments
    lib.ek_hip_sync()
    l0 = lib.ek_hip_launch_count()
    assert ps(capi.F32, p(out), p(x), SZ(12), p(st), SZ(4), 4) == -1 and ps(capi.F32, p(out), p(x), SZ(12), p(st), SZ(4), -1) == -1
    assert b"ek_hip_psum_segments" in lib.ek_hip_last_error()
    assert ps(capi.F32, None, p(x), SZ(12), p(st), SZ(4), 0) == -1 and ps(capi.F32, p(out), None, SZ(12), p(st), SZ(4), 0) == -1
    assert ps(capi.F32, p(out), p(x), SZ(12), None, SZ(4), 0) == -1
    assert b"ek_hip_psum_segments" in lib.ek_hip_last_error()
    for bad in (ctypes.c_void_p(out.ptr + 1), ctypes.c_void_p(out.ptr + 2)):
        assert ps(capi.F32, bad, p(x), SZ(8), p(st), SZ(4), 0) == -1
    assert ps(capi.F32, p(out), ctypes.c_void_p(x.ptr + 2), SZ(8), p(st), SZ(4), 0) == -1
    assert ps(capi.F32, p(out), p(x), SZ(12), ctypes.c_void_p(st.ptr + 2), SZ(3), 0) == -1
    assert ps(capi.BOOL, p(out), p(x), SZ(12), p(st), SZ(4), 0) == -2 and ps(99, p(out), p(x), SZ(12), p(st), SZ(4), 0) == -2
    assert ps(capi.F32, p(out), p(x), SZ(1 << 32), p(st), SZ(4), 0) == -2 and b"2^32" in lib.ek_hip_last_error()
    assert ps(capi.F32, p(out), p(x), SZ(12), p(st), SZ(1 << 32), 0) == -2
    assert ps(capi.F32, None, None, SZ(0), None, SZ(0), 0) == 0 and ps(capi.F32, None, None, SZ(0), p(st), SZ(4), 3) == 0       # no entry
    assert lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), np.full(12, 7, np.float32))
    # the calls after refused ones work
    assert ps(capi.F32, p(out), p(x), SZ(12), p(st), SZ(4), 0) == 0
    assert np.array_equal(out.numpy(), [0, 1, 3, 3, 7, 12, 18, 25, 33, 42, 10, 21])
    assert ps(capi.F32, p(out), p(x), SZ(12), p(st), SZ(4), 3) == 0
    assert np.array_equal(out.numpy(), [3, 2, 0, 39, 35, 30, 24, 17, 9, 0, 11, 0])


# ---- 8. bad starts: inside the test's own memory ------------------------------------------------------------------------------
def bad_starts_run(capi, dt, x, starts, excl, rev, pad=256):
    """x and out are views into larger buffers: `pad` sentinel entries on both sides of each"""
    dt = np.dtype(dt)
    poison = dt.type(1e30) if dt.kind == "f" else dt.type(0x5A5A5A5A)
    mark = dt.type(np.nan) if dt.kind == "f" else dt.type(0x3C3C3C3C)
    assert int(starts.max()) <= x.size + pad                      # no bad value leaves the enclosing allocation
    src = capi.Buf.from_numpy(np.concatenate([np.full(pad, poison, dt), x, np.full(pad, poison, dt)]))
    out = capi.Buf.from_numpy(np.full(x.size + 2 * pad, mark, dt))
    st = capi.Buf.from_numpy(starts.astype(np.uint32))
    flags = (capi.SCAN_EXCLUSIVE if excl else 0) | (capi.SCAN_REVERSE if rev else 0)
    capi.check(capi.lib.ek_hip_psum_segments(src.ek, ctypes.c_void_p(out.ptr + pad * dt.itemsize), ctypes.c_void_p(src.ptr + pad * dt.itemsize),
                                             SZ(x.size), ctypes.c_void_p(st.ptr), SZ(starts.size), flags))
    got = out.numpy()
    assert bits_equal(got[:pad], np.full(pad, mark, dt)) and bits_equal(got[pad + x.size:], np.full(pad, mark, dt)), "written outside out"
    assert bits_equal(src.numpy(), np.concatenate([np.full(pad, poison, dt), x, np.full(pad, poison, dt)])), "the input changed"
    return got[pad:pad + x.size]


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_starts_above_n_are_clamped(capi, dt):
    T = tile_of(capi, dt)
    for n, lengths in ((3000, [5, 0, 700, 64, 1, 2000]), (5 * T + 9, [1] * 40 + [3 * T] + [7] * 100), (3 * T, [100, 2 * T + 5])):
        starts, used = starts_of(lengths, 3)
        assert used < n
        # the last few starts lie behind the end of the array: at n, just above it, and up to the end of the enclosing buffer
        above = np.array([n, n, n + 1, n + 1, n + 7, n + 200, n + 256], np.uint32)
        bad = np.concatenate([starts, above])
        x = exact_data(dt, n, n)
        for excl, rev in MODES:
            got = bad_starts_run(capi, dt, x, bad, excl, rev)
            assert bits_equal(got, reference(x, bad, excl, rev)), (name(dt), n, excl, rev, plan(capi, dt, n, bad.size))
    # every start above n: no entry belongs to a segment
    bad = np.array([1001, 1001, 1100, 1256], np.uint32)
    for excl, rev in MODES:
        assert bits_equal(bad_starts_run(capi, dt, exact_data(dt, 1000, 1), bad, excl, rev), np.zeros(1000, dt))


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_decreasing_starts_stay_inside(capi, dt):
    rng = np.random.default_rng(29)
    T = tile_of(capi, dt)
    cases = []
    for n, m in ((5000, 40), (5000, 3), (9 * T + 5, 2500), (9 * T + 5, 4), (30 * T, 700)):
        cases.append((n, rng.integers(0, n + 256, m).astype(np.uint32)))                       # no order at all
        s = np.sort(rng.integers(0, n, m)).astype(np.uint32)
        cases.append((n, s[::-1].copy()))                                                      # strictly the wrong way round
        s[m // 2] = n + 200                                                                    # one value out of line
        cases.append((n, s))
    for n, bad in cases:
        x = rng.integers(-8, 9, n).astype(dt)
        for excl, rev in MODES:
            got = bad_starts_run(capi, dt, x, bad, excl, rev)
            # every entry was written (the float mark is NaN, the integer mark is no possible sum) and holds a sum of entries of x only
            if np.dtype(dt).kind == "f":
                assert np.all(np.isfinite(got)), (name(dt), n, bad.size, excl, rev)
            assert np.all(np.abs(got.astype(np.float64)) <= 8.0 * n), (name(dt), n, bad.size, excl, rev, plan(capi, dt, n, bad.size))
