"""ek_hip_sort_segments through the C ABI (csrc/segment_sort.hip): the stable sort inside ragged segments.

Reference.  Per clamped segment [lo_j, hi_j) numpy.argsort(segment, kind="stable"); with EK_SORT_DESCENDING numpy.argsort(-segment)
for floating point and numpy.argsort(~segment) for integers.  Entries in front of min(starts[0], n) stay where they are and report
their own position in both index modes.  Permutations are compared exactly, values as bit patterns against a gather of the input
through the reference permutation, so a -0.0, a NaN payload or a denormal that was rebuilt instead of fetched would show.

The tile size T comes from ek_hip_sort_segments_plan with the device's CU count; the largest array here has 16 T entries."""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
PATTERNS = ["random", "equal", "sorted", "reversed", "four", "special"]
SZ = ctypes.c_size_t
GUARD = 77


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, n, m):
    """(tile, tiles, tiles_per_workgroup, workgroups, merges, merge_workgroups, launches, scratch_bytes)"""
    return capi.sort_segments_plan(dt, n, m, True, cu_count())


def tile_of(capi, dt):
    return plan(capi, dt, 10, 1)[0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def from_bits(dt, b):
    dt = np.dtype(dt)
    return np.asarray(b, dtype=np.uint32 if dt.itemsize == 4 else np.uint64).view(dt)


def random_data(dt, n, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    # the whole range of finite bit patterns and then some: exponents of every size, both signs
    b = rng.integers(0, 2 ** (8 * dt.itemsize) - 1, n, dtype=np.uint64, endpoint=True)
    x = from_bits(dt, b.astype(np.uint32) if dt.itemsize == 4 else b).copy()
    x[np.isnan(x)] = 1.5
    return x


def special_values(dt):
    dt = np.dtype(dt)
    if dt == np.float32:
        nans = from_bits(dt, [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC00002, 0x7F800001, 0xFF800003, 0x7FFFFFFF, 0xFFFFFFFF])
        rest = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0, 3.4e38, -3.4e38], dt)
        return np.concatenate([nans, rest, rest[:2], rest[:2]])
    if dt == np.float64:
        nans = from_bits(dt, [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF8000000000002, 0x7FF0000000000001,
                              0xFFF0000000000003, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FF0000100000000, 0xFFF0000100000000])
        rest = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, 1.0, -1.0, 1.7e308, -1.7e308], dt)
        return np.concatenate([nans, rest, rest[:2], rest[:2]])
    info = np.iinfo(dt)
    v = [info.min, info.max, info.min + 1, info.max - 1, 0, 1, info.max // 2, info.max // 2 + 1]
    if dt.kind == "i":
        v += [-1, -2]
    if dt.itemsize == 8:
        v += [(h << 32) | 0x12345678 for h in (0, 1, 2, 0x7FFFFFFF)]            # differ only in the high word
        v += [(0x01234567 << 32) | l for l in (0, 1, 0x80000000, 0xFFFFFFFF)]    # differ only in the low word
        if dt.kind == "u":
            v += [2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 2 ** 64 - 2, (0xFFFFFFFF << 32) | 5]
        else:
            v += [-(h << 32) - 7 for h in (1, 2)]
    return np.array(v, dtype=dt)


def data(dt, n, pattern, seed):
    """the data patterns of test_block_sort_gpu.py over a flat array"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if pattern == "random":
        return random_data(dt, n, seed)
    if pattern == "equal":
        return np.full(n, special_values(dt)[-1] if dt.kind != "f" else -2.5, dt)
    if pattern in ("sorted", "reversed"):
        x = np.sort(random_data(dt, n, seed))
        return np.ascontiguousarray(x[::-1] if pattern == "reversed" else x)
    if pattern == "four":
        four = special_values(dt)[:4] if dt.kind != "f" else np.array([0.0, -0.0, 2.0, -1.0], dt)
        return four[rng.integers(0, 4, n)]
    sv = special_values(dt)
    x = random_data(dt, n, seed)
    pick = rng.random(n) < 0.6
    x[pick] = sv[rng.integers(0, sv.size, int(pick.sum()))]
    return x


def reference(x, starts, desc):
    """(flat, local) permutations for ascending starts: numpy's stable argsort per clamped segment, identity in front of starts[0]"""
    n = x.size
    flat = np.arange(n, dtype=np.int64)
    local = np.arange(n, dtype=np.int64)
    lo = np.minimum(np.asarray(starts, dtype=np.int64), n)
    hi = np.maximum(lo, np.append(lo[1:], n))
    key = x if not desc else (-x if x.dtype.kind == "f" else ~x)
    for a, b in zip(lo, hi):
        if b - a == 1:
            local[a] = 0
        elif b > a:
            p = np.argsort(key[a:b], kind="stable")
            flat[a:b] = a + p
            local[a:b] = p
    return flat, local


def run(capi, x, starts, desc=False, flat=False, values=True, index=True, in_off=0, v_off=0, i_off=0, fill=GUARD):
    """the call on views *_off entries behind a 16-byte boundary; the guard entries around both outputs stay untouched"""
    n = x.size
    base = capi.Buf.from_numpy(np.concatenate([np.zeros(in_off, x.dtype), x]))
    src = base.view(in_off, n)
    sb = capi.Buf.from_numpy(np.asarray(starts, dtype=np.uint32))
    vbase = capi.Buf.from_numpy(from_bits(x.dtype, np.full(n + v_off + 1, fill))) if values else None
    ibase = capi.Buf.from_numpy(np.full(n + i_off + 1, fill, np.uint32)) if index else None
    capi.sort_segments(src, sb, desc, flat, values, index, vbase.view(v_off, n) if values else None, ibase.view(i_off, n) if index else None)
    v = i = None
    if values:
        got = bits(vbase.numpy())
        assert np.all(got[:v_off] == fill) and got[-1] == fill
        v = got[v_off:-1]
    if index:
        got = ibase.numpy()
        assert np.all(got[:i_off] == fill) and got[-1] == fill
        i = got[i_off:-1]
    assert np.array_equal(bits(base.numpy()[in_off:]), bits(x))          # the input is left alone
    assert np.array_equal(sb.numpy(), np.asarray(starts, dtype=np.uint32))
    return v, i


def check(capi, x, starts, desc=False, flat=False, values=True, index=True, what=None, **where):
    what = (what, name(x.dtype), x.size, len(starts), desc, flat, values, index, where)
    v, i = run(capi, x, starts, desc, flat, values, index, **where)
    want_flat, want_local = reference(x, starts, desc)
    if index:
        bad = np.flatnonzero(i != (want_flat if flat else want_local))
        assert bad.size == 0, (what, bad[:4], i[bad[:4]])
    if values:
        bad = np.flatnonzero(v != bits(x[want_flat]))
        assert bad.size == 0, (what, bad[:4])
    return v, i


def short_segments(n, seed):
    """random lengths 0 .. 70 with empty segments, starts[0] > 0 and starts above n"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 71, n // 20)
    lens[rng.random(lens.size) < 0.15] = 0
    s = 37 + np.concatenate([[0], np.cumsum(lens)])
    s = s[s < n + 300]
    assert s[0] > 0 and (s > n).sum() >= 2 and (np.diff(s) == 0).sum() >= 5
    return s


# ---- 1. everything inside tiles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_short_segments_in_every_type_and_pattern(capi, dt, pattern):
    n = 5003
    starts = short_segments(n, 5)
    assert plan(capi, dt, n, len(starts))[1] == 3
    x = data(dt, n, pattern, 11)
    for desc in (False, True):
        check(capi, x, starts, desc, flat=desc, what=pattern)


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------------------
def edge_cases(T):
    singles = list(range(0, 3 * T - 1)) + [3 * T - 1] + list(range(11 * T + 2, 16 * T))
    return {
        "ends at T": (T + 100, [0, 10, T - 30, T, T + 40]),
        "starts at T": (2 * T, [5, T, 2 * T - 1]),
        "[T - 1, T + 1)": (T + 50, [0, T - 1, T + 1]),
        "[T - 1, 4T + 2)": (5 * T, [3, T - 1, 4 * T + 2, 4 * T + 2, 5 * T - 1]),
        "[5T + 7, 6T + 9) in 8T": (8 * T, [0, 100, 5 * T + 7, 6 * T + 9, 7 * T]),
        "one segment of 5T + 1": (5 * T + 1, [0]),
        "8T + 3 at 3T - 1 among singles in 16T": (16 * T, singles),
    }


@pytest.mark.parametrize("pattern", ["random", "equal", "four"])
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_segments_across_tile_edges(capi, dt, pattern):
    T = tile_of(capi, dt)
    for what, (n, starts) in edge_cases(T).items():
        tiles, merges = plan(capi, dt, n, len(starts))[1], plan(capi, dt, n, len(starts))[4]
        assert tiles == -(-n // T) and merges == int(np.ceil(np.log2(tiles))), (what, tiles, merges)
        x = data(dt, n, pattern, n % 97)
        for desc in (False, True):
            check(capi, x, starts, desc, flat=not desc, what=(what, pattern))


# ---- 3. outputs, layouts, alignment ----------------------------------------------------------------------------------------------
def mixed_shape(T):
    """long and short segments, a prefix, empty segments, starts above n"""
    n = 6 * T + 13
    starts = [9, 40, 40, 700, T - 1, T + 1, 2 * T + 5, 2 * T + 6, 5 * T + 100, 5 * T + 100, 6 * T, 6 * T + 12, n + 5, n + 9]
    return n, starts


@pytest.mark.parametrize("dt", [np.float32, np.uint64, np.int32, np.float64], ids=name)
def test_outputs_and_index_layouts(capi, dt):
    T = tile_of(capi, dt)
    for n, starts in (mixed_shape(T), (5003, short_segments(5003, 6))):
        x = data(dt, n, "special", 31)
        for desc, flat in itertools.product((False, True), (False, True)):
            for values, index in ((True, True), (True, False), (False, True)):
                check(capi, x, starts, desc, flat, values, index)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_views_off_a_16_byte_boundary(capi, dt):
    T = tile_of(capi, dt)
    for n, starts in (mixed_shape(T), (5003, short_segments(5003, 7))):
        x = data(dt, n, "special", 41)
        for where in (dict(in_off=1), dict(in_off=3), dict(v_off=1), dict(v_off=3), dict(i_off=1), dict(i_off=3), dict(in_off=1, v_off=3, i_off=1)):
            check(capi, x, starts, desc=bool(where.get("in_off", 0) & 2), flat=bool(where.get("i_off", 0) & 2), **where)


# ---- 4. no segments, more segments than entries, the prefix -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_no_segments_many_segments_and_the_prefix(capi, dt):
    T = tile_of(capi, dt)
    n = 2 * T + 77
    x = data(dt, n, "special", 51)
    for desc, flat in itertools.product((False, True), (False, True)):
        # m == 0: the whole array is a prefix
        v, i = check(capi, x, [], desc, flat)
        assert np.array_equal(i, np.arange(n)) and np.array_equal(v, bits(x))
        # m > n with many equal starts
        starts = np.sort(np.concatenate([np.full(n, 300), np.full(n // 2, T + 5), [120, 2 * T, 2 * T + 70, n, n + 1]]))
        assert len(starts) > n
        v, i = check(capi, x, starts, desc, flat)
        assert np.array_equal(i[:120], np.arange(120)) and np.array_equal(v[:120], bits(x)[:120])
        # starts[0] behind the array: nothing moves
        v, i = check(capi, x, [n + 3, n + 4], desc, flat)
        assert np.array_equal(i, np.arange(n)) and np.array_equal(v, bits(x))
    # a prefix longer than a tile
    check(capi, x, [T + 9, T + 500], True, False)
    check(capi, x, [T + 9, T + 500], False, True)


# ---- 5. bad starts: only the contract ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_bad_starts_keep_the_contract(capi, dt):
    T = tile_of(capi, dt)
    n = 6 * T + 13
    rng = np.random.default_rng(61)
    x = rng.integers(-50, 50, n).astype(dt)                       # (the data never hold the sentinel)
    sentinel = 0xDEADBEEF
    assert not np.any(bits(x) == sentinel)
    dec = np.arange(n + 40, 0, -7)
    bad = {
        "decreasing": dec,
        "decreasing, few": np.array([5 * T, 3 * T + 1, T - 1, 2]),
        "random": rng.integers(0, 2 ** 32, 3000, dtype=np.uint64),
        "random below n": rng.integers(0, n, 500, dtype=np.uint64),
        "saw": np.tile(np.array([0, 4 * T + 3, T + 1, 5 * T]), 50),
    }
    for what, starts in bad.items():
        for desc, flat in itertools.product((False, True), (False, True)):
            v, i = run(capi, x, starts, desc, flat, fill=sentinel)         # (returns OK and checks the guards)
            assert not np.any(v == sentinel), (what, desc, flat, np.flatnonzero(v == sentinel)[:4])
            assert not np.any(i == sentinel), (what, desc, flat, np.flatnonzero(i == sentinel)[:4])
            assert i.max() < n, (what, desc, flat, i.max())
        for values, index in ((True, False), (False, True)):
            v, i = run(capi, x, starts, False, True, values, index, fill=sentinel)
            got = v if values else i
            assert not np.any(got == sentinel), (what, values, index)


# ---- 6. uniform segments are blocks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_uniform_segments_equal_block_sort_bit_for_bit(capi, dt):
    T = tile_of(capi, dt)
    for B in (1, 64, 100, 2048, 2049, 3 * T + 5):
        m = max(2, min(16 * T // B, 3000))
        n = m * B
        assert n <= 16 * T
        x = data(dt, n, "special", B)
        src, sb = capi.Buf.from_numpy(x), capi.Buf.from_numpy((np.arange(m) * B).astype(np.uint32))
        for desc, flat in itertools.product((False, True), (False, True)):
            v, i = capi.sort_segments(src, sb, desc, flat)
            bv, bi = capi.sort_blocks(src, B, desc, flat)
            assert np.array_equal(bits(v.numpy()), bits(bv.numpy())), (B, desc, flat)
            assert np.array_equal(i.numpy(), bi.numpy()), (B, desc, flat)


# ---- 7. reproducibility, step graphs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_two_calls_agree_bit_for_bit(capi, dt):
    T = tile_of(capi, dt)
    for n, starts in (mixed_shape(T), edge_cases(T)["8T + 3 at 3T - 1 among singles in 16T"]):
        src, sb = capi.Buf.from_numpy(data(dt, n, "special", 71)), capi.Buf.from_numpy(np.asarray(starts, np.uint32))
        for desc in (False, True):
            a = capi.sort_segments(src, sb, desc, True)
            b = capi.sort_segments(src, sb, desc, True)
            assert np.array_equal(bits(a[0].numpy()), bits(b[0].numpy())) and np.array_equal(a[1].numpy(), b[1].numpy()), (n, desc)


@pytest.mark.parametrize("first", ["short", "whole"])
def test_a_captured_call_replays_with_other_starts(capi, first):
    """the number of merge passes that the data need is decided on the device: a graph captured with all-short segments sorts one
    whole-array segment on replay, and the other way round"""
    lib = capi.lib
    lib.ek_hip_graph_launch_count.restype = ctypes.c_uint64
    lib.ek_hip_graph_launch_count.argtypes = [ctypes.c_void_p]
    dt = np.float32
    T = tile_of(capi, dt)
    n, m = 8 * T + 3, 400
    short = np.minimum(np.arange(m) * ((n + m - 1) // m), n).astype(np.uint32)
    whole = np.full(m, n, np.uint32)
    whole[0] = 0
    assert np.diff(short.astype(np.int64)).max() < T // 2
    order = [short, whole] if first == "short" else [whole, short]
    xs = [data(dt, n, "special", 81), data(dt, n, "four", 82)]
    src, sb = capi.Buf.from_numpy(xs[0]), capi.Buf.from_numpy(order[0])
    capi.check(lib.ek_hip_graph_begin())
    try:
        v, i = capi.sort_segments(src, sb, False, True)
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        assert lib.ek_hip_graph_launch_count(g) == plan(capi, dt, n, m)[6] == 2 + 4
        for starts, x in ((order[0], xs[0]), (order[1], xs[1]), (order[0], xs[1])):
            for buf, h in ((src, x), (sb, starts)):
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr), h.ctypes.data_as(ctypes.c_void_p), SZ(h.nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            want, _ = reference(x, starts, False)
            assert np.array_equal(i.numpy(), want)
            assert np.array_equal(bits(v.numpy()), bits(x[want]))
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))


# ---- 8. arguments ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_refused(capi):
    lib = capi.lib
    ss = lib.ek_hip_sort_segments
    p = lambda b, off=0: ctypes.c_void_p(b.ptr + off)
    n, m = 24, 3
    x = capi.Buf.from_numpy(np.arange(2 * n, dtype=np.float32))
    v = capi.Buf.from_numpy(np.full(2 * n, 7, np.float32))
    i = capi.Buf.from_numpy(np.full(2 * n, 7, np.uint32))
    s = capi.Buf.from_numpy(np.array([0, 8, 16, 0], np.uint32))
    l0 = lib.ek_hip_launch_count()
    assert ss(capi.F32, p(v), p(i), p(x), SZ(n), p(s), SZ(m), 4) == -1 and b"ek_hip_sort_segments" in lib.ek_hip_last_error()   # unknown flag
    assert ss(capi.F32, None, None, p(x), SZ(n), p(s), SZ(m), 0) == -1                      # no output
    assert ss(capi.F32, p(x), p(i), p(x), SZ(n), p(s), SZ(m), 0) == -1                      # out is in
    assert ss(capi.F32, p(x, 4 * (n - 1)), p(i), p(x), SZ(n), p(s), SZ(m), 0) == -1         # the last entry of in is the first of out
    assert ss(capi.F32, p(v), p(x, 4), p(x), SZ(n), p(s), SZ(m), 0) == -1                   # the index overlaps in
    assert ss(capi.F32, p(v), p(v, 4 * (n - 1)), p(x), SZ(n), p(s), SZ(m), 0) == -1         # the two outputs overlap
    assert ss(capi.F32, p(v, 2), p(i), p(x), SZ(n), p(s), SZ(m), 0) == -1                   # misaligned pointers
    assert ss(capi.F32, p(v), p(i, 2), p(x), SZ(n), p(s), SZ(m), 0) == -1
    assert ss(capi.F32, p(v), p(i), p(x, 1), SZ(n), p(s), SZ(m), 0) == -1
    assert ss(capi.F32, p(v), p(i), p(x), SZ(n), p(s, 2), SZ(m), 0) == -1
    assert ss(capi.F32, p(v), p(i), None, SZ(n), p(s), SZ(m), 0) == -1                      # null pointers
    assert ss(capi.F32, p(v), p(i), p(x), SZ(n), None, SZ(m), 0) == -1
    assert ss(capi.BOOL, p(v), p(i), p(x), SZ(n), p(s), SZ(m), 0) == -2
    assert ss(capi.F32, p(v), p(i), p(x), SZ(2 ** 32), p(s), SZ(m), 0) == -2
    assert ss(capi.F32, p(v), p(i), p(x), SZ(n), p(s), SZ(2 ** 32), 0) == -2
    assert ss(capi.F32, p(v), None, None, SZ(0), None, SZ(m), 0) == 0                       # no entries: no call
    assert lib.ek_hip_launch_count() == l0
    assert np.all(v.numpy() == 7) and np.all(i.numpy() == 7)
    assert ss(capi.F32, p(x, 4 * n), p(i), p(x), SZ(n), p(s), SZ(m), 3) == 0                # adjacent is fine
    assert np.array_equal(x.numpy()[n:n + 9], [7, 6, 5, 4, 3, 2, 1, 0, 15]) and np.array_equal(i.numpy()[:9], [7, 6, 5, 4, 3, 2, 1, 0, 15])
    assert lib.ek_hip_launch_count() == l0 + 1
