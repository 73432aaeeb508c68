"""ek_hip_sort_blocks through the C ABI (csrc/block_sort.hip): the stable sort inside every row of B consecutive entries.

Reference.  Per row numpy.argsort(row, kind="stable"); with EK_SORT_DESCENDING numpy.argsort(-row, kind="stable") for floating point
and numpy.argsort(~row, kind="stable") for integers.  numpy's stable argsort puts every NaN (either sign bit, any payload) behind all
numbers in input order and treats -0.0 and +0.0 as equal, which is the contract.  The permutation is compared exactly; the values
are compared as bit patterns against take_along_axis of the reference permutation, so a -0.0, a NaN payload or a denormal that was
rebuilt instead of fetched would show.

Sizes come from ek_hip_sort_blocks_plan with the device's CU count: tile_rows of the packed route, the chunk of the one-workgroup
route, the merge passes of the chunk-and-merge route.  The largest array here has 3 * (5 * chunk + 1) entries, about 120 Ki."""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
SHORT_B = [1, 2, 3, 5, 63, 64, 65, 100, 255, 256, 257, 1000, 1024, 1025]
GUARD = 77


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, n, B):
    """(route, tile_rows, chunk, merge_passes, workgroups)"""
    return capi.sort_blocks_plan(dt, n, B, True, cu_count())


def chunk_of(capi, dt):
    return plan(capi, dt, 4, 2)[2]


def last_packed(capi, dt):
    """the last row length of route 1, found from the plan: the route changes once between 2 and chunk"""
    lo, hi = 2, chunk_of(capi, dt)
    assert plan(capi, dt, lo, lo)[0] == 1 and plan(capi, dt, hi, hi)[0] == 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(capi, dt, mid, mid)[0] == 1:
            lo = mid
        else:
            hi = mid
    return lo


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def from_bits(dt, b):
    dt = np.dtype(dt)
    return np.asarray(b, dtype=np.uint32 if dt.itemsize == 4 else np.uint64).view(dt)


def reference(x2, desc):
    if not desc:
        return np.argsort(x2, axis=1, kind="stable")
    return np.argsort(-x2 if x2.dtype.kind == "f" else ~x2, axis=1, kind="stable")


def random_data(dt, m, B, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, m * B, dtype=dt, endpoint=True)
    # the whole range of finite bit patterns and then some: exponents of every size, both signs
    b = rng.integers(0, 2 ** (8 * dt.itemsize) - 1, m * B, dtype=np.uint64, endpoint=True)
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
        hi = [(h << 32) | 0x12345678 for h in (0, 1, 2, 0x7FFFFFFF)]            # differ only in the high word
        lo = [(0x01234567 << 32) | l for l in (0, 1, 0x80000000, 0xFFFFFFFF)]    # differ only in the low word
        v += hi + lo
        if dt.kind == "u":
            v += [2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 2 ** 64 - 2, (0xFFFFFFFF << 32) | 5]
        else:
            v += [-(h << 32) - 7 for h in (1, 2)]
    return np.array(v, dtype=dt)


PATTERNS = ["random", "equal", "sorted", "reversed", "four", "special"]


def data(dt, m, B, pattern, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if pattern == "random":
        return random_data(dt, m, B, seed)
    if pattern == "equal":
        return np.full(m * B, special_values(dt)[-1] if dt.kind != "f" else -2.5, dt)
    if pattern in ("sorted", "reversed"):
        x = np.sort(random_data(dt, m, B, seed).reshape(m, B), axis=1)
        return np.ascontiguousarray(x[:, ::-1] if pattern == "reversed" else x).reshape(-1)
    if pattern == "four":
        four = special_values(dt)[:4] if dt.kind != "f" else np.array([0.0, -0.0, 2.0, -1.0], dt)
        return four[rng.integers(0, 4, m * B)]
    # special: the type's edge values, every one several times in most rows, mixed into random entries
    sv = special_values(dt)
    x = random_data(dt, m, B, seed)
    pick = rng.random(m * B) < 0.6
    x[pick] = sv[rng.integers(0, sv.size, int(pick.sum()))]
    return x


def run(capi, x, B, desc=False, flat=False, values=True, index=True, in_off=0, v_off=0, i_off=0):
    """the call on views *_off entries behind a 16-byte boundary; the guard entries around both outputs stay untouched"""
    n = x.size
    base = capi.Buf.from_numpy(np.concatenate([np.zeros(in_off, x.dtype), x]))
    src = base.view(in_off, n)
    vbase = capi.Buf.from_numpy(np.full(n + v_off + 1, GUARD, x.dtype)) if values else None
    ibase = capi.Buf.from_numpy(np.full(n + i_off + 1, GUARD, np.uint32)) if index else None
    capi.sort_blocks(src, B, desc, flat, values, index, vbase.view(v_off, n) if values else None, ibase.view(i_off, n) if index else None)
    v = i = None
    if values:
        got = vbase.numpy()
        assert np.all(got[:v_off] == GUARD) and got[-1] == GUARD
        v = got[v_off:-1]
    if index:
        got = ibase.numpy()
        assert np.all(got[:i_off] == GUARD) and got[-1] == GUARD
        i = got[i_off:-1]
    assert np.array_equal(bits(base.numpy()[in_off:]), bits(x))          # the input is left alone
    return v, i


def check(capi, x, m, B, desc=False, flat=False, values=True, index=True, what=None, **where):
    what = (what, name(x.dtype), m, B, desc, flat, values, index, where, plan(capi, x.dtype, m * B, B))
    v, i = run(capi, x, B, desc, flat, values, index, **where)
    x2 = x.reshape(m, B)
    want = reference(x2, desc)
    if index:
        want_i = want + (np.arange(m)[:, None] * B if flat else 0)
        bad = np.argwhere(i.reshape(m, B) != want_i)
        assert bad.size == 0, (what, bad[:4])
    if values:
        want_v = np.take_along_axis(x2, want, axis=1)
        bad = np.argwhere(bits(v).reshape(m, B) != bits(want_v).reshape(m, B))
        assert bad.size == 0, (what, bad[:4])
    return v, i


def row_counts(tile_rows):
    return sorted({1, max(1, tile_rows - 1), tile_rows + 1, 2 * tile_rows + max(1, tile_rows // 2)})


# ---- 1. row lengths and row counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_short_rows(capi, dt):
    lp = last_packed(capi, dt)
    for B in SHORT_B + [lp, lp + 1]:
        route, tile_rows, chunk, passes, _ = plan(capi, dt, 4 * B, B)
        assert route == (0 if B == 1 else 1 if B <= lp else 2) and passes == 0, (B, route)
        counts = row_counts(tile_rows) if route == 1 else [1, 3]
        for m in counts:
            if route == 1:
                assert plan(capi, dt, m * B, B)[4] == -(-m // tile_rows), (B, m)
            for desc in (False, True):
                check(capi, random_data(dt, m, B, B * 7 + m), m, B, desc, flat=bool((B + m + desc) & 1))


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_rows_around_the_chunk_and_beyond(capi, dt):
    c = chunk_of(capi, dt)
    for B, route, passes in ((c - 1, 2, 0), (c, 2, 0), (c + 1, 3, 1), (2 * c + 5, 3, 2), (3 * c, 3, 2), (5 * c + 1, 3, 3)):
        for m in ((1, 3) if B <= 2 * c + 5 else (2,)):
            got = plan(capi, dt, m * B, B)
            assert (got[0], got[3]) == (route, passes), (B, got)
            for desc in (False, True):
                check(capi, random_data(dt, m, B, B + m), m, B, desc, flat=not desc)


def route_shapes(capi, dt):
    """one shape per route 1 .. 3: more than one tile with a partial last one, two rows, an unpaired run with a short tail"""
    c = chunk_of(capi, dt)
    tr = plan(capi, dt, 400, 100)[1]
    return [(tr + 3, 100), (2, 2500), (2, 2 * c + 5)]


# ---- 2. data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS[1:])
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_data_patterns(capi, dt, pattern):
    shapes = route_shapes(capi, dt) + [(5, 3), (3, 64)]
    for m, B in shapes:
        x = data(dt, m, B, pattern, B)
        for desc in (False, True):
            _, i = check(capi, x, m, B, desc, flat=False, what=pattern)
            if pattern == "equal":
                assert np.array_equal(i.reshape(m, B), np.broadcast_to(np.arange(B), (m, B)))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_nans_and_zeros_keep_their_bits_and_their_order(capi, dt):
    sv = special_values(dt)
    for m, B in route_shapes(capi, dt):
        x = data(dt, m, B, "special", 21)
        assert np.isnan(x).sum() > m and (bits(x) == bits(np.array([-0.0], dt))[0]).sum() > m
        for desc in (False, True):
            v, i = check(capi, x, m, B, desc)
            v2, x2 = v.reshape(m, B), x.reshape(m, B)
            nn = np.isnan(x2).sum(axis=1)
            for r in range(m):
                assert np.isnan(v2[r, B - nn[r]:]).all() and not np.isnan(v2[r, :B - nn[r]]).any()
                # the NaNs of the row in input order, payloads and sign bits intact
                assert np.array_equal(bits(v2[r, B - nn[r]:]), bits(x2[r][np.isnan(x2[r])]))
    assert np.isnan(sv).sum() >= 8


# ---- 3. outputs, layouts, alignment ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.uint64, np.int32, np.float64], ids=name)
def test_outputs_and_index_layouts(capi, dt):
    for m, B in route_shapes(capi, dt) + [(4099, 1)]:
        x = data(dt, m, B, "special", 31)
        for desc, flat in itertools.product((False, True), (False, True)):
            for values, index in ((True, True), (True, False), (False, True)):
                check(capi, x, m, B, desc, flat, values, index)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_views_off_a_16_byte_boundary(capi, dt):
    for m, B in route_shapes(capi, dt) + [(plan(capi, dt, 12, 3)[1] + 1, 3), (7, 1)]:
        x = data(dt, m, B, "special", 41)
        for where in (dict(in_off=1), dict(in_off=3), dict(v_off=1), dict(v_off=3), dict(i_off=1), dict(i_off=3), dict(in_off=1, v_off=3, i_off=1)):
            check(capi, x, m, B, desc=bool(where.get("in_off", 0) & 2), flat=True, **where)


def test_overlapping_arguments_are_refused(capi):
    lib = capi.lib
    sb = lib.ek_hip_sort_blocks
    p = lambda b, off=0: ctypes.c_void_p(b.ptr + off)
    n, B = 24, 3
    x = capi.Buf.from_numpy(np.arange(2 * n, dtype=np.float32))
    v = capi.Buf.from_numpy(np.full(2 * n, 7, np.float32))
    i = capi.Buf.from_numpy(np.full(2 * n, 7, np.uint32))
    l0 = lib.ek_hip_launch_count()
    assert sb(capi.F32, p(x), p(i), p(x), SZ(n), SZ(B), 0) == -1 and b"ek_hip_sort_blocks" in lib.ek_hip_last_error()
    assert sb(capi.F32, p(x, 4 * (n - 1)), p(i), p(x), SZ(n), SZ(B), 0) == -1          # the last entry of in is the first of out
    assert sb(capi.F32, p(v), p(x, 4), p(x), SZ(n), SZ(B), 0) == -1                     # the index overlaps in
    assert sb(capi.F32, None, p(x), p(x), SZ(n), SZ(B), 0) == -1
    assert sb(capi.F32, p(v), p(v, 4 * (n - 1)), p(x), SZ(n), SZ(B), 0) == -1           # the two outputs overlap
    assert sb(capi.F32, p(x, 4 * n), p(i), p(x), SZ(n), SZ(B), 0) == 0                  # adjacent is fine
    # other arguments
    assert sb(capi.F32, None, None, p(x), SZ(n), SZ(B), 0) == -1 and b"ek_hip_sort_blocks" in lib.ek_hip_last_error()
    assert sb(capi.F32, p(v), p(i), p(x), SZ(n), SZ(0), 0) == -1
    assert sb(capi.F32, p(v), p(i), p(x), SZ(n), SZ(5), 0) == -1
    assert sb(capi.F32, p(v), p(i), None, SZ(n), SZ(B), 0) == -1
    assert sb(capi.F32, p(v), p(i), p(x), SZ(n), SZ(B), 4) == -1
    assert sb(capi.BOOL, p(v), p(i), p(x), SZ(n), SZ(B), 0) == -2
    l1 = lib.ek_hip_launch_count()
    assert sb(capi.F32, p(v), None, None, SZ(0), SZ(B), 0) == 0 and lib.ek_hip_launch_count() == l1
    assert np.all(v.numpy() == 7) and np.all(i.numpy()[n:] == 7)
    assert l1 - l0 == 1
    assert sb(capi.F32, p(v), p(i), p(x), SZ(n), SZ(B), 3) == 0
    assert np.array_equal(v.numpy()[:6], [2, 1, 0, 5, 4, 3]) and np.array_equal(i.numpy()[:6], [2, 1, 0, 5, 4, 3])


# ---- 4. reproducibility, step graphs, launches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_two_calls_agree_bit_for_bit(capi, dt):
    seen = set()
    for m, B in route_shapes(capi, dt) + [(4099, 1)]:
        seen.add(plan(capi, dt, m * B, B)[0])
        src = capi.Buf.from_numpy(data(dt, m, B, "special", 51))
        for desc in (False, True):
            a = capi.sort_blocks(src, B, desc, True)
            b = capi.sort_blocks(src, B, desc, True)
            assert np.array_equal(bits(a[0].numpy()), bits(b[0].numpy())) and np.array_equal(a[1].numpy(), b[1].numpy()), (m, B, desc)
    assert seen == {0, 1, 2, 3}


def test_inside_a_step_graph(capi):
    lib = capi.lib
    lib.ek_hip_graph_launch_count.restype = ctypes.c_uint64
    lib.ek_hip_graph_launch_count.argtypes = [ctypes.c_void_p]
    dt = np.float32
    c = chunk_of(capi, dt)
    (m1, B1), (m3, B3) = (plan(capi, dt, 400, 100)[1] + 3, 100), (2, 2 * c + 5)
    passes = plan(capi, dt, m3 * B3, B3)[3]
    assert plan(capi, dt, m1 * B1, B1)[0] == 1 and plan(capi, dt, m3 * B3, B3)[0] == 3 and passes == 2
    h1 = [data(dt, m1, B1, "special", 61), data(dt, m1, B1, "random", 62)]
    h3 = [data(dt, m3, B3, "special", 63), data(dt, m3, B3, "random", 64)]
    s1, s3 = capi.Buf.from_numpy(h1[0]), capi.Buf.from_numpy(h3[0])
    capi.check(lib.ek_hip_graph_begin())
    try:
        o1 = capi.sort_blocks(s1, B1, False, True)
        o3 = capi.sort_blocks(s3, B3, True, False)
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        # route 1: one launch; route 3: the chunk launch and one launch per merge pass, no fill launch
        assert lib.ek_hip_graph_launch_count(g) == 1 + (1 + passes)
        for a, b in zip(h1, h3):
            for buf, h in ((s1, a), (s3, b)):
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr), h.ctypes.data_as(ctypes.c_void_p), SZ(h.nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            for (v, i), h, m, B, desc, flat in ((o1, a, m1, B1, False, True), (o3, b, m3, B3, True, False)):
                want = reference(h.reshape(m, B), desc)
                assert np.array_equal(i.numpy().reshape(m, B), want + (np.arange(m)[:, None] * B if flat else 0))
                assert np.array_equal(bits(v.numpy()).reshape(m, B), bits(np.take_along_axis(h.reshape(m, B), want, axis=1)))
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))
