"""ek_hip_sort through the C ABI (csrc/sort.hip): the stable sort of a whole array, on its radix route (tuning "sort_radix" = 2).

Reference.  numpy.argsort(x, kind="stable"); with EK_SORT_DESCENDING numpy.argsort(-x, kind="stable") for floating point and
numpy.argsort(~x, kind="stable") for integers.  numpy's stable argsort puts every NaN (either sign bit, any payload) behind all
numbers in input order and treats -0.0 and +0.0 as equal, which is the contract.  The permutation is compared exactly; the values
are compared as bit patterns against x[reference], so a -0.0, a NaN payload or a denormal that was rebuilt from its key instead of
fetched would show.

Sizes come from ek_hip_sort_plan with the device's CU count: T is the plan's tile; 3 T + 7 entries put several workgroups and a
partial last tile behind the scans; one shape per element size has two tiles per workgroup."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
GUARD = 77
TRIVIAL, FORWARDED, RADIX = range(3)


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def radix(capi):
    """every n >= 2 takes the radix route; the automatic mode comes back afterwards"""
    capi.set_tuning("sort_radix", 2)
    try:
        yield capi
    finally:
        capi.set_tuning("sort_radix", 1)


def plan(capi, dt, n):
    """(route, passes, tile, tiles_per_workgroup, workgroups, launches, scratch_bytes)"""
    return capi.sort_plan(dt, n, True, cu_count())


def tile_of(capi, dt):
    return plan(capi, dt, 2)[2]


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


def reference(x, desc):
    if not desc:
        return np.argsort(x, kind="stable")
    return np.argsort(-x if x.dtype.kind == "f" else ~x, kind="stable")


def run(capi, x, desc=False, values=True, index=True, in_off=0, v_off=0, i_off=0, flags=None):
    """the call on views *_off entries behind a 16-byte boundary; the guard entries around both outputs stay untouched"""
    n = x.size
    base = capi.Buf.from_numpy(np.concatenate([np.zeros(in_off, x.dtype), x]))
    src = base.view(in_off, n)
    vbase = capi.Buf.from_numpy(np.full(n + v_off + 1, GUARD, x.dtype)) if values else None
    ibase = capi.Buf.from_numpy(np.full(n + i_off + 1, GUARD, np.uint32)) if index else None
    capi.sort(src, desc, values, index, vbase.view(v_off, n) if values else None, ibase.view(i_off, n) if index else None, flags)
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


def check(capi, x, desc=False, values=True, index=True, what=None, want=None, **where):
    what = (what, name(x.dtype), x.size, desc, values, index, where, plan(capi, x.dtype, x.size))
    v, i = run(capi, x, desc, values, index, **where)
    if want is None:
        want = reference(x, desc)
    if index:
        bad = np.flatnonzero(i != want)
        assert bad.size == 0, (what, bad[:4], i[bad[:4]], want[bad[:4]])
    if values:
        bad = np.flatnonzero(bits(v) != bits(x[want]))
        assert bad.size == 0, (what, bad[:4])
    return v, i


# ---- 1. sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_sizes_around_the_tile(radix, dt):
    T = tile_of(radix, dt)
    assert T in (4096, 8192)
    for n in (2, 3, 63, 64, 65, 511, 513, T - 1, T, T + 1, 2 * T + 5, 3 * T + 7):
        route, passes, tile, per, wgs, launches, _ = plan(radix, dt, n)
        assert route == RADIX and passes == np.dtype(dt).itemsize and tile == T and per == 1 and wgs == -(-n // T)
        x = random_data(dt, n, n)
        for desc in (False, True):
            check(radix, x, desc)
    assert plan(radix, dt, 3 * T + 7)[4] == 4        # several workgroups, the last tile partial


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_one_byte_differs(radix, dt):
    """256 random values shifted into byte b, every other byte equal: pass b alone decides the order"""
    dt = np.dtype(dt)
    n = tile_of(radix, dt) + 1
    rng = np.random.default_rng(5)
    U = np.uint32 if dt.itemsize == 4 else np.uint64
    # (the other bytes: a pattern that is a finite number of either float type with any byte replaced)
    rest = U(0x3A5B6C1D) if dt.itemsize == 4 else U(0x3A5B6C1D2E4F5061)
    for b in range(dt.itemsize):
        digit = rng.integers(0, 256, n).astype(U)
        word = (rest & ~(U(0xFF) << U(8 * b))) | (digit << U(8 * b))
        x = from_bits(dt, word).copy()
        if dt.kind == "f":
            assert not np.isnan(x).any()
        assert np.unique(bits(x) >> U(8 * b) & U(0xFF)).size > 200 and np.unique(bits(x) & ~(U(0xFF) << U(8 * b))).size == 1
        for desc in (False, True):
            check(radix, x, desc, what=("byte", b))


# ---- 2. data -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["equal", "sorted", "reversed", "four", "special"])
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_data_patterns(radix, dt, pattern):
    n = 3 * tile_of(radix, dt) + 7
    x = data(dt, n, pattern, 11)
    for desc in (False, True):
        _, i = check(radix, x, desc, what=pattern)
        if pattern == "equal":
            assert np.array_equal(i, np.arange(n))               # stable across waves, tiles and workgroups
        if pattern == "four":
            # inside every run of equal keys the positions ascend
            k = x[i]
            same = k[1:] == k[:-1]
            assert np.all(i[1:][same] > i[:-1][same])


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_nans_and_zeros_keep_their_bits_and_their_order(radix, dt):
    n = 3 * tile_of(radix, dt) + 7
    x = data(dt, n, "special", 21)
    nn = int(np.isnan(x).sum())
    neg_zero, pos_zero = bits(np.array([-0.0], dt))[0], bits(np.array([0.0], dt))[0]
    assert nn > 100 and (bits(x) == neg_zero).sum() > 100 and (bits(x) == pos_zero).sum() > 100
    assert np.isnan(special_values(dt)).sum() >= 8
    for desc in (False, True):
        v, i = check(radix, x, desc)
        assert np.isnan(v[n - nn:]).all() and not np.isnan(v[:n - nn]).any()
        # the NaNs in input order, payloads and sign bits intact
        assert np.array_equal(bits(v[n - nn:]), bits(x[np.isnan(x)])) and np.array_equal(i[n - nn:], np.flatnonzero(np.isnan(x)))
        # both zeros are there, one run, in input order, every one with its own sign bit
        z = np.flatnonzero(v == 0)
        assert z.size == (x == 0).sum() and np.all(np.diff(z) == 1)
        assert np.array_equal(bits(v[z]), bits(x[x == 0])) and {neg_zero, pos_zero} <= set(bits(v[z]).tolist())


# ---- 3. outputs, alignment, refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.uint64, np.int32, np.float64], ids=name)
def test_values_only_index_only_and_both(radix, dt):
    T = tile_of(radix, dt)
    for n in (T + 1, 3 * T + 7):
        x = data(dt, n, "special", 31)
        for desc in (False, True):
            want = reference(x, desc)
            for values, index in ((True, True), (True, False), (False, True)):
                check(radix, x, desc, values, index, want=want)
    # EK_SORT_FLAT_INDEX is accepted and changes nothing
    x = data(dt, T + 1, "random", 32)
    a = run(radix, x, flags=radix.SORT_FLAT_INDEX | radix.SORT_DESCENDING)
    b = run(radix, x, desc=True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[1], reference(x, True))


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_views_off_a_16_byte_boundary(radix, dt):
    n = tile_of(radix, dt) + 1
    x = data(dt, n, "special", 41)
    wants = {d: reference(x, d) for d in (False, True)}
    for where in (dict(in_off=1), dict(in_off=3), dict(v_off=1), dict(v_off=3), dict(i_off=1), dict(i_off=3), dict(in_off=1, v_off=3, i_off=1)):
        desc = bool(where.get("in_off", 0) & 2)
        check(radix, x, desc, want=wants[desc], **where)


def test_refusals_launch_nothing(radix):
    capi = radix
    lib = capi.lib
    so = lib.ek_hip_sort
    p = lambda b, off=0: ctypes.c_void_p(b.ptr + off)
    n = 24
    x = capi.Buf.from_numpy(np.arange(2 * n, dtype=np.float32)[::-1].copy())
    v = capi.Buf.from_numpy(np.full(2 * n, 7, np.float32))
    i = capi.Buf.from_numpy(np.full(2 * n, 7, np.uint32))
    l0 = lib.ek_hip_launch_count()
    # overlap
    assert so(capi.F32, p(x), p(i), p(x), SZ(n), 0) == -1 and b"ek_hip_sort()" in lib.ek_hip_last_error()
    assert so(capi.F32, p(x, 4 * (n - 1)), p(i), p(x), SZ(n), 0) == -1          # the last entry of in is the first of out
    assert so(capi.F32, p(v), p(x, 4), p(x), SZ(n), 0) == -1                     # the index overlaps in
    assert so(capi.F32, None, p(x), p(x), SZ(n), 0) == -1
    assert so(capi.F32, p(v), p(v, 4 * (n - 1)), p(x), SZ(n), 0) == -1           # the two outputs overlap
    # other arguments
    assert so(capi.F32, None, None, p(x), SZ(n), 0) == -1 and b"ek_hip_sort()" in lib.ek_hip_last_error()
    assert so(capi.F32, p(v), p(i), None, SZ(n), 0) == -1
    assert so(capi.F32, p(v), p(i), p(x), SZ(n), 4) == -1 and so(capi.F32, p(v), p(i), p(x), SZ(n), 8 | 1) == -1
    assert so(capi.F32, p(v, 2), p(i), p(x), SZ(n), 0) == -1 and so(capi.F32, p(v), p(i, 2), p(x), SZ(n), 0) == -1
    assert so(capi.F32, p(v), p(i), p(x, 1), SZ(n), 0) == -1 and so(capi.F64, p(v, 4), p(i), p(x), SZ(n // 2), 0) == -1
    assert so(capi.BOOL, p(v), p(i), p(x), SZ(n), 0) == -2 and so(99, p(v), p(i), p(x), SZ(n), 0) == -2
    assert so(capi.F32, p(v), p(i), p(x), SZ(2 ** 32), 0) == -2 and b"2^32 - 1" in lib.ek_hip_last_error()
    # no entries: nothing to do, pointers or not
    assert so(capi.F32, p(v), None, None, SZ(0), 0) == 0 and so(capi.F32, p(v), p(i), p(x), SZ(0), 1) == 0
    assert lib.ek_hip_launch_count() == l0
    assert np.all(v.numpy() == 7) and np.all(i.numpy() == 7)
    # adjacent buffers are fine: the output begins where the input ends
    assert so(capi.F32, p(x, 4 * n), p(i), p(x), SZ(n), 0) == 0
    assert lib.ek_hip_launch_count() - l0 == plan(capi, np.float32, n)[5]
    got = x.numpy()
    assert np.array_equal(got[n:], got[:n][::-1]) and np.array_equal(i.numpy()[:n], np.arange(n)[::-1]) and np.all(i.numpy()[n:] == 7)


# ---- 4. the other route, several tiles per workgroup -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_equal_to_block_sort_of_one_row(radix, dt):
    T = tile_of(radix, dt)
    for n in (T + 1, 3 * T + 7):
        src = radix.Buf.from_numpy(data(dt, n, "special", 51 + n % 7))
        for desc in (False, True):
            a = radix.sort(src, desc)
            b = radix.sort_blocks(src, n, desc, flat=bool(n & 1))
            assert np.array_equal(bits(a[0].numpy()), bits(b[0].numpy())) and np.array_equal(a[1].numpy(), b[1].numpy()), (name(dt), n, desc)


@pytest.mark.parametrize("dt", [np.float32, np.uint64], ids=name)
def test_several_tiles_per_workgroup(radix, dt):
    T = tile_of(radix, dt)
    cu = cu_count()
    first = 2 * cu * T + 1                      # the smallest n of two tiles per workgroup
    assert plan(radix, dt, first - 1)[3] == 1 and plan(radix, dt, first)[3] == 2
    n = first + T + 5
    assert n <= 16 << 20, "the grid rule is too wide for a test"
    route, _, _, per, wgs, _, _ = plan(radix, dt, n)
    assert route == RADIX and per == 2 and wgs * per * T >= n > (wgs - 1) * per * T
    # keys with many ties (stability across a workgroup's tiles) in the low half, random bits in the high half
    rng = np.random.default_rng(71)
    x = random_data(dt, n, 72)
    x[: n // 2] = special_values(dt)[-4:][rng.integers(0, 4, n // 2)]
    rng.shuffle(x)
    check(radix, x, desc=False)


# ---- 5. reproducibility, step graphs, the automatic route ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_two_calls_agree_bit_for_bit(radix, dt):
    src = radix.Buf.from_numpy(data(dt, 3 * tile_of(radix, dt) + 7, "special", 81))
    for desc in (False, True):
        a = radix.sort(src, desc)
        b = radix.sort(src, desc)
        assert np.array_equal(bits(a[0].numpy()), bits(b[0].numpy())) and np.array_equal(a[1].numpy(), b[1].numpy())


def test_inside_a_step_graph(radix):
    capi = radix
    lib = capi.lib
    lib.ek_hip_graph_launch_count.restype = ctypes.c_uint64
    lib.ek_hip_graph_launch_count.argtypes = [ctypes.c_void_p]
    shapes = [(np.float32, 3 * tile_of(capi, np.float32) + 7, False), (np.int64, tile_of(capi, np.int64) + 1, True)]
    hosts = [[data(dt, n, "special", 91), data(dt, n, "random", 92)] for dt, n, _ in shapes]
    srcs = [capi.Buf.from_numpy(h[0]) for h in hosts]
    capi.check(lib.ek_hip_graph_begin())
    try:
        outs = [capi.sort(s, desc) for s, (_, _, desc) in zip(srcs, shapes)]
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        assert lib.ek_hip_graph_launch_count(g) == sum(plan(capi, dt, n)[5] for dt, n, _ in shapes) == 4 * 4 + 4 * 8
        for rnd in (0, 1):
            for buf, h in zip(srcs, hosts):
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr), h[rnd].ctypes.data_as(ctypes.c_void_p), SZ(h[rnd].nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            for (v, i), h, (_, _, desc) in zip(outs, hosts, shapes):
                want = reference(h[rnd], desc)
                assert np.array_equal(i.numpy(), want) and np.array_equal(bits(v.numpy()), bits(h[rnd][want]))
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_the_automatic_route(capi, dt):
    lib = capi.lib
    capi.set_tuning("sort_radix", 1)
    chunk = capi.sort_blocks_plan(dt, 4, 2)[2]
    lo, hi = chunk, 1 << 26
    assert plan(capi, dt, lo)[0] == FORWARDED and plan(capi, dt, hi)[0] == RADIX
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(capi, dt, mid)[0] == FORWARDED else (lo, mid)
    below, above = hi - 1, hi
    for n, route in ((below, FORWARDED), (above, RADIX)):
        x = data(dt, n, "special", 95)
        src = capi.Buf.from_numpy(x)
        l0 = lib.ek_hip_launch_count()
        v, i = capi.sort(src, True)
        l1 = lib.ek_hip_launch_count()
        got = plan(capi, dt, n)
        assert got[0] == route and l1 - l0 == got[5], (n, got, l1 - l0)
        if route == FORWARDED:
            capi.sort_blocks(src, n, True)
            assert lib.ek_hip_launch_count() - l1 == l1 - l0          # what ek_hip_sort_blocks launches
        else:
            assert l1 - l0 == 4 * np.dtype(dt).itemsize
        want = reference(x, True)
        assert np.array_equal(i.numpy(), want) and np.array_equal(bits(v.numpy()), bits(x[want]))
