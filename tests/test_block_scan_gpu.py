"""ek_hip_psum_blocks through the C ABI (csrc/block_scan.hip): prefix sums inside every block of B consecutive entries, inclusive or
exclusive, from the block's start or from its end.

Expected values.  Integers: numpy's cumsum per block in the unsigned type of the same width (wrapping; the inputs span the whole
range, so they do wrap), compared exactly.  Floating point: prefix sums of the same inputs in a wider type (float64 for float32,
numpy's longdouble for float64).  An output with t terms is held to
    |err| <= gamma(t - 1) * sum |x_i|  +  t * u_ref * sum |x_i|,      gamma(k) = k u / (1 - k u),  u = 2^-24 or 2^-53,
the sums running over the output's own terms.  The first part is the textbook bound for ANY order of the t - 1 additions of t terms
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) -- it is what "every output is a sum of its own terms only"
buys, and it is derived, not measured; the second is the reference's own rounding (sequential summation of t terms in the wider
type, u_ref = 2^-53 or half the longdouble epsilon).  On top of that, bit for bit: an exclusive result is the inclusive one moved by
one entry inside each block with +0 in front, an inclusive entry with one term is its input (-0.0 included), a NaN or +inf block
leaves its neighbours alone, two calls agree.

Sizes.  The packed route ends at B = 1024; the chunk of the one-workgroup-per-block route is kScanBlockRows = 4 rows of 256 lanes of one
16-byte vector (csrc/block_scan.hip); a tile of the packed route holds max(N, 16 KiB / size / B rounded down to N) blocks, N = 16 / size.
The routes themselves are asked from ek_hip_psum_blocks_plan with the device's CU count."""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
FLOATS = DTYPES[:2]
FLAGS = list(itertools.product((False, True), (False, True)))          # (exclusive, reverse)
SZ = ctypes.c_size_t
PACKED_B = [1, 2, 3, 5, 63, 64, 65, 100, 255, 256, 257, 1000, 1024]
SPLIT_B = [2 * 16384 + 5, 3 * 16384]


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, n, B):
    return capi.psum_blocks_plan(dt, n, B, cu_count())


def chunk_of(dt):
    return 4 * 256 * (16 // np.dtype(dt).itemsize)


def tile_blocks(dt, B):
    size = np.dtype(dt).itemsize
    N, E = 16 // size, 16384 // size
    return max(N, E // B // N * N)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def data(dt, m, B, seed):
    """mixed signs; integers over the whole range (their sums wrap); -0.0 at the ends of every other block of a float array"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, m * B, dtype=dt, endpoint=True)
    x = rng.standard_normal((m, B)).astype(dt)
    x[::2, 0] = -0.0
    x[::2, -1] = -0.0
    return x.reshape(m * B)


def scan_rows(a2, excl, rev):
    if rev:
        a2 = a2[:, ::-1]
    c = np.cumsum(a2, axis=1, dtype=a2.dtype)
    if excl:
        c = np.concatenate([np.zeros((a2.shape[0], 1), c.dtype), c[:, :-1]], axis=1)
    return c[:, ::-1] if rev else c


def run(capi, x, B, excl, rev, in_off=0, out_off=0, inplace=False):
    """the call on views `in_off` / `out_off` entries behind a 16-byte boundary; the entries around the output stay untouched"""
    n = x.size
    base = capi.Buf.from_numpy(np.concatenate([np.zeros(in_off, x.dtype), x]))
    src = base.view(in_off, n)
    if inplace:
        capi.psum_blocks(src, B, excl, rev, out=src)
        got = base.numpy()
        assert np.all(got[:in_off] == 0)
        return got[in_off:]
    guard = np.full(n + out_off + 1, 77, x.dtype)
    obase = capi.Buf.from_numpy(guard)
    capi.psum_blocks(src, B, excl, rev, out=obase.view(out_off, n))
    got = obase.numpy()
    assert np.all(got[:out_off] == 77) and got[-1] == 77
    return got[out_off:-1]


def check_values(x, got, m, B, excl, rev, what):
    x2, g2 = x.reshape(m, B), got.reshape(m, B)
    if x.dtype.kind != "f":
        U = np.dtype("u%d" % x.dtype.itemsize)
        want = scan_rows(x2.view(U), excl, rev)
        assert np.array_equal(g2.view(U), want), (what, np.argwhere(g2.view(U) != want)[:4])
        return
    wide = np.float64 if x.dtype == np.float32 else np.longdouble
    u = 2.0 ** -24 if x.dtype == np.float32 else 2.0 ** -53
    u_ref = float(np.finfo(wide).eps) / 2
    if wide is np.longdouble and np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        u_ref = 2.0 ** -53                                 # (no wider type here: the reference rounds like the result)
    truth = scan_rows(x2.astype(wide), excl, rev)
    mass = scan_rows(np.abs(x2).astype(np.float64), excl, rev)
    t = np.arange(B) if excl else np.arange(1, B + 1)      # terms per output, in scan order
    if rev:
        t = t[::-1]
    k = np.maximum(t - 1, 0)
    bound = (k * u / (1 - k * u) + t * u_ref) * mass
    err = np.abs(g2.astype(wide) - truth).astype(np.float64)
    print(f"{what}: worst err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3g}")
    assert np.all(err <= bound), (what, np.argwhere(err > bound)[:4], float(np.max(err / np.maximum(bound, 1e-300))))


def check_shape(capi, dt, m, B, seed, **where):
    """all four flag combinations of one shape: values, exclusive == moved inclusive, one-term entries == inputs"""
    x = data(dt, m, B, seed)
    got = {}
    for excl, rev in FLAGS:
        got[excl, rev] = run(capi, x, B, excl, rev, **where)
        check_values(x, got[excl, rev], m, B, excl, rev, (name(dt), m, B, excl, rev, where, plan(capi, dt, m * B, B)))
    x2 = bits(x).reshape(m, B)
    for rev in (False, True):
        inc, exc = bits(got[False, rev]).reshape(m, B), bits(got[True, rev]).reshape(m, B)
        what = (name(dt), m, B, rev, where)
        if not rev:
            assert np.array_equal(exc[:, 1:], inc[:, :-1]) and not exc[:, 0].any(), what
            assert np.array_equal(inc[:, 0], x2[:, 0]), what
        else:
            assert np.array_equal(exc[:, :-1], inc[:, 1:]) and not exc[:, -1].any(), what
            assert np.array_equal(inc[:, -1], x2[:, -1]), what


# ---- 1. block sizes and block counts of the packed route and of one workgroup per block ---------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_packed_block_sizes(capi, dt):
    for B in PACKED_B:
        tb = tile_blocks(dt, B)
        for m in (1, tb, tb + 1):
            regime, _, wgs = plan(capi, dt, m * B, B)
            assert regime == (0 if B == 1 else 1), (B, regime)
            if B > 1:
                assert wgs == (2 if m == tb + 1 else 1), (B, m, wgs)        # one tile exactly / a partial second tile
            check_shape(capi, dt, m, B, B * 7 + m)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_one_workgroup_per_block(capi, dt):
    c = chunk_of(dt)
    for B in (1025, c - 1, c, c + 1, 2 * c + 3):
        for m in (1, 3):
            assert plan(capi, dt, m * B, B)[0] == 2, B
            check_shape(capi, dt, m, B, B + m)


# ---- 2. few large blocks: split ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_split_blocks(capi, dt):
    N = 16 // np.dtype(dt).itemsize
    shorter = 0
    for B in SPLIT_B:
        for m in (1, 2, 3):
            regime, splits, wgs = plan(capi, dt, m * B, B)
            assert regime == 3 and splits >= 2 and wgs == m * splits, (B, m, regime, splits, wgs)
            shorter += B % N != 0                            # pieces are multiples of the vector width: the last one is shorter
            check_shape(capi, dt, m, B, B + m)
    assert shorter                                           # (2 * 16 Ki + 5 entries never divide into whole pieces)


# ---- 3. alignment and aliasing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_alignment_and_aliasing(capi, dt):
    c = chunk_of(dt)
    shapes = [(tile_blocks(dt, 100) + 1, 100), (tile_blocks(dt, 3) + 1, 3), (3, 1025), (2, c + 1), (2, SPLIT_B[0])]
    for m, B in shapes:
        for in_off, out_off in ((0, 1), (1, 0), (1, 1)):
            check_shape(capi, dt, m, B, 5, in_off=in_off, out_off=out_off)
        check_shape(capi, dt, m, B, 6, inplace=True)
        check_shape(capi, dt, m, B, 7, in_off=1, inplace=True)


@pytest.mark.parametrize("dt", FLOATS, ids=name)
def test_packed_result_does_not_depend_on_the_alignment(capi, dt):
    m, B = tile_blocks(dt, 100) + 1, 100
    x = data(dt, m, B, 8)
    for excl, rev in FLAGS:
        a = run(capi, x, B, excl, rev)
        assert np.array_equal(bits(a), bits(run(capi, x, B, excl, rev, in_off=1, out_off=1)))
        assert np.array_equal(bits(a), bits(run(capi, x, B, excl, rev, inplace=True)))


# ---- 4. containment ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", FLOATS, ids=name)
@pytest.mark.parametrize("B", [3, 64, 100])
def test_special_blocks_leave_their_neighbours_alone(capi, dt, B):
    tb = tile_blocks(dt, B)
    m = tb + 3
    nan_blocks, inf_blocks = [1, tb - 1], [3, tb + 1]          # tb - 1: the last block of tile 0; tb, between them, starts tile 1
    x = data(dt, m, B, B)
    y = x.reshape(m, B).copy()
    y[nan_blocks] = np.nan
    y[inf_blocks] = np.inf
    ordinary = np.setdiff1d(np.arange(m), nan_blocks + inf_blocks)
    for excl, rev in FLAGS:
        clean = run(capi, x, B, excl, rev).reshape(m, B)
        got = run(capi, y.reshape(-1), B, excl, rev).reshape(m, B)
        assert np.array_equal(bits(got[ordinary]), bits(clean[ordinary])), (B, excl, rev)
        body = slice(1, None) if excl and not rev else slice(None, -1) if excl else slice(None)
        assert np.isnan(got[nan_blocks][:, body]).all() and np.all(got[inf_blocks][:, body] == np.inf), (B, excl, rev)


@pytest.mark.parametrize("dt", FLOATS, ids=name)
def test_entries_in_front_of_a_nan_are_unaffected(capi, dt):
    c = chunk_of(dt)
    for m, B in ((tile_blocks(dt, 100) + 1, 100), (2, c + 5), (2, SPLIT_B[0])):
        x = data(dt, m, B, 11)
        at = B // 2 + 1
        y = x.reshape(m, B).copy()
        y[:, at] = np.nan
        for excl, rev in FLAGS:
            clean = run(capi, x, B, excl, rev).reshape(m, B)
            got = run(capi, y.reshape(-1), B, excl, rev).reshape(m, B)
            # outputs whose terms do not include entry `at`
            free = np.arange(B) > at - excl if rev else np.arange(B) < at + excl
            assert np.array_equal(bits(got[:, free]), bits(clean[:, free])), (B, excl, rev)
            assert np.isnan(got[:, ~free]).all(), (B, excl, rev)


# ---- 5. reproducibility, step graphs, launches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", FLOATS, ids=name)
def test_two_calls_agree_bit_for_bit(capi, dt):
    c = chunk_of(dt)
    seen = set()
    for m, B in ((4099, 1), (tile_blocks(dt, 100) * 3 + 1, 100), (5, 2 * c + 3), (3, SPLIT_B[0])):
        seen.add(plan(capi, dt, m * B, B)[0])
        src = capi.Buf.from_numpy(data(dt, m, B, 12))
        for excl, rev in FLAGS:
            a = capi.psum_blocks(src, B, excl, rev).numpy()
            b = capi.psum_blocks(src, B, excl, rev).numpy()
            assert np.array_equal(bits(a), bits(b)), (m, B, excl, rev)
    assert seen == {0, 1, 2, 3}


def test_inside_a_step_graph(capi):
    lib = capi.lib
    m, B = 2, SPLIT_B[0]
    assert plan(capi, np.float32, m * B, B)[0] == 3
    h1, h2 = data(np.float32, m, B, 13), data(np.float32, m, B, 14)
    src = capi.Buf.from_numpy(h1)
    held = []
    capi.check(lib.ek_hip_graph_begin())
    try:
        held = [capi.psum_blocks(src, B, excl, rev) for excl, rev in FLAGS]
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        for h in (h1, h2):
            capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(src.ptr), h.ctypes.data_as(ctypes.c_void_p), SZ(h.nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            replayed = [b.numpy() for b in held]
            for (excl, rev), r in zip(FLAGS, replayed):
                assert np.array_equal(bits(r), bits(capi.psum_blocks(src, B, excl, rev).numpy())), (excl, rev)
                check_values(h, r, m, B, excl, rev, ("graph", excl, rev))
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))


def test_arguments(capi):
    lib = capi.lib
    x = capi.Buf.from_numpy(np.arange(12, dtype=np.float32))
    out = capi.Buf.from_numpy(np.full(12, 7, np.float32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    pb = lib.ek_hip_psum_blocks
    assert pb(capi.F32, p(out), p(x), SZ(12), SZ(0), 0) == -1 and b"ek_hip_psum_blocks" in lib.ek_hip_last_error()
    assert pb(capi.F32, p(out), p(x), SZ(12), SZ(5), 0) == -1 and b"ek_hip_psum_blocks" in lib.ek_hip_last_error()
    assert pb(capi.F32, None, p(x), SZ(12), SZ(3), 0) == -1 and b"ek_hip_psum_blocks" in lib.ek_hip_last_error()
    assert pb(capi.F32, p(out), None, SZ(12), SZ(3), 0) == -1
    assert pb(capi.F32, p(out), p(x), SZ(12), SZ(3), 4) == -1 and b"ek_hip_psum_blocks" in lib.ek_hip_last_error()
    assert pb(capi.F32, p(out), p(x), SZ(12), SZ(3), -1) == -1
    assert pb(capi.BOOL, p(out), p(x), SZ(12), SZ(3), 0) == -2 and b"ek_hip_psum_blocks" in lib.ek_hip_last_error()
    assert pb(99, p(out), p(x), SZ(12), SZ(3), 0) == -2
    l0 = lib.ek_hip_launch_count()
    assert pb(capi.F32, None, None, SZ(0), SZ(3), 3) == 0 and lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), np.full(12, 7, np.float32))
    # the calls after refused ones work
    assert pb(capi.F32, p(out), p(x), SZ(12), SZ(3), 0) == 0 and np.array_equal(out.numpy()[:6], [0, 1, 3, 3, 7, 12])
    assert pb(capi.F32, p(out), p(x), SZ(12), SZ(3), 3) == 0 and np.array_equal(out.numpy()[:6], [3, 2, 0, 9, 5, 0])
