"""Inclusive prefix sums (ek_hip_psum) past one look-back window, in every element type and in both modes.

csrc/scan.hip scans tiles of T = 65536 / itemsize elements in one pass: a tile publishes its aggregate and looks back over
the descriptors of its predecessors, 256 per round.  With set_tuning("deterministic", 1) floating point sums take the
three fixed-shape kernels of csrc/reduce.hip instead.  Everything here is compared with NumPy at equal or higher precision:

  * integers: np.cumsum in the unsigned type of the same width (sums wrap), bit for bit;
  * floats whose sums are exact in any order (integer values, sums below 2^24 / 2^53), specials, signed zeros: bit for bit;
  * floats in general: |got - truth| <= D u cumsum|a| with D = psum_depth() counted from the kernels, and at the first and
    last element of every tile the project's statistical model of a rounded sum (conftest.stat_sum_bound), which is what
    notices a wrong tile offset at large i.

Sizes straddle the tile (T), one look-back round (256 T) and several rounds (1024 T, 4097 tiles).
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from conftest import bits_equal, hsum_depth, stat_sum_bound

pytestmark = pytest.mark.gpu

SZ = ctypes.c_size_t
LARGE = {4: (64 << 20) + 5, 8: (32 << 20) + 5}
SIZE_NAMES = ["2", "T-1", "T", "T+1", "2T+1", "255T+7", "256T", "256T+1", "257T+3", "1024T+T/2+1", "large"]


def tile_elems(itemsize):
    return 65536 // itemsize


def size_of(name, itemsize):
    T = tile_elems(itemsize)
    return {"2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "255T+7": 255 * T + 7, "256T": 256 * T,
            "256T+1": 256 * T + 1, "257T+3": 257 * T + 3, "1024T+T/2+1": 1024 * T + T // 2 + 1, "4Mi+5": (4 << 20) + 5,
            "large": LARGE[itemsize]}[name]


@pytest.fixture(params=[0, 1], ids=["lookback", "deterministic"])
def mode(capi, request):
    with deterministic_mode(capi, request.param):
        yield request.param


def psum(capi, a):
    src = capi.Buf.from_numpy(a)
    out = capi.psum(src)
    got = out.numpy()
    src.free(); out.free()
    return got


def upload(capi, buf, a):
    a = np.ascontiguousarray(a)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr), a.ctypes.data_as(ctypes.c_void_p), SZ(a.nbytes)))


def first_mismatch(got, want):
    """(index, got, want, count) of the first element that differs (NaN equals NaN), for the assertion message"""
    if got.shape != want.shape:
        return got.shape, want.shape
    bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))))
    return None if bad.size == 0 else (int(bad[0]), got[bad[0]], want[bad[0]], int(bad.size))


@contextlib.contextmanager
def deterministic_mode(capi, value):
    capi.set_tuning("deterministic", value)
    try:
        yield
    finally:
        capi.set_tuning("deterministic", 0)


# ---- 1. integers: exact, wrapping ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def raw_int_data(itemsize, n, seed):
    u = np.uint32 if itemsize == 4 else np.uint64
    raw = np.random.default_rng(seed).integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
    return raw, np.cumsum(raw, dtype=u)


def int_data(dtype, n, seed):
    """full-range values: the sums wrap every other element and both halves of a 64-bit aggregate vary; the signed types
    see the same bits (two's complement addition is the unsigned one)"""
    raw, want = raw_int_data(np.dtype(dtype).itemsize, n, seed)
    return raw.view(dtype), want.view(dtype)


@pytest.mark.parametrize("dtype", [np.uint32, np.int32, np.uint64, np.int64])            # (fastest: a width shares its data)
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_integer_psum_wraps_exactly(capi, dtype, size):
    n = size_of(size, np.dtype(dtype).itemsize)
    a, want = int_data(dtype, n, seed=n)
    got = psum(capi, a)
    assert got.dtype == want.dtype and np.array_equal(got, want), (n, first_mismatch(got, want))


# ---- 2. floats whose sums are exact in every order: bit for bit, both modes --------------------------------------------------
@functools.lru_cache(maxsize=1)
def exact_float_data(dtype, n, seed):
    """integer-valued, zero-mean inputs whose every partial sum -- in ANY association -- is exactly representable; the
    precondition is asserted on the reference alone.  float32: values in [-4, 4] (the mean -0.5 of integers(-5, 5) would leave
    2^24 near 32 Mi elements); float64: values up to 2^30, so that both halves of a published aggregate carry information."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        v = rng.integers(-4, 5, n)
        limit = 2 ** 24
    else:
        v = rng.integers(-(1 << 30), (1 << 30) + 1, n)
        limit = 2 ** 53
    want = np.cumsum(v, dtype=np.int64)
    assert float(np.abs(np.cumsum(v.astype(np.float64))).max()) < limit, "the inputs do not keep the prefix sums exact"
    # partial sums: a run of consecutive elements is a difference of two prefixes (look-back, Hillis-Steele); the block sums
    # of the three-pass kernels add strided subsets of one chunk, at most max(4096, n / 256) + 256 elements on >= 64 CUs
    assert max(int(want.max()), 0) - min(int(want.min()), 0) < limit
    assert int(np.abs(v).max()) * (max(4096, n // 256) + 256) < limit
    return v.astype(dtype), want.astype(np.float64).astype(dtype)


@pytest.mark.parametrize("deterministic", [0, 1], ids=["lookback", "deterministic"])      # (fastest: the two modes share the data)
@pytest.mark.parametrize("size", SIZE_NAMES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_psum_of_exact_sums_is_bit_exact(capi, deterministic, dtype, size):
    n = size_of(size, np.dtype(dtype).itemsize)
    a, want = exact_float_data(dtype, n, n)
    with deterministic_mode(capi, deterministic):
        got = psum(capi, a)
    assert bits_equal(got, want), (n, first_mismatch(got, want))


# ---- 3. floats in general: worst-case bound everywhere, statistical bound at the tile edges -------------------------------
def psum_depth(n, itemsize, deterministic, num_cu=256):
    """Longest chain of floating point additions behind one output of ek_hip_psum, counted from the kernels.  Every addition
    that is written counts, except in the look-back, where most operands are the identity and the count is by argument.

    Look-back (csrc/scan.hip, k_scan_lookback), V = 16 / itemsize elements per lane and row, `tiles` tiles:
      V - 1   vector-local scan of a lane's V elements;
      6       wave scan (shuffle-up by 1, 2, .. 32); a row's wave total s_wave[r][w] sits behind V - 1 + 6 additions;
      64      aggregate = the 16 x 4 wave totals added in sequence;
      tiles-1 look-back.  exclusive(t) is formed from the inclusive prefix of some tile p < t and the aggregates of tiles
              p + 1 .. t - 1 by the butterfly (6 levels) and the four wave parts of every round; lanes past `nearest` add
              the identity.  Every addition that rounds merges two disjoint non-empty runs of tiles, so a path from
              inclusive(p) to exclusive(t) holds at most t - 1 - p of them, and inclusive(t) = exclusive(t) + aggregate(t)
              one more: depth(inclusive(t)) <= depth(inclusive(p)) + t - p.  With depth(inclusive(0)) = depth(aggregate) the
              exclusive prefix of the last tile sits behind depth(aggregate) + tiles - 1 additions at worst -- one term per
              predecessor tile, which is what a look-back that always stops at its direct predecessor does;
      63      `running` / `before`: the wave totals of the 15 rows before this one (60) and of the waves before this one (3),
              added to the exclusive prefix one at a time;
      2       add = before + incl[r], out = v[j] + add.
    (The path through incl[r] alone, V - 1 + 6 + 2, is shorter.)

    Three-pass (csrc/reduce.hip) on `blocks` chunks of `chunk` elements, as psum_typed() sizes them:
      chunk/256       k_scan_block_sums: a thread adds every 256th element of its chunk in sequence,
      8               block_reduce: six shuffle levels and the two levels over the four wave parts;
      blocks - 1      k_scan_sums_serial: one thread adds the block sums in sequence;
      chunk/256 - 1   k_scan_apply: `carry` takes the total of every 256-element piece before this one,
      1               out = tile[i] + carry.
    (Hillis-Steele inside a piece, 8 additions, then carry: shorter than the path through the block sums.)"""
    if deterministic:
        blocks = max(1, min((n + 4095) // 4096, num_cu * 4))
        chunk = -(-(-(-n // blocks)) // 256) * 256
        blocks = -(-n // chunk)
        return chunk // 256 + 8 + (blocks - 1) + (chunk // 256 - 1) + 1
    V = 16 // itemsize
    tiles = -(-n // tile_elems(itemsize))
    return (V - 1) + 6 + 64 + (tiles - 1) + 63 + 2


def stat_prefix_bound(csum, csq, count, depth, u, sigmas):
    """conftest.stat_sum_bound evaluated for every prefix at once: csum = cumsum(a), csq = cumsum(a * a), count = i + 1"""
    csum, csq, count = np.asarray(csum, np.float64), np.asarray(csq, np.float64), np.asarray(count, np.float64)
    depth = np.asarray(depth, np.float64)
    sigma = u * np.sqrt((depth / 6.0 + 12.0) * csq)
    drift = u * (0.8 * np.abs(csum) + np.abs(csum) / count * depth * np.sqrt(count) / 3.0)
    return sigmas * (sigma + drift)


# 5 standard deviations, the default of conftest.stat_sum_bound.  Checked on a CPU for every case used below: the sequential
# np.cumsum in the type itself (depth i at element i -- deeper than either kernel goes) stays inside the model at every tile
# edge with sigmas = 5; it comes closest, 0.50 of the bound, for float32 at 257 T + 3.  So the default is kept, and
# general_case() asserts the same for the inputs it hands out.
SIGMAS = 5.0


@functools.lru_cache(maxsize=1)
def general_case(dtype_name, n):
    """standard normal inputs, their prefix sums one precision up, cumsum|a|, and what the statistical bound needs at the
    first and last element of every tile"""
    dtype = np.dtype(dtype_name)
    up = np.float64 if dtype == np.float32 else np.longdouble
    if up is np.longdouble:
        assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 on this machine"
    a = np.random.default_rng(n + dtype.itemsize).standard_normal(n).astype(dtype)
    wide = a.astype(up)
    truth = np.cumsum(wide)
    cabs = np.cumsum(np.abs(a), dtype=np.float64)
    T = tile_elems(dtype.itemsize)
    edges = np.unique(np.concatenate([np.arange(0, n, T), np.arange(T - 1, n, T), [n - 1]]))
    csq = np.cumsum(a.astype(np.float64) ** 2)[edges]
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    case = dict(a=a, truth=truth, cabs=cabs, edges=edges, csum_e=truth[edges].astype(np.float64), csq_e=csq, u=u, n=n, dtype=dtype)
    # the model must hold for a sum we can reason about before it judges the kernels: the sequential sum in the type
    # itself, whose depth at element i is i
    seq = np.cumsum(a, dtype=dtype)
    err = np.abs(seq[edges].astype(up) - truth[edges]).astype(np.float64)
    bound = stat_prefix_bound(case["csum_e"], csq, edges + 1, np.maximum(edges, 1), u, SIGMAS)
    case["seq_ratio"] = float((err / bound).max())
    assert case["seq_ratio"] <= 1.0, ("the statistical model does not cover a sequential sum of these inputs", case["seq_ratio"])
    return case


def check_general(got, case, deterministic, num_cu):
    n, u, dtype = case["n"], case["u"], case["dtype"]
    assert got.dtype == dtype and got.shape == (n,)
    D = psum_depth(n, dtype.itemsize, deterministic, num_cu)
    err = np.abs(got.astype(case["truth"].dtype) - case["truth"]).astype(np.float64)
    worst = err / (D * u * case["cabs"])
    e = case["edges"]
    stat = err[e] / stat_prefix_bound(case["csum_e"], case["csq_e"], e + 1, D, u, SIGMAS)
    print(f"psum {dtype.name} n={n} deterministic={deterministic}: D={D}, max err / (D u cumsum|a|) = {np.nanmax(worst):.3g}, "
          f"max err / statistical bound at the tile edges = {stat.max():.3g} (sequential CPU sum: {case['seq_ratio']:.3g})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= D * u * case["cabs"]), (int(np.argmax(worst)), float(np.nanmax(worst)))
    assert np.all(stat <= 1.0), (int(e[np.argmax(stat)]), float(stat.max()))


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_prefix_bound_is_the_projects_model():
    """stat_prefix_bound is conftest.stat_sum_bound, prefix by prefix"""
    a = np.random.default_rng(5).standard_normal(5000) + 0.25
    cs, cq = np.cumsum(a), np.cumsum(a * a)
    for i in (0, 1, 17, 4999):
        mine = stat_prefix_bound(cs[i], cq[i], i + 1, 300, 2.0 ** -24, 5.0)
        assert abs(mine - stat_sum_bound(a[:i + 1], 300)) <= 1e-12 * mine


@pytest.mark.parametrize("deterministic", [0, 1], ids=["lookback", "deterministic"])      # (fastest: the two modes share a case)
@pytest.mark.parametrize("size", ["257T+3", "4Mi+5", "large"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_psum_general_within_bounds(capi, deterministic, dtype, size):
    case = general_case(dtype, size_of(size, np.dtype(dtype).itemsize))
    with deterministic_mode(capi, deterministic):
        got = psum(capi, case["a"])
    check_general(got, case, deterministic, device_cus())


# ---- 6. determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_deterministic_psum_repeats_bit_for_bit(capi, dtype):
    case = general_case(dtype, (4 << 20) + 5)
    with deterministic_mode(capi, 1):
        first, second = psum(capi, case["a"]), psum(capi, case["a"])
    assert first.tobytes() == second.tobytes()
    check_general(first, case, 1, device_cus())


# ---- 4. special values -------------------------------------------------------------------------------------------------
def sequential(a):
    """the reference's recurrence (out[0] = a[0], out[i] = out[i - 1] + a[i]) in NumPy"""
    return np.add.accumulate(a)


@pytest.mark.parametrize("size", ["2", "T+1", "257T+3"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zeros(capi, oracle, mode, dtype, size):
    """the identity of IEEE addition is -0.0: a prefix of negative zeros sums to -0.0, and +0.0 from the first +0.0 on"""
    n = size_of(size, np.dtype(dtype).itemsize)
    T = tile_elems(np.dtype(dtype).itemsize)
    all_neg = np.full(n, -0.0, dtype)
    head = np.zeros(n, dtype); head[0] = -0.0
    late = np.full(n, -0.0, dtype); late[min(2 * T + 77, n - 1)] = 0.0          # the first +0.0 inside the third tile
    for name, a in (("all -0.0", all_neg), ("-0.0 then +0.0", head), ("+0.0 inside a tile", late)):
        want = sequential(a)
        assert np.signbit(want[0]) and (name != "all -0.0" or np.all(np.signbit(want)))
        if np.dtype(dtype) == np.float32:
            assert bits_equal(oracle.psum(a), want), name
        got = psum(capi, a)
        assert bits_equal(got, want), (name, n, first_mismatch(np.signbit(got), np.signbit(want)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_infinities_and_nan(capi, mode, dtype):
    """+inf in tile 3 and -inf in tile 300 among small integers: exact below p, +inf on [p, q), NaN from q on -- in any
    association, because output i is a sum over exactly the elements 0 .. i; and a single NaN"""
    T = tile_elems(np.dtype(dtype).itemsize)
    n = 301 * T + 5
    base, exact = exact_float_data(dtype, n, seed=17)
    p, q = 3 * T + 1234, 300 * T + 4321
    a = base.copy(); a[p] = np.inf; a[q] = -np.inf
    want = exact.copy(); want[p:q] = np.inf; want[q:] = np.nan
    got = psum(capi, a)
    assert bits_equal(got, want), first_mismatch(got, want)
    for at in (0, T - 1, 257 * T + 2, n - 1):
        a = base.copy(); a[at] = np.nan
        want = exact.copy(); want[at:] = np.nan
        got = psum(capi, a)
        assert bits_equal(got, want), (at, first_mismatch(got, want))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_denormals_are_not_flushed(capi, mode, dtype):
    """multiples of the smallest denormal: every sum is an exact denormal (or zero), in any order"""
    T = tile_elems(np.dtype(dtype).itemsize)
    n = 3 * T + 5
    tiny = np.finfo(dtype).smallest_subnormal
    k = np.random.default_rng(23).integers(-4, 5, n)
    ksum = np.cumsum(k)
    assert np.abs(ksum).max() < 2 ** 20 and np.abs(ksum).max() > 8
    a, want = (k * tiny).astype(dtype), (ksum * tiny).astype(dtype)
    assert np.all((a == 0) == (k == 0)) and np.abs(want).max() < np.finfo(dtype).tiny      # denormal all the way
    assert bits_equal(sequential(a), want)
    got = psum(capi, a)
    assert bits_equal(got, want), first_mismatch(got, want)


# ---- 5. pointer alignment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift_in,shift_out", [(1, 1), (1, 0), (0, 1)], ids=["both", "in", "out"])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_misaligned_pointers(capi, dtype, shift_in, shift_out):
    """views one element into a buffer are not 16-byte aligned: the kernel takes its element-wise loads and stores, and
    writes nothing outside out[0 .. n)"""
    dtype = np.dtype(dtype)
    n = 3 * tile_elems(dtype.itemsize) + 5
    a, want = int_data(dtype, n, seed=n + shift_in + 2 * shift_out)
    guard = dtype.type(0xA5A5A5A5A5A5A5A5 & int(np.iinfo(dtype).max))
    src_all, out_all = capi.Buf(dtype, n + 2), capi.Buf(dtype, n + 2)
    src, out = src_all.view(shift_in, n), out_all.view(shift_out, n)
    assert (src.ptr % 16 != 0) == bool(shift_in) and (out.ptr % 16 != 0) == bool(shift_out)
    upload(capi, src, a)
    capi.check(capi.lib.ek_hip_memset(ctypes.c_void_p(out_all.ptr), 0xA5, SZ((n + 2) * dtype.itemsize)))
    capi.check(capi.lib.ek_hip_psum(src.ek, ctypes.c_void_p(out.ptr), ctypes.c_void_p(src.ptr), SZ(n)))
    whole = out_all.numpy()
    got = whole[shift_out:shift_out + n]
    assert np.array_equal(got, want), first_mismatch(got, want)
    assert np.all(whole[:shift_out] == guard) and np.all(whole[shift_out + n:] == guard)


# ---- 7. capture and replay -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,deterministic", [(np.uint32, 0), (np.float32, 0), (np.float32, 1)],
                         ids=["uint32", "float32", "float32-deterministic"])
def test_psum_in_a_captured_step_graph(capi, dtype, deterministic):
    """every replay re-arms the descriptors and the ticket (the memset is part of the graph) and reads the CURRENT input"""
    lib = capi.lib
    n = 300 * tile_elems(4) + 9
    make = (lambda seed: int_data(dtype, n, seed)) if np.dtype(dtype).kind == "u" else (lambda seed: exact_float_data(dtype, n, seed))
    src, out = capi.Buf(dtype, n), capi.Buf(dtype, n)
    upload(capi, src, make(100)[0])
    with deterministic_mode(capi, deterministic):
        capi.sync()
        capi.check(lib.ek_hip_graph_begin())
        try:
            rc = lib.ek_hip_psum(src.ek, ctypes.c_void_p(out.ptr), ctypes.c_void_p(src.ptr), SZ(n))
        finally:
            g = ctypes.c_void_p()
            capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
        try:
            capi.check(rc)
            for seed in (101, 102, 103):
                a, want = make(seed)
                upload(capi, src, a)
                capi.check(lib.ek_hip_memset(ctypes.c_void_p(out.ptr), 0x5A, SZ(n * np.dtype(dtype).itemsize)))
                capi.check(lib.ek_hip_graph_launch(g))
                got = out.numpy()
                assert bits_equal(got, want), (seed, first_mismatch(got, want))
        finally:
            capi.check(lib.ek_hip_graph_destroy(g))
    # and the eager library is alive
    a, want = make(104)
    assert bits_equal(psum(capi, a), want)


# ---- 8. error paths ------------------------------------------------------------------------------------------------------
def test_error_paths(capi):
    lib = capi.lib
    a = np.arange(1, 9, dtype=np.float32)
    src, out = capi.Buf.from_numpy(a), capi.Buf.from_numpy(np.full(8, 77.0, np.float32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    assert lib.ek_hip_psum(capi.F32, None, p(src), SZ(8)) == -1 and b"null" in lib.ek_hip_last_error()
    assert lib.ek_hip_psum(capi.F32, p(out), None, SZ(8)) == -1
    assert lib.ek_hip_psum(capi.BOOL, p(out), p(src), SZ(8)) == -2 and b"unsupported" in lib.ek_hip_last_error()
    assert lib.ek_hip_psum(99, p(out), p(src), SZ(8)) == -2
    assert lib.ek_hip_psum(capi.F32, p(out), p(src), SZ(0)) == 0
    capi.sync()
    assert np.array_equal(out.numpy(), np.full(8, 77.0, np.float32))       # nothing above touched the output
    capi.check(lib.ek_hip_psum(capi.F32, p(out), p(src), SZ(8)))
    assert np.array_equal(out.numpy(), np.cumsum(a, dtype=np.float32))


# ---- 9. consumers: compress() and the tape ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ekc():
    import enoki_amd.hip as m
    return m


@pytest.fixture(scope="module")
def ek():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


def compress_values(kind, n, rng):
    if kind == "Float32":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "Float64":
        return rng.standard_normal(n)
    dtype = {"UInt32": np.uint32, "UInt64": np.uint64, "Int64": np.int64}[kind]
    return int_data(dtype, n, int(rng.integers(1 << 30)))[0]


@pytest.mark.parametrize("n", [257 * 16384 + 3, (4 << 20) + 5], ids=["257T+3", "4Mi+5"])
@pytest.mark.parametrize("kind", ["Float32", "Float64", "UInt32", "UInt64", "Int64"])
def test_compress_large_and_degenerate_masks(ekc, kind, n):
    """compress() = psum of the mask as uint32 + scatter: a[m] in order, bit for bit, whatever the mask"""
    rng = np.random.default_rng(n)
    a = compress_values(kind, n, rng)
    dev = getattr(ekc, kind)(a)
    masks = {"random": rng.integers(0, 2, n).astype(bool), "all": np.ones(n, bool), "none": np.zeros(n, bool),
             "first": np.arange(n) == 0, "last": np.arange(n) == n - 1, "tile ends": np.arange(n) % 16384 == 16383}
    for name, m in masks.items():
        got = ekc.compress(dev, ekc.Mask(m.astype(np.uint8))).numpy()
        want = a[m]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert got.dtype == want.dtype and bits_equal(got, want), name


def test_tape_psum_adjoint_and_forward_beyond_one_window(ek):
    """y = hsum(psum(x) * w): dy/dx[j] is the suffix sum of w from j on (the adjoint is reverse . psum . reverse), exact for
    integer-valued w; forward mode through psum: d psum(x)[i] is the prefix sum of dx"""
    n = 257 * 16384 + 3
    rng = np.random.default_rng(n)
    hx, hw = rng.integers(-4, 5, n), rng.integers(-4, 5, n)
    suffix = np.cumsum(hw[::-1])[::-1]
    assert np.abs(suffix).max() < 2 ** 24 and np.abs(np.cumsum(hx)).max() < 2 ** 22       # products and sums stay exact
    x, w = ek.Float32(hx.astype(np.float32)), ek.Float32(hw.astype(np.float32))
    ek.set_requires_gradient(x)
    y = ek.hsum(ek.psum(x) * w)
    ek.backward(y)
    g = ek.gradient(x).numpy()
    want = suffix.astype(np.float32)
    assert bits_equal(g, want), first_mismatch(g, want)
    terms = np.cumsum(hx) * hw
    assert abs(float(ek.detach(y).numpy()[0]) - float(terms.sum())) <= 2.0 ** -24 * hsum_depth(n) * float(np.abs(terms).sum())
    # forward mode, vector seed: t -> x = t * c -> z = psum(x) * w; dz/dt seeded with 1 is psum(c) * w
    hc = rng.integers(-4, 5, n)
    assert np.abs(np.cumsum(hc)).max() < 2 ** 22
    t = ek.Float32(np.ones(n, np.float32)); c = ek.Float32(hc.astype(np.float32))
    ek.set_requires_gradient(t)
    z = ek.psum(t * c) * w
    ek.forward(t)
    dz = ek.gradient(z).numpy()
    want = (np.cumsum(hc) * hw).astype(np.float32)
    assert bits_equal(dz, want), first_mismatch(dz, want)
    # forward mode straight into psum: the scalar seed of forward(x) stands for n ones, d psum(x)[i] = i + 1
    x2 = ek.Float32(hx.astype(np.float32))
    ek.set_requires_gradient(x2)
    z2 = ek.psum(x2) * w
    ek.forward(x2)
    dz2 = ek.gradient(z2).numpy()
    want = ((np.arange(n) + 1) * hw).astype(np.float32)            # (i + 1) w: below 2^24, or 4 (i + 1) with i + 1 < 2^24
    assert np.array_equal(want.astype(np.int64), (np.arange(n) + 1) * hw)
    assert bits_equal(dz2, want), first_mismatch(dz2, want)
