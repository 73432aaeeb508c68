"""Horizontal reductions (csrc/reduce.hip) past one grid trip, in every element type and through every loader.

Stage 1 is a grid of `grid` blocks of 256 lanes; a lane takes the 16-byte vectors v0, v0 + T, v0 + 2 T, v0 + 3 T (T = 256 grid)
into four accumulators and strides on by 4 T; the elements behind the last whole vector go to accumulator 0, one per lane.  So the
sizes below are vector counts around the lane count of a wave and a block, the point where one block's four slots fill (1024), the
block counts 255 / 256 / 257 (stage 2 folds the partials with a stride of 256) and, with the grid at its cap, T, the end of the
first trip (4 T), 5 T + 3 and 8 T + 1 (three trips) -- each with 0, 1 and N - 1 elements behind the last vector.  The cap is
min(#CU x reduce_blocks_per_cu, 2048): the setting 1 brings three trips down to 2 Mi float32 elements, 4 is the default and 64
reaches 2048 blocks.

Everything is compared with something outside the code under test:
  1. data whose every partial result is exact in any order (small integers as floats, powers of two, wrapping integers): bit for bit;
  2. one distinguished entry among neutral ones, moved to every structural position: bit for bit;
  3. normal data: |error| against math.fsum / a sum of logs in long double, within the worst-case bound counted from the kernel
     (reduce_depth) and within the project's statistical model of a rounded sum (stat_bound = conftest.stat_sum_bound with u free);
  4. model_reduce(): the documented tree in NumPy, in the element type -- bit for bit for hsum and hprod;
  5. the fused loaders (chains, maps on load, safe_mul) against the reduction of the materialised array: bit for bit;
  6. views that are not 16-byte aligned, between poisoned neighbours;
  7. special values, empty inputs, error codes, repeats, one captured graph.
"""
import contextlib
import ctypes
import functools
import math

import numpy as np
import pytest

from conftest import bits_equal, stat_sum_bound

pytestmark = pytest.mark.gpu

SZ = ctypes.c_size_t
FLOATS = [np.float32, np.float64]
INTS = [np.int32, np.uint32, np.int64, np.uint64]
OPS = ["hsum", "hprod", "hmin", "hmax"]
SIGMAS = 5.0                    # conftest.stat_sum_bound's default; model_reduce() alone stays inside it (asserted per case)


# ---- geometry: what reduce_launch() computes ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def grid_cap(bpc):
    return min(device_cus() * bpc, 2048)


def reduce_grid(n, N, bpc):
    items = (n // N + 3) // 4 + 1
    return max(1, min(-(-items // 256), grid_cap(bpc)))


def nvec_of(name, bpc):
    """vector count behind a size name; T is the lane count of the capped grid"""
    T = 256 * grid_cap(bpc)
    if name[0] == "g":                      # a count that launches this many blocks
        return 4 * 256 * (int(name[1:]) - 1)
    if name[0].isdigit() and "T" not in name:
        return int(name)
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "4T-1": 4 * T - 1, "4T": 4 * T, "4T+1": 4 * T + 1, "5T+3": 5 * T + 3,
            "8T+1": 8 * T + 1}[name]


TAILS = (0, 1, -1)                          # -1: N - 1
SMALL = ["0", "1", "2", "255", "256", "257"] + [str(v) for v in range(1020, 1029)]
# (setting of reduce_blocks_per_cu, size name, tails)
CASES = [(1, s, TAILS) for s in SMALL + ["T-1", "T", "T+1", "4T-1", "4T", "4T+1", "5T+3", "8T+1"]]
CASES += [(4, s, TAILS) for s in ("g255", "g256", "g257")]
for _bpc in (4, 64):                        # the trip boundary only, one tail each
    CASES += [(_bpc, "4T-1", (-1,)), (_bpc, "4T", (0,)), (_bpc, "4T+1", (1,))]
CASE_IDS = [f"bpc{b}-{s}" for b, s, _ in CASES]
BOUNDARY = [(1, "4T-1", TAILS), (1, "4T", TAILS), (1, "4T+1", TAILS), (1, "8T+1", (-1,))]
BOUNDARY_IDS = [f"bpc{b}-{s}" for b, s, _ in BOUNDARY]


def sizes_of(case, N):
    """the element counts of a case, ascending: [(n, grid)]"""
    bpc, name, tails = case
    nvec = nvec_of(name, bpc)
    out = []
    for t in tails:
        n = nvec * N + (N - 1 if t < 0 else t)
        if n >= 1 and (n, reduce_grid(n, N, bpc)) not in out:
            out.append((n, reduce_grid(n, N, bpc)))
    if name[0] == "g":
        assert all(g == min(int(name[1:]), grid_cap(bpc)) for _, g in out)
    return sorted(out)


@pytest.fixture
def blocks_per_cu(capi):
    """`with blocks_per_cu(v):` runs a block under the tuning reduce_blocks_per_cu = v; the default, 4, is back after the block
    and, whatever happened, after the test"""
    @contextlib.contextmanager
    def setting(value):
        capi.set_tuning("reduce_blocks_per_cu", value)
        try:
            yield
        finally:
            capi.set_tuning("reduce_blocks_per_cu", 4)
    try:
        yield setting
    finally:
        capi.set_tuning("reduce_blocks_per_cu", 4)


def test_geometry_helpers(capi):
    """the size names mean what the docstring says on this device"""
    cus = device_cus()
    assert cus >= 1
    for bpc in (1, 4, 64):
        S, T = grid_cap(bpc), 256 * grid_cap(bpc)
        assert reduce_grid(4 * T * 4 - 4, 4, bpc) == S and reduce_grid((8 * T + 1) * 4, 4, bpc) == S
        assert reduce_grid(4, 4, bpc) == 1
    assert grid_cap(64) == 2048 or cus < 32
    if grid_cap(4) >= 257:
        assert [reduce_grid(nvec_of(f"g{g}", 4) * 2, 2, 4) for g in (255, 256, 257)] == [255, 256, 257]


# ---- device helpers ----------------------------------------------------------------------------------------------------------
def p(buf):
    return ctypes.c_void_p(buf.ptr)


def upload(capi, buf, a, offset=0):
    a = np.ascontiguousarray(a, dtype=buf.dtype)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr + offset * buf.dtype.itemsize),
                                                a.ctypes.data_as(ctypes.c_void_p), SZ(a.nbytes)))


def scalar(buf):
    v = buf.numpy()[0]
    buf.free()
    return v


def reduce(capi, op, buf, n=None):
    return scalar(capi.reduce(op, buf if n is None else buf.view(0, n)))


def same(got, want):
    return bits_equal(np.asarray([got]), np.asarray([want], dtype=np.asarray(got).dtype))


def guarded_view(capi, a, offset, guard):
    """`a` on the device at element `offset` of a larger, 16-byte aligned buffer whose other elements are `guard`"""
    N = 16 // a.dtype.itemsize
    whole = np.full(a.size + 2 * N, guard, a.dtype)
    whole[offset:offset + a.size] = a
    big = capi.Buf.from_numpy(whole)
    assert big.ptr % 16 == 0
    view = big.view(offset, a.size)
    assert (view.ptr % 16 != 0) == (offset % N != 0)
    return big, view


# ---- the documented tree, on the host ----------------------------------------------------------------------------------------
COMBINE = {"hsum": np.add, "hprod": np.multiply}


def model_block_tree(v, f):
    """block_reduce() as thread 0 sees it: v is (blocks, 256); the shuffle-down butterfly of a wave leaves in lane 0
    ((l + l+32) + (l+16 + l+48)) + .., then (w0 + w1) + (w2 + w3)"""
    w = v.reshape(-1, 4, 64)
    d = 32
    while d >= 1:
        w = f(w[..., :d], w[..., d:2 * d])
        d >>= 1
    w = w[..., 0]
    return f(f(w[:, 0], w[:, 1]), f(w[:, 2], w[:, 3]))


def model_reduce(a, op, grid, vec_ok=True):
    """hsum / hprod of `a` in its own type, in the order of k_reduce_stage1 + k_reduce_stage2 on `grid` blocks"""
    f, dt = COMBINE[op], a.dtype
    ident = dt.type(0 if op == "hsum" else 1)
    n, N, total = a.size, 16 // a.dtype.itemsize, 256 * grid
    if n == 1:
        return a[0]                                     # (ek_hip_reduce copies a single element)
    with np.errstate(all="ignore"):
        acc = np.full((4, total), ident, dt)
        nvec = n // N if vec_ok else 0
        body = a[:nvec * N].reshape(nvec, N)
        for start in range(0, nvec, total):             # slot by slot: accumulator k = slot % 4, trips in order
            k = (start // total) % 4
            blk = body[start:start + total]
            for i in range(N):                          # the elements of a vector in order
                acc[k, :blk.shape[0]] = f(acc[k, :blk.shape[0]], blk[:, i])
        for start in range(nvec * N, n, total):         # the tail, one element per lane and step, into accumulator 0
            seg = a[start:start + total]
            acc[0, :seg.size] = f(acc[0, :seg.size], seg)
        lane = f(f(acc[0], acc[1]), f(acc[2], acc[3]))
        partials = model_block_tree(lane.reshape(grid, 256), f)
        v = np.full(256, ident, dt)
        for start in range(0, grid, 256):               # stage 2: lane i folds partials i, i + 256, ..
            seg = partials[start:start + 256]
            v[:seg.size] = f(v[:seg.size], seg)
        return model_block_tree(v.reshape(1, 256), f)[0]


def reduce_depth(n, N, grid, vec_ok=True):
    """longest chain of roundings behind the result, counted from the kernels: per accumulator N combines per vector and one
    vector per trip of 4 T vectors, the tail into accumulator 0, (a0 + a1) + (a2 + a3), six shuffle steps, (w0 + w1) + (w2 + w3);
    stage 2: ceil(grid / 256) combines per lane, six shuffle steps and the wave merge"""
    total = 256 * grid
    nvec = n // N if vec_ok else 0
    trips = -(-nvec // (4 * total))
    tail = -(-(n - nvec * N) // total)
    return N * trips + tail + 2 + 6 + 2 + -(-grid // 256) + 6 + 2


def stat_bound(total, sumsq, n, depth, u, sigmas=SIGMAS):
    """conftest.stat_sum_bound with the unit roundoff as a parameter (so that it serves float64) and the moments passed in"""
    sigma = u * math.sqrt((depth / 6.0 + 12.0) * sumsq)
    drift = u * (0.8 * abs(total) + abs(total) / max(n, 1) * depth * math.sqrt(n) / 3.0)
    return sigmas * (sigma + drift)


def test_stat_bound_is_the_projects_model():
    a = np.random.default_rng(5).standard_normal(5000) + 0.25
    for m in (1, 2, 17, 5000):
        t = a[:m]
        mine = stat_bound(float(t.sum()), float((t * t).sum()), m, 300, 2.0 ** -24)
        assert abs(mine - stat_sum_bound(t, 300)) <= 1e-12 * mine


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def exact_sum(a):
    """sum(a) as S + rest: math.fsum rounds the sum once, to S, and fsum(a, -S) is what that rounding left"""
    vals = a.astype(np.float64).tolist()
    S = math.fsum(vals)
    vals.append(-S)
    return S, math.fsum(vals)


def check_sum(got, model, a, grid, vec_ok=True):
    n, N, u = a.size, 16 // a.dtype.itemsize, unit_roundoff(a.dtype)
    D = reduce_depth(n, N, grid, vec_ok)
    a64 = a.astype(np.float64)
    mag, sumsq = float(np.abs(a64).sum()), float((a64 * a64).sum())
    S, rest = exact_sum(a)
    err_model, err = abs((float(model) - S) - rest), abs((float(got) - S) - rest)
    worst, stat = D * u * mag, stat_bound(S, sumsq, n, D, u)
    assert err_model <= worst and err_model <= stat, ("the bounds do not hold for the reference tree itself", n, err_model, worst, stat)
    assert err <= worst, (n, err, worst)
    assert err <= stat, (n, err, stat)


def check_prod(got, model, a, grid):
    """A product carries one factor (1 + d), |d| <= u, per multiplication that rounds -- at most n - 1, the ones with the
    identity are exact -- wherever it sits in the tree: worst case (n - 1) u to first order, gamma_(n-1) in full; as noise of
    variance <= u^2 / 3 each, u sqrt(n / 3) standard deviations.  In float32 the roundings of (1 + a)(1 + b) with |a|, |b| ~ 1e-3
    are not zero-mean: the cross term a b is often below one ulp, and where a < 0 < b puts 1 + a + b halfway between two floats
    above 1 it is a b < 0 that breaks the tie, always downwards.  IEEE arithmetic on the CPU shows a mean of -0.011 u per
    multiplication among the factors themselves and less further up the tree (0.006, 0.004, ..); the bound allows u / 64 per
    multiplication as drift.  In float64 a b is 10^9 ulp and there is none.  The truth is exp(sum log a_i) in long double;
    its own error, 2^-63 (log2 n + 2) sum|log a_i|, is added to both bounds.
    For products these bounds are a sanity check: beyond 10^5 float32 factors the drift term dominates and a factor 1 +- 1e-3
    more or less would pass it, as it passes gamma_(n-1).  What pins hprod is the bit equality with model_reduce() at the same
    sizes and the exact products of test_exact_float_sums_and_products."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 on this machine"
    n, u = a.size, unit_roundoff(a.dtype)
    wide = a.astype(np.longdouble)
    assert np.all(wide > 0)
    logs = np.log(wide)
    truth = np.exp(np.sum(logs))
    slack = float(2.0 ** -63 * (math.log2(n) + 2) * np.sum(np.abs(logs)))
    m = max(n - 1, 1)
    worst = m * u / (1 - m * u) + slack
    drift = m * u / 64 if a.dtype == np.float32 else 0.0
    stat = SIGMAS * u * math.sqrt(m / 3.0) + drift + u + slack
    err = float(abs(np.longdouble(got) / truth - 1))
    err_model = float(abs(np.longdouble(model) / truth - 1))
    assert err_model <= worst and err_model <= stat, ("the bounds do not hold for the reference tree itself", n, err_model, worst, stat)
    assert err <= worst, (n, err, worst)
    assert err <= stat, (n, err, stat)


# ---- 1. exact data: bit for bit in any order ---------------------------------------------------------------------------------
def exact_sum_data(dtype, n, seed, wide=False):
    """nonzero values of {-2, -1, 1, 2} (wide, float64 only: odd integers up to 2^30, so that the low half of the 8-byte sum
    carries bits): every partial sum of any subset is an integer below 2^24 / 2^53, exact in the type"""
    rng = np.random.default_rng(seed)
    if wide:
        v = rng.integers(-(1 << 29), 1 << 29, n) * 2 + 1
    else:
        v = rng.choice(np.array([-2, -1, 1, 2]), n)
    assert np.all(v != 0) and int(np.abs(v).sum()) <= (2 ** 24 if np.dtype(dtype) == np.float32 else 2 ** 53)
    a = v.astype(dtype)
    assert np.array_equal(a.astype(np.int64), v)
    return a, v


def exact_prod_data(dtype, n, seed):
    """ones with at most 100 entries of {2, 0.5, -1}: every sub-product is a signed power of two within 2^+-100"""
    rng = np.random.default_rng(seed)
    a = np.ones(n, dtype)
    where = rng.choice(n, min(n, 100), replace=False)
    a[where] = rng.choice(np.array([2.0, 0.5, -1.0]), where.size)
    assert np.count_nonzero(a != 1) <= 100 and set(np.unique(a)) <= {-1.0, 0.5, 1.0, 2.0}
    return a


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_exact_float_sums_and_products(capi, blocks_per_cu, case, dtype):
    N = 16 // np.dtype(dtype).itemsize
    sizes = sizes_of(case, N)
    top = sizes[-1][0]
    flavours = [False, True] if dtype == np.float64 and top <= 1 << 22 else [False]
    with blocks_per_cu(case[0]):
        for wide in flavours:
            a, v = exact_sum_data(dtype, top, top + wide, wide)
            buf = capi.Buf.from_numpy(a)
            for n, grid in sizes:
                want = dtype(int(v[:n].sum()))
                assert int(want) == int(v[:n].sum())
                assert same(reduce(capi, "hsum", buf, n), want), ("hsum", n, grid, wide)
            buf.free()
        a = exact_prod_data(dtype, top, top)
        buf = capi.Buf.from_numpy(a)
        for n, grid in sizes:
            e = a[:n]
            want = dtype((-1.0) ** np.count_nonzero(e == -1) * 2.0 ** (np.count_nonzero(e == 2) - np.count_nonzero(e == 0.5)))
            assert same(reduce(capi, "hprod", buf, n), want), ("hprod", n, grid)
        buf.free()


@functools.lru_cache(maxsize=2)
def raw_ints(itemsize, n):
    u = np.uint32 if itemsize == 4 else np.uint64
    return np.random.default_rng(n + itemsize).integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)


@pytest.mark.parametrize("dtype", INTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_integer_reductions_wrap_exactly(capi, blocks_per_cu, case, dtype):
    """full-range values: sums and products wrap at every step, both halves of a 64-bit partial vary"""
    dtype = np.dtype(dtype)
    sizes = sizes_of(case, 16 // dtype.itemsize)
    raw = raw_ints(dtype.itemsize, sizes[-1][0])
    a = raw.view(dtype)
    odd = (raw | raw.dtype.type(1)).view(dtype)                 # odd factors: the product keeps all its bits
    with blocks_per_cu(case[0]):
        buf, obuf = capi.Buf.from_numpy(a), capi.Buf.from_numpy(odd)
        for n, grid in sizes:
            want = {"hsum": np.add.reduce(raw[:n], dtype=raw.dtype).view(dtype), "hmin": a[:n].min(), "hmax": a[:n].max()}
            for op, w in want.items():
                got = reduce(capi, op, buf, n)
                assert got.dtype == dtype and got == w, (op, n, grid, got, w)
            got, w = reduce(capi, "hprod", obuf, n), np.multiply.reduce(raw[:n] | raw.dtype.type(1), dtype=raw.dtype).view(dtype)
            assert got == w and got != 0, ("hprod", n, grid, got, w)
        buf.free(); obuf.free()


# ---- 3 + 4. normal data: the host model bit for bit, and both bounds ---------------------------------------------------------
@functools.lru_cache(maxsize=2)
def normal_data(dtype_name, n):
    rng = np.random.default_rng(n + np.dtype(dtype_name).itemsize)
    a = rng.standard_normal(n).astype(dtype_name)
    return a, (1 + 1e-3 * rng.standard_normal(n)).astype(dtype_name)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_normal_data_matches_the_model_within_bounds(capi, blocks_per_cu, case, dtype):
    """the result is a function of (n, grid): model_reduce() bit for bit; and it is a good sum"""
    N = 16 // np.dtype(dtype).itemsize
    sizes = sizes_of(case, N)
    a, f = normal_data(np.dtype(dtype).name, sizes[-1][0])
    with blocks_per_cu(case[0]):
        abuf, fbuf = capi.Buf.from_numpy(a), capi.Buf.from_numpy(f)
        for n, grid in sizes:
            got, model = reduce(capi, "hsum", abuf, n), model_reduce(a[:n], "hsum", grid)
            assert same(got, model), ("hsum", n, grid, got, model)
            got_p, model_p = reduce(capi, "hprod", fbuf, n), model_reduce(f[:n], "hprod", grid)
            assert same(got_p, model_p), ("hprod", n, grid, got_p, model_p)
            # (the truths cost host time, 2 s at 8 Mi elements: every size at the setting 1 and of the block counts 255 .. 257, the
            #  larger grids' trip boundary at one size)
            if n >= 2 and (case[0] == 1 or case[1] in ("g255", "g256", "g257", "4T+1")):
                check_sum(got, model, a[:n], grid)
                check_prod(got_p, model_p, f[:n], grid)
        abuf.free(); fbuf.free()


# ---- 2. one distinguished entry at every structural position -----------------------------------------------------------------
def structural_positions(n, N, grid):
    """element 0, the last one, the ends of the vector body, every tail element, both ends of the first and last vector of
    every unroll slot (slot s = vectors s T .. (s + 1) T - 1; every fourth slot starts a trip)"""
    total, nvec = 256 * grid, n // N
    pos = {0, n - 1} | set(range(nvec * N, n))
    if nvec:
        pos |= {nvec * N - 1}
    for s in range(-(-nvec // total)):
        for v in (s * total, min((s + 1) * total, nvec) - 1):
            pos |= {v * N, v * N + N - 1}
    return sorted(pos)


ONE_HOT = {"hsum": (0, 1, 1), "hprod": (1, 3, 3), "hmin": (7, 3, 3), "hmax": (7, 9, 9)}      # op: (background, entry, result)


@pytest.mark.parametrize("dtype", FLOATS + [np.int32, np.uint64])
@pytest.mark.parametrize("name", ["1027", "5T+3", "8T+1"])
def test_one_entry_at_every_structural_position(capi, blocks_per_cu, name, dtype):
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    n = nvec_of(name, 1) * N + N - 1
    with blocks_per_cu(1):
        grid = reduce_grid(n, N, 1)
        where = structural_positions(n, N, grid)
        assert len(where) >= 2 + N and (name != "8T+1" or len(where) >= 30)
        for op, (back, entry, want) in ONE_HOT.items():
            buf = capi.Buf.from_numpy(np.full(n, back, dtype))
            for at in where:
                upload(capi, buf, [entry], at)
                got = reduce(capi, op, buf)
                upload(capi, buf, [back], at)
                assert same(got, dtype.type(want)), (op, n, at, got)
            assert same(reduce(capi, op, buf), dtype.type(back if op != "hsum" else 0)), op
            buf.free()


@pytest.mark.parametrize("name", ["1027", "8T+1"])
def test_one_mask_byte_at_every_structural_position(capi, blocks_per_cu, name):
    n = nvec_of(name, 1) * 16 + 15
    with blocks_per_cu(1):
        where = structural_positions(n, 16, reduce_grid(n, 16, 1))
        zeros, ones = capi.Buf.from_numpy(np.zeros(n, np.uint8)), capi.Buf.from_numpy(np.ones(n, np.uint8))
        for at in where:
            upload(capi, zeros, [1], at)
            upload(capi, ones, [0], at)
            got = [capi.mask_reduce(op, zeros) for op in ("any", "count", "all")] + [capi.mask_reduce(op, ones) for op in ("all", "count", "any")]
            upload(capi, zeros, [0], at)
            upload(capi, ones, [1], at)
            assert got == [1, 1, 0, 0, n - 1, 1], (n, at, got)
        assert [capi.mask_reduce(op, zeros) for op in ("any", "count", "all")] == [0, 0, 0]
        assert [capi.mask_reduce(op, ones) for op in ("any", "count", "all")] == [1, n, 1]
        zeros.free(); ones.free()


# ---- mask reductions at the same sizes (N = 16 bytes per access) -------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_mask_reductions_past_one_trip(capi, blocks_per_cu, case):
    """random bytes of {0, 1, 2, 0x80, 0xFF}: anything but 0 counts as set"""
    sizes = sizes_of(case, 16)
    m = np.random.default_rng(sizes[-1][0]).choice(np.array([0, 0, 0, 1, 2, 0x80, 0xFF], np.uint8), sizes[-1][0])
    with blocks_per_cu(case[0]):
        buf = capi.Buf.from_numpy(m)
        for n, grid in sizes:
            cnt = int(np.count_nonzero(m[:n]))
            got = [capi.mask_reduce(op, buf.view(0, n)) for op in ("count", "any", "all")]
            assert got == [cnt, int(cnt != 0), int(cnt == n)], (n, grid, got, cnt)
        buf.free()


# ---- 5. the fused loaders build the same tree --------------------------------------------------------------------------------
def chains_for(capi, a, x, b, one):
    """(name, base, operands, maps); `one` is a one-element device array"""
    dt = a.dtype.type
    return [("fmadd(a, x, b) | sin", "fmadd", (a, x, b), ("sin",)),
            ("fmadd(a, 0.5, b) | exp, sin", "fmadd", (a, dt(0.5), b), ("exp", "sin")),
            ("fmadd(a, x, [c]) | sqrt", "fmadd", (a, x, one), ("sqrt",)),                    # NaN where the argument is negative
            ("fmadd(a, 1e-3, 1)", "fmadd", (a, dt(1e-3), dt(1.0)), ()),                      # factors near 1: a finite product
            ("mul(a, x)", "mul", (a, x), ()),
            ("a | abs, sqrt, rcp", None, (a,), ("abs", "sqrt", "rcp")),
            ("a | log", None, (a,), ("log",)),                                               # NaN, -inf at 0
            ("mulsub(a, x, b) | tanh", "mulsub", (a, x, b), ("tanh",))]                      # a second-wave map


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("case", BOUNDARY, ids=BOUNDARY_IDS)
def test_fused_reductions_are_the_tree_of_the_plain_one(capi, blocks_per_cu, case, dtype):
    """reduce_chain / reduce_map / hsum_safe_mul == reduce(materialised array), bit for bit, for all four ops; the NaNs that
    sqrt and log produce go through the minNum / maxNum combine of hmin / hmax inside the fused kernels too"""
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    sizes = sizes_of(case, N)
    top = sizes[-1][0]
    rng = np.random.default_rng(top)
    ha, hx, hb = (rng.standard_normal(top).astype(dtype) for _ in range(3))
    ha[::1001] = 0.0
    hw, hg = ha.copy(), hx.copy()
    hw[5::97] = 0.0; hg[5::97] = np.inf                       # zeros against infinities, both ways round
    hg[11::89] = 0.0; hw[11::89] = -np.inf
    with blocks_per_cu(case[0]):
        A, X, B, W, G = (capi.Buf.from_numpy(h) for h in (ha, hx, hb, hw, hg))
        one = capi.Buf.from_numpy(np.array([0.25], dtype))
        for n, grid in sizes:
            a, x, b, w, g = (t.view(0, n) for t in (A, X, B, W, G))
            for name, base, srcs, maps in chains_for(capi, a, x, b, one):
                mat = capi.map_chain(base, srcs, maps)
                host = mat.numpy()
                assert name.endswith(("sqrt", "log")) == bool(np.isnan(host).any()), name
                for op in OPS:
                    fused, plain = scalar(capi.reduce_chain(op, base, srcs, maps)), reduce(capi, op, mat)
                    assert same(fused, plain), (name, op, n, grid, fused, plain)
                    if op in ("hmin", "hmax") and not np.isnan(host).all():
                        assert not np.isnan(fused), (name, op)
                mat.free()
            for m in ("exp", "sqrt", "tanh"):                 # first wave, first wave with NaNs, second wave
                mat = capi.unary(m, a)
                for op in OPS:
                    fused, plain = scalar(capi.reduce_map(op, m, a)), reduce(capi, op, mat)
                    assert same(fused, plain), (m, op, n, grid, fused, plain)
                mat.free()
            for ww, gg in ((w, g), (dtype.type(1.0), g), (w, one)):           # (the last two sum to an infinity)
                mat = capi.binary("safe_mul", ww, gg, n=n)
                fused, plain = scalar(capi.hsum_safe_mul(ww, gg, n=n)), reduce(capi, "hsum", mat)
                assert (np.isfinite(plain) or ww is not w or gg is not g) and same(fused, plain), (n, grid, fused, plain)
                mat.free()
            with np.errstate(all="ignore"):
                terms = np.where((hw[:n] == 0) | (hg[:n] == 0), dtype.type(0), hw[:n] * hg[:n])
            assert same(scalar(capi.hsum_safe_mul(w, g)), model_reduce(terms, "hsum", grid)), (n, grid)
        for t in (A, X, B, W, G, one):
            t.free()


@pytest.mark.parametrize("dtype", FLOATS)
def test_fused_reductions_of_one_element(capi, dtype):
    """ek_hip_reduce copies a single element; the fused entry points return the single term likewise -- a -0.0 stays -0.0
    (0 + -0.0 would be +0.0), for every op"""
    dtype = np.dtype(dtype)
    small = dtype.type(1e-30 if dtype == np.float32 else 1e-200)           # small * small underflows to zero
    for value in (-0.0, 0.0, 2.5, -np.inf, np.nan):
        a = capi.Buf.from_numpy(np.array([value], dtype))
        b = capi.Buf.from_numpy(np.array([-0.0], dtype))
        for op in OPS:
            for base, srcs, maps in ((None, (a,), ("neg", "neg")), ("mul", (a, dtype.type(1.0)), ()), ("fmadd", (a, dtype.type(1.0), b), ("abs", "neg")),
                                     ("fmadd", (a, b, b), ())):
                mat = capi.map_chain(base, srcs, maps)
                assert mat.n == 1
                fused, plain = scalar(capi.reduce_chain(op, base, srcs, maps)), reduce(capi, op, mat)
                assert same(fused, plain) and same(plain, mat.numpy()[0]), (value, op, base, maps, fused, plain)
                mat.free()
            for m in ("neg", "abs", "sqrt", "tanh"):
                mat = capi.unary(m, a)
                fused, plain = scalar(capi.reduce_map(op, m, a)), reduce(capi, op, mat)
                assert same(fused, plain), (value, op, m, fused, plain)
                mat.free()
        for w, g in ((a, b), (a, dtype.type(-1.0)), (-small, capi.Buf.from_numpy(np.array([small], dtype)))):
            mat = capi.binary("safe_mul", w, g, n=1)
            fused, plain = scalar(capi.hsum_safe_mul(w, g, n=1)), reduce(capi, "hsum", mat)
            assert same(fused, plain), (value, fused, plain)
            mat.free()
    neg, pos = capi.Buf.from_numpy(np.array([-0.0], dtype)), capi.Buf.from_numpy(np.array([0.0], dtype))
    for got in (capi.reduce_chain("hsum", None, (neg,), ()), capi.reduce_map("hsum", "neg", pos),
                capi.hsum_safe_mul(-small, capi.Buf.from_numpy(np.array([small], dtype)), n=1)):
        assert same(scalar(got), dtype.type(-0.0))


# ---- 6. views that are not 16-byte aligned, between poisoned neighbours ------------------------------------------------------
UNALIGNED = ["1027", "5T+3"]


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_float_views(capi, blocks_per_cu, name, dtype):
    """vec_ok = 0: every element goes through the scalar loop into accumulator 0.  Exact data: the result of the aligned copy;
    normal data: model_reduce(vec_ok=False).  The neighbours are NaN (infinities for hmin / hmax)."""
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    n = nvec_of(name, 1) * N + 1
    ex, v = exact_sum_data(dtype, n, n)
    pr = exact_prod_data(dtype, n, n)
    a, f = normal_data(dtype.name, n)
    with blocks_per_cu(1):
        grid = reduce_grid(n, N, 1)
        assert same(reduce(capi, "hsum", capi.Buf.from_numpy(ex)), dtype.type(int(v.sum())))
        for off in range(1, N):
            # (minNum / maxNum would ignore a NaN neighbour: an infinity of the right sign there)
            for op, h, guard in (("hsum", ex, np.nan), ("hprod", pr, np.nan), ("hmin", a, -np.inf), ("hmax", a, np.inf)):
                big, view = guarded_view(capi, h, off, guard)
                aligned = capi.Buf.from_numpy(h)
                got, want = reduce(capi, op, view), reduce(capi, op, aligned)
                assert np.isfinite(got) and same(got, want), (op, n, off, got, want)
                big.free(); aligned.free()
            for op, h in (("hsum", a), ("hprod", f)):
                big, view = guarded_view(capi, h, off, np.nan)
                got, model = reduce(capi, op, view), model_reduce(h, op, grid, vec_ok=False)
                assert same(got, model), (op, n, off, got, model)
                if op == "hsum":
                    check_sum(got, model, h, grid, vec_ok=False)
                else:
                    check_prod(got, model, h, grid)
                big.free()


@pytest.mark.parametrize("dtype", INTS)
@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_integer_views(capi, blocks_per_cu, name, dtype):
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    n = nvec_of(name, 1) * N + 1
    one = raw_ints(dtype.itemsize, n).dtype.type(1)
    raw = (raw_ints(dtype.itemsize, n) >> one) | one        # odd (the product keeps its bits); the guard, all ones, is an extreme
    a = raw.view(dtype)
    with blocks_per_cu(1):
        for off in range(1, N):
            big, view = guarded_view(capi, a, off, np.array(-1).astype(dtype))
            want = {"hsum": np.add.reduce(raw, dtype=raw.dtype).view(dtype), "hprod": np.multiply.reduce(raw, dtype=raw.dtype).view(dtype), "hmin": a.min(), "hmax": a.max()}
            for op, w in want.items():
                got = reduce(capi, op, view)
                assert got == w, (op, n, off, got, w)
            big.free()


@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_mask_views(capi, blocks_per_cu, name):
    """bytes other than 0 and 1 count as set on the scalar path as on the vector path; the neighbours are set"""
    n = nvec_of(name, 1) * 16 + 1
    m = np.random.default_rng(n).choice(np.array([0, 0, 0, 1, 2, 0x80, 0xFF], np.uint8), n)
    cnt = int(np.count_nonzero(m))
    with blocks_per_cu(1):
        aligned = capi.Buf.from_numpy(m)
        assert capi.mask_reduce("count", aligned) == cnt
        for off in range(1, 16):
            for h, c in ((m, cnt), (np.zeros(n, np.uint8), 0)):
                big, view = guarded_view(capi, h, off, 1)
                got = [capi.mask_reduce(op, view) for op in ("count", "any", "all")]
                assert got == [c, int(c != 0), 0], (n, off, got, c)
                big.free()
        aligned.free()


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_fused_operands(capi, blocks_per_cu, name, dtype):
    """one operand of a chain / of safe_mul off alignment, the others aligned: the whole reduction takes the scalar loop, the
    tree of a plain reduction over an unaligned array"""
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    n = nvec_of(name, 1) * N + 1
    rng = np.random.default_rng(n + 1)
    ha, hx, hb = (rng.standard_normal(n).astype(dtype) for _ in range(3))
    hw = ha.copy(); hw[3::50] = 0.0
    hg = hx.copy(); hg[3::50] = np.inf
    with blocks_per_cu(1):
        grid = reduce_grid(n, N, 1)
        X, B, G = (capi.Buf.from_numpy(h) for h in (hx, hb, hg))
        for off in range(1, N):
            big, a = guarded_view(capi, ha, off, np.nan)
            for base, srcs, maps in (("fmadd", (a, X, B), ("sin",)), ("mul", (X, a), ()), (None, (a,), ("sqrt",))):
                mat = capi.map_chain(base, srcs, maps)
                host = mat.numpy()
                moved, mview = guarded_view(capi, host, off, np.nan)
                for op in OPS:
                    fused = scalar(capi.reduce_chain(op, base, srcs, maps))
                    assert same(fused, reduce(capi, op, mview)), (base, op, n, off)
                    if op in ("hmin", "hmax"):
                        assert same(fused, reduce(capi, op, mat)) and not np.isnan(fused), (base, op, n, off)
                    elif not np.isnan(host).any():
                        assert same(fused, model_reduce(host, op, grid, vec_ok=False)), (base, op, n, off)
                mat.free(); moved.free()
            big.free()
            big, w = guarded_view(capi, hw, off, np.nan)
            mat = capi.binary("safe_mul", w, G)
            host = mat.numpy()
            fused = scalar(capi.hsum_safe_mul(w, G))
            assert np.isfinite(fused) and same(fused, model_reduce(host, "hsum", grid, vec_ok=False)), (n, off)
            mat.free(); big.free()
        for t in (X, B, G):
            t.free()


# ---- 7. special values and small cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS)
def test_hsum_of_infinities_and_nan(capi, blocks_per_cu, dtype):
    """ones (an exact sum) with +inf, +inf and -inf, and a NaN at every structural position of a three-trip array"""
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    n = nvec_of("8T+1", 1) * N + N - 1
    with blocks_per_cu(1):
        where = structural_positions(n, N, reduce_grid(n, N, 1))
        buf = capi.Buf.from_numpy(np.ones(n, dtype))
        assert same(reduce(capi, "hsum", buf), dtype.type(n))
        for at in where:
            upload(capi, buf, [np.nan], at)
            got = reduce(capi, "hsum", buf)
            upload(capi, buf, [1.0], at)
            assert np.isnan(got), (n, at, got)
        for at, other in ((where[0], where[-1]), (where[-1], where[len(where) // 2]), (where[len(where) // 2], where[1])):
            upload(capi, buf, [np.inf], at)
            assert same(reduce(capi, "hsum", buf), dtype.type(np.inf)), at
            assert same(reduce(capi, "hmax", buf), dtype.type(np.inf)) and same(reduce(capi, "hmin", buf), dtype.type(1.0))
            upload(capi, buf, [-np.inf], other)
            assert np.isnan(reduce(capi, "hsum", buf)), (at, other)
            upload(capi, buf, [1.0], at)
            assert same(reduce(capi, "hsum", buf), dtype.type(-np.inf)), other
            upload(capi, buf, [1.0], other)
        assert same(reduce(capi, "hsum", buf), dtype.type(n))
        buf.free()


@pytest.mark.parametrize("dtype", FLOATS)
def test_denormal_sums_are_not_flushed(capi, blocks_per_cu, dtype):
    """multiples of the smallest denormal: every partial sum is an exact denormal"""
    dtype = np.dtype(dtype)
    N = 16 // dtype.itemsize
    tiny = np.finfo(dtype).smallest_subnormal
    with blocks_per_cu(1):
        for name in ("2", "1027", "5T+3"):
            n = nvec_of(name, 1) * N + N - 1
            k = np.random.default_rng(n).integers(-3, 5, n)
            a = (k * tiny).astype(dtype)
            want = dtype.type(int(k.sum()) * tiny)
            assert np.all((a == 0) == (k == 0)) and abs(int(k.sum())) < 2 ** 22 and abs(want) < np.finfo(dtype).tiny
            assert n < 10000 or abs(int(k.sum())) > 1000
            assert same(reduce(capi, "hsum", capi.Buf.from_numpy(a)), want), (n, int(k.sum()))


def test_hsum_of_negative_zeros(capi, blocks_per_cu, oracle):
    """the reference starts its lanes from zero<Packet>() (dynamic.h:632-647): -0.0 survives only as a single element"""
    with blocks_per_cu(1):
        for dtype in FLOATS:
            N = 16 // np.dtype(dtype).itemsize
            for n in (1, 2, N - 1, N, N + 1, 1027 * N + 1, nvec_of("4T+1", 1) * N + 1):
                a = np.full(n, -0.0, dtype)
                want = dtype(-0.0) if n == 1 else dtype(0.0)
                if dtype == np.float32:
                    assert same(oracle.reduce("hsum", a), want), n
                assert same(reduce(capi, "hsum", capi.Buf.from_numpy(a)), want), (dtype, n)


def test_empty_inputs(capi, oracle):
    for dtype in FLOATS + INTS:
        empty = np.empty(0, dtype)
        for op in OPS:
            if dtype == np.float64:         # (the oracle has no float64 reduction: dynamic.h:633, 651, 669, 687 literally)
                want = {"hsum": 0.0, "hprod": 1.0, "hmin": np.finfo(np.float64).max, "hmax": np.finfo(np.float64).tiny}[op]
            else:
                want = oracle.reduce(op, empty)
            got = scalar(capi.reduce(op, capi.Buf.from_numpy(empty)))
            assert got.dtype == np.dtype(dtype) and same(got, dtype(want)), (dtype, op, got, want)
    empty = capi.Buf.from_numpy(np.empty(0, np.uint8))
    assert [capi.mask_reduce(op, empty) for op in ("all", "any", "count")] == [oracle.mask_reduce(op, np.empty(0, np.uint8)) for op in ("all", "any", "count")] == [1, 0, 0]
    assert scalar(capi.hsum_safe_mul(capi.Buf.from_numpy(np.empty(0, np.float32)), np.float32(1.0), n=0)) == 0


def test_error_codes(capi):
    lib = capi.lib
    INVALID, UNSUPPORTED = -1, -2
    src, out = capi.Buf.from_numpy(np.arange(1, 9, dtype=np.float32)), capi.Buf.from_numpy(np.full(1, 77.0, np.float32))
    isrc = capi.Buf.from_numpy(np.arange(1, 9, dtype=np.int32))
    mask = capi.Buf.from_numpy(np.ones(8, np.uint8))
    res = ctypes.c_uint64(99)
    ch, _, _ = capi._chain(None, (src,), ("sin",))
    osrc, oisrc = capi.operand(src), capi.operand(isrc)
    HSUM, SIN = capi.REDUCE["hsum"], capi.UNARY["sin"]
    assert lib.ek_hip_reduce(HSUM, capi.F32, None, p(src), SZ(8)) == INVALID and b"null" in lib.ek_hip_last_error()
    assert lib.ek_hip_reduce(HSUM, capi.F32, p(out), None, SZ(8)) == INVALID
    assert lib.ek_hip_reduce(4, capi.F32, p(out), p(src), SZ(8)) == INVALID and b"unknown op" in lib.ek_hip_last_error()
    assert lib.ek_hip_reduce(-1, capi.F32, p(out), p(src), SZ(8)) == INVALID
    assert lib.ek_hip_reduce(HSUM, capi.BOOL, p(out), p(src), SZ(8)) == UNSUPPORTED
    assert lib.ek_hip_reduce(HSUM, 99, p(out), p(src), SZ(0)) == UNSUPPORTED
    assert lib.ek_hip_reduce_chain(HSUM, capi.F32, None, ctypes.byref(ch), SZ(8)) == INVALID
    assert lib.ek_hip_reduce_chain(HSUM, capi.F32, p(out), None, SZ(8)) == INVALID
    assert lib.ek_hip_reduce_chain(HSUM, capi.F32, p(out), ctypes.byref(ch), SZ(0)) == INVALID and b"empty" in lib.ek_hip_last_error()
    assert lib.ek_hip_reduce_chain(4, capi.F32, p(out), ctypes.byref(ch), SZ(8)) == INVALID
    assert lib.ek_hip_reduce_chain(HSUM, capi.I32, p(out), ctypes.byref(ch), SZ(8)) == UNSUPPORTED
    assert lib.ek_hip_reduce_map(HSUM, SIN, capi.F32, None, p(src), SZ(8)) == INVALID
    assert lib.ek_hip_reduce_map(HSUM, SIN, capi.F32, p(out), None, SZ(8)) == INVALID
    assert lib.ek_hip_reduce_map(HSUM, SIN, capi.F32, p(out), p(src), SZ(0)) == INVALID and b"empty" in lib.ek_hip_last_error()
    assert lib.ek_hip_reduce_map(4, SIN, capi.F32, p(out), p(src), SZ(8)) == INVALID
    assert lib.ek_hip_reduce_map(HSUM, capi.UNARY["floor"], capi.F32, p(out), p(src), SZ(8)) == UNSUPPORTED
    assert lib.ek_hip_reduce_map(HSUM, SIN, capi.U64, p(out), p(isrc), SZ(8)) == UNSUPPORTED
    assert lib.ek_hip_hsum_safe_mul(capi.F32, None, ctypes.byref(osrc), ctypes.byref(osrc), SZ(8)) == INVALID
    assert lib.ek_hip_hsum_safe_mul(capi.F32, p(out), None, ctypes.byref(osrc), SZ(8)) == INVALID
    assert lib.ek_hip_hsum_safe_mul(capi.I32, p(out), ctypes.byref(oisrc), ctypes.byref(oisrc), SZ(8)) == UNSUPPORTED
    assert lib.ek_hip_mask_reduce(capi.MASK_REDUCE["count"], p(mask), SZ(8), None) == INVALID
    assert lib.ek_hip_mask_reduce(capi.MASK_REDUCE["count"], None, SZ(8), ctypes.byref(res)) == INVALID
    assert lib.ek_hip_mask_reduce(3, p(mask), SZ(8), ctypes.byref(res)) == INVALID
    capi.sync()
    assert out.numpy()[0] == 77.0 and res.value == 99                  # nothing above touched an output
    capi.check(lib.ek_hip_reduce(HSUM, capi.F32, p(out), p(src), SZ(8)))
    assert out.numpy()[0] == 36.0


@pytest.mark.parametrize("dtype", FLOATS)
def test_repeated_calls_return_the_same_bits(capi, blocks_per_cu, dtype):
    N = 16 // np.dtype(dtype).itemsize
    n = nvec_of("5T+3", 1) * N + 1
    a, f = normal_data(np.dtype(dtype).name, n)
    with blocks_per_cu(1):
        for op, h in (("hsum", a), ("hprod", f)):
            buf = capi.Buf.from_numpy(h)
            assert len({reduce(capi, op, buf).tobytes() for _ in range(5)}) == 1, op
            buf.free()


def test_hsum_in_a_captured_graph(capi, blocks_per_cu):
    """three replays with new contents in the same buffer; the eager reductions in between use the context's scratch, larger
    than and apart from the graph's own"""
    lib = capi.lib
    n = nvec_of("8T+1", 1) * 4 + 3
    src, out = capi.Buf(np.float32, n), capi.Buf(np.float32, 1)
    other = capi.Buf.from_numpy(np.full(n, 3.0, np.float32))
    upload(capi, src, normal_data("float32", n)[0])
    with blocks_per_cu(1):
        grid = reduce_grid(n, 4, 1)
        capi.sync()
        capi.check(lib.ek_hip_graph_begin())
        try:
            rc = lib.ek_hip_reduce(capi.REDUCE["hsum"], capi.F32, p(out), p(src), SZ(n))
        finally:
            g = ctypes.c_void_p()
            capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
        try:
            capi.check(rc)
            for seed in (1, 2, 3):
                a = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
                upload(capi, src, a)
                upload(capi, out, [np.nan])
                capi.set_tuning("reduce_blocks_per_cu", 64)
                try:
                    assert reduce(capi, "hsum", other) == 3.0 * n
                finally:
                    capi.set_tuning("reduce_blocks_per_cu", 1)
                capi.check(lib.ek_hip_graph_launch(g))
                got = out.numpy()[0]
                assert same(got, model_reduce(a, "hsum", grid)), (seed, got)
        finally:
            capi.check(lib.ek_hip_graph_destroy(g))
    assert same(reduce(capi, "hsum", src), model_reduce(a, "hsum", reduce_grid(n, 4, 4)))      # and the eager library is alive
    for t in (src, out, other):
        t.free()
