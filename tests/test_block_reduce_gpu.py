"""ek_hip_reduce_blocks and ek_hip_repeat through the C ABI (csrc/block_reduce.hip): out[j] = op over in[j * B : (j + 1) * B], and
out[i] = in[i // B].

Expected values are numpy's over reshape(m, B).  Integers (wrapping), hmin / hmax (minNum / maxNum, -0 < +0), float sums of
small-integer data and float products over {+-1, +-2, +-0.5} (at most 100 entries per block differ from +-1, so that no partial
product leaves the exponent range in any order) are exact in every summation order and compared bit for bit.  Float sums of random
data are compared with a float64 (f32) or math.fsum (f64) sum under the order-independent bound  gamma_(B-1) * sum |x_i|  with
gamma_k = k u / (1 - k u), u = 2^-24 or 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any order of
B - 1 additions): derived, not measured.  The block sizes at which the route changes are asked from ek_hip_reduce_blocks_plan."""
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
FIXED_B = [1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 1000, 1024, 4099]
FIXED_M = [1, 2, 3, 63, 64, 65, 257]


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, n, B):
    return capi.reduce_blocks_plan(dt, n, B, cu_count())


# ---- data and expected values ----------------------------------------------------------------------------------------
def exact_data(dt, op, m, B, seed):
    """inputs whose reduction is exact in every order (see the module docstring)"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    n = m * B
    if dt.kind != "f":
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        return v | dt.type(1) if op == "hprod" else v               # odd factors: the wrapped product keeps information
    if op == "hsum":
        return rng.integers(-8, 9, n).astype(dt)
    if op == "hprod":
        v = rng.choice(np.array([1.0, -1.0], dt), n).reshape(m, B)
        k = min(B, 100)
        cols = rng.integers(0, B, (m, k))
        v[np.arange(m)[:, None], cols] = rng.choice(np.array([2.0, -2.0, 0.5, -0.5, 1.0, -1.0], dt), (m, k))
        return v.reshape(n)
    v = (rng.standard_normal(n) * 100).astype(dt)
    for value in (np.nan, -0.0, 0.0, np.inf, -np.inf):
        v[rng.integers(0, n, max(1, n // 16))] = value
    return v


def min_max(x2, op):
    """minNum / maxNum per row with -0 < +0 (numpy's fmin / fmax leave the sign of a zero result open)"""
    r = (np.fmin if op == "hmin" else np.fmax).reduce(x2, axis=1)
    zero = r == 0
    if zero.any():
        neg = ((x2 == 0) & np.signbit(x2)).any(axis=1)
        pos = ((x2 == 0) & ~np.signbit(x2)).any(axis=1)
        r = r.copy()
        r[zero] = np.where(neg[zero], -0.0, 0.0) if op == "hmin" else np.where(pos[zero], 0.0, -0.0)
    return r


def expected(x, op, m, B):
    x2 = x.reshape(m, B)
    with np.errstate(all="ignore"):
        if op == "hsum":
            return np.add.reduce(x2, axis=1, dtype=x.dtype)
        if op == "hprod":
            return np.multiply.reduce(x2, axis=1, dtype=x.dtype)
        if x.dtype.kind == "f":
            return min_max(x2, op)
        return (np.minimum if op == "hmin" else np.maximum).reduce(x2, axis=1)


def gamma_bound(x, m, B):
    u = 2.0 ** -24 if x.dtype == np.float32 else 2.0 ** -53
    k = B - 1
    return k * u / (1 - k * u) * np.abs(x.reshape(m, B).astype(np.float64)).sum(axis=1)


def true_sums(x, m, B):
    if x.dtype == np.float32:
        return x.reshape(m, B).astype(np.float64).sum(axis=1)
    return np.array([math.fsum(row) for row in x.reshape(m, B)])


def check_exact(capi, dt, op, m, B, seed, offset=0):
    x = exact_data(dt, op, m, B, seed)
    if offset:
        base = capi.Buf.from_numpy(np.concatenate([np.zeros(offset, x.dtype), x]))
        src = base.view(offset, x.size)
    else:
        src = capi.Buf.from_numpy(x)
    got = capi.reduce_blocks(op, src, B).numpy()
    want = expected(x, op, m, B)
    assert bits_equal(got, want), (name(dt), op, m, B, offset, plan(capi, dt, m * B, B), np.flatnonzero(got != want)[:8])


def first_b_where(pred, lo, hi):
    """smallest B in (lo, hi] with pred(B); pred is monotone, false at lo and true at hi"""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


def regime_edges(capi, dt):
    """(B3, m3): the smallest B that leaves the packed route at m3 = 3 blocks; (B4, m4): the smallest B that is split at m4 = 2"""
    m3, m4 = 3, 2
    top = CAP // 4
    assert plan(capi, dt, 2 * m3, 2)[0] == 2 and plan(capi, dt, top * m3, top)[0] >= 3
    B3 = first_b_where(lambda B: plan(capi, dt, B * m3, B)[0] >= 3, 2, top)
    assert plan(capi, dt, top * m4, top)[0] == 4
    B4 = first_b_where(lambda B: plan(capi, dt, B * m4, B)[0] == 4, 2, top)
    return (B3, m3), (B4, m4)


# ---- 1. every regime's edges and the fixed list ------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_fixed_block_sizes(capi, dt, op):
    for B in FIXED_B:
        for m in FIXED_M:
            if m * B <= CAP:
                check_exact(capi, dt, op, m, B, 1000 * B + m)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_edges_of_every_regime(capi, dt, op):
    (B3, m3), (B4, m4) = regime_edges(capi, dt)
    assert plan(capi, dt, (B3 - 1) * m3, B3 - 1)[0] == 2 and plan(capi, dt, B3 * m3, B3)[0] == 3
    assert plan(capi, dt, (B4 - 1) * m4, B4 - 1)[0] == 3 and plan(capi, dt, B4 * m4, B4)[0] == 4
    for B0, ms in ((B3, (m3, 64)), (B4, (m4, 3))):
        for B in (B0 - 1, B0, B0 + 1):
            for m in ms:
                if m * B <= CAP:
                    check_exact(capi, dt, op, m, B, B + m)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_float_sums_of_random_data_within_the_gamma_bound(capi, dt):
    (B3, m3), (B4, m4) = regime_edges(capi, dt)
    shapes = [(m, B) for B in FIXED_B for m in (1, 3, 65) if m * B <= CAP] + [(m3, B3 - 1), (m3, B3 + 1), (m4, B4 + 1), (3, B4 - 1)]
    rng = np.random.default_rng(7)
    for m, B in shapes:
        x = (rng.standard_normal(m * B) * np.exp(rng.uniform(-3, 3, m * B))).astype(dt)
        got = capi.reduce_blocks("hsum", capi.Buf.from_numpy(x), B).numpy().astype(np.float64)
        err, bound = np.abs(got - true_sums(x, m, B)), gamma_bound(x, m, B)
        assert np.all(err <= bound), (name(dt), m, B, float((err - bound).max()))


# ---- 2. nothing leaks between neighbouring blocks ----------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_no_leakage_between_neighbours(capi, dt):
    (_, _), (B4, _) = regime_edges(capi, dt)
    shapes = [(B, 9) for B in (3, 64, 65, 4099)] + [(B4 + 3, 3)]
    assert plan(capi, dt, (B4 + 3) * 3, B4 + 3)[0] == 4
    for B, m in shapes:
        for j in (0, m // 2, m - 1):
            for at in (0, B - 1):
                for special in (np.nan, np.inf, -np.inf, 1e30):
                    x = np.zeros(m * B, dt)
                    x[j * B + at] = special
                    got = capi.reduce_blocks("hsum", capi.Buf.from_numpy(x), B).numpy()
                    want = np.zeros(m, dt)
                    want[j] = special
                    assert bits_equal(got, want), (name(dt), B, m, j, at, special, got[max(0, j - 1):j + 2])


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_min_num_max_num(capi, dt):
    (B3, _), (B4, _) = regime_edges(capi, dt)
    for B in (2, 5, 64, B3, B4):
        m = 4
        x = np.full((m, B), np.nan, dt)
        x[0, :] = 3.0
        x[0, B // 2] = np.nan                        # a NaN inside a block is ignored
        x[2, 0], x[2, B - 1] = -0.0, 0.0             # block 1 stays all NaN; block 2 is {-0, +0} and NaN
        x[3, :] = 0.0
        x[3, B - 1] = -0.0
        buf = capi.Buf.from_numpy(x.reshape(-1))
        lo, hi = capi.reduce_blocks("hmin", buf, B).numpy(), capi.reduce_blocks("hmax", buf, B).numpy()
        assert lo[0] == 3 and hi[0] == 3 and np.isnan(lo[1]) and np.isnan(hi[1]), (B, lo, hi)
        for j in (2, 3):
            assert lo[j] == 0 and np.signbit(lo[j]) and hi[j] == 0 and not np.signbit(hi[j]), (B, j, lo, hi)


# ---- 3. misaligned base pointers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_misaligned_base_pointers(capi, dt):
    (_, _), (B4, m4) = regime_edges(capi, dt)
    offsets = (1, 2, 3) if np.dtype(dt).itemsize == 4 else (1,)
    for offset in offsets:
        for op in OPS:
            for B, m in ((4, 65), (5, 65), (64, 65), (1000, 5), (B4 + 1, m4), (2000, 3)):
                check_exact(capi, dt, op, m, B, 31 * B + offset, offset=offset)
    # the result of a sum does not leave the gamma bound at any alignment either
    if np.dtype(dt).kind == "f":
        rng = np.random.default_rng(3)
        for B, m in ((5, 65), (1000, 5), (B4 + 1, m4), (2000, 3)):
            x = rng.standard_normal(m * B).astype(dt)
            base = capi.Buf.from_numpy(np.concatenate([np.zeros(1, dt), x]))
            got = capi.reduce_blocks("hsum", base.view(1, x.size), B).numpy().astype(np.float64)
            assert np.all(np.abs(got - true_sums(x, m, B)) <= gamma_bound(x, m, B)), (name(dt), B, m)


# ---- 4. the split regime ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1 << 20, (1 << 20) + 1, 3 * (1 << 18) + 5])
def test_split_regime(capi, B):
    rng = np.random.default_rng(B)
    for m in (1, 2, 3, 5):
        n = m * B
        regime, splits, _ = plan(capi, np.float32, n, B)
        xi = rng.integers(-8, 9, n).astype(np.float32)
        buf = capi.Buf.from_numpy(xi)
        got = capi.reduce_blocks("hsum", buf, B).numpy()
        assert np.array_equal(got, xi.reshape(m, B).sum(axis=1, dtype=np.float64).astype(np.float32))
        x = rng.standard_normal(n).astype(np.float32)
        buf = capi.Buf.from_numpy(x)
        got = capi.reduce_blocks("hsum", buf, B).numpy()
        if m == 1:
            assert regime == 1 and bits_equal(got, capi.reduce("hsum", buf).numpy())
        else:
            assert regime == 4 and splits >= 2
        assert np.all(np.abs(got.astype(np.float64) - true_sums(x, m, B)) <= gamma_bound(x, m, B))
        u = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        ubuf = capi.Buf.from_numpy(u)
        for op in ("hsum", "hmin", "hmax"):
            assert np.array_equal(capi.reduce_blocks(op, ubuf, B).numpy(), expected(u, op, m, B)), (op, m, B)


# ---- 5. run-to-run identity ------------------------------------------------------------------------------------------------
def test_run_to_run_identity(capi):
    (B3, m3), (B4, m4) = regime_edges(capi, np.float32)
    rng = np.random.default_rng(11)
    for B, m in ((7, 4099), (100, 1001), (B3 + 1, 257), (B4 + 1, 3), (1 << 19, 2)):
        buf = capi.Buf.from_numpy(rng.standard_normal(m * B).astype(np.float32))
        runs = [capi.reduce_blocks("hsum", buf, B).numpy() for _ in range(3)]
        assert bits_equal(runs[0], runs[1]) and bits_equal(runs[0], runs[2]), (B, m)


# ---- 6. repeat -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.uint32, np.float64, np.int64], ids=name)
def test_repeat(capi, dt):
    rng = np.random.default_rng(5)
    pad, mark = 4, 0x7FFFFFF7                                   # (no entry has this value)
    for B in (1, 2, 3, 4, 5, 64, 65, 1000):
        for m in (1, 2, 63, 64, 65, 257):
            x = rng.integers(-1 << 30, 1 << 30, m).astype(dt)
            src = capi.Buf.from_numpy(x)
            want = np.repeat(x, B)
            assert bits_equal(capi.repeat(src, B).numpy(), want), (name(dt), B, m)
            for offset in ((1, 2, 3) if np.dtype(dt).itemsize == 4 else (1,)):
                sentinel = np.full(m * B + 2 * pad, mark, dt)
                out = capi.Buf.from_numpy(sentinel)
                capi.repeat(src, B, out=out.view(offset, m * B))
                got = out.numpy()
                assert bits_equal(got[offset:offset + m * B], want), (name(dt), B, m, offset)
                assert np.all(got[:offset] == dt(mark)) and np.all(got[offset + m * B:] == dt(mark)), (name(dt), B, m, offset)   # nothing outside
    # more than one trip of the grid, and a misaligned INPUT
    m, B = (1 << 20) + 3, 7
    x = rng.integers(-1 << 30, 1 << 30, m + 1).astype(dt)
    base = capi.Buf.from_numpy(x)
    assert bits_equal(capi.repeat(base.view(1, m), B).numpy(), np.repeat(x[1:], B))


# ---- 7. past 2^32 elements -------------------------------------------------------------------------------------------------
def test_past_2_to_the_32_elements(capi):
    free, total = SZ(), SZ()
    capi.check(capi.lib.ek_hip_mem_get_info(ctypes.byref(free), ctypes.byref(total)))
    if free.value < 40e9:
        pytest.skip("needs 40 GB of free device memory")
    B, m = 64, (1 << 26) + 3
    n = m * B
    assert n == (1 << 32) + 192
    ar = capi.arange(np.uint32, m)
    r = capi.repeat(ar, B)
    one = np.empty(1, np.uint32)
    for at in (0, (1 << 32) - 1, 1 << 32, n - 1):
        capi.check(capi.lib.ek_hip_memcpy_to_host(one.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(r.ptr + 4 * at), SZ(4)))
        assert one[0] == at // B, at
    for op in ("hmin", "hmax"):
        got = capi.reduce_blocks(op, r, B)
        assert capi.mask_reduce("all", capi.compare("eq", got, ar)) == 1, op
        del got
    got = capi.reduce_blocks("hsum", r, B)
    assert capi.mask_reduce("all", capi.compare("eq", got, capi.binary("mul", ar, np.uint32(B)))) == 1
    tail = got.view(m - 4, 4).numpy()
    assert np.array_equal(tail, ((np.arange(m - 4, m, dtype=np.uint64) * B) & 0xFFFFFFFF).astype(np.uint32))


# ---- 8. arguments ----------------------------------------------------------------------------------------------------------
def test_arguments(capi):
    lib = capi.lib
    x = capi.Buf.from_numpy(np.arange(12, dtype=np.float32))
    out = capi.Buf.from_numpy(np.full(12, 7, np.float32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    rb, rp = lib.ek_hip_reduce_blocks, lib.ek_hip_repeat
    assert rb(0, capi.F32, p(out), p(x), SZ(12), SZ(0)) == -1
    assert rb(0, capi.F32, p(out), p(x), SZ(12), SZ(5)) == -1 and b"blocks" in lib.ek_hip_last_error()
    assert rb(0, capi.F32, None, p(x), SZ(12), SZ(3)) == -1 and rb(0, capi.F32, p(out), None, SZ(12), SZ(3)) == -1
    assert rb(4, capi.F32, p(out), p(x), SZ(12), SZ(3)) == -1 and rb(-1, capi.F32, p(out), p(x), SZ(12), SZ(3)) == -1
    assert rb(0, capi.BOOL, p(out), p(x), SZ(12), SZ(3)) == -2 and rb(0, 99, p(out), p(x), SZ(12), SZ(3)) == -2
    assert rp(capi.F32, p(out), p(x), SZ(3), SZ(0)) == -1 and rp(capi.BOOL, p(out), p(x), SZ(3), SZ(2)) == -2
    assert rp(capi.F32, None, p(x), SZ(3), SZ(2)) == -1 and rp(capi.F32, p(out), None, SZ(3), SZ(2)) == -1
    l0 = lib.ek_hip_launch_count()
    assert rb(0, capi.F32, None, None, SZ(0), SZ(3)) == 0 and rp(capi.F32, None, None, SZ(0), SZ(3)) == 0
    assert lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), np.full(12, 7, np.float32))
    # the calls after refused ones work; B == 1 copies, B == n is the whole-array reduction
    assert rb(0, capi.F32, p(out), p(x), SZ(12), SZ(3)) == 0 and np.array_equal(out.numpy()[:4], [3, 12, 21, 30])
    assert np.array_equal(capi.reduce_blocks("hmax", x, 1).numpy(), np.arange(12, dtype=np.float32))
    assert np.array_equal(capi.repeat(x, 1).numpy(), np.arange(12, dtype=np.float32))
    big = capi.Buf.from_numpy(np.random.default_rng(1).standard_normal(100003).astype(np.float32))
    for op in OPS:
        assert bits_equal(capi.reduce_blocks(op, big, big.n).numpy(), capi.reduce(op, big).numpy()), op


# ---- 9. inside a step graph ------------------------------------------------------------------------------------------------
def test_inside_a_step_graph(capi):
    lib = capi.lib
    (_, _), (B4, m4) = regime_edges(capi, np.float32)
    rng = np.random.default_rng(13)
    Bp, mp, Bs, ms, Br, mr = 33, 3001, B4 + 5, 3, 5, 1001
    assert plan(capi, np.float32, Bp * mp, Bp)[0] == 2 and plan(capi, np.float32, Bs * ms, Bs)[0] == 4
    h1 = [rng.standard_normal(k).astype(np.float32) for k in (Bp * mp, Bs * ms, mr)]
    h2 = [rng.standard_normal(k).astype(np.float32) for k in (Bp * mp, Bs * ms, mr)]
    xs = [capi.Buf.from_numpy(h) for h in h1]
    held = []
    capi.check(lib.ek_hip_graph_begin())
    try:
        held = [capi.reduce_blocks("hsum", xs[0], Bp), capi.reduce_blocks("hsum", xs[1], Bs), capi.repeat(xs[2], Br)]
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        for hosts in (h1, h2):
            for buf, h in zip(xs, hosts):
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr), h.ctypes.data_as(ctypes.c_void_p), SZ(h.nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            replayed = [b.numpy() for b in held]
            eager = [capi.reduce_blocks("hsum", xs[0], Bp).numpy(), capi.reduce_blocks("hsum", xs[1], Bs).numpy(), capi.repeat(xs[2], Br).numpy()]
            for a, b in zip(replayed, eager):
                assert bits_equal(a, b)
            assert np.array_equal(replayed[2], np.repeat(hosts[2], Br))
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))
