"""`op(gather(A, idx[, mask]), x, c)` with a HOST SCALAR c -- `fmadd(gather(A, idx), x, 0.5f)`, `gather(A, idx) * x + 0.5f`, the way
a texture lookup times a weight plus a bias is usually written -- stays in bucket order: one partition, gather + fma + f + hsum and
the adjoint sums out of LDS-resident table slices whose {a, c} records all carry the scalar, and backward() is one fold.

Truth and bounds are those of the two-table step with B = full(K, c) (conftest.cfg3b_variant_truth, the reference build's
cfg3b_variant): unmasked, gather(B, idx) IS c in every lane.  Under a mask only the gather of A is masked: a masked-out lane's u is
fma(0, x, +-c) = +-c, not 0, and the truth is corrected for that in the test."""
import ctypes
import json

import numpy as np
import pytest

import oracle_lib as ol
from conftest import bits_equal, cfg3b_variant_truth, hash_u32, hsum_depth, uniform_pm1

pytestmark = pytest.mark.gpu
N, K = 1 << 20, (1 << 18) + 5

# spelling -> (the two-table spelling with the same signs, sign of c as it enters u, the kernel that consumed the gather in
# ELEMENT order before this shape stayed in bucket order)
SPELLINGS = {
    "fmadd": ("fmadd", +1, "gather_fmadd"),
    "fmsub": ("fmadd", -1, "gather_fmsub"),
    "fnmadd": ("b-a*x", +1, "gather_fnmadd"),
    "fnmsub": ("b-a*x", -1, "gather_fnmsub"),
    "a*x+c": ("a*x+b", +1, "gather_mul"),
    "c+a*x": ("b+a*x", +1, "gather_mul"),
    "a*x-c": ("a*x+b", -1, "gather_mul"),
    "c-a*x": ("b-a*x", +1, "gather_mul"),
}
ELEMENT_ORDER = ("gather", "gather_pair_fmadd", "scatter_add_partition", "scatter_add_count", "hsum_map")


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


@pytest.fixture(scope="module")
def ref():
    try:
        return ol.ref()
    except Exception:
        pytest.skip("oracle/_ref is not built")


@pytest.fixture(scope="module")
def data():
    A, x = uniform_pm1(K, 6), uniform_pm1(N, 2)
    idx = (hash_u32(np.arange(N, dtype=np.uint64), 4) % np.uint32(K)).astype(np.uint32)
    mask = (hash_u32(np.arange(N, dtype=np.uint64), 5) & 3) != 0             # 75 % active, drawn like test_neighbours_gpu.py
    return A, x, idx, mask


_truths = {}


def truth(data, spelling, c, func="sin", seed=1.0, masked=False):
    """the two-table truth with B = full(K, +-c), computed once per case and shared"""
    key = (spelling, c, func, seed, masked)
    if key not in _truths:
        A, x, idx, mask = data
        two, sign, _ = SPELLINGS[spelling]
        B = np.full(K, sign * c, np.float32)
        _truths[key] = (B, cfg3b_variant_truth(A, B, x, idx, mask=mask if masked else None, func=func, seed=seed, spelling=two))
    return _truths[key]


def kernels(m, fn):
    m.hip_profile_begin()
    out = fn()
    prof = json.loads(m.hip_profile_end())
    return out, {k["kernel"]: k["launches"] for k in prof if k["launches"]}


def expression(ad, a, xd, c, spelling, F):
    cc = F(c)
    return {"fmadd": lambda: ad.fmadd(a, xd, cc), "fmsub": lambda: ad.fmsub(a, xd, cc), "fnmadd": lambda: ad.fnmadd(a, xd, cc),
            "fnmsub": lambda: ad.fnmsub(a, xd, cc), "a*x+c": lambda: a * xd + cc, "c+a*x": lambda: cc + a * xd,
            "a*x-c": lambda: a * xd - cc, "c-a*x": lambda: cc - a * xd}[spelling]()


def run(ad, A, x, idx, c, spelling="fmadd", func="sin", seed=1.0, mask=None, f64=False):
    F = ad.Float64 if f64 else ad.Float32
    dA = F(A)
    ad.set_requires_gradient(dA)
    di, xd = ad.UInt32(idx), F(x)
    a = ad.gather(dA, di, ad.Mask(mask)) if mask is not None else ad.gather(dA, di)
    y = ad.hsum(getattr(ad, func)(expression(ad, a, xd, c, spelling, F)))
    z = y if seed == 1.0 else y * seed
    ad.backward(z)
    return float(ad.detach(z).numpy()[0]), ad.gradient(dA).numpy()


def assert_bucket_order(ks, spelling, partitions=1):
    assert ks.get("bucket_partition") == partitions, ks
    assert ks.get("bucket_pair_fma_reduce_adjoint") == partitions and "bucket_accumulate" not in ks, ks
    assert ks.get("scatter_add_fold") == partitions, ks          # backward(): ONE fold of the per-piece tables, nothing else
    assert not any(k in ks for k in ELEMENT_ORDER + (SPELLINGS[spelling][2],)), ks


def assert_in_bounds(y, gA, t, extra_y=0.0, truth_shift=0.0):
    ty = t["y"] + truth_shift
    assert abs(y - ty) <= t["y_bound"] + extra_y, (y, ty, t["y_bound"] + extra_y)
    err = np.abs(gA - t["gA"])
    assert np.all(err <= t["gA_bound"]), float((err / np.maximum(t["gA_bound"], 1e-30)).max())


CASES = [(s, "sin", 0.5, 1.0) for s in SPELLINGS] + [
    ("fmsub", "cos", -0.25, 1.0), ("c-a*x", "cos", -0.25, 1.0),
    ("fnmadd", "exp", 0.5, 2.0), ("a*x-c", "exp", 0.5, 2.0),
    ("c+a*x", "sqrt", 3.0, 1.0),                                  # u > 0
    ("fmadd", "sin", 0.0, 1.0), ("a*x+c", "sin", 0.0, 1.0),       # c = +0.0: the one whose zeros differ from the bare product's
]


@pytest.mark.parametrize("spelling,func,c,seed", CASES, ids=[f"{s}-{f}-{c}" for s, f, c, _ in CASES])
def test_scalar_addend_matches_the_reference_and_stays_in_bucket_order(ad, ref, data, spelling, func, c, seed):
    """Before this shape stayed in bucket order the gather was consumed in ELEMENT order -- by `gather_fmadd` / `gather_fmsub` /
    `gather_fnmadd` / `gather_fnmsub` for the fma family, by `gather_mul` (and an `add` / `sub` of its own) for the operator
    spellings -- followed by `hsum_map` and an element-order scatter_add (`scatter_add_count`, `scatter_add_partition`).  None of
    them may appear any more: one partition, the forward + adjoint kernel, one fold."""
    A, x, idx, _ = data
    if c == 0.0:
        # lanes whose product is a zero of either sign: a*x + (+0) is +0 where the bare product (staged with -0) keeps -0
        x = x.copy(); x[:4] = (0.0, -0.0, 0.0, -0.0)
        A = A.copy(); A[idx[5]] = 0.0
        B = np.full(K, 0.0, np.float32)
        t = cfg3b_variant_truth(A, B, x, idx, func=func, seed=seed, spelling=SPELLINGS[spelling][0])
    else:
        B, t = truth(data, spelling, c, func, seed)
    (y, gA), ks = kernels(ad, lambda: run(ad, A, x, idx, c, spelling, func, seed))
    assert_in_bounds(y, gA, t)
    assert abs(y - t["y"]) <= t["y_stat_bound"], (y, t["y"], t["y_stat_bound"])
    ry, rgA, _, _ = ref.cfg3b_variant(A, B, x, idx, func=func, seed=seed, spelling=SPELLINGS[spelling][0])
    assert abs(y - ry) <= t["y_bound"] + abs(ry - t["y"])
    assert np.all(np.abs(gA - rgA) <= 2 * t["gA_bound"])
    assert_bucket_order(ks, spelling)
    if c == 0.0:
        # the bits of u, element order: one rounding of the exact product for the fma, the rounded product for the operators --
        # the same number either way -- plus +0: no lane is -0
        di, xd, dA = ad.UInt32(idx), ad.Float32(x), ad.Float32(A)
        u = expression(ad, ad.gather(dA, di), xd, 0.0, spelling, ad.Float32)
        assert "host scalar" in u.explain()
        want = (A.astype(np.float64)[idx] * x.astype(np.float64)).astype(np.float32) + np.float32(0.0)
        assert np.count_nonzero(want == 0) >= 5 and not np.any(np.signbit(want[want == 0]))
        # ... and in bucket order: 1 / u tells the zeros apart (order-independent, so bit for bit)
        lo = ad.hmin(ad.rcp(u)).numpy()
        got = u.numpy()                                            # (forces u in element order)
        assert bits_equal(got, want)
        assert np.isfinite(lo[0]) or lo[0] == np.inf
        assert bits_equal(lo, ad.hmin(ad.rcp(ad.Float32(want))).numpy())


@pytest.mark.parametrize("spelling", ["fmadd", "a*x-c"])
@pytest.mark.parametrize("func,c", [("sin", 0.5), ("exp", 0.5)])
def test_masked_gathers_count_the_scalar_in_the_dropped_lanes(ad, data, spelling, func, c):
    """Only the gather is masked: a masked-out lane's u is fma(0, x, +-c) = +-c (-c for fmsub / fnmsub / a*x - c), so it adds
    f(+-c) to y where the two-table truth (both gathers masked, u = 0) has f(0).  It gives no gradient."""
    A, x, idx, mask = data
    _, t = truth(data, spelling, c, func, 1.0, masked=True)
    f = {"sin": np.sin, "exp": np.exp}[func]
    sc = float(SPELLINGS[spelling][1] * c)
    n_off = int(np.count_nonzero(~mask))
    (y, gA), ks = kernels(ad, lambda: run(ad, A, x, idx, c, spelling, func, mask=mask))
    assert_in_bounds(y, gA, t, extra_y=2.0 ** -24 * hsum_depth(N) * n_off * abs(f(sc)), truth_shift=n_off * (f(sc) - f(0.0)))
    assert_bucket_order(ks, spelling)


def test_masked_out_lane_with_an_infinite_x_is_nan(ad, data):
    A, x, idx, mask = data
    x = x.copy()
    off = np.flatnonzero(~mask)
    x[off[off.size // 3]] = np.inf                                 # u = fma(0, inf, c) = NaN, like the lane-by-lane evaluation
    (y, gA), ks = kernels(ad, lambda: run(ad, A, x, idx, 0.5, mask=mask))
    assert np.isnan(y) and np.all(np.isfinite(gA))
    assert_bucket_order(ks, "fmadd")


def test_sin_and_cos_steps_are_bit_reproducible(ad, data):
    """K <= 1 Mi: the adjoint sums of sin / cos are formed in 64-bit fixed point -- the order of the additions cannot matter"""
    A, x, idx, _ = data
    for func, c in (("sin", 0.5), ("cos", -0.25)):
        y1, g1 = run(ad, A, x, idx, c, "fmadd", func)
        y2, g2 = run(ad, A, x, idx, c, "fmadd", func)
        assert np.float32(y1).tobytes() == np.float32(y2).tobytes(), func
        assert bits_equal(g1, g2), func


def test_float64(ad):
    """the kernel family as the two-table float64 step shows it: count / scan / partition lists, the forward + adjoint kernel,
    a fold -- bounds from the float64 evaluation with eps = 2^-53"""
    n, k, c = 1 << 19, (1 << 15) + 3, 0.5
    A, x = uniform_pm1(k, 6).astype(np.float64), uniform_pm1(n, 2).astype(np.float64)
    idx = (hash_u32(np.arange(n, dtype=np.uint64), 4) % np.uint32(k)).astype(np.uint32)
    (y, gA), ks = kernels(ad, lambda: run(ad, A, x, idx, c, f64=True))
    eps = 2.0 ** -53
    u = A[idx] * x + c
    s, cs = np.sin(u), np.cos(u) * x
    cnt = np.bincount(idx, minlength=k)
    assert abs(y - s.sum()) <= eps * (hsum_depth(n) * np.abs(s).sum() + 8 * n)
    want = np.bincount(idx, weights=cs, minlength=k)
    assert np.all(np.abs(gA - want) <= eps * (cnt * np.bincount(idx, weights=np.abs(cs), minlength=k) + 8 * cnt))
    assert ks.get("bucket_count") == 1 and ks.get("bucket_scan") == 1 and ks.get("bucket_partition") == 1, ks
    assert ks.get("bucket_pair_fma_reduce_adjoint") == 1 and ks.get("scatter_add_fold") == 1 and "bucket_accumulate" not in ks, ks
    assert not any(kk in ks for kk in ELEMENT_ORDER + ("gather_fmadd",)), ks


def test_sliced_table(ad):
    """K > 8 Mi float32 entries: one object per slice, each stages the scalar.  Eager only (no capture at this size)."""
    n, k, c = 1 << 22, (9 << 20) + 7, 0.5
    A, x = uniform_pm1(k, 6), uniform_pm1(n, 2)
    idx = (hash_u32(np.arange(n, dtype=np.uint64), 4) % np.uint32(k)).astype(np.uint32)
    span = 1 << 22
    idx[idx // span == 1] %= np.uint32(span)                        # slice 1 receives no element
    (y, gA), ks = kernels(ad, lambda: run(ad, A, x, idx, c))
    t = cfg3b_variant_truth(A, np.full(k, c, np.float32), x, idx)
    assert_in_bounds(y, gA, t)
    assert ks.get("bucket_slice_partition") == 1, ks
    assert not any(kk in ks for kk in ELEMENT_ORDER + ("gather_fmadd",)), ks
    assert np.array_equal(gA[span:2 * span], np.zeros(span, np.float32))


def _refill(capi, arr, host):
    host = np.ascontiguousarray(host)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(arr.data_ptr()), host.ctypes.data_as(ctypes.c_void_p),
                                                ctypes.c_size_t(host.nbytes)))


def test_step_graph(ad, capi, data):
    A, hx, hidx, _ = data
    c = 0.5
    A0, x, idx = ad.Float32(A), ad.Float32(hx), ad.UInt32(hidx)
    out = {}

    def step():
        dA = ad.Float32(A0)
        ad.set_requires_gradient(dA)
        y = ad.hsum(ad.sin(ad.fmadd(ad.gather(dA, idx), x, ad.Float32(c))))
        ad.backward(y)
        out["y"], out["gA"] = ad.detach(y), ad.gradient(dA)

    def check(t):
        assert_in_bounds(float(out["y"].numpy()[0]), out["gA"].numpy(), t)

    _, t = truth(data, "fmadd", c)
    l0 = ad.hip_launch_count()
    _, ks = kernels(ad, step)
    eager_launches = ad.hip_launch_count() - l0
    check(t)
    assert_bucket_order(ks, "fmadd")
    ad.hip_graph_begin()
    step()
    g = ad.hip_graph_end()
    try:
        per_step = ad.hip_graph_launch_count(g)
        # (an eager step may skip the clear of a reused block of partition counters)
        assert eager_launches <= per_step <= eager_launches + 1, (eager_launches, per_step)
        ad.hip_graph_launch(g)
        check(t)
        hx2 = uniform_pm1(N, 12)
        hidx2 = (hash_u32(np.arange(N, dtype=np.uint64), 14) % np.uint32(K)).astype(np.uint32)
        _refill(capi, x, hx2)
        _refill(capi, idx, hidx2)
        ad.hip_graph_launch(g)
        check(cfg3b_variant_truth(A, np.full(K, c, np.float32), hx2, hidx2))
    finally:
        ad.hip_graph_destroy(g)


def test_c_abi_directly(capi, data):
    A, x, idx, _ = data
    c = 0.5
    _, t = truth(data, "fmadd", c)
    dA, dx, di = capi.Buf.from_numpy(A), capi.Buf.from_numpy(x), capi.Buf.from_numpy(idx)
    b = capi.Bucketed("fmadd", dA, dx, c, di)
    try:
        y = float(b.reduce("hsum", "sin", keep=False).numpy()[0])
    finally:
        b.destroy()
    assert abs(y - t["y"]) <= t["y_bound"], (y, t["y"], t["y_bound"])
    h = ctypes.c_void_p()
    rc = capi.lib.ek_hip_bucketed_pair_create_scalar(dA.ek, di.ek, 99, ctypes.c_void_p(dA.ptr), ctypes.c_uint64(0), ctypes.c_size_t(dA.n),
                                                     ctypes.c_void_p(dx.ptr), ctypes.c_void_p(di.ptr), None, ctypes.c_size_t(di.n),
                                                     ctypes.c_uint(0), ctypes.byref(h))
    assert rc == -1 and not h.value            # EK_ERR_INVALID (enoki_hip.h: ek_status)


@pytest.mark.parametrize("module", ["enoki_amd.hip_autodiff", "enoki.hip_autodiff"])
def test_a_literal_addend_arrives_as_a_host_scalar(module, data):
    """`Float32(c)` is an immediate, not a size-1 device array: both spellings form the node (nothing runs), in either package"""
    import importlib
    m = importlib.import_module(module)
    m.hip_init(0)
    A, x, idx, _ = data
    dA = m.Float32(A)
    m.set_requires_gradient(dA)
    di, xd = m.UInt32(idx), m.Float32(x)
    assert "host scalar" in m.Float32(0.5).explain()
    l0 = m.hip_launch_count()
    u1 = m.fmadd(m.gather(dA, di), xd, m.Float32(0.5))
    u2 = m.gather(dA, di) * xd + m.Float32(0.5)
    u3 = m.gather(dA, di) * xd + 0.5                              # a python float takes the same path
    for u in (u1, u2, u3):
        assert "host scalar" in u.explain() and "BUCKET ORDER" in u.explain(), u.explain()
    assert m.hip_launch_count() == l0
