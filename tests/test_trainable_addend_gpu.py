"""`op(gather(A, idx[, mask]), x, c)` with a host scalar c that REQUIRES A GRADIENT -- the bias of "texture lookup times a weight plus
a bias" in a program that trains it -- stays in bucket order: the forward + adjoint kernel already sums f'(u) per table entry (plane 0 of
its per-piece tables), and backward() gets d/dc from ONE fold of that plane (ek_hip_bucketed_addend_adjoint) next to the fold for A.

Truth for gradient(c), float64:  sigma * seed * (sum over ALL n lanes of f'(u_i)),  sigma the sign of c in the spelling; a lane the
partition dropped has u = sigma c.  Bound, from the project's own terms (nothing fitted to the output):
    sum_k gB_bound[k]                        of conftest.cfg3b_variant_truth with B = full(K, sigma c): the per-entry sums
  + eps * hsum_depth(K) * sum_k |gB[k]|      the sum across the K entry values
  + eps * hsum_depth(N) * n_off * |f'(sigma c)|   the dropped lanes' term, as test_scalar_addend_gpu.py forms it for y."""
import json

import numpy as np
import pytest

import oracle_lib as ol
import test_scalar_addend_gpu as base
from conftest import bits_equal, cfg3b_variant_truth, hash_u32, hsum_depth, uniform_pm1

pytestmark = pytest.mark.gpu
N, K = base.N, base.K
SPELLINGS = base.SPELLINGS
EPS = 2.0 ** -24
# what the element-order evaluation of this shape launches (the parent sent a differentiable c there)
ELEMENT_ORDER = ("gather_fmadd", "gather_fmsub", "gather_fnmadd", "gather_fnmsub", "gather_mul", "hsum_map", "scatter_add_partition",
                 "scatter_add_count", "hsum_safe_mul")
DF = {"sin": np.cos, "cos": lambda v: -np.sin(v), "exp": np.exp, "sqrt": lambda v: 0.5 / np.sqrt(v)}


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


@pytest.fixture(scope="module")
def ref():
    """the reference build, or None (said aloud) where oracle/_ref does not exist; a build that FAILS is an error, not None"""
    try:
        return ol.ref()
    except FileNotFoundError as e:
        print(f"oracle/_ref is not built ({e}): the comparison with the reference's own gB does not run")
        return None


@pytest.fixture(scope="module")
def data():
    A, x = uniform_pm1(K, 6), uniform_pm1(N, 2)
    idx = (hash_u32(np.arange(N, dtype=np.uint64), 4) % np.uint32(K)).astype(np.uint32)
    mask = (hash_u32(np.arange(N, dtype=np.uint64), 5) & 3) != 0             # 75 % active, drawn like test_scalar_addend_gpu.py
    return A, x, idx, mask


def kernels(m, fn):
    """launches by kernel name, SUMMED: the profile keeps one entry per (name, size), so the slices of a large table -- same kernel,
    different table sizes -- come as several entries of one name"""
    m.hip_profile_begin()
    out = fn()
    ks = {}
    for k in json.loads(m.hip_profile_end()):
        if k["launches"]:
            ks[k["kernel"]] = ks.get(k["kernel"], 0) + k["launches"]
    return out, ks


def zipf_indices(n):
    """log-uniform indices as NEIGHBOURS["zipf"] (test_headline_parity_gpu.py) draws them, magnitudes 0 .. 17 so that every index is
    inside K = 2^18 + 5: entries 0 .. 4094 -- all of quarter-size bucket 0 -- receive the magnitudes 0 .. 11, two thirds of all lookups"""
    m = (hash_u32(np.arange(n, dtype=np.uint64), 8) % np.uint32(18)).astype(np.uint32)
    lo = ((np.uint32(1) << m) - np.uint32(1)).astype(np.uint32)
    return (lo + (hash_u32(np.arange(n, dtype=np.uint64), 9) & lo)).astype(np.uint32)


def step(ad, A, x, idx, c, spelling="fmadd", func="sin", seed=1.0, mask=None, f64=False, trainable=True, device=False):
    """one training step; (y, gA, gc) -- gc None when c does not require a gradient.  device: c as a size-1 DEVICE array"""
    F = ad.Float64 if f64 else ad.Float32
    dA, dc = F(A), (F(np.array([c], np.float64 if f64 else np.float32)) if device else F(c))
    ad.set_requires_gradient(dA)
    if trainable:
        ad.set_requires_gradient(dc)
    di, xd = ad.UInt32(idx), F(x)
    a = ad.gather(dA, di, ad.Mask(mask)) if mask is not None else ad.gather(dA, di)
    cc = dc
    u = {"fmadd": lambda: ad.fmadd(a, xd, cc), "fmsub": lambda: ad.fmsub(a, xd, cc), "fnmadd": lambda: ad.fnmadd(a, xd, cc),
         "fnmsub": lambda: ad.fnmsub(a, xd, cc), "a*x+c": lambda: a * xd + cc, "c+a*x": lambda: cc + a * xd,
         "a*x-c": lambda: a * xd - cc, "c-a*x": lambda: cc - a * xd}[spelling]()
    y = ad.hsum(getattr(ad, func)(u))
    z = y if seed == 1.0 else y * seed
    ad.backward(z)
    gc = float(ad.gradient(dc).numpy()[0]) if trainable else None
    return float(ad.detach(z).numpy()[0]), ad.gradient(dA).numpy(), gc


def gc_truth(t, sigma, c, func, seed, n_off=0, eps=EPS, n=N):
    """(truth, bound) of gradient(c) from the two-table truth `t` with B = full(K, sigma c); n_off lanes were dropped"""
    k = t["gB"].size
    dropped = n_off * seed * float(DF[func](np.float64(sigma * c)))
    want = sigma * (float(t["gB"].sum()) + dropped)
    bound = float(t["gB_bound"].sum()) + eps * hsum_depth(k) * float(np.abs(t["gB"]).sum()) + eps * hsum_depth(n) * abs(dropped)
    return want, bound


def assert_bucket_order(ks, spelling, folds=1):
    base.assert_bucket_order(ks, spelling)
    assert ks.get("addend_adjoint_fold") == folds, ks               # the gradient of c: ONE fold of plane 0
    assert not any(k in ks for k in ELEMENT_ORDER), ks


CASES = [(s, "sin", 0.5, 1.0) for s in SPELLINGS] + [
    ("fmsub", "cos", -0.25, 1.0), ("c-a*x", "cos", -0.25, 1.0),
    ("fnmadd", "exp", 0.5, 2.0), ("a*x-c", "exp", 0.5, 2.0),
    ("c+a*x", "sqrt", 3.0, 1.0), ("fmadd", "sqrt", 3.0, 2.0),     # u > 0
    ("fmadd", "sin", 0.5, 2.0),
]


@pytest.mark.parametrize("spelling,func,c,seed", CASES, ids=[f"{s}-{f}-{c}-{sd}" for s, f, c, sd in CASES])
def test_trainable_host_scalar_stays_in_bucket_order(ad, ref, data, spelling, func, c, seed):
    """Fails without ek_hip_bucketed_addend_adjoint: DiffArray's guard sent a scalar addend that requires a gradient to the
    element-order kernels (`gather_fmadd` / `gather_mul`, `hsum_map`, an element-order scatter_add, `hsum_safe_mul` for c)."""
    A, x, idx, _ = data
    B, t = base.truth(data, spelling, c, func, seed)
    sigma = SPELLINGS[spelling][1]
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, c, spelling, func, seed))
    want, bound = gc_truth(t, sigma, c, func, seed)
    print(f"gc {gc!r} truth {want!r} |error| {abs(gc - want):.3e} bound {bound:.3e}")
    base.assert_in_bounds(y, gA, t)
    assert abs(gc - want) <= bound, (gc, want, bound)
    if ref is not None:
        _, _, rgB, _ = ref.cfg3b_variant(A, B, x, idx, func=func, seed=seed, spelling=SPELLINGS[spelling][0])
        assert abs(gc - sigma * float(rgB.astype(np.float64).sum())) <= 2 * bound
    assert_bucket_order(ks, spelling)
    if func in ("sin", "cos"):
        # the fixed-point path: the step with a constant c gives the same bits -- the fold for c is on top of it, not instead
        y0, gA0, _ = step(ad, A, x, idx, c, spelling, func, seed, trainable=False)
        assert np.float32(y).tobytes() == np.float32(y0).tobytes() and bits_equal(gA, gA0)


DEVICE_CASES = [("fmadd", "sin", 0.5, 1.0), ("a*x-c", "sin", 0.5, 1.0), ("fnmsub", "cos", -0.25, 1.0), ("c-a*x", "exp", 0.5, 2.0)]


@pytest.mark.parametrize("trainable", [True, False], ids=["differentiable", "constant"])
@pytest.mark.parametrize("spelling,func,c,seed", DEVICE_CASES, ids=[f"{s}-{f}-{c}-{sd}" for s, f, c, sd in DEVICE_CASES])
def test_device_scalar_stays_in_bucket_order(ad, ref, data, spelling, func, c, seed, trainable):
    """c = Float32(np.array([0.5], np.float32)): a size-1 DEVICE array, what c is after `c = c - lr * gradient(c)`.  Fails without
    ek_hip_bucketed_pair_create_scalar_device: that shape ran in element order ("its value is not known on the host")."""
    A, x, idx, _ = data
    B, t = base.truth(data, spelling, c, func, seed)
    sigma = SPELLINGS[spelling][1]
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, c, spelling, func, seed, trainable=trainable, device=True))
    base.assert_in_bounds(y, gA, t)
    base.assert_bucket_order(ks, spelling)
    assert not any(k in ks for k in ELEMENT_ORDER), ks
    if trainable:
        want, bound = gc_truth(t, sigma, c, func, seed)
        print(f"gc {gc!r} truth {want!r} |error| {abs(gc - want):.3e} bound {bound:.3e}")
        assert abs(gc - want) <= bound, (gc, want, bound)
        if ref is not None:
            _, _, rgB, _ = ref.cfg3b_variant(A, B, x, idx, func=func, seed=seed, spelling=SPELLINGS[spelling][0])
            assert abs(gc - sigma * float(rgB.astype(np.float64).sum())) <= 2 * bound
        assert ks.get("addend_adjoint_fold") == 1, ks
        if func in ("sin", "cos"):
            y0, gA0, _ = step(ad, A, x, idx, c, spelling, func, seed, trainable=False, device=True)
            assert np.float32(y).tobytes() == np.float32(y0).tobytes() and bits_equal(gA, gA0)
    else:
        assert "addend_adjoint_fold" not in ks, ks


def test_forming_the_node_with_a_device_scalar_launches_nothing(ad, data):
    A, x, idx, _ = data
    dA, di, xd = ad.Float32(A), ad.UInt32(idx), ad.Float32(x)
    dc = ad.Float32(np.array([0.5], np.float32))
    ad.set_requires_gradient(dA)
    ad.set_requires_gradient(dc)
    assert "evaluated array" in dc.explain()
    l0 = ad.hip_launch_count()
    u1 = ad.fmadd(ad.gather(dA, di), xd, dc)
    u2 = ad.gather(dA, di) * xd - dc
    for u in (u1, u2):
        assert "device addend" in u.explain() and "BUCKET ORDER" in u.explain(), u.explain()
    assert ad.hip_launch_count() == l0


def test_step_graph_with_a_device_scalar(ad, capi, data):
    """the captured step reads c on the stream: a replay sees the value the element holds at replay time"""
    A, hx, hidx, _ = data
    A0, x, idx = ad.Float32(A), ad.Float32(hx), ad.UInt32(hidx)
    c_dev = ad.Float32(np.array([0.5], np.float32))
    out = {}

    def one():
        dA, dc = ad.Float32(A0), ad.Float32(c_dev)
        ad.set_requires_gradient(dA)
        ad.set_requires_gradient(dc)
        y = ad.hsum(ad.sin(ad.fmadd(ad.gather(dA, idx), x, dc)))
        ad.backward(y)
        out["y"], out["gA"], out["gc"] = ad.detach(y), ad.gradient(dA), ad.gradient(dc)

    def check(t, c):
        base.assert_in_bounds(float(out["y"].numpy()[0]), out["gA"].numpy(), t)
        want, bound = gc_truth(t, 1, c, "sin", 1.0)
        gc = float(out["gc"].numpy()[0])
        print(f"gc {gc!r} truth {want!r} |error| {abs(gc - want):.3e} bound {bound:.3e}")
        assert abs(gc - want) <= bound, (gc, want, bound)

    _, t = base.truth(data, "fmadd", 0.5)
    l0 = ad.hip_launch_count()
    _, ks = kernels(ad, one)
    eager_launches = ad.hip_launch_count() - l0
    check(t, 0.5)
    assert_bucket_order(ks, "fmadd")
    ad.hip_graph_begin()
    one()
    g = ad.hip_graph_end()
    try:
        per_step = ad.hip_graph_launch_count(g)
        assert eager_launches - 1 <= per_step <= eager_launches + 1, (eager_launches, per_step)
        ad.hip_graph_launch(g)
        check(t, 0.5)
        hx2 = uniform_pm1(N, 12)
        hidx2 = (hash_u32(np.arange(N, dtype=np.uint64), 14) % np.uint32(K)).astype(np.uint32)
        c2 = np.float32(-0.75)
        base._refill(capi, x, hx2)
        base._refill(capi, idx, hidx2)
        base._refill(capi, c_dev, np.array([c2], np.float32))
        ad.hip_graph_launch(g)
        check(cfg3b_variant_truth(A, np.full(K, c2, np.float32), hx2, hidx2), float(c2))
    finally:
        ad.hip_graph_destroy(g)


def test_three_optimiser_steps_on_arrays_stay_in_bucket_order(ad, data):
    """c = c - 0.1 * gradient(c) on ARRAYS, for the mean y = hsum(sin(u)) / N (seed 2^-20): from step 2 on c is a size-1 device array.
    Every step is one partition, the forward + adjoint kernel and the two folds; c after step 3 against the float64 loop, bound
    propagated as in the host-scalar loop below."""
    A, x, idx, _ = data
    seed = 2.0 ** -20
    c, c64, err = ad.Float32(0.5), 0.5, 0.0
    ax64 = A.astype(np.float64)[idx] * x.astype(np.float64)
    state = {}

    def one():
        dA, dc = ad.Float32(A), ad.Float32(state["c"])
        ad.set_requires_gradient(dA)
        ad.set_requires_gradient(dc)
        z = ad.hsum(ad.sin(ad.fmadd(ad.gather(dA, ad.UInt32(idx)), ad.Float32(x), dc))) * seed
        ad.backward(z)
        state["new"] = ad.detach(dc) - ad.gradient(dc) * 0.1

    for k in range(3):
        state["c"] = c
        c32_before = np.float32(c.numpy()[0])
        _, ks = kernels(ad, one)
        assert_bucket_order(ks, "fmadd")
        c = state["new"]
        assert "evaluated array" in c.explain(), c.explain()               # a size-1 DEVICE array from here on
        t = cfg3b_variant_truth(A, np.full(K, c32_before, np.float32), x, idx, seed=seed)
        _, bound = gc_truth(t, 1, float(c32_before), "sin", seed)
        u64 = ax64 + c64
        err = err + 0.1 * (bound + seed * float(np.abs(np.sin(u64)).sum()) * err) + 4 * EPS * (abs(c64) + 0.1)
        c64 = c64 - 0.1 * seed * float(np.cos(u64).sum())
        got = float(c.numpy()[0])
        print(f"c {got!r} float64 loop {c64!r} |error| {abs(got - c64):.3e} bound {err:.3e}")
        assert abs(got - c64) <= err, (got, c64, err)


@pytest.mark.parametrize("spelling,func,c", [("fmadd", "sin", 0.5), ("a*x-c", "sin", 0.5), ("fmsub", "exp", 0.5)])
def test_masked_gathers_count_the_dropped_lanes_in_the_gradient(ad, data, spelling, func, c):
    """a masked-out lane's u is +-c: it adds f'(+-c) to the gradient of c (and nothing to the gradient of A)"""
    A, x, idx, mask = data
    _, t = base.truth(data, spelling, c, func, 1.0, masked=True)
    sigma = SPELLINGS[spelling][1]
    n_off = int(np.count_nonzero(~mask))
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, c, spelling, func, mask=mask))
    want, bound = gc_truth(t, sigma, c, func, 1.0, n_off=n_off)
    print(f"gc {gc!r} truth {want!r} |error| {abs(gc - want):.3e} bound {bound:.3e}")
    assert abs(gc - want) <= bound, (gc, want, bound)
    assert np.all(np.abs(gA - t["gA"]) <= t["gA_bound"])
    assert_bucket_order(ks, spelling)


def test_dropped_lane_with_an_infinite_x_makes_the_gradient_nan(ad, data):
    A, x, idx, mask = data
    x = x.copy()
    off = np.flatnonzero(~mask)
    x[off[off.size // 3]] = np.inf                                 # u = fma(0, inf, c) = NaN, like the lane-by-lane evaluation
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, 0.5, mask=mask))
    assert np.isnan(y) and np.isnan(gc) and np.all(np.isfinite(gA))
    assert_bucket_order(ks, "fmadd")


@pytest.mark.parametrize("indices,func", [("uniform", "sin"), ("zipf", "sin"), ("uniform", "exp"), ("zipf", "exp")])
def test_every_layout_of_plane_0(ad, capi, data, indices, func):
    """uniform + sin: every bucket is one piece and holds floats; zipf + sin: the hot bucket is cut into several pieces that hold
    64-bit fixed-point sums; exp: half-size buckets whose pieces ran under the exchange locks and hold floats.
    Which layout a case really has is read from the partition itself: the same (index, x) with the hints the tape gives
    (reduce_bucketed_: ADJOINT, and BOUNDED for sin / cos) through capi, and ek_hip_bucketed_piece_counts."""
    A, x, idx, _ = data
    c = 0.5
    if indices == "zipf":
        idx = zipf_indices(N)
        assert int(idx.max()) < K
    hints = capi.Bucketed.HINT_ADJOINT | (capi.Bucketed.HINT_BOUNDED if func == "sin" else 0)
    b = capi.Bucketed("fmadd", capi.Buf.from_numpy(A), capi.Buf.from_numpy(x), c, capi.Buf.from_numpy(idx), hints=hints)
    try:
        pieces, largest = b.piece_counts()
    finally:
        b.destroy()
    print(f"{indices} {func}: {pieces} pieces, at most {largest} per bucket")
    assert pieces >= 1 and (largest > 1 if indices == "zipf" else largest == 1), (pieces, largest)
    t = cfg3b_variant_truth(A, np.full(K, c, np.float32), x, idx, func=func)
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, c, "fmadd", func))
    want, bound = gc_truth(t, 1, c, func, 1.0)
    print(f"gc {gc!r} truth {want!r} |error| {abs(gc - want):.3e} bound {bound:.3e}")
    base.assert_in_bounds(y, gA, t)
    assert abs(gc - want) <= bound, (gc, want, bound)
    assert_bucket_order(ks, "fmadd")


def test_sin_and_cos_steps_are_bit_reproducible(ad, data):
    """fixed-point entry sums, then additions in an order fixed by the entry index: y, gA AND gc repeat bit for bit"""
    A, x, idx, _ = data
    for func, c, ii in (("sin", 0.5, idx), ("cos", -0.25, idx), ("sin", 0.5, zipf_indices(N))):
        y1, g1, c1 = step(ad, A, x, ii, c, "fmadd", func)
        y2, g2, c2 = step(ad, A, x, ii, c, "fmadd", func)
        assert np.float32(y1).tobytes() == np.float32(y2).tobytes(), func
        assert bits_equal(g1, g2) and np.float32(c1).tobytes() == np.float32(c2).tobytes(), func


def test_float64(ad):
    """no finish ticket for 8-byte elements: the fold, then the small final launch.  eps = 2^-53."""
    n, k, c = 1 << 19, (1 << 15) + 3, 0.5
    A, x = uniform_pm1(k, 6).astype(np.float64), uniform_pm1(n, 2).astype(np.float64)
    idx = (hash_u32(np.arange(n, dtype=np.uint64), 4) % np.uint32(k)).astype(np.uint32)
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, c, f64=True))
    eps = 2.0 ** -53
    u = A[idx] * x + c
    s, cs = np.sin(u), np.cos(u)
    cnt = np.bincount(idx, minlength=k)
    assert abs(y - s.sum()) <= eps * (hsum_depth(n) * np.abs(s).sum() + 8 * n)
    gB = np.bincount(idx, weights=cs, minlength=k)
    gB_bound = eps * (cnt * np.bincount(idx, weights=np.abs(cs), minlength=k) + 8 * cnt)
    bound = float(gB_bound.sum()) + eps * hsum_depth(k) * float(np.abs(gB).sum())
    print(f"gc {gc!r} truth {float(gB.sum())!r} |error| {abs(gc - gB.sum()):.3e} bound {bound:.3e}")
    assert abs(gc - float(gB.sum())) <= bound
    assert ks.get("bucket_pair_fma_reduce_adjoint") == 1 and ks.get("scatter_add_fold") == 1 and ks.get("addend_adjoint_fold") == 1, ks
    assert not any(kk in ks for kk in ELEMENT_ORDER), ks


@pytest.mark.parametrize("k", [(1 << 20) + 5, (1 << 21) + 5, (1 << 22) + 5], ids=["K1Mi+5", "K2Mi+5", "K4Mi+5"])
def test_large_tables(ad, k):
    """K = 2^20 + 5: beyond the fixed-point tables, half-size buckets, float planes, one fold.
    K = 2^21 + 5: two slices of half-size buckets (the second holds five entries and receives no element): one fold PER SLICE and the
    launch that combines them; a lane that one slice dropped is the other's -- it must be counted once.
    K = 2^22 + 5: two slices of FULL-size buckets -- the forward pass forms no early sums there (enoki_hip.h: the adjoint hint is
    ignored beyond 256 half-size buckets per slice pair), so the gradient of c is the bucket-ordered reduction per slice, by design."""
    n, c = 1 << 20, 0.5
    A, x = uniform_pm1(k, 6), uniform_pm1(n, 2)
    idx = (hash_u32(np.arange(n, dtype=np.uint64), 4) % np.uint32(k)).astype(np.uint32)
    last = np.uint32((k - 5))
    idx[idx >= last] %= last                                        # the five entries of the last bucket / slice receive nothing
    (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, c))
    print(ks)
    t = cfg3b_variant_truth(A, np.full(k, c, np.float32), x, idx)
    want, bound = gc_truth(t, 1, c, "sin", 1.0, n=n)
    print(f"gc {gc!r} truth {want!r} |error| {abs(gc - want):.3e} bound {bound:.3e}")
    base.assert_in_bounds(y, gA, t)
    assert abs(gc - want) <= bound, (gc, want, bound)
    assert not any(kk in ks for kk in ELEMENT_ORDER), ks
    slices = 1 if k < (1 << 21) else 2
    assert ks.get("bucket_partition") == slices, ks
    if k < (1 << 22):
        assert ks.get("bucket_pair_fma_reduce_adjoint") == slices and ks.get("addend_adjoint_fold") == slices, ks
        assert ks.get("scatter_add_fold") == slices and "bucket_accumulate" not in ks, ks
        assert ks.get("reduce_stage2", 0) == (2 if slices == 2 else 0), ks              # the launches that combine the slices
    else:
        assert "addend_adjoint_fold" not in ks and "bucket_pair_fma_reduce_adjoint" not in ks, ks
        # per slice: the forward reduction (which keeps u in list order), the reduction of cos over the kept u for c, and the
        # accumulation + fold for A; the two combine launches
        assert ks.get("bucket_pair_fma_reduce") == slices and ks.get("bucket_reduce_kept") == slices, ks
        assert ks.get("bucket_accumulate") == slices and ks.get("scatter_add_fold") == slices and ks.get("reduce_stage2") == 2, ks


def test_c_abi_directly(ad, capi, data):
    A, x, idx, _ = data
    c = 0.5
    _, t = base.truth(data, "fmadd", c)
    want, bound = gc_truth(t, 1, c, "sin", 1.0)
    dA, dx, di = capi.Buf.from_numpy(A), capi.Buf.from_numpy(x), capi.Buf.from_numpy(idx)

    def run(hints, **keep):
        b = capi.Bucketed("fmadd", dA, dx, c, di, hints=hints)
        try:
            y = float(b.reduce("hsum", "sin", **keep).numpy()[0])
            return y, float(b.addend_adjoint("cos").numpy()[0]), float(b.addend_adjoint("cos", scale=-2.0).numpy()[0])
        finally:
            b.destroy()

    # hinted: the reduce call formed the sums of cos(u) per entry -- answered from plane 0
    (y, gc, gc2), ks = kernels(ad, lambda: run(capi.Bucketed.HINT_ADJOINT | capi.Bucketed.HINT_BOUNDED, keep=True, keep_op="cos"))
    assert abs(y - t["y"]) <= t["y_bound"]
    assert abs(gc - want) <= bound and abs(gc2 + 2.0 * want) <= 2.0 * bound + 2.0 * EPS * abs(want), (gc, gc2, want, bound)
    assert ks.get("addend_adjoint_fold") == 2 and ks.get("bucket_pair_fma_reduce_adjoint") == 1 and "bucket_pair_fma_reduce" not in ks, ks
    # unhinted: no early sums -- one bucket-ordered reduction per call, same bounds (plus the depth of that reduction's own tree)
    (y, gc, gc2), ks = kernels(ad, lambda: run(0, keep=False))
    slack = EPS * hsum_depth(N) * float(np.abs(t["gB"]).sum())
    assert abs(gc - want) <= bound + slack and abs(gc2 + 2.0 * want) <= 2.0 * (bound + slack) + 2.0 * EPS * abs(want), (gc, gc2, want, bound)
    assert "addend_adjoint_fold" not in ks and ks.get("bucket_pair_fma_reduce") == 3, ks
    assert not any(kk in ks for kk in ELEMENT_ORDER), ks
    # a two-table object has no scalar addend
    two = capi.Bucketed("fmadd", dA, dx, capi.Buf.from_numpy(np.full(K, c, np.float32)), di)
    try:
        with pytest.raises(capi.EnokiHipError, match=r"\[-1\]"):           # EK_ERR_INVALID (enoki_hip.h: ek_status)
            two.addend_adjoint("cos")
    finally:
        two.destroy()


def test_three_optimiser_steps_stay_in_bucket_order(ad, data):
    """c <- c - 0.1 * gradient(c) for the mean y = hsum(sin(u)) / N (seed 2^-20, so that a step moves c by less than 0.1), the new value
    handed back as a host scalar: every step is one partition, the forward + adjoint kernel and the two folds.  c after step 3 against
    the float64 loop: the error of gc is its bound plus |d gc / dc| <= seed * sum |sin(u)| times the error c already has; a step
    adds 0.1 times that and the roundings of the update."""
    A, x, idx, _ = data
    seed = 2.0 ** -20
    c32, c64, err = np.float32(0.5), 0.5, 0.0
    ax64 = A.astype(np.float64)[idx] * x.astype(np.float64)
    for _ in range(3):
        (y, gA, gc), ks = kernels(ad, lambda: step(ad, A, x, idx, float(c32), seed=seed))
        assert_bucket_order(ks, "fmadd")
        t = cfg3b_variant_truth(A, np.full(K, c32, np.float32), x, idx, seed=seed)
        _, bound = gc_truth(t, 1, float(c32), "sin", seed)
        u64 = ax64 + c64
        err = err + 0.1 * (bound + seed * float(np.abs(np.sin(u64)).sum()) * err) + 4 * EPS * (abs(c64) + 0.1)
        c64 = c64 - 0.1 * seed * float(np.cos(u64).sum())
        c32 = np.float32(c32 - np.float32(0.1) * np.float32(gc))
        print(f"c {float(c32)!r} float64 loop {c64!r} |error| {abs(float(c32) - c64):.3e} bound {err:.3e}")
        assert abs(float(c32) - c64) <= err, (float(c32), c64, err)
