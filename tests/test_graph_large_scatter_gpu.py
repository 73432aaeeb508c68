"""Element-order scatter_add of float32 values into more than 4 Mi bins inside step graphs: the pairs are split by slice of 4 Mi
bins, every slice partitions its own run into one page pool sized on the device, ONE launch adds all slices' pieces in the LDS and
ONE launch folds them.  Nothing is read back, so the call can be captured, and every replay follows the slice populations of the
index array it finds.  Truth is NumPy in float64; the bound is the class-D bound of test_scatter_add_binned_f32."""
import ctypes
import json

import numpy as np
import pytest

from conftest import hsum_depth

pytestmark = pytest.mark.gpu

SPAN = 1 << 22          # bins per slice of a float32 table (256 buckets of 16 Ki)
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def ek():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


def _refill(capi, arr, host):
    host = np.ascontiguousarray(host)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(arr.data_ptr()), host.ctypes.data_as(ctypes.c_void_p),
                                                ctypes.c_size_t(host.nbytes)))


def _skewed(rng, n, K):
    return ((rng.zipf(1.3, n).astype(np.uint64) * 2654435761) % K).astype(np.uint32)


def _truth(K, idx, val, target=None):
    """float64 sums per bin and the class-D bound count * 2^-24 * (|target| + sum |value|), count = additions into the bin + 1"""
    ii = idx.astype(np.int64)
    v = val.astype(np.float64)
    t0 = np.zeros(K) if target is None else target.astype(np.float64)
    truth = t0 + np.bincount(ii, weights=v, minlength=K)
    mag = np.abs(t0) + np.bincount(ii, weights=np.abs(v), minlength=K)
    cnt = np.bincount(ii, minlength=K) + 1
    return truth, cnt * EPS * mag + 1e-30


def _check(got, K, idx, val, what):
    truth, bound = _truth(K, idx, val)
    err = np.abs(got.astype(np.float64) - truth)
    worst = float((err / bound).max())
    print(f"{what}: max |got - truth| / bound = {worst:.3g}, max |err| = {float(err.max()):.3g}")
    assert np.all(err <= bound), (what, worst)


def _kernels(ek, fn):
    l0 = ek.hip_launch_count()
    ek.hip_profile_begin()
    fn()
    ks = {k["kernel"]: k["launches"] for k in json.loads(ek.hip_profile_end()) if k["launches"]}
    return ks, ek.hip_launch_count() - l0


def _assert_device_sized(ks, S, calls=1):
    # the split by slice under its own names, a partition and a directory per slice, nothing of the host-sized path
    assert ks.get("scatter_add_slice_count") == calls and ks.get("scatter_add_slice_partition") == calls, ks
    assert ks.get("bucket_partition") == calls * S and ks.get("bucket_directory") == calls * S, ks
    assert ks.get("bucket_accumulate") == calls and ks.get("scatter_add_fold") == calls, ks
    assert not any(k in ks for k in ("scatter_add_count", "scatter_add_partition", "scatter_add")), ks


@pytest.mark.parametrize("K", [16 << 20, (9 << 20) + 7])
def test_scatter_add_into_a_large_table_is_captured_and_follows_the_slice_populations(ek, capi, K):
    n = 4 << 20
    rng = np.random.default_rng(K + 1)
    hv = rng.standard_normal(n).astype(np.float32)
    hidx = rng.integers(0, K, n).astype(np.uint32)
    v, idx = ek.Float32(hv), ek.UInt32(hidx)
    out = {}

    def step():
        t = ek.Float32.zero(K)                          # the fill is part of the step: every replay starts from zeros
        ek.scatter_add(t, v, idx)
        out["t"] = t

    S = (K + SPAN - 1) // SPAN
    ks, eager_launches = _kernels(ek, step)
    _check(out["t"].numpy(), K, hidx, hv, "eager")
    _assert_device_sized(ks, S)
    l0 = ek.hip_launch_count()
    ek.hip_graph_begin()                                # (the host-sized path refused this capture: "... captured step graph ...")
    try:
        step()
    finally:
        g = ek.hip_graph_end()
    try:
        per_step = ek.hip_graph_launch_count(g)
        assert ek.hip_launch_count() - l0 == per_step
        assert per_step <= 6 + 3 * S, (per_step, S)
        assert eager_launches <= per_step <= eager_launches + S, (eager_launches, per_step)
        # 1: uniform indices
        ek.hip_graph_launch(g)
        _check(out["t"].numpy(), K, hidx, hv, "replay, uniform")
        # 2: every index in slice 0: the bins of the other slices are exactly zero, not the previous replay's
        hidx2 = rng.integers(0, SPAN, n).astype(np.uint32)
        _refill(capi, idx, hidx2)
        ek.hip_graph_launch(g)
        got = out["t"].numpy()
        _check(got, K, hidx2, hv, "replay, slice 0 only")
        assert np.all(got[SPAN:] == 0.0), int(np.count_nonzero(got[SPAN:]))
        # 3: skewed indices over the whole table
        hidx3 = _skewed(rng, n, K)
        _refill(capi, idx, hidx3)
        ek.hip_graph_launch(g)
        _check(out["t"].numpy(), K, hidx3, hv, "replay, skewed")
        # 4: every index in ONE 16 Ki bucket of slice 1 (the directory's hot-bucket copy), everything else empty
        lo = SPAN + 5 * 16384
        hidx4 = (lo + rng.integers(0, 16384, n)).astype(np.uint32)
        _refill(capi, idx, hidx4)
        ek.hip_graph_launch(g)
        got = out["t"].numpy()
        _check(got, K, hidx4, hv, "replay, one bucket")
        assert np.all(got[:lo] == 0.0) and np.all(got[lo + 16384:] == 0.0)
        # 5: all indices equal (the last bin of the table)
        hidx5 = np.full(n, K - 1, np.uint32)
        _refill(capi, idx, hidx5)
        ek.hip_graph_launch(g)
        got = out["t"].numpy()
        _check(got, K, hidx5, hv, "replay, all equal")
        assert np.all(got[:K - 1] == 0.0)
        # 6: the values refilled too
        hv6 = rng.standard_normal(n).astype(np.float32)
        _refill(capi, v, hv6)
        _refill(capi, idx, hidx3)
        ek.hip_graph_launch(g)
        _check(out["t"].numpy(), K, hidx3, hv6, "replay, new values")
        # the eager step on the same inputs agrees within the same bound
        step()
        _check(out["t"].numpy(), K, hidx3, hv6, "eager again")
    finally:
        ek.hip_graph_destroy(g)


def test_masked_scatter_add_with_int32_indices_into_a_large_table_is_captured(ek, capi):
    """a mask array, int32 indices, some of them beyond the table: dropped; small integer values make every sum exact"""
    n, K = 4 << 20, (9 << 20) + 7
    S = (K + SPAN - 1) // SPAN
    rng = np.random.default_rng(11)

    def inputs():
        hidx = rng.integers(0, K, n).astype(np.int32)
        out_of_range = rng.random(n) < 0.05
        # beyond the table: inside the last slice's unused part, beyond the last slice, and up to the largest int32
        beyond = np.where(rng.random(n) < 0.5, rng.integers(K, S * SPAN + 1000, n), rng.integers(K, 2 ** 31, n))
        hidx = np.where(out_of_range, beyond, hidx).astype(np.int32)
        return hidx, rng.random(n) < 0.75, rng.integers(-3, 4, n).astype(np.float32)

    def want(hidx, hmask, hv):
        keep = hmask & (hidx.astype(np.int64) < K)
        return np.bincount(hidx[keep].astype(np.int64), weights=hv[keep].astype(np.float64), minlength=K)

    hidx, hmask, hv = inputs()
    v, idx, m = ek.Float32(hv), ek.Int32(hidx), ek.Mask(hmask)
    out = {}

    def step():
        t = ek.Float32.zero(K)
        ek.scatter_add(t, v, idx, m)
        out["t"] = t

    ks, eager_launches = _kernels(ek, step)
    assert np.array_equal(out["t"].numpy().astype(np.float64), want(hidx, hmask, hv))
    _assert_device_sized(ks, S)
    ek.hip_graph_begin()
    try:
        step()
    finally:
        g = ek.hip_graph_end()
    try:
        per_step = ek.hip_graph_launch_count(g)
        assert per_step <= 6 + 3 * S and eager_launches <= per_step <= eager_launches + S, (eager_launches, per_step)
        ek.hip_graph_launch(g)
        assert np.array_equal(out["t"].numpy().astype(np.float64), want(hidx, hmask, hv))
        hidx2, hmask2, hv2 = inputs()
        _refill(capi, idx, hidx2); _refill(capi, m, hmask2.astype(np.uint8)); _refill(capi, v, hv2)
        ek.hip_graph_launch(g)
        assert np.array_equal(out["t"].numpy().astype(np.float64), want(hidx2, hmask2, hv2))
        # every lane masked out: nothing is added anywhere
        _refill(capi, m, np.zeros(n, np.uint8))
        ek.hip_graph_launch(g)
        assert not out["t"].numpy().any()
    finally:
        ek.hip_graph_destroy(g)


def test_backward_of_two_gathers_from_a_large_table_is_captured(ek, capi):
    """y = hsum(gather(A, i) * gather(A, j)) with two index arrays is not in the bucket-ordered menu: its backward is two element-order
    scatter_adds into the 16 Mi bins of A's gradient, dA[k] = sum_{i_e = k} A[j_e] + sum_{j_e = k} A[i_e]"""
    n, K = 4 << 20, 16 << 20
    S = K // SPAN
    rng = np.random.default_rng(5)
    hA = rng.uniform(-1, 1, K).astype(np.float32)
    hi, hj = rng.integers(0, K, n).astype(np.uint32), rng.integers(0, K, n).astype(np.uint32)
    A0, i, j = ek.Float32(hA), ek.UInt32(hi), ek.UInt32(hj)
    out = {}

    def step():
        A = ek.Float32(A0)
        ek.set_requires_gradient(A)
        y = ek.hsum(ek.gather(A, i) * ek.gather(A, j))
        ek.backward(y)
        out["y"], out["gA"] = ek.detach(y), ek.gradient(A)

    def check(hi, hj, what):
        a64 = hA.astype(np.float64)
        terms = a64[hi.astype(np.int64)] * a64[hj.astype(np.int64)]
        y, y_true = float(out["y"].numpy()[0]), float(terms.sum())
        # (as cfg3b_truth: a sum of n terms in any order of depth d, every term within 4 * 2^-24 of its exact value)
        y_bound = EPS * (hsum_depth(n) * float(np.abs(terms).sum()) + 4 * n)
        print(f"{what}: |y - truth| = {abs(y - y_true):.3g} (bound {y_bound:.3g})")
        assert abs(y - y_true) <= y_bound, (what, y, y_true, y_bound)
        # the gradient: both streams of exact float32 values into one table
        _check(out["gA"].numpy(), K, np.concatenate([hi, hj]), np.concatenate([hA[hj.astype(np.int64)], hA[hi.astype(np.int64)]]), what)

    ks, _ = _kernels(ek, step)
    check(hi, hj, "eager")
    _assert_device_sized(ks, S, calls=2)
    ek.hip_graph_begin()
    try:
        step()
    finally:
        g = ek.hip_graph_end()
    try:
        ek.hip_graph_launch(g)
        check(hi, hj, "replay")
        hi2 = _skewed(rng, n, K)
        _refill(capi, i, hi2)
        ek.hip_graph_launch(g)
        check(hi2, hj, "replay, skewed i")
        hi3 = rng.integers(3 * SPAN, K, n).astype(np.uint32)          # i in the last slice only
        _refill(capi, i, hi3)
        ek.hip_graph_launch(g)
        check(hi3, hj, "replay, i in one slice")
    finally:
        ek.hip_graph_destroy(g)


@pytest.mark.parametrize("kind", ["float64", "uint32"])
def test_other_element_types_keep_the_host_sized_path_and_its_refusal(ek, kind):
    """8-byte and integer streams into more than 4 Mi bins still read their slice populations back: exact eagerly, refused under a
    capture with a message that names the type; the capture stays valid and the library usable"""
    n, K = 1 << 21, 9_000_001
    rng = np.random.default_rng(3)
    hidx = rng.integers(0, K, n).astype(np.uint32)
    idx = ek.UInt32(hidx)
    if kind == "float64":
        Array, hv, name = ek.Float64, rng.integers(1, 4, n).astype(np.float64), "float64"
    else:
        Array, hv, name = ek.UInt32, rng.integers(1, 4, n).astype(np.uint32), "32-bit integer"
    v = Array(hv)
    want = np.bincount(hidx, weights=hv.astype(np.float64), minlength=K)

    def eager():
        t = Array.zero(K)
        ek.scatter_add(t, v, idx)
        return t

    out = {}
    ks, _ = _kernels(ek, lambda: out.update(t=eager()))
    assert np.array_equal(out["t"].numpy().astype(np.float64), want)
    assert "scatter_add_count" in ks and "scatter_add_slice_count" not in ks, ks
    w = None
    ek.hip_graph_begin()
    try:
        t = Array.zero(K)
        with pytest.raises(RuntimeError, match="captured step graph") as e:
            ek.scatter_add(t, v, idx)
        assert name in str(e.value), str(e.value)
        w = ek.Float32.full(2.0, 1024) * ek.Float32(3.0)            # ordinary work is still recorded
    finally:
        g = ek.hip_graph_end()
    try:
        ek.hip_graph_launch(g)
        assert np.all(w.numpy() == 6.0)
    finally:
        ek.hip_graph_destroy(g)
    assert np.array_equal(eager().numpy().astype(np.float64), want)
