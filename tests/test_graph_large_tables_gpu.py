"""Step graphs over tables of three or more slices (K > 8 Mi entries): the split by slice sizes its work on the device, so the
step can be captured, and every replay follows the slice populations of the index array it finds -- also when they change
between replays (one slice holding every element, the others none)."""
import ctypes
import json

import numpy as np
import pytest

from conftest import cfg3b_truth, cfg3b_variant_truth

pytestmark = pytest.mark.gpu

SPAN = 1 << 22          # entries per slice of a float32 table (256 buckets of 16 Ki)


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


def _check_cfg3b(out, t, K_used=None):
    y, gA, gB = float(out["y"].numpy()[0]), out["gA"].numpy(), out["gB"].numpy()
    assert abs(y - t["y"]) <= t["y_bound"], (y, t["y"], t["y_bound"])
    for name, g in (("gA", gA), ("gB", gB)):
        err = np.abs(g - t[name])
        assert np.all(err <= t[name + "_bound"]), (name, float((err / np.maximum(t[name + "_bound"], 1e-30)).max()))
        if K_used is not None:
            assert np.all(g[K_used:] == 0.0), (name, int(np.count_nonzero(g[K_used:])))
    return y, gA, gB


@pytest.mark.parametrize("K", [16 << 20, (9 << 20) + 7])
def test_cfg3b_sliced_table_step_graph_follows_the_slice_populations(ek, capi, K):
    n = 4 << 20
    rng = np.random.default_rng(K)
    hA, hB = rng.uniform(-1, 1, K).astype(np.float32), rng.uniform(-1, 1, K).astype(np.float32)
    hx = rng.uniform(-1, 1, n).astype(np.float32)
    hidx = rng.integers(0, K, n).astype(np.uint32)
    A0, B0, x, idx = ek.Float32(hA), ek.Float32(hB), ek.Float32(hx), ek.UInt32(hidx)
    out = {}

    def step():
        A, B = ek.Float32(A0), ek.Float32(B0)
        ek.set_requires_gradient(A); ek.set_requires_gradient(B)
        y = ek.hsum(ek.sin(ek.fmadd(ek.gather(A, idx), x, ek.gather(B, idx))))
        ek.backward(y)
        out["y"], out["gA"], out["gB"] = ek.detach(y), ek.gradient(A), ek.gradient(B)

    t = cfg3b_truth(hA, hB, hx, hidx)
    S = (K + SPAN - 1) // SPAN
    l0 = ek.hip_launch_count()
    ek.hip_profile_begin()
    step()                                             # eager: the same bounds as the replays
    ks = {k["kernel"]: k["launches"] for k in json.loads(ek.hip_profile_end()) if k["launches"]}
    eager_launches = ek.hip_launch_count() - l0
    _check_cfg3b(out, t)
    # the sliced bucket-ordered path: ONE split by slice, a partition and a directory per slice, nothing in element order
    assert ks.get("bucket_slice_partition") == 1 and ks.get("bucket_partition") == S and ks.get("bucket_directory") == S, ks
    assert not any(k in ks for k in ("gather_pair_fmadd", "gather", "scatter_add_partition", "scatter_add_count")), ks
    l0 = ek.hip_launch_count()
    ek.hip_graph_begin()
    step()
    g = ek.hip_graph_end()
    try:
        per_step = ek.hip_graph_launch_count(g)
        assert ek.hip_launch_count() - l0 == per_step
        # (an eager step may skip the counter-block clears of reused MetaRing blocks, one per slice at most)
        assert eager_launches <= per_step <= eager_launches + S, (eager_launches, per_step)
        # 1: uniform indices
        ek.hip_graph_launch(g)
        _check_cfg3b(out, t)
        # 2: every element in slice 0, slices 1 .. S-1 empty: their gradients are exactly zero, not the previous replay's
        hidx2 = rng.integers(0, SPAN, n).astype(np.uint32)
        _refill(capi, idx, hidx2)
        ek.hip_graph_launch(g)
        _check_cfg3b(out, cfg3b_truth(hA, hB, hx, hidx2), K_used=SPAN)
        # 3: skewed indices over the whole table
        hidx3 = _skewed(rng, n, K)
        _refill(capi, idx, hidx3)
        ek.hip_graph_launch(g)
        t3 = cfg3b_truth(hA, hB, hx, hidx3)
        _check_cfg3b(out, t3)
        # 4: every element in ONE bucket of slice 1 (128 Ki full pages: the directory's hot-bucket copy), the rest empty
        hidx4 = (SPAN + 5 * 16384 + rng.integers(0, 16384, n)).astype(np.uint32)
        _refill(capi, idx, hidx4)
        ek.hip_graph_launch(g)
        t4 = cfg3b_truth(hA, hB, hx, hidx4)
        _check_cfg3b(out, t4)
        gA4 = out["gA"].numpy()
        assert np.all(gA4[:SPAN + 5 * 16384] == 0.0) and np.all(gA4[SPAN + 6 * 16384:] == 0.0)
        # the eager step on the same inputs agrees within the same bounds
        _refill(capi, idx, hidx3)
        step()
        _check_cfg3b(out, t3)
    finally:
        ek.hip_graph_destroy(g)


def test_masked_reduction_over_a_sliced_table_step_graph_carries_the_non_finite_flag(ek, capi):
    n, K = 4 << 20, 16 << 20
    rng = np.random.default_rng(7)
    hA, hB = rng.uniform(-1, 1, K).astype(np.float32), rng.uniform(-1, 1, K).astype(np.float32)
    hx = rng.uniform(-1, 1, n).astype(np.float32)
    hidx = rng.integers(0, K, n).astype(np.uint32)
    hmask = rng.random(n) < 0.75
    A, B, x, idx, m = ek.Float32(hA), ek.Float32(hB), ek.Float32(hx), ek.UInt32(hidx), ek.Mask(hmask)
    out = {}

    def step():
        return ek.hsum(ek.sin(ek.fmadd(ek.gather(A, idx, m), x, ek.gather(B, idx, m))))

    t = cfg3b_variant_truth(hA, hB, hx, hidx, mask=hmask)
    assert abs(float(step().numpy()[0]) - t["y"]) <= t["y_bound"]
    ek.hip_graph_begin()
    out["y"] = step()
    g = ek.hip_graph_end()
    try:
        ek.hip_graph_launch(g)
        assert abs(float(out["y"].numpy()[0]) - t["y"]) <= t["y_bound"]
        # a masked-out lane whose x is infinite: u = 0 * inf = NaN, and so is the sum -- as in the eager result
        off = int(np.flatnonzero(~hmask)[0])
        hx_bad = hx.copy(); hx_bad[off] = np.inf
        _refill(capi, x, hx_bad)
        ek.hip_graph_launch(g)
        assert np.isnan(float(out["y"].numpy()[0]))
        assert np.isnan(float(step().numpy()[0]))
        _refill(capi, x, hx)
        ek.hip_graph_launch(g)
        y = float(out["y"].numpy()[0])
        assert np.isfinite(y) and abs(y - t["y"]) <= t["y_bound"]
    finally:
        ek.hip_graph_destroy(g)
