"""Value partitions of more than 128 buckets stage their records as two planes in rings of 96 and write 64-element pages
(csrc/ek_paged.h: k_page_partition<.., Planes>).  The cfg3b step at 256 buckets -- y = hsum(sin(A[idx] x + B[idx])) and both
gradient tables -- against the float64 truth and the class-D bounds of conftest.cfg3b_truth, through the C ABI, for every shape
of input the partition treats differently: the vector and the ragged loader, masks, 64-bit indices, a ragged last bucket, and
SKEWED indices, which live in the overflow round (a bucket's second page half in the ring, half in registers).  That the skewed
inputs really take that round is asserted with the host model of tests/test_paged_ring_model.py.
"""
import json

import numpy as np
import pytest

from conftest import cfg3b_truth, cfg3b_variant_truth, uniform_pm1
from test_paged_ring_model import TILE, overflow_tiles

pytestmark = pytest.mark.gpu

K1 = 1 << 20                     # 256 quarter-size buckets of 4 Ki entries: fixed-point adjoint sums
N = 1 << 21


def up(capi, a):
    return capi.Buf.from_numpy(a)


def tables(K, seed):
    return uniform_pm1(K, seed + 1).astype(np.float32), uniform_pm1(K, seed + 2).astype(np.float32)


def step(capi, dA, dB, dx, di, K, dm=None):
    """one cfg3b step: (y, gA, gB, {kernel: (launches, elements)})"""
    capi.profile_begin()
    b = capi.Bucketed("fmadd", dA, dx, dB, di, hints=capi.Bucketed.HINT_ADJOINT | capi.Bucketed.HINT_BOUNDED, mask=dm)
    y = float(b.reduce("hsum", "sin", keep=True, keep_op="cos").numpy()[0])
    gB, gA = up(capi, np.zeros(K, np.float32)), up(capi, np.zeros(K, np.float32))
    b.scatter_add([gB, gA], [("cos", 0, False), ("cos", 0, True)], fresh=[1, 1])
    ks = {k["kernel"]: (k["launches"], k["elements"]) for k in capi.profile_end() if k["launches"]}
    out = (y, gA.numpy().copy(), gB.numpy().copy(), ks)
    b.destroy()
    return out


def check(capi, A, B, x, idx, mask=None, dx=None, di=None, dm=None, twice=True):
    K = A.size
    dA, dB = up(capi, A), up(capi, B)
    dx = up(capi, x) if dx is None else dx
    di = up(capi, idx) if di is None else di
    if mask is not None and dm is None:
        dm = up(capi, mask.astype(np.uint8))
    y, gA, gB, ks = step(capi, dA, dB, dx, di, K, dm)
    assert ks.get("bucket_partition", (0, 0))[0] == 1 and ks.get("bucket_directory", (0, 0))[0] == 1, ks
    t = cfg3b_truth(A, B, x, idx) if mask is None else cfg3b_variant_truth(A, B, x, idx, mask=mask)
    ey, eA, eB = abs(y - t["y"]), np.abs(gA - t["gA"]), np.abs(gB - t["gB"])
    print(f"y error {ey:.3e} (bound {t['y_bound']:.3e}), gA worst {float((eA / (t['gA_bound'] + 1e-300)).max()):.3e} "
          f"and gB worst {float((eB / (t['gB_bound'] + 1e-300)).max()):.3e} of their bounds")
    assert ey <= t["y_bound"]
    assert np.all(eA <= t["gA_bound"]) and np.all(eB <= t["gB_bound"])
    # entries nothing points at stay zero
    assert not gA[t["cnt"] == 0].any() and not gB[t["cnt"] == 0].any()
    if twice:
        y2, hA, hB, _ = step(capi, dA, dB, dx, di, K, dm)
        assert np.float32(y2).view(np.uint32) == np.float32(y).view(np.uint32), (y, y2)
        assert np.array_equal(gA.view(np.uint32), hA.view(np.uint32)) and np.array_equal(gB.view(np.uint32), hB.view(np.uint32))
    return ks


def takes_overflow_round(idx, shift=12, mask=None):
    """share of the tiles in which the model's ring of 96 overflows (chunks of 2 tiles: 2 Mi elements over 256 workgroups);
    dropped lanes go to a ring of their own that is not looked at"""
    b = idx.astype(np.int64) >> shift
    if mask is not None:
        b = np.where(mask, b, 256)
    n = (len(b) // (2 * TILE)) * 2 * TILE
    b = b[:n].reshape(-1, 2, TILE)
    return overflow_tiles(lambda t: b[:, t, :], b.shape[0], 2, 257, cap=96, page=64, n_real=256) / (n // TILE)


def test_geometry_is_64_element_pages_at_256_buckets(capi):
    """the directory mark reports the partition's page slots: W * ((chunk >> 6) + 256) for K = 1 Mi.  128 tiles: one tile per
    workgroup on any device of at least 128 CUs (an MI355X has 256), so W = 128 and chunk = 4096 whatever the CU count"""
    n = 128 * TILE
    A, B = tables(K1, 3)
    x = uniform_pm1(n, 5).astype(np.float32)
    idx = np.random.default_rng(3).integers(0, K1, n).astype(np.uint32)
    ks = check(capi, A, B, x, idx, twice=False)
    W, chunk = 128, TILE
    assert ks["bucket_directory"][1] == W * ((chunk >> 6) + 256), ks


def test_uniform_indices(capi):
    A, B = tables(K1, 11)
    x = uniform_pm1(N, 13).astype(np.float32)
    idx = np.random.default_rng(11).integers(0, K1, N).astype(np.uint32)
    assert takes_overflow_round(idx) <= 0.01
    check(capi, A, B, x, idx)


def test_ragged_size_and_unaligned_operands(capi):
    """n is not a multiple of the tile and neither x nor the index array starts on a 16-byte boundary: the ragged loader"""
    n = N + 4099
    A, B = tables(K1, 21)
    x = uniform_pm1(n + 3, 23).astype(np.float32)
    idx = np.random.default_rng(21).integers(0, K1, n + 1).astype(np.uint32)
    bx, bi = up(capi, x), up(capi, idx)
    check(capi, A, B, x[3:], idx[1:], dx=bx.view(3, n), di=bi.view(1, n))


def test_ragged_last_bucket(capi):
    K = K1 - 5
    A, B = tables(K, 31)
    x = uniform_pm1(N, 33).astype(np.float32)
    idx = np.random.default_rng(31).integers(0, K, N).astype(np.uint32)
    idx[:64] = K - 1
    check(capi, A, B, x, idx)


def test_mask_array(capi):
    A, B = tables(K1, 41)
    x = uniform_pm1(N + 777, 43).astype(np.float32)
    idx = np.random.default_rng(41).integers(0, K1, x.size).astype(np.uint32)
    mask = np.random.default_rng(42).integers(0, 4, x.size) != 0            # 75 % set
    check(capi, A, B, x, idx, mask=mask)


def test_mask_array_over_skewed_indices(capi):
    A, B = tables(K1, 45)
    x = uniform_pm1(N, 47).astype(np.float32)
    idx = np.random.default_rng(45).integers(5 << 12, 6 << 12, N).astype(np.uint32)
    mask = np.random.default_rng(46).integers(0, 4, N) != 0
    assert takes_overflow_round(idx, mask=mask) == 1.0
    check(capi, A, B, x, idx, mask=mask)


def log_uniform(n, seed):
    """the skew of bench.py's cfg3b_zipf: a magnitude m uniform in 0 .. 19, then an index uniform in [2^m - 1, 2^(m+1) - 2]"""
    rng = np.random.default_rng(seed)
    lo = (np.uint32(1) << rng.integers(0, 20, n).astype(np.uint32)) - np.uint32(1)
    return (lo + (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & lo)).astype(np.uint32)


def test_log_uniform_indices_live_in_the_overflow_round(capi):
    A, B = tables(K1, 51)
    x = uniform_pm1(N + 1234, 53).astype(np.float32)
    idx = log_uniform(x.size, 51)
    assert takes_overflow_round(idx) == 1.0
    check(capi, A, B, x, idx)


def test_all_indices_equal(capi):
    A, B = tables(K1, 61)
    x = uniform_pm1(N + 100, 63).astype(np.float32)
    idx = np.full(x.size, 777777, np.uint32)
    assert takes_overflow_round(idx) == 1.0
    check(capi, A, B, x, idx)


def test_one_bucket_spread_over_its_entries(capi):
    A, B = tables(K1, 71)
    x = uniform_pm1(N, 73).astype(np.float32)
    idx = np.random.default_rng(71).integers(200 << 12, 201 << 12, N).astype(np.uint32)
    assert takes_overflow_round(idx) == 1.0
    check(capi, A, B, x, idx)


@pytest.mark.parametrize("arrivals", [97, 127, 128, 129, 160, 191, 192, 193])
def test_overflow_by_a_few_elements(capi, arrivals):
    """every tile brings ONE bucket `arrivals` elements and spreads the rest: around the edges of the overflow round -- the ring
    of 96 just exceeded, the second page just not / just / more than completed, with every origin (0, 64, 32) coming up"""
    tiles = 6 * 256                                             # six tiles per workgroup of a 256-CU device
    rng = np.random.default_rng(arrivals)
    idx = rng.integers(0, K1, (tiles, TILE)).astype(np.uint32)
    idx[idx >> 12 == 9] += np.uint32(1 << 12)                   # nobody else in bucket 9
    for t in range(tiles):
        at = rng.permutation(TILE)[:arrivals]
        idx[t, at] = rng.integers(9 << 12, 10 << 12, arrivals).astype(np.uint32)
    idx = idx.ravel()
    A, B = tables(K1, 81)
    x = uniform_pm1(idx.size, 83).astype(np.float32)
    check(capi, A, B, x, idx, twice=False)


def test_two_mi_entries_under_locks(capi):
    """K = 2 Mi: 256 half-size buckets, the adjoint sums under the exchange locks (float additions in page order: the class-D
    bounds apply, not bit identity)"""
    K = 1 << 21
    A, B = tables(K, 91)
    x = uniform_pm1(N + 555, 93).astype(np.float32)
    idx = np.random.default_rng(91).integers(0, K, x.size).astype(np.uint32)
    check(capi, A, B, x, idx, twice=False)
    idx = (log_uniform(x.size, 92).astype(np.uint64) * 2 % K).astype(np.uint32)
    assert takes_overflow_round(idx, shift=13) == 1.0
    check(capi, A, B, x, idx, twice=False)


def test_64_bit_indices_through_the_array_api():
    """the step as bench.py spells it, with a UInt64 index array"""
    import enoki_amd.hip_autodiff as ad
    ad.hip_init(0)
    A, B = tables(K1, 101)
    x = uniform_pm1(N + 4099, 103).astype(np.float32)
    idx = log_uniform(x.size, 101)
    idx[::2] = np.random.default_rng(102).integers(0, K1, idx[::2].size).astype(np.uint32)

    def run():
        dA, dB = ad.Float32(A), ad.Float32(B)
        ad.set_requires_gradient(dA); ad.set_requires_gradient(dB)
        di = ad.UInt64(idx.astype(np.uint64))
        y = ad.hsum(ad.sin(ad.fmadd(ad.gather(dA, di), ad.Float32(x), ad.gather(dB, di))))
        ad.backward(y)
        return float(ad.detach(y).numpy()[0]), ad.gradient(dA).numpy(), ad.gradient(dB).numpy()

    ad.hip_profile_begin()
    y, gA, gB = run()
    ks = {k["kernel"]: k["launches"] for k in json.loads(ad.hip_profile_end()) if k["launches"]}
    assert ks.get("bucket_partition") == 1 and ks.get("bucket_pair_fma_reduce_adjoint") == 1, ks
    t = cfg3b_truth(A, B, x, idx)
    assert abs(y - t["y"]) <= t["y_bound"]
    assert np.all(np.abs(gA - t["gA"]) <= t["gA_bound"]) and np.all(np.abs(gB - t["gB"]) <= t["gB_bound"])
    y2, hA, hB = run()
    assert y2 == y and np.array_equal(gA.view(np.uint32), hA.view(np.uint32)) and np.array_equal(gB.view(np.uint32), hB.view(np.uint32))


@pytest.mark.parametrize("logk", [21, 22])
@pytest.mark.parametrize("pattern", ["uniform", "log-uniform"])
def test_scatter_add_into_2_and_4_mi_bins(capi, logk, pattern):
    """the element-order scatter_add of float32 values into 2 - 4 Mi bins partitions its input with the same kernel (up to 256
    buckets): every bin within the class-D bound of its float64 sum, untouched bins keep what they held"""
    K, n = 1 << logk, (1 << 22) + 4099
    v = uniform_pm1(n, logk).astype(np.float32)
    if pattern == "uniform":
        idx = np.random.default_rng(logk).integers(0, K, n).astype(np.uint32)
    else:
        idx = (log_uniform(n, logk).astype(np.uint64) * (K >> 20) + 3).astype(np.uint32) % np.uint32(K)
    held = uniform_pm1(K, 7).astype(np.float32)
    t = up(capi, held)
    capi.profile_begin()
    capi.scatter_add(t, up(capi, v), up(capi, idx))
    ks = {k["kernel"]: k["launches"] for k in capi.profile_end() if k["launches"]}
    print(ks)
    got = t.numpy().astype(np.float64)
    ii = idx.astype(np.int64)
    cnt = np.bincount(ii, minlength=K)
    want = held.astype(np.float64) + np.bincount(ii, weights=v.astype(np.float64), minlength=K)
    bound = 2.0 ** -24 * (cnt + 1) * (np.abs(held.astype(np.float64)) + np.bincount(ii, weights=np.abs(v.astype(np.float64)), minlength=K))
    assert np.all(np.abs(got - want) <= bound + 1e-300), float((np.abs(got - want) / (bound + 1e-300)).max())
    assert np.array_equal(t.numpy()[cnt == 0], held[cnt == 0])
