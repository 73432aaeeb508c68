"""The refined stream of a kept bucket partition (csrc/ek_refine.h, bucket_refine.hip): at the first step that
stands on a kept partition the elements of every piece are stored once more in the order of their table entries, four to a group
that shares one entry, and the fixed-point forward + adjoint kernel of every later step walks those groups -- one record read and
two 64-bit LDS adds per group.  The sums are exact 64-bit integers of individually rounded terms, so nothing may change:

  * every fixed-point step is bit-identical to the same step with `partition_refine` = 0 (the page walk on the kept partition) and
    to a step with `partition_cache` = 0 (fresh partition, page walk), and lies within conftest.cfg3b_truth / cfg3b_variant_truth;
  * pieces that fall under the exchange locks (a NaN table entry, an infinite x) walk their pages as before: float sums, whose
    order varies -- truth bounds only.

n = 300 007 lookups into K = 65 536 entries (the shape of test_partition_cache_gpu.py: the smallest that takes the hinted
fixed-point kernel), `partition_refine` = 2: at 4.6 lookups per entry the automatic mode builds no stream."""
import gc
import re

import numpy as np
import pytest

from conftest import bits_equal, cfg3b_variant_truth, hash_u32
from test_partition_cache_gpu import N, K, captured_launches, counted, is_hit, partitions, same_bits, within_truth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


@pytest.fixture
def refine2(ad):
    ad.hip_set_tuning("partition_refine", 2)
    yield
    ad.hip_set_tuning("partition_refine", 1)


_HOST = {}


def host(seed=1):
    if seed not in _HOST:
        rng = np.random.default_rng(1000 * seed + 11)
        h = dict(A=rng.uniform(-1, 1, K).astype(np.float32), B=rng.uniform(-1, 1, K).astype(np.float32),
                 x=rng.uniform(-1, 1, N).astype(np.float32), idx=rng.integers(0, K, N).astype(np.uint32),
                 mask=(rng.integers(0, 4, N) != 0))
        for a in h.values():
            a.setflags(write=False)
        _HOST[seed] = h
    return _HOST[seed]


def refines(ks):
    return ks.get("bucket_refine", 0)


FORMS = {  # name: (form, func, spelling for the truth, seed)
    "pair": ("pair", "sin", "fmadd", 1.0), "scalar": ("scalar", "sin", "fmadd", 1.0), "product": ("product", "sin", "a*x", 1.0),
    "cos": ("pair", "cos", "fmadd", 1.0), "a*x+b": ("a*x+b", "sin", "a*x+b", 1.0), "b-a*x": ("b-a*x", "sin", "b-a*x", 1.0),
    "seed3": ("pair", "sin", "fmadd", 3.0)}


def step(ad, hA, hB, x, idx, mask=None, name="pair"):
    """one step over the caller's x / idx / mask arrays and FRESH leaves; -> (y, gA, gB) on the host (gB: None without a table B)"""
    form, func, _, seed = FORMS[name]
    A, B = ad.Float32(hA), ad.Float32(hB)
    ad.set_requires_gradient(A); ad.set_requires_gradient(B)
    a = ad.gather(A, idx, mask) if mask is not None else ad.gather(A, idx)
    with_b = form not in ("scalar", "product")
    if with_b:
        b = ad.gather(B, idx, mask) if mask is not None else ad.gather(B, idx)
    if form == "pair":
        u = ad.fmadd(a, x, b)
    elif form == "scalar":
        u = ad.fmadd(a, x, ad.Float32(0.5))
    elif form == "product":
        u = a * x
    elif form == "a*x+b":
        u = a * x + b
    else:
        u = b - a * x
    y = ad.hsum(ad.sin(u) if func == "sin" else ad.cos(u))
    ad.backward(y * seed if seed != 1.0 else y)
    return ad.detach(y).numpy().copy(), ad.gradient(A).numpy().copy(), (ad.gradient(B).numpy().copy() if with_b else None)


def truth(h, hidx, name="pair", hmask=None, hx=None, hA=None):
    form, func, spelling, seed = FORMS[name]
    hB = np.full(K, 0.5, np.float32) if form == "scalar" else h["B"]
    t = cfg3b_variant_truth(h["A"] if hA is None else hA, hB, h["x"] if hx is None else hx, hidx, mask=hmask, func=func, seed=seed,
                            spelling=spelling)
    # (y itself is not seeded: the seed multiplies what backward() sends down)
    t0 = cfg3b_variant_truth(h["A"] if hA is None else hA, hB, h["x"] if hx is None else hx, hidx, mask=hmask, func=func, spelling=spelling)
    t["y"], t["y_bound"] = t0["y"], t0["y_bound"]
    return t, (("y", "gA", "gB") if form not in ("scalar", "product") else ("y", "gA"))


def arrays(ad, hx, hidx, hmask=None, idx64=False):
    idx = ad.UInt32(hidx)
    return ad.Float32(hx), (ad.UInt64(idx) if idx64 else idx), (ad.Mask(hmask) if hmask is not None else None)


def three_steps(ad, h, hidx, name="pair", hmask=None, idx64=False, hx=None, hA=None):
    """three steps over one (x, idx, mask): the partition, the first hit (which refines), a later hit; -> results, launches"""
    x, idx, mask = arrays(ad, h["x"] if hx is None else hx, hidx, hmask, idx64)
    out = [counted(ad, lambda: step(ad, h["A"] if hA is None else hA, h["B"], x, idx, mask, name)) for _ in range(3)]
    return [r for r, _ in out], [k for _, k in out]


def reference_steps(ad, h, hidx, name="pair", hmask=None, idx64=False):
    """the same step on the kept partition's PAGES (partition_refine = 0, second step of a pair) and on a fresh partition
    (partition_cache = 0)"""
    ad.hip_set_tuning("partition_refine", 0)
    try:
        x, idx, mask = arrays(ad, h["x"], hidx, hmask, idx64)
        step(ad, h["A"], h["B"], x, idx, mask, name)
        pages, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, mask, name))
        assert is_hit(k) and refines(k) == 0, k
    finally:
        ad.hip_set_tuning("partition_refine", 2)
    ad.hip_set_tuning("partition_cache", 0)
    try:
        x, idx, mask = arrays(ad, h["x"], hidx, hmask, idx64)
        fresh = step(ad, h["A"], h["B"], x, idx, mask, name)
    finally:
        ad.hip_set_tuning("partition_cache", 1)
    return pages, fresh


def check_fixed(ad, h, hidx, name="pair", hmask=None, idx64=False):
    rs, ks = three_steps(ad, h, hidx, name, hmask, idx64)
    assert partitions(ks[0]) == 1 and refines(ks[0]) == 0, ks[0]
    assert refines(ks[1]) >= 1 and is_hit(ks[1]), ks[1]
    assert refines(ks[2]) == 0 and is_hit(ks[2]), ks[2]
    assert same_bits(rs[0], rs[1]) and same_bits(rs[0], rs[2])
    pages, fresh = reference_steps(ad, h, hidx, name, hmask, idx64)
    assert same_bits(rs[1], pages) and same_bits(rs[2], fresh)
    t, what = truth(h, hidx, name, hmask)
    assert within_truth(rs[2], t, what)
    return rs, ks


def test_the_first_hit_refines_and_later_hits_only_read(ad, refine2):
    check_fixed(ad, host(1), host(1)["idx"])


@pytest.mark.parametrize("name", [n for n in FORMS if n != "pair"])
def test_forms(ad, refine2, name):
    check_fixed(ad, host(1), host(1)["idx"], name)


def zipf_indices(n):
    """log-uniform indices as bench.py's cfg3b_zipf draws them, magnitudes 0 .. 15: every index below K = 2^16"""
    m = (hash_u32(np.arange(n, dtype=np.uint64), 8) % np.uint32(16)).astype(np.uint32)
    lo = ((np.uint32(1) << m) - np.uint32(1)).astype(np.uint32)
    return (lo + (hash_u32(np.arange(n, dtype=np.uint64), 9) & lo)).astype(np.uint32)


def pattern(name):
    rng = np.random.default_rng(77)
    if name == "arange":                 # N = 4 K + 37 863: runs of 4 and 5 -- one group and two
        return (np.arange(N, dtype=np.uint64) % K).astype(np.uint32)
    if name == "distinct4096":           # about 73 per entry, the entries spread over all buckets
        return (rng.integers(0, 4096, N) * 16 + 5).astype(np.uint32)
    if name == "one_entry":
        return np.full(N, 12345, np.uint32)
    if name == "one_bucket":             # entries 8192 .. 12287: the third bucket of 4 Ki entries
        return (8192 + rng.integers(0, 4096, N)).astype(np.uint32)
    return zipf_indices(N)


@pytest.mark.parametrize("name", ["arange", "distinct4096", "one_entry", "one_bucket", "zipf"])
def test_index_patterns(ad, capi, refine2, name):
    h = host(1)
    hidx = pattern(name)
    assert int(hidx.max()) < K
    if name in ("one_bucket", "one_entry"):
        # the bucket is cut into several pieces: 64-bit partial tables and the integer fold run
        hints = capi.Bucketed.HINT_ADJOINT | capi.Bucketed.HINT_BOUNDED
        b = capi.Bucketed("fmadd", capi.Buf.from_numpy(h["A"]), capi.Buf.from_numpy(h["x"]), capi.Buf.from_numpy(h["B"]), capi.Buf.from_numpy(hidx),
                          hints=hints)
        try:
            pieces, largest = b.piece_counts()
        finally:
            b.destroy()
        assert largest > 1 and pieces == largest, (pieces, largest)
    check_fixed(ad, h, hidx)


@pytest.mark.parametrize("name", ["idx64", "masked", "all_false"])
def test_index_and_mask_forms(ad, refine2, name):
    h = host(1)
    if name == "idx64":
        check_fixed(ad, h, h["idx"], idx64=True)
    elif name == "masked":
        check_fixed(ad, h, h["idx"], hmask=h["mask"])
    else:
        rs, _ = check_fixed(ad, h, h["idx"], hmask=np.zeros(N, bool))
        assert float(rs[2][0][0]) == 0.0 and not rs[2][1].any() and not rs[2][2].any()


def test_two_to_the_eighteen_plus_one(ad, refine2):
    """the smallest n of the bucket-ordered path, plus one: a last page with one element"""
    n = (1 << 18) + 1
    h = host(1)
    hs = dict(A=h["A"], B=h["B"], x=h["x"][:n], idx=h["idx"][:n])
    x, idx = ad.Float32(hs["x"]), ad.UInt32(hs["idx"])
    out = [counted(ad, lambda: step(ad, hs["A"], hs["B"], x, idx)) for _ in range(3)]
    assert refines(out[1][1]) >= 1 and is_hit(out[1][1]) and is_hit(out[2][1]) and refines(out[2][1]) == 0, [k for _, k in out]
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][0], out[2][0])
    assert within_truth(out[2][0], cfg3b_variant_truth(hs["A"], hs["B"], hs["x"], hs["idx"]))


def test_a_nan_table_entry_sends_one_piece_under_locks(ad, refine2):
    h = host(1)
    hA = h["A"].copy()
    bad = 3 * 4096 + 17
    hA[bad] = np.nan
    rs, ks = three_steps(ad, h, h["idx"], hA=hA)
    assert refines(ks[1]) >= 1 and is_hit(ks[1]) and is_hit(ks[2]), ks
    t = cfg3b_variant_truth(np.where(np.isnan(hA), np.float32(0), hA), h["B"], h["x"], h["idx"])
    hit = h["idx"] == bad
    assert hit.any()
    for y, gA, gB in rs[1:]:
        assert np.isnan(y[0]) and np.isnan(gA[bad]) and np.isnan(gB[bad])
        ok = np.ones(K, bool)
        ok[bad] = False
        assert np.all(np.isfinite(gA[ok])) and np.all(np.isfinite(gB[ok]))
        assert np.all(np.abs(gA[ok] - t["gA"][ok]) <= t["gA_bound"][ok]) and np.all(np.abs(gB[ok] - t["gB"][ok]) <= t["gB_bound"][ok])
    # the other buckets ran in fixed point from the refined stream: their entries repeat bit for bit
    other = np.ones(K, bool)
    other[3 * 4096:4 * 4096] = False
    assert bits_equal(rs[1][1][other], rs[2][1][other]) and bits_equal(rs[1][2][other], rs[2][2][other])
    assert bits_equal(rs[0][1][other], rs[2][1][other])


def test_an_infinite_x_sends_every_piece_under_locks(ad, refine2):
    h = host(1)
    hx = h["x"].copy()
    hx[N // 3] = np.inf
    rs, ks = three_steps(ad, h, h["idx"], hx=hx)
    assert refines(ks[1]) >= 1 and is_hit(ks[1]) and is_hit(ks[2]), ks
    e = int(h["idx"][N // 3])
    finite = hx.copy()
    finite[N // 3] = 0.0
    t = cfg3b_variant_truth(h["A"], h["B"], finite, h["idx"])
    ok = np.ones(K, bool)
    ok[e] = False
    for y, gA, gB in rs:
        assert np.isnan(y[0]) and np.isnan(gA[e])
        assert np.all(np.abs(gA[ok] - t["gA"][ok]) <= t["gA_bound"][ok]) and np.all(np.abs(gB[ok] - t["gB"][ok]) <= t["gB_bound"][ok])


def live_bytes(ad):
    gc.collect()
    return int(re.search(r"live bytes\s*:\s*(\d+)", ad.hip_whos()).group(1))


def test_the_stream_dies_with_the_partition(ad, refine2):
    h = host(1)
    step(ad, h["A"], h["B"], *arrays(ad, h["x"], h["idx"], h["mask"]))
    base = live_bytes(ad)
    x, idx, mask = arrays(ad, h["x"], h["idx"], h["mask"])
    with_arrays = live_bytes(ad)
    step(ad, h["A"], h["B"], x, idx, mask)
    kept = live_bytes(ad)
    _, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, mask))
    assert refines(k) >= 1 and is_hit(k), k
    assert live_bytes(ad) > kept > with_arrays                    # the partition, then its refined stream on top
    del idx
    assert live_bytes(ad) < with_arrays
    del x, mask
    assert live_bytes(ad) == base


def test_capture_after_a_refined_step(ad, refine2):
    h = host(1)
    ad.hip_set_tuning("partition_cache", 0)
    try:
        x0, idx0 = ad.Float32(h["x"]), ad.UInt32(h["idx"])
        out0 = {"A0": ad.Float32(h["A"]), "B0": ad.Float32(h["B"])}
        step(ad, h["A"], h["B"], x0, idx0)
        g0 = captured_launches(ad, h, x0, idx0, out0)
        expected = ad.hip_graph_launch_count(g0)
        ad.hip_graph_destroy(g0)
        del out0, x0, idx0
    finally:
        ad.hip_set_tuning("partition_cache", 1)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    out = {"A0": ad.Float32(h["A"]), "B0": ad.Float32(h["B"])}
    step(ad, h["A"], h["B"], x, idx)
    r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
    assert refines(k) >= 1 and is_hit(k), k
    g = captured_launches(ad, h, x, idx, out)
    try:
        assert ad.hip_graph_launch_count(g) == expected
        ad.hip_graph_launch(g)
        assert same_bits((out["y"].numpy(), out["gA"].numpy(), out["gB"].numpy()), r)
    finally:
        ad.hip_graph_destroy(g)


def test_the_automatic_mode_builds_no_stream_for_this_sparse_shape(ad, capfd):
    h = host(1)
    assert N < 8 * K
    ad.hip_set_log_level(2)
    try:
        x, idx, _ = arrays(ad, h["x"], h["idx"])
        out = [counted(ad, lambda: step(ad, h["A"], h["B"], x, idx)) for _ in range(3)]
    finally:
        ad.hip_set_log_level(0)
    assert all(refines(k) == 0 for _, k in out) and is_hit(out[1][1]) and is_hit(out[2][1]), [k for _, k in out]
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][0], out[2][0])
    err = capfd.readouterr().err
    assert len(re.findall(r"\[partition cache\] refined stream: skipped", err)) == 1, err[-2000:]


def test_the_switch_off_never_refines(ad):
    h = host(1)
    ad.hip_set_tuning("partition_refine", 0)
    try:
        x, idx, _ = arrays(ad, h["x"], h["idx"])
        out = [counted(ad, lambda: step(ad, h["A"], h["B"], x, idx)) for _ in range(3)]
    finally:
        ad.hip_set_tuning("partition_refine", 1)
    assert all(refines(k) == 0 for _, k in out) and is_hit(out[2][1])
    with pytest.raises(Exception):
        ad.hip_set_tuning("partition_refine", 3)
