"""search_sorted: per needle the number of entries of a sorted table before it (right: not after it), one kernel (csrc/search.hip).

Expected values are that count: numpy.searchsorted(side="left" / "right") for every needle that is not NaN, 0 for a NaN needle (the
comparisons are the type's own: a NaN compares false against every entry; numpy answers K).  Every comparison below is exact equality
of uint32 arrays.  The table sizes at which the kernel changes its shape -- resident whole in LDS, sampled with `stride`, how many
steps in global memory -- are asked from ek_hip_search_sorted_plan, not copied."""
import ctypes
import json

import numpy as np
import pytest

from conftest import SPECIALS_F32, SPECIALS_F64

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
# one grid trip of the kernel: 2 workgroups per CU x 512 lanes x 4 needles per lane (csrc/search.hip)
BLOCKS_PER_CU, BLOCK, NEEDLES_PER_LANE = 2, 512, 4


def name(dt):
    return np.dtype(dt).name


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def ekc():
    import enoki_amd.hip as m
    m.hip_init(0)
    return m


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


def expected(table, needles, right):
    want = np.searchsorted(table, needles, side="right" if right else "left").astype(np.uint32)
    if needles.dtype.kind == "f":
        want[np.isnan(needles)] = 0
    return want


def extremes(dt):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return np.array([-np.inf, np.inf, np.finfo(dt).min, np.finfo(dt).max, -0.0, 0.0], dt)
    return np.array([np.iinfo(dt).min, np.iinfo(dt).max, 0, 1], dt)


def neighbours(v):
    """(next representable value below, above) of every entry; integer types saturate"""
    if v.dtype.kind == "f":
        return np.nextafter(v, v.dtype.type(-np.inf)), np.nextafter(v, v.dtype.type(np.inf))
    info = np.iinfo(v.dtype)
    return np.where(v > info.min, v - v.dtype.type(1), v), np.where(v < info.max, v + v.dtype.type(1), v)


def sorted_table(dt, K, seed):
    """K sorted entries with repeats, spread over a range well inside the type"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind == "f":
        t = (rng.standard_normal(K) * 100.0).astype(dt)
        t = np.round(t * 8) / 8 if K > 8 else t                 # ties
    elif dt.kind == "u":
        t = rng.integers(0, min(np.iinfo(dt).max, 16 * K + 1000), K, dtype=np.uint64, endpoint=True)
        t = (t + np.uint64(np.iinfo(dt).max // 2 - 8 * K)).astype(dt)        # straddles the sign bit of the signed twin
    else:
        t = rng.integers(-8 * K - 500, 8 * K + 500, K, dtype=np.int64).astype(dt)
    return np.sort(t)


def needles_for(table, n, seed):
    """random over 1.25 x the table's range; in front: copies of table entries, of their neighbours below and above, the extremes"""
    rng = np.random.default_rng(seed)
    dt, K = table.dtype, table.size
    if dt.kind == "f":
        lo, hi = float(table[0]), float(table[-1])
        span = max(hi - lo, 8.0)
        v = rng.uniform(lo - 0.125 * span, hi + 0.125 * span, n).astype(dt)
    else:
        lo, hi, info = int(table[0]), int(table[-1]), np.iinfo(dt)
        span = max(hi - lo, 8)
        v = rng.integers(max(info.min, lo - span // 8), min(info.max, hi + span // 8), n, dtype=dt, endpoint=True)
    picks = table[rng.integers(0, K, min(K, 1000))]
    below, above = neighbours(picks)
    front = np.concatenate([picks, below, above, extremes(dt)])
    m = min(front.size, n)
    v[:m] = front[:m]
    return v


def run(capi, dtable, dneedles, n, right):
    out = capi.Buf(np.uint32, n)
    capi.check(capi.lib.ek_hip_search_sorted(dtable.ek, ctypes.c_void_p(out.ptr), ctypes.c_void_p(dtable.ptr), SZ(dtable.n),
                                             ctypes.c_void_p(dneedles.ptr), SZ(n), int(right)))
    return out.numpy()


# ---- 1. sizes from the plan ----------------------------------------------------------------------------------------
K_NAMES = ["1", "2", "63", "64", "65", "1000", "R-1", "R", "R+1", "R*stride/2+3", "2^20+3"]


def plan_sizes(capi, dt):
    R = capi.search_sorted_plan(dt, 1 << 31)[0]                  # every sample slot is in use for a table this large
    big = (1 << 20) + 3
    _, stride, steps = capi.search_sorted_plan(dt, big)
    if steps < 2:
        big = 4 * R * stride + 3
        _, stride, steps = capi.search_sorted_plan(dt, big)
    assert steps >= 2 and stride == 1 << steps
    return R, stride, dict(zip(K_NAMES, [1, 2, 63, 64, 65, 1000, R - 1, R, R + 1, R * stride // 2 + 3, big]))


def needle_counts():
    trip = BLOCKS_PER_CU * cu_count() * BLOCK * NEEDLES_PER_LANE
    past = 262144 + 77
    return [1, 63, 64 * 4 + 1, past if past > trip else trip + 77]


@pytest.mark.parametrize("k_name", K_NAMES)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_sizes_from_the_plan(capi, dt, k_name):
    R, stride, sizes = plan_sizes(capi, dt)
    K = sizes[k_name]
    resident, s, steps = capi.search_sorted_plan(dt, K)
    assert (s == 1 and steps == 0 and resident == K) if K <= R else (s > 1 and resident <= R and resident * s <= K < (resident + 1) * s)
    counts = needle_counts()
    table = sorted_table(dt, K, 11)
    needles = needles_for(table, max(counts), 12)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        want = expected(table, needles, right)                   # once; a shorter call searches a prefix of the same needles
        for n in counts:
            got = run(capi, dtable, dneedles, n, right)
            assert np.array_equal(got, want[:n]), (name(dt), K, n, right, np.flatnonzero(got != want[:n])[:8])


# ---- 2. runs of duplicates across sample boundaries ----------------------------------------------------------------
@pytest.mark.parametrize("run_length", ["stride-1", "stride", "2*stride+1"])
@pytest.mark.parametrize("dt", [np.float32, np.uint32], ids=name)
def test_runs_of_duplicates_straddle_sample_boundaries(capi, dt, run_length):
    R, stride0, _ = plan_sizes(capi, dt)
    K = 4 * R * stride0
    _, stride, steps = capi.search_sorted_plan(dt, K)
    assert stride > 1 and steps >= 2
    L = {"stride-1": stride - 1, "stride": stride, "2*stride+1": 2 * stride + 1}[run_length]
    runs = -(-K // L)
    assert runs < 1 << 24
    if np.dtype(dt).kind == "f":
        values = (np.arange(runs, dtype=np.int64) - runs // 2).astype(dt) * dt(0.5)   # distinct, ascending, exact
    else:
        values = (np.arange(runs, dtype=np.int64) * 3 + (1 << 31) - runs).astype(dt)  # ... and across the sign bit of int32
    table = np.repeat(values, L)[:K]
    assert table.size == K and np.all(np.diff(table.astype(np.float64)) >= 0)
    first = np.arange(runs, dtype=np.int64) * L
    end = np.minimum(first + L, K)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(values)
    assert np.array_equal(run(capi, dtable, dneedles, runs, False), first.astype(np.uint32))
    assert np.array_equal(run(capi, dtable, dneedles, runs, True), end.astype(np.uint32))


# ---- 3. specials ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_float_specials(capi, dt):
    tiny = dt(1e-45) if dt == np.float32 else dt(5e-324)
    base = np.array([-np.inf, -1, -tiny, -0.0, 0.0, tiny, 1, np.inf], dt)
    assert base[2] != 0 and base[5] != 0                         # the smallest denormals, not flushed by numpy
    table = np.sort(np.concatenate([base] * 9)[:65], kind="stable")
    needles = (SPECIALS_F32 if dt == np.float32 else SPECIALS_F64).copy()
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        got = run(capi, dtable, dneedles, needles.size, right)
        assert np.all(got[np.isnan(needles)] == 0)
        assert np.array_equal(got, expected(table, needles, right)), (right, needles[got != expected(table, needles, right)])
    # -0.0 < 0.0 is false: the two zeros are one value on both sides; the denormals next to them are not
    z = run(capi, dtable, capi.Buf.from_numpy(np.array([-0.0, 0.0, -tiny, tiny], dt)), 4, False)
    assert z[0] == z[1] and z[2] < z[0] < z[3]


@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=name)
def test_unsigned_types_compare_unsigned(capi, dt):
    top = 1 << (8 * np.dtype(dt).itemsize - 1)
    table = np.sort(np.array([0, 1, top - 2, top - 1, top, top + 1, top + 7, 2 * top - 2, 2 * top - 1] * 8, dt))
    needles = np.array([0, 1, 2, top - 1, top, top + 1, top + 2, top + 8, 2 * top - 3, 2 * top - 2, 2 * top - 1], dt)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        assert np.array_equal(run(capi, dtable, dneedles, needles.size, right), expected(table, needles, right))


# ---- 4. the parent's spelling --------------------------------------------------------------------------------------
def test_equals_the_binary_search_spelling(ekc, ad):
    rng = np.random.default_rng(2)
    K, n = 1000, 4099
    table = np.sort(rng.standard_normal(K).astype(np.float32))
    needles = (rng.standard_normal(n) * 1.5).astype(np.float32)
    needles[::97] = np.nan
    needles[5:K:7] = table[5:K:7]
    want = expected(table, needles, False)
    for mod in (ekc, ad):
        T, Nd = mod.Float32(table), mod.Float32(needles)
        last = mod.UInt32(np.array([K - 1], np.uint32))
        loop = mod.binary_search(0, K, lambda i: mod.gather(T, mod.min(i, last)) < Nd).numpy()
        got = mod.search_sorted(T, Nd)
        assert type(got) is mod.UInt32
        assert np.array_equal(got.numpy(), loop) and np.array_equal(loop, want)
        assert np.array_equal(mod.search_sorted(T, Nd, right=True).numpy(), expected(table, needles, True))
    T, Nd = ad.Float32(table), ad.Float32(needles)
    ad.set_requires_gradient(T)
    ad.set_requires_gradient(Nd)
    got = ad.search_sorted(T, Nd)
    assert not ad.requires_gradient(got) and np.array_equal(got.numpy(), want)
    import enoki as ek
    assert np.array_equal(ek.search_sorted(ekc.Float32(table), ekc.Float32(needles)).numpy(), want)
    assert np.array_equal(ek.search_sorted(T, Nd, True).numpy(), expected(table, needles, True))
    # the other element types reach the kernel from python as well
    for mod in (ekc, ad):
        for cls, dt in (("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)):
            t = sorted_table(dt, 300, 3)
            v = needles_for(t, 777, 4)
            A = getattr(mod, cls)
            assert np.array_equal(mod.search_sorted(A(t), A(v), True).numpy(), expected(t, v, True)), cls


# ---- 5. one launch -------------------------------------------------------------------------------------------------
def profiled(m, fn):
    m.hip_profile_begin()
    out = fn()
    return out, {k["kernel"]: k["launches"] for k in json.loads(m.hip_profile_end()) if k["launches"]}


def test_one_launch_and_nothing_else(ekc):
    rng = np.random.default_rng(5)
    table = np.sort(rng.standard_normal(5000).astype(np.float32))
    hx = rng.standard_normal(70001).astype(np.float32)
    T, x = ekc.Float32(table), ekc.Float32(hx)
    l0 = ekc.hip_launch_count()
    got, ks = profiled(ekc, lambda: ekc.search_sorted(T, x))
    assert ekc.hip_launch_count() - l0 == 1 and ks == {"search_sorted": 1}, ks
    assert not any(k.startswith(("gather", "select", "compare")) for k in ks)
    assert np.array_equal(got.numpy(), expected(table, hx, False))
    # an unevaluated needle operand is evaluated first: two launches
    l0 = ekc.hip_launch_count()
    got, ks = profiled(ekc, lambda: ekc.search_sorted(T, x * 2))
    assert ekc.hip_launch_count() - l0 == 2 and ks.get("search_sorted") == 1 and sum(ks.values()) == 2, ks
    assert np.array_equal(got.numpy(), expected(table, hx * np.float32(2), False))


# ---- 6. element-aligned pointers -----------------------------------------------------------------------------------
def test_pointers_that_are_only_element_aligned(capi):
    n = 1025
    table = sorted_table(np.float32, 3000, 21)
    needles = needles_for(table, n, 22)
    want = expected(table, needles, True)
    dtable = capi.Buf.from_numpy(table)
    aligned = run(capi, dtable, capi.Buf.from_numpy(needles), n, True)
    assert np.array_equal(aligned, want)
    shifted = capi.Buf.from_numpy(np.concatenate([np.zeros(1, np.float32), needles]))
    out = capi.Buf.from_numpy(np.full(n + 2, 0xDEADBEEF, np.uint32))
    for needle_off, out_off in ((1, 0), (0, 1), (1, 1)):
        src = shifted.view(1, n) if needle_off else capi.Buf.from_numpy(needles)
        capi.check(capi.lib.ek_hip_memset(ctypes.c_void_p(out.ptr), 0xEE, SZ(4 * (n + 2))))
        capi.check(capi.lib.ek_hip_search_sorted(capi.F32, ctypes.c_void_p(out.ptr + 4 * out_off), ctypes.c_void_p(dtable.ptr), SZ(table.size),
                                                 ctypes.c_void_p(src.ptr), SZ(n), 1))
        got = out.numpy()
        assert np.array_equal(got[out_off:out_off + n], aligned), (needle_off, out_off)
        assert np.all(got[:out_off] == 0xEEEEEEEE) and np.all(got[out_off + n:] == 0xEEEEEEEE)      # nothing written outside


# ---- 7. inside a step graph ----------------------------------------------------------------------------------------
def _refill(capi, arr, host):
    host = np.ascontiguousarray(host)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(arr.data_ptr()), host.ctypes.data_as(ctypes.c_void_p), SZ(host.nbytes)))


def test_inside_a_step_graph(ekc, capi):
    K, n = (1 << 17) + 9, 50001                                  # sampled: the replay reads the table in LDS and in global memory
    assert capi.search_sorted_plan(np.float32, K)[2] >= 1
    t1, t2 = sorted_table(np.float32, K, 31), sorted_table(np.float32, K, 32) * np.float32(0.5)
    v1, v2 = needles_for(t1, n, 33), needles_for(t2, n, 34)
    T, Nd = ekc.Float32(t1), ekc.Float32(v1)
    held = {}
    ekc.hip_graph_begin()
    held["out"] = ekc.search_sorted(T, Nd, True)
    g = ekc.hip_graph_end()
    try:
        assert ekc.hip_graph_launch_count(g) == 1
        ekc.hip_graph_launch(g)
        assert np.array_equal(held["out"].numpy(), expected(t1, v1, True))
        _refill(capi, Nd, v2)
        _refill(capi, T, t2)
        ekc.hip_graph_launch(g)
        assert np.array_equal(held["out"].numpy(), expected(t2, v2, True))
    finally:
        ekc.hip_graph_destroy(g)


# ---- 8. error codes ------------------------------------------------------------------------------------------------
def test_error_codes(capi):
    lib = capi.lib
    table, needles = capi.Buf.from_numpy(np.arange(8, dtype=np.float32)), capi.Buf.from_numpy(np.array([2.5, 9, -1], np.float32))
    out = capi.Buf.from_numpy(np.full(3, 7, np.uint32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    call = lib.ek_hip_search_sorted
    assert call(capi.F32, None, p(table), SZ(8), p(needles), SZ(3), 0) == -1 and b"null" in lib.ek_hip_last_error()
    assert call(capi.F32, p(out), p(table), SZ(8), None, SZ(3), 0) == -1
    assert call(capi.F32, p(out), None, SZ(8), p(needles), SZ(3), 0) == -1
    assert call(capi.BOOL, p(out), p(table), SZ(8), p(needles), SZ(3), 0) == -2 and b"unsupported" in lib.ek_hip_last_error()
    assert call(99, p(out), p(table), SZ(8), p(needles), SZ(3), 0) == -2
    assert call(capi.F32, p(out), p(table), SZ(1 << 32), p(needles), SZ(1), 0) == -2         # refused before any memory is touched
    l0 = lib.ek_hip_launch_count()
    assert call(capi.F32, None, None, SZ(8), None, SZ(0), 0) == 0 and lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), [7, 7, 7])
    assert call(capi.F32, p(out), None, SZ(0), p(needles), SZ(3), 1) == 0                     # an empty table: zeros
    assert np.array_equal(out.numpy(), [0, 0, 0])
    r, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    plan = lib.ek_hip_search_sorted_plan
    assert plan(capi.BOOL, SZ(8), ctypes.byref(r), ctypes.byref(s), ctypes.byref(g)) == -2
    assert plan(99, SZ(8), ctypes.byref(r), ctypes.byref(s), ctypes.byref(g)) == -2
    assert plan(capi.F64, SZ(1 << 32), ctypes.byref(r), ctypes.byref(s), ctypes.byref(g)) == -2
    assert plan(capi.F64, SZ(0), ctypes.byref(r), ctypes.byref(s), ctypes.byref(g)) == 0 and (r.value, s.value, g.value) == (0, 1, 0)
    # the call after a refused one works
    assert call(capi.F32, p(out), p(table), SZ(8), p(needles), SZ(3), 0) == 0
    assert np.array_equal(out.numpy(), [3, 8, 0])
