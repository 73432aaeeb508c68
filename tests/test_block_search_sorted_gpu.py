"""block_search_sorted: every needle searched in its own sorted row of a row-major table, one kernel (csrc/block_search.hip).

Expected values are numpy.searchsorted(table[r * B:(r + 1) * B], v, side) per row, 0 for a NaN needle (the comparisons are the
type's own).  Every comparison is exact equality of uint32 arrays.  The sizes at which the kernel changes its shape -- rows per
tile, workgroups per row, resident / sampled rows and their stride, staged or global indexed needles -- are asked from
ek_hip_search_sorted_blocks_plan, not copied.  One case (more tiles than one grid trip) needs about 2 Mi table entries: a trip is
two workgroups per compute unit, and a tile of one row cannot be smaller than half the LDS plus one entry."""
import ctypes
import json

import numpy as np
import pytest

from conftest import SPECIALS_F32, SPECIALS_F64

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
LDS = 64 * 1024
TILE, SAMPLED, INDEXED_LDS, INDEXED_GLOBAL, ONE_ROW = 1, 2, 3, 4, 5
BLOCKS_PER_CU = 2                                               # the grid of every route (csrc/ek_search.h)


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


def expected(table, needles, B, right, rows=None):
    """table: R * B entries; needles: blocked (rows None) or with one row per needle, clamped to R - 1"""
    R = table.size // B
    side = "right" if right else "left"
    want = np.empty(needles.size, np.uint32)
    if rows is None:
        M = needles.size // R
        for r in range(R):
            want[r * M:(r + 1) * M] = np.searchsorted(table[r * B:(r + 1) * B], needles[r * M:(r + 1) * M], side=side)
    else:
        rows = np.minimum(rows.astype(np.int64), R - 1)
        for r in np.unique(rows):
            sel = rows == r
            want[sel] = np.searchsorted(table[r * B:(r + 1) * B], needles[sel], side=side)
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


def sorted_rows(dt, R, B, seed):
    """R rows of B sorted entries with repeats; every row has its own offset and the offsets DESCEND, so the table as a whole is not
    sorted and a search that strays into the next row finds smaller entries there"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    shift = (R - 1 - np.arange(R, dtype=np.int64))[:, None] * 3
    if dt.kind == "f":
        t = np.round(rng.standard_normal((R, B)) * 100.0 * 8) / 8 + shift
    elif dt.kind == "u":
        t = rng.integers(0, 16 * B + 1000, (R, B), dtype=np.uint64) + shift.astype(np.uint64)
        t = t + np.uint64(np.iinfo(dt).max // 2 - 8 * B - 3 * R)                 # straddles the sign bit of the signed twin
    else:
        t = rng.integers(-8 * B - 500, 8 * B + 500, (R, B)) + shift
    return np.sort(t.astype(dt), axis=1).reshape(-1)


def needles_for(table, B, n, seed, rows=None):
    """random over 1.25 x the table's range; every 5th needle a copy of an entry of ITS row or that entry's neighbour below or above;
    the extremes in front"""
    rng = np.random.default_rng(seed)
    dt, R = table.dtype, table.size // B
    if dt.kind == "f":
        lo, hi = float(table.min()), float(table.max())
        span = max(hi - lo, 8.0)
        v = rng.uniform(lo - 0.125 * span, hi + 0.125 * span, n).astype(dt)
    else:
        lo, hi, info = int(table.min()), int(table.max()), np.iinfo(dt)
        span = max(hi - lo, 8)
        v = rng.integers(max(info.min, lo - span // 8), min(info.max, hi + span // 8), n, dtype=dt, endpoint=True)
    e = np.arange(0, n, 5)
    row = (e // (n // R)) if rows is None else np.minimum(rows[e].astype(np.int64), R - 1)
    picks = table[row * B + rng.integers(0, B, e.size)]
    below, above = neighbours(picks)
    v[e] = np.choose(rng.integers(0, 3, e.size), [picks, below, above])
    ext = extremes(dt)
    m = min(ext.size, n)
    v[:m] = ext[:m]
    return v


def run(capi, dtable, B, dneedles, n, right, drows=None):
    out = capi.Buf(np.uint32, n)
    capi.check(capi.lib.ek_hip_search_sorted_blocks(dtable.ek, ctypes.c_void_p(out.ptr), ctypes.c_void_p(dtable.ptr), SZ(dtable.n // B), SZ(B),
                                                    ctypes.c_void_p(dneedles.ptr), SZ(n), ctypes.c_void_p(drows.ptr) if drows else None,
                                                    int(right)))
    return out.numpy()


def check_blocked(capi, dt, R, B, M, seed=11, table=None):
    table = sorted_rows(dt, R, B, seed) if table is None else table
    needles = needles_for(table, B, R * M, seed + 1)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        want = expected(table, needles, B, right)
        got = run(capi, dtable, B, dneedles, R * M, right)
        assert got.max() <= B
        assert np.array_equal(got, want), (name(dt), R, B, M, right, np.flatnonzero(got != want)[:8])


# ---- 1. sizes from the plan ----------------------------------------------------------------------------------------
B_NAMES = ["1", "2", "3", "63", "64", "65", "1000", "cap-1", "cap", "cap+1", "two-steps"]
NEEDLES_PER_ROW = [1, 3, 4, 5, 257]


def block_sizes(capi, dt):
    cap = LDS // np.dtype(dt).itemsize
    deep = 2 * cap + 3
    while capi.search_sorted_blocks_plan(dt, 3, deep, 3 * 65536, False, cu_count())[5] < 2:
        deep += cap
    return cap, dict(zip(B_NAMES, [1, 2, 3, 63, 64, 65, 1000, cap - 1, cap, cap + 1, deep]))


@pytest.mark.parametrize("b_name", B_NAMES)
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_sizes_from_the_plan(capi, dt, b_name):
    cap, sizes = block_sizes(capi, dt)
    B = sizes[b_name]
    R = max(2, min(301, (1 << 18) // B))                         # odd, and at least two rows: one row is another route
    table = sorted_rows(dt, R, B, 11)
    for M in NEEDLES_PER_ROW:
        route, t, s, resident, stride, steps = capi.search_sorted_blocks_plan(dt, R, B, R * M, False, cu_count())
        assert route == (TILE if B <= cap else SAMPLED) and (route == SAMPLED or t * B <= cap)
        assert resident * stride <= B < (resident + 1) * stride
        check_blocked(capi, dt, R, B, M, table=table)
    if b_name == "two-steps":
        assert capi.search_sorted_blocks_plan(dt, R, B, R * 65536, False, cu_count())[5] >= 2
        assert capi.search_sorted_blocks_plan(dt, R, B, R * 4, False, cu_count())[5] >= 2        # ... and more with few needles


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_a_row_split_over_several_workgroups(capi, dt):
    cap, sizes = block_sizes(capi, dt)
    R, M = 3, 100003
    for B in (1000, sizes["two-steps"]):
        route, t, s, *_ = capi.search_sorted_blocks_plan(dt, R, B, R * M, False, cu_count())
        assert route == (TILE if B <= cap else SAMPLED) and t == 1 and s >= 2 and M % s != 0
        check_blocked(capi, dt, R, B, M)


def test_more_tiles_than_one_grid_trip(capi):
    dt = np.float64
    cap = LDS // 8
    B, R, M = cap // 2 + 1, BLOCKS_PER_CU * cu_count() + 3, 3
    route, t, s, *_ = capi.search_sorted_blocks_plan(dt, R, B, R * M, False, cu_count())
    assert route == TILE and t == 1 and s == 1 and R > BLOCKS_PER_CU * cu_count()
    check_blocked(capi, dt, R, B, M)


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_a_last_tile_of_fewer_rows(capi, dt):
    B, M = 64, 64
    t = capi.search_sorted_blocks_plan(dt, 4096, B, 4096 * M, False, cu_count())[1]
    R = 3 * t + t // 2 + 1
    route, t2, s, *_ = capi.search_sorted_blocks_plan(dt, R, B, R * M, False, cu_count())
    assert route == TILE and t2 > 1 and R % t2 != 0
    check_blocked(capi, dt, R, B, M)
    # ... and many tiles whose needles start at every alignment: M odd
    R = 4096 + 5
    for B in range(61, 100):                                     # the first row length whose tiles hold no whole number of items
        route, t3, s, *_ = capi.search_sorted_blocks_plan(dt, R, B, R * 7, False, cu_count())
        if (t3 * 7) % 4 != 0:
            break
    assert route == TILE and 1 < t3 < R and R % t3 != 0 and (t3 * 7) % 4 != 0
    check_blocked(capi, dt, R, B, 7)


# ---- 2. rows that would fool a global search -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["descending", "touching"])
@pytest.mark.parametrize("B", [1, 5, 64, 1000, "cap", "cap+1", "two-steps"])
@pytest.mark.parametrize("dt", [np.float32, np.uint64], ids=name)
def test_no_entry_leaks_across_a_row_boundary(capi, dt, B, layout):
    cap, sizes = block_sizes(capi, dt)
    B = sizes[B] if isinstance(B, str) else B
    R, run_len = 6, min(B, 4)
    rows = []
    for r in range(R):
        # descending: row r + 1 lies wholly below row r; touching: row r ends with a run of the value row r + 1 begins with
        start = (R - r) * 4 * B if layout == "descending" else r * 2 * (B - 1)
        row = (1 << 20) + start + 2 * np.arange(B, dtype=np.int64)
        row[B - run_len:] = row[-1]
        row[:run_len] = row[0]
        rows.append(row)
    assert all(np.all(np.diff(x) >= 0) for x in rows)
    assert all((rows[r + 1][-1] < rows[r][0]) if layout == "descending" else (rows[r + 1][0] == rows[r][-1]) for r in range(R - 1))
    table = np.concatenate(rows).astype(dt)
    # per row: the first and last value of the row, of the row before and of the row after, and their neighbours below and above
    edges = [np.array([rows[q % R][0], rows[q % R][-1]], np.int64) for q in range(-1, R + 1)]
    needles = []
    for r in range(R):
        edge = np.concatenate(edges[r:r + 3]).astype(dt)
        lo, hi = neighbours(edge)
        needles.append(np.concatenate([edge, lo, hi]))
    M = needles[0].size
    needles = np.concatenate(needles)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        got = run(capi, dtable, B, dneedles, R * M, right)
        assert got.max() <= B
        assert np.array_equal(got, expected(table, needles, B, right)), (B, right, got)
    # the same needles with their rows given, against their own row and against its neighbours
    own = np.repeat(np.arange(R, dtype=np.uint32), M)
    for shift in (0, 1, R - 1):
        ri = ((own + shift) % R).astype(np.uint32)
        for right in (False, True):
            got = run(capi, dtable, B, dneedles, R * M, right, capi.Buf.from_numpy(ri))
            assert got.max() <= B and np.array_equal(got, expected(table, needles, B, right, ri)), (B, shift, right)


# ---- 3. runs of duplicates across sample boundaries, in a row that is not row 0 -------------------------------------
@pytest.mark.parametrize("run_length", ["stride-1", "stride", "2*stride+1"])
@pytest.mark.parametrize("dt", [np.float32, np.uint32], ids=name)
def test_runs_of_duplicates_straddle_sample_boundaries(capi, dt, run_length):
    cap, sizes = block_sizes(capi, dt)
    B, R, M = sizes["two-steps"], 3, 65536
    route, t, s, resident, stride, steps = capi.search_sorted_blocks_plan(dt, R, B, R * M, False, cu_count())
    assert route == SAMPLED and stride >= 4 and steps >= 2
    L = {"stride-1": stride - 1, "stride": stride, "2*stride+1": 2 * stride + 1}[run_length]
    runs = -(-B // L)
    assert runs <= M
    if np.dtype(dt).kind == "f":
        values = (np.arange(runs, dtype=np.int64) - runs // 2).astype(dt) * dt(0.5)   # distinct, ascending, exact
    else:
        values = (np.arange(runs, dtype=np.int64) * 3 + (1 << 31) - runs).astype(dt)  # ... and across the sign bit of int32
    row = np.repeat(values, L)[:B]
    other = sorted_rows(dt, 1, B, 5)
    table = np.concatenate([other, row, other])
    needles = np.concatenate([np.resize(values, M)] * 3)         # rows 0 and 2 search the same needles in another row
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    first = np.resize(np.arange(runs, dtype=np.int64) * L, M)
    end = np.minimum(first + L, B)
    for right, want_row in ((False, first), (True, end)):
        got = run(capi, dtable, B, dneedles, R * M, right)
        assert np.array_equal(got[M:2 * M], want_row.astype(np.uint32))
        assert np.array_equal(got, expected(table, needles, B, right))


# ---- 4. specials ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_float_specials(capi, dt):
    tiny = dt(1e-45) if dt == np.float32 else dt(5e-324)
    base = np.array([-np.inf, -1, -tiny, -0.0, 0.0, tiny, 1, np.inf], dt)
    assert base[2] != 0 and base[5] != 0
    B = 65
    row_a = np.sort(np.concatenate([base] * 9)[:B], kind="stable")
    row_b = np.sort(np.concatenate([base[::-1]] * 9)[:B], kind="stable")
    table = np.concatenate([row_b, row_a, row_b])
    specials = (SPECIALS_F32 if dt == np.float32 else SPECIALS_F64).copy()
    needles = np.concatenate([specials] * 3)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        got = run(capi, dtable, B, dneedles, needles.size, right)
        assert np.all(got[np.isnan(needles)] == 0)
        assert np.array_equal(got, expected(table, needles, B, right)), right
    z = run(capi, dtable, B, capi.Buf.from_numpy(np.array([-0.0, 0.0, -tiny, tiny] * 3, dt)), 12, False)[4:8]
    assert z[0] == z[1] and z[2] < z[0] < z[3]


@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=name)
def test_unsigned_types_compare_unsigned(capi, dt):
    top = 1 << (8 * np.dtype(dt).itemsize - 1)
    row = np.sort(np.array([0, 1, top - 2, top - 1, top, top + 1, top + 7, 2 * top - 2, 2 * top - 1] * 8, dt))
    low = np.sort(np.array([0, 1, 2, 3, top - 2, top - 1] * 12, dt))
    table = np.concatenate([low, row, low])
    needles = np.array([0, 1, 2, top - 1, top, top + 1, top + 2, top + 8, 2 * top - 3, 2 * top - 2, 2 * top - 1] * 3, dt)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        assert np.array_equal(run(capi, dtable, row.size, dneedles, needles.size, right), expected(table, needles, row.size, right))


# ---- 5. indexed needles --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [INDEXED_LDS, INDEXED_GLOBAL])
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_indexed_needles(capi, dt, route):
    cap = LDS // np.dtype(dt).itemsize
    R, B = (7, cap // 7) if route == INDEXED_LDS else (37, 1000)
    M = 1201
    n = R * M
    assert capi.search_sorted_blocks_plan(dt, R, B, n, True, cu_count())[0] == route
    if route == INDEXED_LDS:                                     # ... and one entry more per row no longer fits
        assert capi.search_sorted_blocks_plan(dt, R, B + 1, n, True, cu_count())[0] == INDEXED_GLOBAL
    table = sorted_rows(dt, R, B, 41)
    dtable = capi.Buf.from_numpy(table)
    rng = np.random.default_rng(42)
    ascending = (np.arange(n) // M).astype(np.uint32)
    beyond = rng.integers(0, 2 * R, n).astype(np.uint32)
    beyond[::13] = 0xFFFFFFFF
    beyond[1::13] = R
    beyond[2::13] = 0x80000000
    for label, rows in (("random", rng.integers(0, R, n).astype(np.uint32)), ("one row", np.full(n, R // 2, np.uint32)),
                        ("ascending", ascending), ("beyond", beyond)):
        needles = needles_for(table, B, n, 43, rows)
        dneedles, drows = capi.Buf.from_numpy(needles), capi.Buf.from_numpy(rows)
        for right in (False, True):
            got = run(capi, dtable, B, dneedles, n, right, drows)
            assert got.max() <= B
            assert np.array_equal(got, expected(table, needles, B, right, rows)), (label, right)
            if label == "ascending":
                assert np.array_equal(got, run(capi, dtable, B, dneedles, n, right)), "equals the blocked call"
            for short in (1, 3, 5):                              # fewer needles than one item, and a tail
                assert np.array_equal(run(capi, dtable, B, dneedles, short, right, drows), got[:short])


# ---- 6. one row is search_sorted ------------------------------------------------------------------------------------
def profiled(m, fn):
    m.hip_profile_begin()
    out = fn()
    return out, {k["kernel"]: k["launches"] for k in json.loads(m.hip_profile_end()) if k["launches"]}


@pytest.mark.parametrize("B", [1000, (1 << 17) + 9])
def test_one_row_is_search_sorted(capi, ekc, B):
    dt, n = np.float32, 70001
    assert capi.search_sorted_blocks_plan(dt, 1, B, n, False, cu_count())[0] == ONE_ROW
    table = sorted_rows(dt, 1, B, 51)
    needles = needles_for(table, B, n, 52)
    dtable, dneedles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    for right in (False, True):
        got, ks = profiled(ekc, lambda: run(capi, dtable, B, dneedles, n, right))
        assert ks == {"search_sorted": 1}, ks
        assert np.array_equal(got, capi.search_sorted(dtable, dneedles, right).numpy())
        assert np.array_equal(got, expected(table, needles, B, right))


# ---- 7. the parent's spelling --------------------------------------------------------------------------------------
def test_equals_the_binary_search_spelling(ekc, ad):
    rng = np.random.default_rng(2)
    R, B, M = 13, 1000, 317
    n = R * M
    table = sorted_rows(np.float32, R, B, 61)
    needles = needles_for(table, B, n, 62)
    needles[::97] = np.nan
    rows = rng.integers(0, R, n).astype(np.uint32)
    blocked_rows = (np.arange(n) // M).astype(np.uint32)
    for mod in (ekc, ad):
        T, Nd = mod.Float32(table), mod.Float32(needles)
        last, width = mod.UInt32(np.array([B - 1], np.uint32)), mod.UInt32(np.array([B], np.uint32))
        for row_host, kwargs in ((blocked_rows, {}), (rows, {"rows": mod.UInt32(rows)})):
            row = mod.UInt32(row_host)
            loop = mod.binary_search(0, B, lambda i: mod.gather(T, row * width + mod.min(i, last)) < Nd).numpy()
            got = mod.block_search_sorted(T, Nd, B, **kwargs)
            assert type(got) is mod.UInt32
            assert np.array_equal(got.numpy(), loop) and np.array_equal(loop, expected(table, needles, B, False, row_host))
            assert np.array_equal(mod.block_search_sorted(T, Nd, B, right=True, **kwargs).numpy(), expected(table, needles, B, True, row_host))
    T, Nd = ad.Float32(table), ad.Float32(needles)
    ad.set_requires_gradient(T)
    ad.set_requires_gradient(Nd)
    got = ad.block_search_sorted(T, Nd, B)
    assert not ad.requires_gradient(got) and np.array_equal(got.numpy(), expected(table, needles, B, False))
    got = ad.block_search_sorted(T, Nd, B, rows=ad.UInt32(rows))
    assert not ad.requires_gradient(got) and np.array_equal(got.numpy(), expected(table, needles, B, False, rows))
    import enoki as ek
    assert np.array_equal(ek.block_search_sorted(ekc.Float32(table), ekc.Float32(needles), B).numpy(), expected(table, needles, B, False))
    assert np.array_equal(ek.block_search_sorted(T, Nd, B, True).numpy(), expected(table, needles, B, True))
    # what the binding layer refuses
    with pytest.raises(Exception):
        ekc.block_search_sorted(ekc.Float32(table), ekc.Float32(needles[:n - 1]), B)
    with pytest.raises(Exception):
        ekc.block_search_sorted(ekc.Float32(table), ekc.Float32(needles), B + 1)
    with pytest.raises(Exception):
        ekc.block_search_sorted(ekc.Float32(table), ekc.Float32(needles), B, rows=ekc.UInt32(rows[:5]))
    with pytest.raises(TypeError):
        ekc.block_search_sorted(ekc.Float32(table), ekc.UInt32(rows), B)
    # the other element types reach the kernel from python as well
    for mod in (ekc, ad):
        for cls, dt in (("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)):
            t = sorted_rows(dt, 5, 300, 3)
            v = needles_for(t, 300, 5 * 155, 4)
            A = getattr(mod, cls)
            assert np.array_equal(mod.block_search_sorted(A(t), A(v), 300, True).numpy(), expected(t, v, 300, True)), cls


# ---- 8. one launch -------------------------------------------------------------------------------------------------
def test_one_launch_and_nothing_else(ekc):
    rng = np.random.default_rng(5)
    R, B, M = 48, 100, 1400                                      # (a multiple of the 3 rows of `big` as well)
    table = sorted_rows(np.float32, R, B, 71)
    hx = (rng.standard_normal(R * M) * 100).astype(np.float32)
    rows = rng.integers(0, R, R * M).astype(np.uint32)
    T, x, rw = ekc.Float32(table), ekc.Float32(hx), ekc.UInt32(rows)
    big = ekc.Float32(sorted_rows(np.float32, 3, 20000, 72))
    for fn, want in ((lambda: ekc.block_search_sorted(T, x, B), expected(table, hx, B, False)),
                     (lambda: ekc.block_search_sorted(T, x, B, rows=rw), expected(table, hx, B, False, rows)),
                     (lambda: ekc.block_search_sorted(big, x, 20000), None),
                     (lambda: ekc.block_search_sorted(big, x, 20000, rows=rw), None)):
        l0 = ekc.hip_launch_count()
        got, ks = profiled(ekc, fn)
        assert ekc.hip_launch_count() - l0 == 1 and ks == {"block_search_sorted": 1}, ks
        assert want is None or np.array_equal(got.numpy(), want)
    # an unevaluated needle operand is evaluated first: two launches
    l0 = ekc.hip_launch_count()
    got, ks = profiled(ekc, lambda: ekc.block_search_sorted(T, x * 2, B))
    assert ekc.hip_launch_count() - l0 == 2 and ks.get("block_search_sorted") == 1 and sum(ks.values()) == 2, ks
    assert np.array_equal(got.numpy(), expected(table, hx * np.float32(2), B, False))


# ---- 9. element-aligned pointers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
@pytest.mark.parametrize("shape", ["tile", "sampled", "indexed"])
def test_pointers_that_are_only_element_aligned(capi, dt, shape):
    cap = LDS // np.dtype(dt).itemsize
    R, B, M = (9, 333, 115) if shape != "sampled" else (3, cap + 5, 347)
    n = R * M
    table = sorted_rows(dt, R, B, 21)
    rows = (np.arange(n) * 7 % R).astype(np.uint32) if shape == "indexed" else None
    needles = needles_for(table, B, n, 22, rows)
    want = expected(table, needles, B, True, rows)
    lib = capi.lib
    shifted_table = capi.Buf.from_numpy(np.concatenate([np.zeros(1, dt), table]))
    shifted_needles = capi.Buf.from_numpy(np.concatenate([np.zeros(1, dt), needles]))
    shifted_rows = capi.Buf.from_numpy(np.concatenate([np.zeros(1, np.uint32), rows])) if rows is not None else None
    aligned_table, aligned_needles = capi.Buf.from_numpy(table), capi.Buf.from_numpy(needles)
    aligned_rows = capi.Buf.from_numpy(rows) if rows is not None else None
    out = capi.Buf(np.uint32, n + 2)
    for table_off, needle_off, out_off in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 0, 0)):
        tb = shifted_table.view(1, R * B) if table_off else aligned_table
        nd = shifted_needles.view(1, n) if needle_off else aligned_needles
        rw = None if rows is None else (shifted_rows.view(1, n) if needle_off else aligned_rows)
        capi.check(lib.ek_hip_memset(ctypes.c_void_p(out.ptr), 0xEE, SZ(4 * (n + 2))))
        capi.check(lib.ek_hip_search_sorted_blocks(tb.ek, ctypes.c_void_p(out.ptr + 4 * out_off), ctypes.c_void_p(tb.ptr), SZ(R), SZ(B),
                                                   ctypes.c_void_p(nd.ptr), SZ(n), ctypes.c_void_p(rw.ptr) if rw else None, 1))
        got = out.numpy()
        assert np.array_equal(got[out_off:out_off + n], want), (table_off, needle_off, out_off)
        assert np.all(got[:out_off] == 0xEEEEEEEE) and np.all(got[out_off + n:] == 0xEEEEEEEE)      # nothing written outside


# ---- 10. inside a step graph ---------------------------------------------------------------------------------------
def _refill(capi, arr, host):
    host = np.ascontiguousarray(host)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(arr.data_ptr()), host.ctypes.data_as(ctypes.c_void_p), SZ(host.nbytes)))


@pytest.mark.parametrize("shape", ["tile", "sampled"])
def test_inside_a_step_graph(ekc, capi, shape):
    R, B, M = (300, 100, 167) if shape == "tile" else (3, (1 << 17) + 9, 16667)
    assert capi.search_sorted_blocks_plan(np.float32, R, B, R * M, False, cu_count())[0] == (TILE if shape == "tile" else SAMPLED)
    t1, t2 = sorted_rows(np.float32, R, B, 31), sorted_rows(np.float32, R, B, 32) * np.float32(0.5)
    v1, v2 = needles_for(t1, B, R * M, 33), needles_for(t2, B, R * M, 34)
    T, Nd = ekc.Float32(t1), ekc.Float32(v1)
    held = {}
    ekc.hip_graph_begin()
    held["out"] = ekc.block_search_sorted(T, Nd, B, True)
    g = ekc.hip_graph_end()
    try:
        assert ekc.hip_graph_launch_count(g) == 1
        ekc.hip_graph_launch(g)
        assert np.array_equal(held["out"].numpy(), expected(t1, v1, B, True))
        _refill(capi, Nd, v2)
        _refill(capi, T, t2)
        ekc.hip_graph_launch(g)
        assert np.array_equal(held["out"].numpy(), expected(t2, v2, B, True))
    finally:
        ekc.hip_graph_destroy(g)


# ---- 11. error codes -----------------------------------------------------------------------------------------------
def test_error_codes(capi):
    lib = capi.lib
    table = capi.Buf.from_numpy(np.array([0, 1, 2, 3, 10, 11, 12, 13], np.float32))          # two rows of four
    needles = capi.Buf.from_numpy(np.array([2.5, 9, -1, 11], np.float32))
    rows = capi.Buf.from_numpy(np.array([1, 0, 7, 1], np.uint32))
    out = capi.Buf.from_numpy(np.full(4, 7, np.uint32))
    p = lambda b: ctypes.c_void_p(b.ptr) if b is not None else None
    call = lambda ty, o, t, R, B, v, n, rw, right=0: lib.ek_hip_search_sorted_blocks(ty, p(o), p(t), SZ(R), SZ(B), p(v), SZ(n), p(rw), right)
    INVALID, UNSUPPORTED = -1, -2
    assert call(capi.F32, None, table, 2, 4, needles, 4, None) == INVALID and b"null" in lib.ek_hip_last_error()
    assert call(capi.F32, out, table, 2, 4, None, 4, None) == INVALID
    assert call(capi.F32, out, None, 2, 4, needles, 4, None) == INVALID
    assert call(capi.F32, out, table, 2, 0, needles, 4, None) == INVALID                     # B = 0
    assert call(capi.F32, out, table, 2, 4, needles, 3, None) == INVALID                     # 3 needles over 2 rows
    assert call(capi.F32, out, table, 0, 4, needles, 4, None) == INVALID                     # needles and no row
    assert call(capi.F32, out, table, 0, 4, needles, 4, rows) == INVALID
    assert call(capi.BOOL, out, table, 2, 4, needles, 4, None) == UNSUPPORTED and b"unsupported" in lib.ek_hip_last_error()
    assert call(99, out, table, 2, 4, needles, 4, None) == UNSUPPORTED
    assert call(capi.F32, out, table, 1 << 16, 1 << 16, needles, 1 << 16, None) == UNSUPPORTED     # refused before any memory is touched
    assert call(capi.F32, out, table, 1 << 31, 2, needles, 4, rows) == UNSUPPORTED
    l0 = lib.ek_hip_launch_count()
    assert call(capi.F32, None, None, 2, 4, None, 0, None) == 0 and call(capi.F32, None, None, 0, 4, None, 0, None) == 0
    assert call(capi.F32, None, None, 2, 4, None, 0, rows) == 0 and lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), [7, 7, 7, 7])
    # the call after a refused one works, blocked and indexed (row 7 is row 1)
    assert call(capi.F32, out, table, 2, 4, needles, 4, None) == 0
    assert np.array_equal(out.numpy(), [3, 4, 0, 1])
    assert call(capi.F32, out, table, 2, 4, needles, 4, rows, 1) == 0
    assert np.array_equal(out.numpy(), [0, 4, 0, 2])
    assert call(capi.F32, out, table, 2, 4, needles, 3, rows) == 0                           # indexed: any number of needles
