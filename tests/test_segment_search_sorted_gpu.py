"""ek_hip_search_sorted_segments through the C ABI (csrc/segment_search.hip): every needle searched in its own ragged segment
[lo_j, hi_j) of a flat table, lo_j = min(table_starts[j], nt), hi_j = max(lo_j, min(table_starts[j + 1], nt)), table_starts[m] := nt.
The segment of needle e is the last j with needle_starts[j] <= e (none in front of needle_starts[0]) or min(rows[e], m - 1).

Every comparison is exact equality of uint32 arrays with numpy.searchsorted(table[lo_j:hi_j], v, side) per segment -- 0 for a NaN
needle, an empty segment and a needle without a segment; with `flat` plus lo_j (0 without a segment).  There is no tolerance
anywhere.  The sizes at which the kernel changes shape (needles per tile, starts per window, staged entries, workgroups) are asked
from ek_hip_search_sorted_segments_plan.  Bad index arrays are only ever tried on views into larger buffers of the test's own, no
bad value exceeds the enclosing allocation, and they are the inputs the clamp rule is designed for."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]           # (right, flat)
SZ = ctypes.c_size_t
TABLE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 1000]
NEEDLE_COUNTS = [0, 1, 5, 64, 300]


def name(dt):
    return np.dtype(dt).name


@functools.lru_cache(None)
def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(capi, dt, nt, m, n, indexed=False):
    """(route, tile_needles, tiles_per_workgroup, workgroups, lds_entries, window)"""
    return capi.search_sorted_segments_plan(dt, nt, m, n, indexed, cu_count())


def tile_of(capi, dt):
    return plan(capi, dt, 1, 1, 1)[1]


# ---- data ------------------------------------------------------------------------------------------------------------------
def starts_of(lengths, gap=0):
    lengths = np.asarray(lengths, np.int64)
    ends = gap + np.cumsum(lengths)
    return (ends - lengths).astype(np.uint32), int(ends[-1]) if lengths.size else gap


def bounds(table_starts, nt):
    s = np.minimum(table_starts.astype(np.int64), nt)
    nxt = np.concatenate([s[1:], [nt]]) if s.size else s
    return s, np.maximum(s, nxt)


def ragged_table(dt, lengths, seed):
    """sorted entries with repeats per segment; the segments' offsets DESCEND, so the table as a whole is not sorted and a search
    that strays into a neighbour finds smaller entries behind and larger ones in front"""
    rng = np.random.default_rng(seed)
    dt, lengths = np.dtype(dt), np.asarray(lengths, np.int64)
    m, nt = lengths.size, int(lengths.sum())
    seg = np.repeat(np.arange(m), lengths)
    shift = (m - 1 - seg) * 3
    if dt.kind == "f":
        t = np.round(rng.standard_normal(nt) * 100.0 * 8) / 8 + shift
    elif dt.kind == "u":
        t = rng.integers(0, 20000, nt, dtype=np.uint64) + shift.astype(np.uint64) + np.uint64(np.iinfo(dt).max // 2 - 10000 - 3 * m)
    else:
        t = rng.integers(-10000, 10000, nt) + shift
    t = t.astype(dt)
    order = np.lexsort((t, seg))                                   # sorted inside every segment
    return t[order]


def extremes(dt):
    dt = np.dtype(dt)
    if dt.kind == "f":
        info = np.finfo(dt)
        return np.array([-np.inf, np.inf, info.min, info.max, -0.0, 0.0, np.nan, info.tiny], dt)
    info = np.iinfo(dt)
    return np.array([info.min, info.max, 0, 1], dt)


def neighbours(picks):
    if picks.dtype.kind == "f":
        return np.nextafter(picks, picks.dtype.type(-np.inf)), np.nextafter(picks, picks.dtype.type(np.inf))
    return picks - picks.dtype.type(1), picks + picks.dtype.type(1)


def owners(needle_starts, n):
    """the segment of every needle under ascending needle_starts, -1 for none"""
    return np.searchsorted(needle_starts, np.arange(n, dtype=np.int64), side="right").astype(np.int64) - 1


def needles_for(table, table_starts, seg, seed):
    """random over 1.25 x the table's range; every 5th needle a copy of an entry of ITS segment or that entry's neighbour below or
    above; the extremes (NaN among them) in front, and for floats a NaN every 97 needles"""
    rng = np.random.default_rng(seed)
    dt, n = table.dtype, seg.size
    lo, hi = bounds(table_starts, table.size)
    if table.size == 0:
        v = np.zeros(n, dt)
    elif dt.kind == "f":
        a, b = float(table.min()), float(table.max())
        span = max(b - a, 8.0)
        v = rng.uniform(a - 0.125 * span, b + 0.125 * span, n).astype(dt)
    else:
        a, b = int(table.min()), int(table.max())
        span = max(b - a, 8)
        v = rng.integers(a - span // 8, b + span // 8, n, dtype=dt, endpoint=True)
    e = np.arange(0, n, 5)
    j = seg[e]
    e, j = e[j >= 0], j[j >= 0]
    length = (hi - lo)[j]
    e, j, length = e[length > 0], j[length > 0], length[length > 0]
    if e.size:
        picks = table[lo[j] + (rng.integers(0, 1 << 30, e.size) % length)]
        below, above = neighbours(picks)
        v[e] = np.choose(rng.integers(0, 3, e.size), [picks, below, above])
    if dt.kind == "f":
        v[7::97] = np.nan
    ext = extremes(dt)
    k = min(ext.size, n)
    v[:k] = ext[:k]
    return v


def reference(table, table_starts, needles, seg, right, flat):
    """numpy.searchsorted per segment; seg: the segment of every needle, -1 for none"""
    lo, hi = bounds(table_starts, table.size)
    out = np.zeros(needles.size, np.int64)
    order = np.argsort(seg, kind="stable")
    cut = np.searchsorted(seg[order], np.arange(table_starts.size + 1))
    side = "right" if right else "left"
    for j in np.flatnonzero(np.diff(cut)):
        idx = order[cut[j]:cut[j + 1]]
        out[idx] = np.searchsorted(table[lo[j]:hi[j]], needles[idx], side)
    if needles.dtype.kind == "f":
        out[np.isnan(needles)] = 0
    if flat:
        out = out + np.where(seg >= 0, lo[np.maximum(seg, 0)] if lo.size else 0, 0)
    return out.astype(np.uint32)


def case_from(dt, lengths, counts, seed, gap=0):
    """(table, table_starts, needles, needle_starts, seg): segment j has lengths[j] entries and counts[j] needles; `gap` needles in
    front belong to no segment"""
    table_starts, nt = starts_of(lengths)
    needle_starts, n = starts_of(counts, gap)
    table = ragged_table(dt, lengths, seed)
    seg = owners(needle_starts, n)
    return table, table_starts, needles_for(table, table_starts, seg, seed + 1), needle_starts, seg


class Device:
    """the buffers of one case, uploaded once"""
    def __init__(self, capi, table, table_starts, needles, needle_starts=None, rows=None):
        self.capi = capi
        self.table, self.tstarts, self.needles = (capi.Buf.from_numpy(a) for a in (table, table_starts.astype(np.uint32), needles))
        self.nstarts = capi.Buf.from_numpy(needle_starts.astype(np.uint32)) if needle_starts is not None else None
        self.rows = capi.Buf.from_numpy(rows.astype(np.uint32)) if rows is not None else None

    def run(self, right=False, flat=False):
        return self.capi.search_sorted_segments(self.table, self.tstarts, self.needles, self.nstarts, self.rows, right, flat).numpy()


def check_case(capi, case, label=""):
    table, table_starts, needles, needle_starts, seg = case
    dev = Device(capi, table, table_starts, needles, needle_starts)
    for right, flat in FLAGS:
        got = dev.run(right, flat)
        want = reference(table, table_starts, needles, seg, right, flat)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (label, name(table.dtype), right, flat, bad.size, bad[:5], got[bad[:5]], want[bad[:5]], seg[bad[:5]])


# ---- 1. length mixes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_length_mixes(capi, dt):
    rng = np.random.default_rng(3)
    lengths, counts = rng.choice(TABLE_LENGTHS, 400), rng.choice(NEEDLE_COUNTS, 400)
    case = case_from(dt, lengths, counts, 5, gap=3)
    assert case[3][0] > 0 and case[2].size > 6 * tile_of(capi, dt)
    check_case(capi, case, "mix")
    # ... and a few needles only, the last segments without any
    check_case(capi, case_from(dt, [3, 0, 64, 1000, 5], [1, 5, 5, 0, 0], 7, gap=1), "few")


# ---- 2. a segment that LDS cannot take, and one it just can, between short ones inside one tile of needles ----------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_long_segment_between_short_ones(capi, dt):
    _, tile, _, _, L, _ = plan(capi, dt, 1, 1, 1)
    for lengths, counts in (([5, 64, L + 1, 3, 64], [10, 50, 300, 10, 50]), ([L, 3, 64], [300, 10, 50]), ([5, L, 3], [10, 300, 10]),
                            ([L + 1], [100]), ([L - 64, 64, 1], [200, 50, 7])):
        assert sum(counts) < tile
        check_case(capi, case_from(dt, lengths, counts, 11), str(lengths))


# ---- 3. more starts than one window inside one tile ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int64], ids=name)
def test_more_starts_than_one_window(capi, dt):
    _, tile, _, _, _, W = plan(capi, dt, 1, 1, 1)
    m = W + 1
    # one needle per segment; as many segments again behind, so that the tile after the full window starts somewhere inside
    check_case(capi, case_from(dt, np.arange(2 * m) % 4 + 1, np.ones(2 * m, np.int64), 13, gap=5), "one needle each")
    # W + 1 segments without entries and without needles in front of a populated one, in the middle of a tile
    lengths = [40] + [0] * m + [100, 7]
    counts = [300] + [0] * m + [500, 2 * tile]
    check_case(capi, case_from(dt, lengths, counts, 17), "empty segments")
    # ... and such segments WITH entries (nobody searches them; the span in front of the populated one is longer than LDS takes)
    check_case(capi, case_from(dt, [40] + [30] * m + [100, 7], counts, 19), "idle segments")


# ---- 4. tile seams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_tile_seams(capi, dt):
    tile = tile_of(capi, dt)
    # a segment's needles straddle a boundary (and one segment covers three tiles)
    check_case(capi, case_from(dt, [64, 65, 1000, 3, 64], [tile - 10, 30, 3 * tile + 5, tile - 25, 9], 23), "straddle")
    # a needle segment begins exactly at a boundary; so does the first one
    case = case_from(dt, [63, 64, 0, 65, 1000], [tile, 100, 0, tile - 100, 2 * tile], 29)
    assert case[3][0] == 0 and case[3][1] == tile and case[3][4] == 2 * tile
    check_case(capi, case, "exact")


# ---- 5. several tiles per workgroup, one tile more than a full grid ---------------------------------------------------------------
def test_several_tiles_per_workgroup(capi):
    dt = np.float32
    rng = np.random.default_rng(31)
    tile = tile_of(capi, dt)
    cap, above = 1, 1 << 20                                         # the most workgroups: the most tiles that get one each
    while above - cap > 1:
        mid = (cap + above) // 2
        cap, above = (mid, above) if plan(capi, dt, 1, 1, mid * tile)[2] == 1 else (cap, mid)
    assert plan(capi, dt, 1, 1, cap * tile)[2:4] == (1, cap) and cap >= cu_count()
    for n_goal, per in ((cap * tile + tile // 2, 2), (2 * cap * tile + 7, 3)):
        m = n_goal // 125                                          # (the last segment takes the needles that are left)
        counts = rng.integers(0, 241, m)
        counts[-1] += n_goal - 3 - counts.sum()
        lengths = rng.choice(TABLE_LENGTHS + [200, 300], m)
        case = case_from(dt, lengths, counts, 37, gap=3)
        got = plan(capi, dt, case[0].size, m, case[2].size)
        assert case[2].size == n_goal and got[2] == per and got[3] * per * tile >= n_goal, got
        dev = Device(capi, *case[:4])
        for right, flat in ((False, True), (True, False)):
            assert np.array_equal(dev.run(right, flat), reference(case[0], case[1], case[2], case[4], right, flat)), (n_goal, right, flat)


# ---- 6. misaligned views ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_misaligned_views(capi, dt):
    rng = np.random.default_rng(41)
    tile = tile_of(capi, dt)
    lengths, counts = rng.choice(TABLE_LENGTHS, 60), rng.choice(NEEDLE_COUNTS, 60)
    counts[10] = tile + 13
    table, table_starts, needles, needle_starts, seg = case_from(dt, lengths, counts, 43, gap=2)
    n, pad, mark = needles.size, 64, np.uint32(0xDEADBEEF)
    rows = np.maximum(seg, 0).astype(np.uint32)
    for o_out, o_needles, o_table, o_ts, o_ns in ((1, 2, 3, 1, 2), (3, 1, 1, 2, 3), (2, 3, 2, 3, 1), (0, 1, 0, 0, 0), (3, 0, 0, 1, 0)):
        def shifted(a, off):
            buf = capi.Buf.from_numpy(np.concatenate([np.zeros(4 + off, a.dtype), a]))       # 16-byte aligned + off elements
            return buf, buf.view(4 + off, a.size)
        out = capi.Buf.from_numpy(np.full(n + 2 * pad, mark, np.uint32))
        keep = [shifted(a, off) for a, off in ((needles, o_needles), (table, o_table), (table_starts, o_ts), (needle_starts, o_ns), (rows, o_ns))]
        vn, vt, vts, vns, vr = (v for _, v in keep)
        for right, flat in FLAGS:
            for indexed in (False, True):
                capi.search_sorted_segments(vt, vts, vn, None if indexed else vns, vr if indexed else None, right, flat,
                                            out=out.view(pad + o_out, n))
                got = out.numpy()
                assert np.all(got[:pad + o_out] == mark) and np.all(got[pad + o_out + n:] == mark), "written outside out"
                want = reference(table, table_starts, needles, np.where(indexed, np.maximum(seg, 0), seg), right, flat)
                assert np.array_equal(got[pad + o_out:pad + o_out + n], want), (name(dt), o_out, right, flat, indexed)


# ---- 7. a row per needle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_rows_mode(capi, dt):
    rng = np.random.default_rng(47)
    bound = plan(capi, dt, 1, 1, 1, True)[4]
    for nt, route in ((bound - 1, 2), (bound, 2), (bound + 1, 3)):
        m = 37
        cuts = np.sort(rng.integers(0, nt + 1, m - 1))
        lengths = np.diff(np.concatenate([[0], cuts, [nt]]))
        lengths[5] += lengths[6]; lengths[6] = 0                               # an empty segment
        n = 5003
        assert plan(capi, dt, nt, m, n, True)[0] == route
        table_starts, _ = starts_of(lengths)
        table = ragged_table(dt, lengths, 53)
        rows = rng.integers(0, m + 6, n).astype(np.uint32)                      # random order; rows >= m are clamped
        rows[:3] = [0xFFFFFFFF, m, m - 1]
        seg = np.minimum(rows.astype(np.int64), m - 1)
        needles = needles_for(table, table_starts, seg, 59)
        dev = Device(capi, table, table_starts, needles, rows=rows)
        for right, flat in FLAGS:
            assert np.array_equal(dev.run(right, flat), reference(table, table_starts, needles, seg, right, flat)), (name(dt), nt, right, flat)


# ---- 8. cross-checks, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_against_the_block_and_whole_table_searches(capi, dt):
    rng = np.random.default_rng(61)
    for R, B, M in ((300, 64, 70), (7, 1000, 513), (1, 5000, 3000)):
        lengths = np.full(R, B)
        table = ragged_table(dt, lengths, 67)
        table_starts = (np.arange(R) * B).astype(np.uint32)
        needle_starts = (np.arange(R) * M).astype(np.uint32)
        seg = owners(needle_starts, R * M)
        needles = needles_for(table, table_starts, seg, 71)
        rows = rng.integers(0, R + 3, R * M).astype(np.uint32)
        dev, devr = Device(capi, table, table_starts, needles, needle_starts), Device(capi, table, table_starts, needles, rows=rows)
        lo = np.minimum(rows, R - 1) * np.uint32(B)
        for right in (False, True):
            blocks = capi.search_sorted_blocks(dev.table, dev.needles, B, right).numpy()
            mine = dev.run(right)
            assert np.array_equal(mine, blocks), (name(dt), R, B, right)
            assert np.array_equal(dev.run(right, True), mine + (seg * B).astype(np.uint32))
            blocks = capi.search_sorted_blocks(dev.table, dev.needles, B, right, rows=devr.rows).numpy()
            assert np.array_equal(devr.run(right), blocks)
            assert np.array_equal(devr.run(right, True), blocks + lo)
            if R == 1:
                assert np.array_equal(mine, capi.search_sorted(dev.table, dev.needles, right).numpy())


# ---- 9. run-to-run identity ----------------------------------------------------------------------------------------------------------------
def test_run_to_run_identity(capi):
    rng = np.random.default_rng(73)
    _, tile, _, _, L, W = plan(capi, np.float32, 1, 1, 1)
    for lengths, counts in ((rng.choice(TABLE_LENGTHS, 500), rng.choice(NEEDLE_COUNTS, 500)), ([5, L + 1, 9], [tile, tile, 5]),
                            ([2] * (W + 9), [1] * (W + 9))):
        case = case_from(np.float32, lengths, counts, 79, gap=1)
        dev = Device(capi, *case[:4])
        for right, flat in FLAGS:
            runs = [dev.run(right, flat) for _ in range(3)]
            assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ---- 10. inside a step graph, replayed after the CONTENTS of both starts arrays changed -------------------------------------------------------
def test_inside_a_step_graph(capi):
    lib = capi.lib
    rng = np.random.default_rng(83)
    m, nt, n = 200, 30000, 3 * tile_of(capi, np.float32) + 77

    def host():
        cuts = np.sort(rng.integers(0, nt + 1, m - 1))
        lengths = np.diff(np.concatenate([[0], cuts, [nt]]))
        counts = np.diff(np.concatenate([[0], np.sort(rng.integers(0, n - 4, m - 1)), [n - 5]]))
        return case_from(np.float32, lengths, counts, int(rng.integers(1 << 30)), gap=5)
    h1, h2 = host(), host()
    assert all(h[0].size == nt and h[2].size == n for h in (h1, h2)) and not np.array_equal(h1[1], h2[1]) and not np.array_equal(h1[3], h2[3])
    dev = Device(capi, *h1[:4])
    modes = [(False, False), (True, True)]
    capi.check(lib.ek_hip_graph_begin())
    try:
        held = [dev.capi.search_sorted_segments(dev.table, dev.tstarts, dev.needles, dev.nstarts, None, *mode) for mode in modes]
    finally:
        g = ctypes.c_void_p()
        capi.check(lib.ek_hip_graph_end(ctypes.byref(g)))
    try:
        for h in (h1, h2, h1):
            for buf, a in zip((dev.table, dev.tstarts, dev.needles, dev.nstarts), h[:4]):
                capi.check(lib.ek_hip_memcpy_to_device(ctypes.c_void_p(buf.ptr), a.ctypes.data_as(ctypes.c_void_p), SZ(a.nbytes)))
            capi.check(lib.ek_hip_graph_launch(g))
            for b, mode in zip(held, modes):
                want = reference(h[0], h[1], h[2], h[4], *mode)
                assert np.array_equal(b.numpy(), want) and np.array_equal(dev.run(*mode), want)
    finally:
        capi.check(lib.ek_hip_graph_destroy(g))


# ---- 11. arguments ------------------------------------------------------------------------------------------------------------------------------
def test_arguments(capi):
    lib = capi.lib
    table = capi.Buf.from_numpy(np.array([1, 2, 3, 10, 20, 5, 6, 7, 8], np.float32))
    ts = capi.Buf.from_numpy(np.array([0, 3, 5], np.uint32))
    needles = capi.Buf.from_numpy(np.array([2.5, 0, 15, 99, 6, 6], np.float32))
    ns = capi.Buf.from_numpy(np.array([0, 2, 4], np.uint32))
    rows = capi.Buf.from_numpy(np.array([0, 0, 1, 1, 2, 9], np.uint32))
    out = capi.Buf.from_numpy(np.full(6, 77, np.uint32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    f = lib.ek_hip_search_sorted_segments
    call = lambda **kw: f(*[{**dict(type=capi.F32, out=p(out), table=p(table), nt=SZ(9), ts=p(ts), m=SZ(3), needles=p(needles), n=SZ(6),
                                     ns=p(ns), rows=None, flags=0), **kw}[k]
                            for k in ("type", "out", "table", "nt", "ts", "m", "needles", "n", "ns", "rows", "flags")])
    lib.ek_hip_sync()
    l0 = lib.ek_hip_launch_count()
    assert call(rows=p(rows)) == -1 and b"ek_hip_search_sorted_segments" in lib.ek_hip_last_error()       # both owners
    assert call(ns=None) == -1                                                                            # neither
    assert call(flags=4) == -1 and call(flags=-1) == -1
    assert call(out=None) == -1 and call(table=None) == -1 and call(ts=None) == -1 and call(needles=None) == -1
    assert call(out=ctypes.c_void_p(out.ptr + 2)) == -1 and call(needles=ctypes.c_void_p(needles.ptr + 1)) == -1
    assert call(ts=ctypes.c_void_p(ts.ptr + 2), m=SZ(2)) == -1 and call(ns=ctypes.c_void_p(ns.ptr + 1)) == -1
    assert call(type=capi.BOOL) == -2 and call(type=99) == -2
    assert call(nt=SZ(1 << 32)) == -2 and b"2^32" in lib.ek_hip_last_error()
    assert call(m=SZ(1 << 32)) == -2 and call(n=SZ(1 << 32)) == -2
    assert call(ns=None, rows=p(rows), m=SZ(0), ts=None) == -1                                            # rows and no segment
    assert call(n=SZ(0)) == 0 and call(n=SZ(0), out=None, needles=None, ns=None, rows=p(rows)) == 0       # no needle: nothing to do
    assert lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), np.full(6, 77, np.uint32))
    with pytest.raises(ValueError):
        capi.search_sorted_segments(table, ts, needles)
    with pytest.raises(ValueError):
        capi.search_sorted_segments(table, ts, needles, ns, rows)
    # the calls after refused ones work
    assert call() == 0 and np.array_equal(out.numpy(), [2, 0, 1, 2, 1, 1])
    assert call(flags=3) == 0 and np.array_equal(out.numpy(), [2, 0, 4, 5, 7, 7])
    assert call(ns=None, rows=p(rows), flags=1) == 0 and np.array_equal(out.numpy(), [2, 0, 1, 2, 2, 2])
    # empty sizes: no table entries and no segments give zeros
    assert call(nt=SZ(0), table=None, flags=3) == 0 and np.array_equal(out.numpy(), np.zeros(6, np.uint32))
    out2 = capi.Buf.from_numpy(np.full(6, 77, np.uint32))
    assert call(out=p(out2), m=SZ(0), ts=None, ns=None, flags=2) == 0 and np.array_equal(out2.numpy(), np.zeros(6, np.uint32))
    empty = capi.Buf(np.uint32, 0)
    assert capi.search_sorted_segments(table, empty, needles, empty).numpy().tolist() == [0] * 6
    assert capi.search_sorted_segments(table, ts, capi.Buf(np.float32, 0), ns).n == 0


# ---- 12. bad index arrays: inside the test's own memory, every result in its documented range -----------------------------------------------------
def guarded_run(capi, table, table_starts, needles, needle_starts, rows, right, flat, pad=256):
    """table, needles and out are views into larger buffers with `pad` sentinel entries on both sides"""
    dt = table.dtype
    poison = dt.type(1e30) if dt.kind == "f" else dt.type(0x5A5A5A5A)
    mark = np.uint32(0xDEADBEEF)
    assert int(table_starts.max()) <= table.size + pad                                   # no bad value leaves the enclosing allocation
    assert needle_starts is None or int(needle_starts.max()) <= needles.size + pad
    wrap = lambda a: np.concatenate([np.full(pad, poison, dt), a, np.full(pad, poison, dt)])
    src, ndl = capi.Buf.from_numpy(wrap(table)), capi.Buf.from_numpy(wrap(needles))
    out = capi.Buf.from_numpy(np.full(needles.size + 2 * pad, mark, np.uint32))
    ts = capi.Buf.from_numpy(table_starts.astype(np.uint32))
    ns = capi.Buf.from_numpy(needle_starts.astype(np.uint32)) if needle_starts is not None else None
    rw = capi.Buf.from_numpy(rows.astype(np.uint32)) if rows is not None else None
    capi.search_sorted_segments(src.view(pad, table.size), ts, ndl.view(pad, needles.size), ns, rw, right, flat, out=out.view(pad, needles.size))
    got = out.numpy()
    assert np.all(got[:pad] == mark) and np.all(got[pad + needles.size:] == mark), "written outside out"
    assert np.array_equal(src.numpy(), wrap(table)), "the table changed"
    return got[pad:pad + needles.size]


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_starts_above_the_arrays_are_clamped(capi, dt):
    tile = tile_of(capi, dt)
    lengths, counts = [5, 0, 700, 64, 1, 2000], [9, 3, tile + 50, 0, 300, 64]
    table, table_starts, needles, needle_starts, seg = case_from(dt, lengths, counts, 89, gap=2)
    nt, n = table.size, needles.size
    # the last few starts lie behind the end of their array: at it, just above it, and up to the end of the enclosing buffer
    ts = np.concatenate([table_starts, np.array([nt, nt + 1, nt + 7, nt + 200, nt + 256], np.uint32)])
    ns = np.concatenate([needle_starts, np.array([n, n, n + 1, n + 100, n + 256], np.uint32)])
    ts[3] = nt + 100                                                            # and one in the middle: segment 2 runs to the end
    lo, hi = bounds(ts, nt)
    assert hi[2] == nt and lo[3] == nt
    for right, flat in FLAGS:
        got = guarded_run(capi, table, ts, needles, ns, None, right, flat)
        if not flat:
            assert np.all(got <= np.where(seg >= 0, (hi - lo)[np.maximum(seg, 0)], 0)), (name(dt), right)
        assert np.all(got <= nt)
        # every segment but the one that now runs over unsorted entries has its exact result
        ok = seg != 2
        assert np.array_equal(got[ok], reference(table, ts, needles, seg, right, flat)[ok]), (name(dt), right, flat)
    # every start above its array: no needle has a segment
    for right, flat in FLAGS:
        got = guarded_run(capi, table, np.full(4, nt + 9, np.uint32), needles, np.array([n, n + 1, n + 2, n + 256], np.uint32), None, right, flat)
        assert np.array_equal(got, np.zeros(n, np.uint32))


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_decreasing_starts_and_unsorted_segments_stay_inside(capi, dt):
    rng = np.random.default_rng(97)
    _, tile, _, _, L, W = plan(capi, dt, 1, 1, 1)
    for nt, n, m in ((5000, 3000, 40), (5000, 5 * tile + 9, 3), (3 * L + 5, 4 * tile, 2 * W + 100), (60000, 2 * tile + 1, 700)):
        table = rng.integers(-1000, 1000, nt).astype(dt)                        # no order at all inside any segment
        needles = rng.integers(-1200, 1200, n).astype(dt)
        rows = rng.integers(0, m + 100, n).astype(np.uint32)
        cases = [(rng.integers(0, nt + 256, m), rng.integers(0, n + 256, m))]   # no order at all
        s, t = np.sort(rng.integers(0, nt, m)), np.sort(rng.integers(0, n, m))
        cases.append((s[::-1].copy(), t[::-1].copy()))                          # strictly the wrong way round
        cases.append((s, t[::-1].copy()))
        s2, t2 = s.copy(), t.copy()
        s2[m // 2], t2[m // 3] = nt + 200, n + 200                              # one value out of line
        cases.append((s2, t2))
        cases.append((s, t))                                                    # good starts, unsorted entries
        for k, (ts, ns) in enumerate(cases):
            lo, hi = bounds(ts, nt)
            longest = int((hi - lo).max())
            for right, flat in ((False, False), (True, True)):
                got = guarded_run(capi, table, ts, needles, ns, None, right, flat)
                assert np.all(got <= (nt if flat else longest)), (name(dt), nt, n, m, k, right, flat)
                if k == 4:                                                      # the assignment is known: the needle's own segment
                    seg = owners(ns.astype(np.uint32), n)
                    own = np.where(seg >= 0, (hi - lo)[np.maximum(seg, 0)], 0)
                    base = np.where(seg >= 0, lo[np.maximum(seg, 0)], 0) if flat else 0
                    assert np.all(got.astype(np.int64) - base >= 0) and np.all(got.astype(np.int64) - base <= own)
                got = guarded_run(capi, table, ts, needles, None, rows, right, flat)
                seg = np.minimum(rows.astype(np.int64), m - 1)
                base = lo[seg] if flat else 0
                assert np.all(got.astype(np.int64) - base >= 0) and np.all(got.astype(np.int64) - base <= (hi - lo)[seg])
