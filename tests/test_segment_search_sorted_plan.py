"""ek_hip_search_sorted_segments_plan, the host-only report of what ek_hip_search_sorted_segments does (csrc/segment_search.hip), no
GPU needed.

The header comment of segment_search.hip says: with needle_starts route 1 (paired tiles) whatever the sizes; with a row per needle
route 2 while the whole table fits 64 KiB of LDS and route 3 above.  A tile is 512 lanes x 4 needles; tiles = ceil(n / tile),
tiles_per_workgroup = ceil(tiles / min(tiles, 2 x #CU)), workgroups = ceil(tiles / tiles_per_workgroup).  lds_entries is what one
tile can stage of its segments' entries (48 KiB - 256 B, the rest of the 64 KiB holds the window of starts) or the whole-table
bound of route 2; window is the starts one tile can stage: a tile of one-needle segments, the start in front and the one behind.
The plan depends on nothing but its arguments, never on what a starts array holds."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
TILE, PER_CU, LDS_BYTES, SPAN_BYTES = 512 * 4, 2, 64 * 1024, 48 * 1024 - 256
TOP = (1 << 32) - 1


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


def name(dt):
    return np.dtype(dt).name


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_routes_and_their_boundary(capi, dt):
    size = np.dtype(dt).itemsize
    plan = lambda nt, m, n, indexed, cu=0: capi.search_sorted_segments_plan(dt, nt, m, n, indexed, cu)
    span, whole = plan(1, 1, 1, False)[4], plan(1, 1, 1, True)[4]
    assert span == SPAN_BYTES // size and whole == LDS_BYTES // size
    # needle_starts: one route whatever the table is; the staged span and the window fit the LDS next to each other
    for nt in (0, 1, span - 1, span, span + 1, whole, whole + 1, 1 << 26, TOP):
        for m in (0, 1, 1000, TOP):
            route, tile, per, workgroups, lds, window = plan(nt, m, 5000, False)
            assert (route, tile, lds) == (1, TILE, span) and window >= TILE + 2 and per >= 1 and workgroups >= 1
            assert lds * size + (2 * window + 1) * 4 <= LDS_BYTES
    # rows: the boundary between the staged and the global route is exactly at lds_entries
    for m in (1, 7, 1 << 20):
        for n in (1, 5000, 1 << 26):
            assert [plan(nt, m, n, True)[0] for nt in (0, 1, whole - 1, whole, whole + 1, 2 * whole, TOP)] == [2, 2, 2, 2, 3, 3, 3]
            assert plan(whole, m, n, True)[4:] == (whole, 0) and plan(whole + 1, m, n, True)[4:] == (whole, 0)
    # no needles: no route, no workgroups
    for indexed in (False, True):
        assert plan(100, 5, 0, indexed)[:4] == (0, TILE, 0, 0)
    assert capi.SEGMENT_SEARCH_ROUTES[plan(10, 1, 1, False)[0]] == "paired-tiles"
    assert capi.SEGMENT_SEARCH_ROUTES[plan(10, 1, 1, True)[0]] == "indexed-lds"


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_the_grid_covers_the_needles(capi, dt):
    for indexed in (False, True):
        for cu in (0, 1, 64, 256, 304):
            cap = (cu or 256) * PER_CU
            for n in (1, 2, TILE - 1, TILE, TILE + 1, cap * TILE, cap * TILE + 1, 2 * cap * TILE + 1, (1 << 26) + 5, TOP):
                for nt, m in ((1000, 10), (1 << 24, 1 << 20), (0, 1)):
                    route, tile, per, workgroups, lds, window = capi.search_sorted_segments_plan(dt, nt, m, n, indexed, cu)
                    tiles = -(-n // tile)
                    assert route > 0 and tile > 0 and per > 0 and workgroups > 0 and lds > 0
                    assert (window > 0) == (not indexed)
                    assert 1 <= workgroups <= cap and (workgroups - 1) * per < tiles <= workgroups * per
                    assert workgroups * per * tile >= n
                    assert per == -(-tiles // min(tiles, cap))
    # one tile more than a full grid: every workgroup owns two
    assert capi.search_sorted_segments_plan(dt, 10, 1, 512 * TILE, False, 256)[2:4] == (1, 512)
    assert capi.search_sorted_segments_plan(dt, 10, 1, 512 * TILE + 1, False, 256)[2:4] == (2, 257)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_plan_depends_on_its_arguments_alone(capi, dt):
    shapes = [(1000, 10, 500, False, 0), (1 << 20, 3, 1 << 22, False, 256), (1 << 26, 1000, 77, True, 64), (0, 5, 9, True, 0), (77, 0, 3, False, 0)]
    first = [capi.search_sorted_segments_plan(dt, *s) for s in shapes]
    for _ in range(3):
        assert [capi.search_sorted_segments_plan(dt, *s) for s in reversed(shapes)][::-1] == first
    for n in (5000, 1 << 20, 1 << 26):
        assert capi.search_sorted_segments_plan(dt, 999, 3, n, False, 0) == capi.search_sorted_segments_plan(dt, 999, 3, n, False, 256)
        same = {4: [np.float32, np.int32, np.uint32], 8: [np.float64, np.int64, np.uint64]}[np.dtype(dt).itemsize]
        assert len({capi.search_sorted_segments_plan(t, 99999, 9, n, ix, 0) for t in same for ix in (True,)}) == 1


def test_refusals(capi):
    lib = capi.lib
    r = ctypes.c_int()
    v = [SZ() for _ in range(5)]
    out = [ctypes.byref(r)] + [ctypes.byref(x) for x in v]
    f = lib.ek_hip_search_sorted_segments_plan
    assert f(capi.F32, SZ(100), SZ(10), SZ(50), 0, 0, *out) == 0
    assert f(capi.BOOL, SZ(100), SZ(10), SZ(50), 0, 0, *out) == -2 and f(99, SZ(100), SZ(10), SZ(50), 0, 0, *out) == -2
    assert f(capi.F32, SZ(1 << 32), SZ(10), SZ(50), 0, 0, *out) == -2 and f(capi.F32, SZ(100), SZ(1 << 32), SZ(50), 0, 0, *out) == -2
    assert f(capi.F32, SZ(100), SZ(10), SZ(1 << 32), 1, 0, *out) == -2
    assert b"2^32" in lib.ek_hip_last_error() and b"ek_hip_search_sorted_segments_plan" in lib.ek_hip_last_error()
    assert f(capi.F32, SZ(TOP), SZ(TOP), SZ(TOP), 0, 0, *out) == 0
    assert f(capi.F32, SZ(100), SZ(10), SZ(50), 0, -1, *out) == -1
    # a row per needle and no segment to search; without needles there is nothing to refuse
    assert f(capi.F32, SZ(100), SZ(0), SZ(50), 1, 0, *out) == -1 and f(capi.F32, SZ(100), SZ(0), SZ(0), 1, 0, *out) == 0
    assert f(capi.F32, SZ(100), SZ(0), SZ(50), 0, 0, *out) == 0
    # any of the outputs may be left out
    assert f(capi.F32, SZ(100), SZ(10), SZ(50), 0, 0, None, None, None, None, None, None) == 0
