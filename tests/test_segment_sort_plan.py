"""ek_hip_sort_segments_plan, the host-only report of what ek_hip_sort_segments does (csrc/segment_sort.hip), no GPU needed.

The header comment of segment_sort.hip says: ONE route.  tile = 2048 consecutive entries, tiles = ceil(n / tile),
tiles_per_workgroup = ceil(tiles / min(tiles, 8 x #CU)), workgroups = ceil(tiles / tiles_per_workgroup), merges = ceil(log2(tiles))
merge launches of `tiles` workgroups, launches = 1 for one tile and 2 + merges otherwise, scratch = one buffer of n composites
(8 bytes for 4-byte types, 12 for 8-byte types, rounded up to 16 bytes), two from two merges on, plus tiles + 1 words; everything
but the tile is 0 for n == 0 or m == 0.  The rule is restated here in python; the plan depends on nothing but its arguments."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
TILE, PER_CU = 2048, 8


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


def name(dt):
    return np.dtype(dt).name


def rule(dt, n, m, cu=0):
    """(tile, tiles, tiles_per_workgroup, workgroups, merges, merge_workgroups, launches, scratch_bytes)"""
    if n == 0 or m == 0:
        return (TILE, 0, 0, 0, 0, 0, 0, 0)
    tiles = -(-n // TILE)
    cap = min(tiles, (cu or 256) * PER_CU)
    per = -(-tiles // cap)
    workgroups = -(-tiles // per)
    merges = (tiles - 1).bit_length()
    if merges == 0:
        return (TILE, 1, 1, 1, 0, 0, 1, 0)
    buf = -(-n * (8 if np.dtype(dt).itemsize == 4 else 12) // 16) * 16
    return (TILE, tiles, per, workgroups, merges, tiles, 2 + merges, buf * (2 if merges > 1 else 1) + (tiles + 1) * 4)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_plan_numbers(capi, dt):
    plan = lambda n, m, cu=0: capi.sort_segments_plan(dt, n, m, True, cu)
    cb = 8 if np.dtype(dt).itemsize == 4 else 12
    # a handful by hand
    assert plan(5000, 70) == (TILE, 3, 1, 3, 2, 3, 4, 2 * 5000 * cb + 4 * 4)
    assert plan(TILE, 1) == (TILE, 1, 1, 1, 0, 0, 1, 0)
    assert plan(TILE + 1, 1) == (TILE, 2, 1, 2, 1, 2, 3, ((TILE + 1) * cb + 15) // 16 * 16 + 3 * 4)
    assert plan(4 * TILE, 9) == (TILE, 4, 1, 4, 2, 4, 4, 2 * 4 * TILE * cb + 5 * 4)
    assert plan(1 << 26, 1 << 20, 256) == (TILE, 1 << 15, 16, 2048, 15, 1 << 15, 17, 2 * (1 << 26) * cb + ((1 << 15) + 1) * 4)
    # zero launches for n == 0 (and for m == 0, which is a copy and a count)
    assert plan(0, 0) == plan(0, 5) == plan(100, 0) == (TILE, 0, 0, 0, 0, 0, 0, 0)
    top = (1 << 32) - 1
    for n in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE, 1000 * TILE - 1, 1024 * TILE, 1024 * TILE + 1, (1 << 26) + 5, top):
        for m in (1, 7, 1 << 20, top):
            for cu in (0, 1, 64, 256, 304):
                got = plan(n, m, cu)
                assert got == rule(dt, n, m, cu), (name(dt), n, m, cu)
                _, tiles, per, workgroups, merges, merge_wg, launches, scratch = got
                # merges == ceil(log2(tiles)); no merge launches and no scratch for one tile
                assert (1 << merges) >= tiles and (merges == 0 or (1 << (merges - 1)) < tiles)
                assert (merges == 0) == (tiles == 1) == (scratch == 0) == (launches == 1) == (merge_wg == 0)
                assert 1 <= workgroups <= (cu or 256) * PER_CU and (workgroups - 1) * per < tiles <= workgroups * per
                assert scratch <= 2 * (n * cb + 15) + (tiles + 1) * 4


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_plan_depends_on_its_arguments_alone(capi, dt):
    shapes = [(1000, 10, True, 0), (1 << 20, 3, False, 256), (1 << 26, 1000, True, 64), (0, 5, True, 0), (77, 0, False, 0)]
    first = [capi.sort_segments_plan(dt, *s) for s in shapes]
    for _ in range(3):
        assert [capi.sort_segments_plan(dt, *s) for s in reversed(shapes)][::-1] == first
    for n in (5000, 1 << 20, 1 << 26):
        # compute_units == 0 means 256; neither the number of segments (beyond m == 0) nor want_index enters; types of a size share a plan
        assert capi.sort_segments_plan(dt, n, 3, True, 0) == capi.sort_segments_plan(dt, n, 3, True, 256)
        assert len({capi.sort_segments_plan(dt, n, m, w, 64) for m in (1, 2, 1000, 1 << 30) for w in (False, True)}) == 1
        same = {4: [np.float32, np.int32, np.uint32], 8: [np.float64, np.int64, np.uint64]}[np.dtype(dt).itemsize]
        assert len({capi.sort_segments_plan(t, n, 9, True, 0) for t in same}) == 1


def test_refusals(capi):
    lib = capi.lib
    v = [SZ() for _ in range(6)]
    mg, l = ctypes.c_int(), ctypes.c_int()
    out = (ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]), ctypes.byref(v[3]), ctypes.byref(mg), ctypes.byref(v[4]),
           ctypes.byref(l), ctypes.byref(v[5]))
    f = lib.ek_hip_sort_segments_plan
    assert f(capi.F32, SZ(100), SZ(10), 1, 0, *out) == 0
    # bad type
    assert f(capi.BOOL, SZ(100), SZ(10), 1, 0, *out) == -2 and f(99, SZ(100), SZ(10), 1, 0, *out) == -2
    # bad shape: more than 2^32 - 1 entries or segments
    assert f(capi.F32, SZ(1 << 32), SZ(10), 1, 0, *out) == -2 and f(capi.F32, SZ(100), SZ(1 << 32), 1, 0, *out) == -2
    assert b"2^32" in lib.ek_hip_last_error() and b"ek_hip_sort_segments_plan" in lib.ek_hip_last_error()
    assert f(capi.F32, SZ((1 << 32) - 1), SZ((1 << 32) - 1), 1, 0, *out) == 0
    # a negative CU count
    assert f(capi.F32, SZ(100), SZ(10), 1, -1, *out) == -1
    # any of the outputs may be left out
    assert f(capi.F32, SZ(100), SZ(10), 0, 0, None, None, None, None, None, None, None, None) == 0
