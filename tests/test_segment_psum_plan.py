"""ek_hip_psum_segments_plan, the host-only report of what ek_hip_psum_segments does (csrc/segment_scan.hip), no GPU needed.

The header comment of segment_scan.hip says: ONE route.  tile = 16 KiB / sizeof(T) consecutive output entries,
tiles = ceil(n / tile), tiles_per_workgroup = ceil(tiles / min(tiles, 4 x #CU)), workgroups = ceil(tiles / tiles_per_workgroup),
launches = 1 for one workgroup and 3 otherwise; the last three are 0 for n == 0 or m == 0.  The rule is restated here in python; the
plan depends on nothing but its arguments (not on m beyond m == 0, not on anything a device could tell)."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
SZ = ctypes.c_size_t
TILE_BYTES, PER_CU = 16 * 1024, 4


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


def name(dt):
    return np.dtype(dt).name


def rule(dt, n, m, cu=0):
    """(tile, tiles_per_workgroup, workgroups, launches) as the header comment of segment_scan.hip states it"""
    tile = TILE_BYTES // np.dtype(dt).itemsize
    if n == 0 or m == 0:
        return tile, 0, 0, 0
    tiles = -(-n // tile)
    cap = min(tiles, (cu or 256) * PER_CU)
    per = -(-tiles // cap)
    workgroups = -(-tiles // per)
    return tile, per, workgroups, 1 if workgroups == 1 else 3


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_the_plan_at_its_edges(capi, dt):
    plan = lambda n, m, cu=0: capi.psum_segments_plan(dt, n, m, cu)
    tile = TILE_BYTES // np.dtype(dt).itemsize
    assert plan(0, 0) == (tile, 0, 0, 0) and plan(0, 5) == (tile, 0, 0, 0) and plan(100, 0) == (tile, 0, 0, 0)
    for m in (1, 2, 1000):
        # one tile, one workgroup, one launch up to `tile` entries; two of each (three launches) from tile + 1 on
        for n in (1, tile - 1, tile):
            assert plan(n, m) == (tile, 1, 1, 1), (n, m)
        assert plan(tile + 1, m) == (tile, 1, 2, 3)
        for cu in (0, 1, 64, 256, 304):
            cap = (cu or 256) * PER_CU
            # up to the grid cap every workgroup owns one tile; one tile more and every workgroup owns two
            assert plan(cap * tile, m, cu) == (tile, 1, cap, 3 if cap > 1 else 1)
            assert plan(cap * tile + 1, m, cu) == (tile, 2, -(-(cap + 1) // 2), 3)
            assert plan(2 * cap * tile + 1, m, cu) == (tile, 3, -(-(2 * cap + 1) // 3), 3)
    # every shape of a grid of (n, m, cu) against the rule
    top = (1 << 32) - 1
    for n in (0, 1, 2, tile - 1, tile, tile + 1, 3 * tile, 1000 * tile - 1, 1024 * tile, 1024 * tile + 1, 1 << 26, (1 << 26) + 5, top):
        for m in (0, 1, 7, 1 << 20, top):
            for cu in (0, 1, 64, 256, 304):
                got = plan(n, m, cu)
                assert got == rule(dt, n, m, cu), (name(dt), n, m, cu)
                if n and m:
                    _, per, workgroups, _ = got
                    tiles = -(-n // tile)
                    assert 1 <= workgroups <= (cu or 256) * PER_CU and (workgroups - 1) * per < tiles <= workgroups * per


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_plan_depends_on_its_arguments_alone(capi, dt):
    shapes = [(1000, 10, 0), (1 << 20, 3, 256), (1 << 26, 1000, 64), (0, 5, 0), (77, 0, 0)]
    first = [capi.psum_segments_plan(dt, *s) for s in shapes]
    for _ in range(3):
        assert [capi.psum_segments_plan(dt, *s) for s in reversed(shapes)][::-1] == first
    for n in (5000, 1 << 20, 1 << 26):
        # compute_units == 0 means 256; the number of segments does not enter beyond m == 0; types of a size share their plan
        assert capi.psum_segments_plan(dt, n, 3, 0) == capi.psum_segments_plan(dt, n, 3, 256)
        assert len({capi.psum_segments_plan(dt, n, m, 64) for m in (1, 2, 1000, 1 << 30)}) == 1
        same = {4: [np.float32, np.int32, np.uint32], 8: [np.float64, np.int64, np.uint64]}[np.dtype(dt).itemsize]
        assert len({capi.psum_segments_plan(t, n, 9, 0) for t in same}) == 1


def test_refusals(capi):
    lib = capi.lib
    t, p, w, l = SZ(), SZ(), SZ(), ctypes.c_int()
    out = (ctypes.byref(t), ctypes.byref(p), ctypes.byref(w), ctypes.byref(l))
    f = lib.ek_hip_psum_segments_plan
    assert f(capi.F32, SZ(100), SZ(10), 0, *out) == 0
    assert f(capi.BOOL, SZ(100), SZ(10), 0, *out) == -2 and f(99, SZ(100), SZ(10), 0, *out) == -2
    assert f(capi.F32, SZ(1 << 32), SZ(10), 0, *out) == -2 and f(capi.F32, SZ(100), SZ(1 << 32), 0, *out) == -2
    assert b"2^32" in lib.ek_hip_last_error() and b"ek_hip_psum_segments_plan" in lib.ek_hip_last_error()
    assert f(capi.F32, SZ((1 << 32) - 1), SZ((1 << 32) - 1), 0, *out) == 0
    assert f(capi.F32, SZ(100), SZ(10), -1, *out) == -1
    # any of the outputs may be left out
    assert f(capi.F32, SZ(100), SZ(10), 0, None, None, None, None) == 0
