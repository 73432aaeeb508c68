"""ek_hip_reduce_segments_plan, the host-only report of the route ek_hip_reduce_segments takes (csrc/block_segments.hip), no GPU
needed.

The header comment of block_segments.hip says: with mean = ceil(n / m), route 1 (grouped) while n <= 1024 m, with
G = 2^ceil(log2(clamp(mean, 1, 64))) lanes per segment and W segments per workgroup, W = the segments that fill a 16 KiB tile at
the mean length, rounded down to a multiple of the 256 / G groups, at least one round of groups and at most 2048; beyond, route 3
(split) for fewer than 2 x #CU segments whose mean is cut into at least two pieces by the rule of the block reductions (about
4 x #CU workgroups, pieces of at least 8192 entries, at most 1024 pieces, pieces a multiple of the vector width), and route 2 (one
workgroup per segment) otherwise.  The rule is restated here in python; the plan depends on nothing but its arguments."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
NOTHING, GROUPED, SEGMENT, SPLIT = range(4)
SZ = ctypes.c_size_t
MAX_GRID = 0x7FFFFFFF
PACKED_MAX, TILE_BYTES, MIN_PIECE, MAX_PIECES, PER_WORKGROUP_MAX = 1024, 16 * 1024, 8192, 1024, 2048


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


def name(dt):
    return np.dtype(dt).name


def rule(dt, n, m, cu=0):
    """(route, group_lanes, splits, workgroups) as the header comment of block_segments.hip states it"""
    elem = np.dtype(dt).itemsize
    cu = cu or 256
    if m == 0:
        return NOTHING, 0, 1, 0
    mean = -(-n // m)
    if n <= PACKED_MAX * m:
        G = 1
        while G < min(max(mean, 1), 64):
            G *= 2
        groups = 256 // G
        W = min(max((TILE_BYTES // elem) // max(mean, 1) // groups * groups, groups), PER_WORKGROUP_MAX)
        return GROUPED, G, 1, min(-(-m // W), MAX_GRID)
    splits = 1
    if m < 2 * cu:
        N = 16 // elem
        S = min(-(-4 * cu // m), mean // MIN_PIECE, MAX_PIECES)
        if S >= 2:
            P = -(-(-(-mean // S)) // N) * N
            count = -(-mean // P)
            if count >= 2:
                splits = count
    return (SPLIT if splits > 1 else SEGMENT), 0, splits, min(m * splits, MAX_GRID)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_the_three_routes_at_their_edges(capi, dt):
    plan = lambda n, m, cu=0: capi.reduce_segments_plan(dt, n, m, cu)
    assert sorted(capi.SEGMENT_ROUTES) == [NOTHING, GROUPED, SEGMENT, SPLIT]
    assert plan(0, 0) == (NOTHING, 0, 1, 0) and plan(100, 0) == (NOTHING, 0, 1, 0)
    for m in (1, 2, 3, 511, 512, 1000, 100003):
        # the grouped route ends where the mean passes 1024 entries
        assert plan(0, m)[0] == GROUPED and plan(m, m)[0] == GROUPED
        assert plan(1024 * m, m)[0] == GROUPED and plan(1024 * m + 1, m)[0] != GROUPED
        # the lanes per segment follow the mean: 1, 1, 2, 4, 4, .., 64 from a mean of 33 on
        for mean, G in ((0, 1), (1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 64), (1024, 64)):
            assert plan(mean * m, m)[:2] == (GROUPED, G), (m, mean)
        if m > 1:
            assert plan(2 * m + 1, m)[1] == 4 and plan(2 * m, m)[1] == 2          # (the mean is rounded up)
        # the split route: fewer than 2 x #CU segments of a mean of at least 16 Ki entries
        for cu in (0, 64, 256, 304):
            few = m < 2 * (cu or 256)
            assert plan(16384 * m, m, cu)[0] == (SPLIT if few else SEGMENT), (m, cu)
            assert plan(16383 * m, m, cu)[0] == SEGMENT and plan(1025 * m, m, cu)[0] == SEGMENT
    for cu in (64, 256, 304):
        assert plan((1 << 20) * (2 * cu - 1), 2 * cu - 1, cu)[0] == SPLIT and plan((1 << 20) * 2 * cu, 2 * cu, cu)[0] == SEGMENT
    # every shape of a grid of (n, m, cu) against the rule
    for m in (1, 2, 3, 7, 64, 511, 512, 513, 4099, 1 << 20):
        for mean in (0, 1, 2, 3, 7, 63, 64, 65, 1000, 1024, 1025, 5000, 16383, 16384, 16385, 100000, 1 << 20, 3 << 20):
            for extra in (0, 1, m - 1):
                n = mean * m + extra
                if n >= 1 << 32:
                    continue
                for cu in (0, 1, 64, 256, 304):
                    assert plan(n, m, cu) == rule(dt, n, m, cu), (name(dt), n, m, cu)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_grids_and_pieces(capi, dt):
    plan = lambda n, m, cu=0: capi.reduce_segments_plan(dt, n, m, cu)
    top = (1 << 32) - 1
    for n, m in ((top, top), (top, 1), (0, top), (top, 3), (top, 5000000), (top, top // 1024), (top, top // 1025)):
        route, G, splits, workgroups = plan(n, m)
        assert (route, G, splits, workgroups) == rule(dt, n, m) and 1 <= workgroups <= MAX_GRID
    # a split segment is cut into 2 .. 1024 pieces of at least 8192 entries at the mean, about 4 x #CU workgroups in all
    for cu in (64, 256):
        for m in (1, 2, 3, 100, 2 * cu - 1):
            for mean in (16384, 20000, 1 << 20, (1 << 22) + 1):
                route, _, splits, workgroups = plan(mean * m, m, cu)
                assert route == SPLIT and 2 <= splits <= MAX_PIECES and workgroups == m * splits
                assert -(-mean // splits) >= MIN_PIECE // 2 and workgroups <= 4 * cu + m + splits
    # a workgroup of the grouped route owns at most 2048 segments
    for m in (1, 2048, 2049, 1 << 20):
        assert plan(m, m)[3] == -(-m // 2048)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_plan_depends_on_its_arguments_alone(capi, dt):
    shapes = [(1000, 10, 0), (1 << 20, 3, 256), (1 << 20, 1000, 64), (0, 5, 0), (77, 0, 0)]
    first = [capi.reduce_segments_plan(dt, *s) for s in shapes]
    for _ in range(3):
        assert [capi.reduce_segments_plan(dt, *s) for s in reversed(shapes)][::-1] == first
    # compute_units == 0 means 256; 4- and 8-byte types of a kind share their plan
    for n, m in ((1 << 20, 3), (1 << 24, 500), (5000, 10)):
        assert capi.reduce_segments_plan(dt, n, m, 0) == capi.reduce_segments_plan(dt, n, m, 256)
        same = {4: [np.float32, np.int32, np.uint32], 8: [np.float64, np.int64, np.uint64]}[np.dtype(dt).itemsize]
        assert len({capi.reduce_segments_plan(t, n, m, 0) for t in same}) == 1


def test_refusals(capi):
    lib = capi.lib
    r, g, s, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), SZ()
    out = (ctypes.byref(r), ctypes.byref(g), ctypes.byref(s), ctypes.byref(w))
    f = lib.ek_hip_reduce_segments_plan
    assert f(capi.F32, SZ(100), SZ(10), 0, *out) == 0
    assert f(capi.BOOL, SZ(100), SZ(10), 0, *out) == -2 and f(99, SZ(100), SZ(10), 0, *out) == -2
    assert f(capi.F32, SZ(1 << 32), SZ(10), 0, *out) == -2 and f(capi.F32, SZ(100), SZ(1 << 32), 0, *out) == -2
    assert b"2^32" in lib.ek_hip_last_error()
    assert f(capi.F32, SZ((1 << 32) - 1), SZ(10), 0, *out) == 0
    assert f(capi.F32, SZ(100), SZ(10), -1, *out) == -1
    # any of the outputs may be left out
    assert f(capi.F32, SZ(100), SZ(10), 0, None, None, None, None) == 0
