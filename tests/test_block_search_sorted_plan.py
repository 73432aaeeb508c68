"""ek_hip_search_sorted_blocks_plan, the host-only report of the route ek_hip_search_sorted_blocks takes (csrc/block_search.hip), no
GPU needed.

Structural facts only: blocked needles go to the tile route exactly while a row fits the 64 KiB of LDS and to the sampled route
beyond; one row is forwarded; indexed needles are staged whole exactly while the table fits; a tile never exceeds the LDS; a
sampled row satisfies resident * stride <= B < (resident + 1) * stride with stride = 2^global_steps; a row is only split when a tile
is one row; every refusal of the entry is a refusal of the plan."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
LDS = 64 * 1024
NONE, TILE, SAMPLED, INDEXED_LDS, INDEXED_GLOBAL, ONE_ROW = range(6)
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


def name(dt):
    return np.dtype(dt).name


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_route_boundaries(capi, dt):
    cap = LDS // np.dtype(dt).itemsize
    plan = lambda R, B, n, indexed=False, cu=0: capi.search_sorted_blocks_plan(dt, R, B, n, indexed, cu)
    assert sorted(capi.BLOCK_SEARCH_ROUTES) == [NONE, TILE, SAMPLED, INDEXED_LDS, INDEXED_GLOBAL, ONE_ROW]
    for R in (2, 3, 1000):
        for M in (1, 5, 4096):
            assert plan(R, 1, R * M)[0] == TILE and plan(R, cap, R * M)[0] == TILE
            assert plan(R, cap + 1, R * M)[0] == SAMPLED
    for B in (1, cap, cap + 1, 1 << 20):
        assert plan(1, B, 77)[0] == ONE_ROW
        assert plan(1, B, 77, indexed=True)[0] == (INDEXED_LDS if B <= cap else INDEXED_GLOBAL)
    assert plan(4, cap // 4, 9, indexed=True)[0] == INDEXED_LDS and plan(4, cap // 4 + 1, 9, indexed=True)[0] == INDEXED_GLOBAL
    assert plan(5, 7, 0)[0] == NONE and plan(0, 7, 0)[0] == NONE and plan(5, 7, 0, indexed=True)[0] == NONE


@pytest.mark.parametrize("cu", [0, 64, 256, 304])
@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_sizes_are_consistent(capi, dt, cu):
    size = np.dtype(dt).itemsize
    cap = LDS // size
    rng = np.random.default_rng(7)
    rows = [2, 3, 17, 511, 512, 513, 5000, 1 << 20]
    blocks = [1, 2, 3, 63, 64, 65, 1000, cap // 2, cap // 2 + 1, cap - 1, cap, cap + 1, 2 * cap + 1, 100000, (1 << 20) + 3]
    per_row = [1, 3, 4, 5, 257, 2048, 8191, 8192, 65536, 65537, 1 << 20, 1 << 24]
    seen = set()
    for R in rows:
        for B in blocks:
            if R * B >= 1 << 32:
                continue
            for M in per_row:
                route, t, s, resident, stride, steps = capi.search_sorted_blocks_plan(dt, R, B, R * M, False, cu)
                seen.add(route)
                assert route == (TILE if B <= cap else SAMPLED)
                assert 1 <= t <= R
                assert t * B * size <= LDS or route == SAMPLED
                assert s >= 1 and (s == 1 or t == 1)              # only a tile of one row is split
                assert s == 1 or M // s >= 2048                   # a piece keeps every lane busy
                assert t == 1 or t * M <= 65536                   # where the reciprocal multiply of the kernel is exact
                assert stride == 1 << steps and resident * stride <= B < (resident + 1) * stride
                assert resident * size <= LDS and resident >= 1
                if route == TILE:
                    assert (resident, stride, steps) == (B, 1, 0)
                else:
                    assert t == 1 and stride >= 2 and resident >= min(512, cap) // 2
    assert seen == {TILE, SAMPLED}
    for _ in range(200):
        R, B = int(rng.integers(1, 3000)), int(rng.integers(1, 3 * cap))
        n = int(rng.integers(1, 1 << 22))
        route, t, s, resident, stride, steps = capi.search_sorted_blocks_plan(dt, R, B, n, True, cu)
        assert route == (INDEXED_LDS if R * B <= cap else INDEXED_GLOBAL)
        assert (resident, stride, steps) == (B, 1, 0)


def test_many_needles_of_few_rows_are_split(capi):
    cap = LDS // 4
    # 64 rows on 256 compute units: every row is searched by several workgroups, on both blocked routes
    for B in (1024, cap, cap + 1, 1 << 20):
        route, t, s, *_ = capi.search_sorted_blocks_plan(np.float32, 64, B, 64 << 20, False, 256)
        assert t == 1 and s >= 2 and 64 * s >= 2 * 256, (B, t, s)
    # enough rows to fill the device: no split
    assert capi.search_sorted_blocks_plan(np.float32, 1 << 16, 1024, 1 << 26, False, 256)[1:3] == (16, 1)
    # a sampled row with few needles stages fewer samples and takes more steps in global memory
    few = capi.search_sorted_blocks_plan(np.float32, 3, 1 << 20, 3 * 4, False, 256)
    many = capi.search_sorted_blocks_plan(np.float32, 3, 1 << 20, 3 << 16, False, 256)
    assert few[0] == many[0] == SAMPLED and few[3] < many[3] and few[5] > many[5] and many[3] == cap


def test_refusals(capi):
    lib = capi.lib
    outs = [ctypes.c_int(-7) for _ in range(6)]
    refs = [ctypes.byref(x) for x in outs]
    plan = lambda ty, R, B, n, indexed: lib.ek_hip_search_sorted_blocks_plan(ty, SZ(R), SZ(B), SZ(n), indexed, 0, *refs)
    assert plan(capi.F32, 4, 0, 8, 0) == -1 and b"0 entries" in lib.ek_hip_last_error()       # EK_ERR_INVALID
    assert plan(capi.F32, 4, 8, 9, 0) == -1                                                   # 9 needles over 4 rows
    assert plan(capi.F32, 0, 8, 9, 0) == -1 and plan(capi.F32, 0, 8, 9, 1) == -1              # needles and no row
    assert plan(capi.BOOL, 4, 8, 8, 0) == -2 and plan(99, 4, 8, 8, 0) == -2                   # EK_ERR_UNSUPPORTED
    assert plan(capi.F64, 1 << 16, 1 << 16, 1 << 16, 0) == -2 and b"2^32" in lib.ek_hip_last_error()
    assert plan(capi.F64, 1 << 16, (1 << 16) - 1, 1 << 16, 0) == 0
    assert outs[0].value == SAMPLED
    assert plan(capi.F32, 4, 8, 9, 1) == 0 and outs[0].value == INDEXED_LDS                   # indexed: any number of needles
    assert lib.ek_hip_search_sorted_blocks_plan(capi.F32, SZ(4), SZ(8), SZ(8), 0, 0, *([None] * 6)) == 0
