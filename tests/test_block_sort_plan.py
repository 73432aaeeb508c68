"""ek_hip_sort_blocks_plan, the host-only report of the route ek_hip_sort_blocks takes (csrc/block_sort.hip), no GPU needed.

The header comment of block_sort.hip says: route 0 at B == 1; route 1 (packed) up to B == 2048 with 2048 / P rows per tile, P = B
rounded up to a power of two; route 2 (one workgroup per row) up to the chunk, 8192 entries for 4-byte and 4096 for 8-byte types;
route 3 (chunks and merges) beyond, with ceil(log2(ceil(B / chunk))) merge launches.  Every refusal of the entry's shape checks is a
refusal of the plan."""
import ctypes
import math

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
TRIVIAL, PACKED, ROW, MERGED = range(4)
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


def name(dt):
    return np.dtype(dt).name


def pow2_ceil(v):
    return 1 << (v - 1).bit_length()


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_route_boundaries(capi, dt):
    plan = lambda n, B, cu=0: capi.sort_blocks_plan(dt, n, B, True, cu)
    assert sorted(capi.BLOCK_SORT_ROUTES) == [TRIVIAL, PACKED, ROW, MERGED]
    chunk = plan(4, 2)[2]
    assert chunk == (8192 if np.dtype(dt).itemsize == 4 else 4096)
    for m in (1, 3, 1000):
        assert plan(m, 1)[0] == TRIVIAL
        assert plan(2 * m, 2)[0] == PACKED and plan(2048 * m, 2048)[0] == PACKED
        assert plan(2049 * m, 2049)[0] == ROW and plan(chunk * m, chunk)[0] == ROW
        assert plan((chunk + 1) * m, chunk + 1)[0] == MERGED and plan((1 << 20) * m, 1 << 20)[0] == MERGED
    assert plan(0, 7)[0] == TRIVIAL
    # the chunk is reported for every shape, and neither the CU count nor the index request moves a boundary
    for B in (1, 2, 2048, 2049, chunk, chunk + 1):
        for cu in (0, 64, 256, 304):
            for want_index in (False, True):
                assert capi.sort_blocks_plan(dt, 6 * B, B, want_index, cu) == plan(6 * B, B)
        assert plan(6 * B, B)[2] == chunk


def test_the_chunk_of_8_byte_types_is_no_larger(capi):
    c = {np.dtype(dt).itemsize: capi.sort_blocks_plan(dt, 4, 2)[2] for dt in DTYPES}
    assert c[8] <= c[4]
    assert len({capi.sort_blocks_plan(dt, 4, 2)[2] for dt in DTYPES if np.dtype(dt).itemsize == 8}) == 1


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_packed_tiles(capi, dt):
    for B in (2, 3, 5, 63, 64, 65, 100, 255, 256, 257, 1000, 1024, 1025, 2047, 2048):
        for m in (1, 7, 100, 12345):
            route, tile_rows, _, passes, wgs = capi.sort_blocks_plan(dt, m * B, B)
            assert route == PACKED and passes == 0
            assert tile_rows == 2048 // pow2_ceil(B) and tile_rows >= 1 and tile_rows * B <= 2048
            assert wgs == -(-m // tile_rows)


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_merge_passes(capi, dt):
    chunk = capi.sort_blocks_plan(dt, 4, 2)[2]
    for B in (2049, chunk - 1, chunk):
        route, _, _, passes, wgs = capi.sort_blocks_plan(dt, 3 * B, B)
        assert (route, passes, wgs) == (ROW, 0, 3)
    for B in (chunk + 1, 2 * chunk, 2 * chunk + 1, 2 * chunk + 5, 3 * chunk, 4 * chunk, 4 * chunk + 1, 5 * chunk + 1, 1 << 20, (1 << 20) + 1,
              (1 << 26) - 3, 1 << 26):
        for m in (1, 3):
            route, _, c, passes, wgs = capi.sort_blocks_plan(dt, m * B, B)
            runs = -(-B // chunk)
            assert route == MERGED and c == chunk
            assert passes == math.ceil(math.log2(runs)) and (1 << passes) >= runs > (1 << (passes - 1))
            assert wgs == m * runs                 # the first launch sorts every chunk of every row


def test_refusals(capi):
    lib = capi.lib
    outs = [ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()]
    refs = [ctypes.byref(o) for o in outs]
    pl = lambda ty, n, B, cu=0: lib.ek_hip_sort_blocks_plan(ty, SZ(n), SZ(B), 1, cu, *refs)
    assert pl(capi.F32, 12, 0) == -1 and b"ek_hip_sort_blocks_plan" in lib.ek_hip_last_error()
    assert pl(capi.F32, 12, 5) == -1 and b"no whole number of blocks" in lib.ek_hip_last_error()
    assert pl(capi.F32, 12, 24) == -1
    assert pl(capi.F32, 12, 3, -1) == -1
    assert pl(capi.BOOL, 12, 3) == -2 and pl(99, 12, 3) == -2
    # 2^32 - 1 entries are the most; one more is refused as unsupported, whatever the block
    assert pl(capi.F32, 2 ** 32 - 1, 3) == 0 and pl(capi.F64, 2 ** 32 - 1, 2 ** 32 - 1) == 0
    assert pl(capi.F32, 2 ** 32, 2) == -2 and b"2^32 - 1" in lib.ek_hip_last_error()
    assert pl(capi.U64, 2 ** 32, 2 ** 32) == -2 and pl(capi.I32, 2 ** 40, 1) == -2
    with pytest.raises(capi.EnokiHipError):
        capi.sort_blocks_plan(np.float32, 10, 3)
    # null result pointers are allowed
    assert lib.ek_hip_sort_blocks_plan(capi.F32, SZ(12), SZ(3), 0, 0, None, None, None, None, None) == 0
