"""ek_hip_psum_blocks_plan, the host-only report of the route ek_hip_psum_blocks takes (csrc/block_scan.hip), no GPU needed.

The thresholds are structural: regime 0 (copy or zero fill) exactly at B = 1; 1 (packed) up to the tile's capacity of 1024 entries;
2 (one workgroup per block) beyond; 3 (split) for fewer than 2 blocks per compute unit of at least 16 Ki entries, where the block is
cut into S = min(ceil(4 CU / m), B / 8 Ki, 1024) pieces that are multiples of the vector width: splits >= 2 exactly in regime 3, every
piece holds an entry ((splits - 1) * piece < B for the rounded piece), and the grid of the first launch is never empty."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
CU = 256
SPLIT_MIN = 16384


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_regime_boundaries(capi, dt):
    plan = lambda n, B, cu=CU: capi.psum_blocks_plan(dt, n, B, cu)
    for m in (1, 7, 4096):
        assert plan(m, 1)[0] == 0
        assert plan(m * 2, 2)[0] == 1 and plan(m * 1024, 1024)[0] == 1
        assert plan(m * 1025, 1025)[0] == 2                    # (too short to split whatever the block count)
    # m just below and at 2 x CU, with blocks large enough to split
    B = 4 * SPLIT_MIN
    assert plan((2 * CU - 1) * B, B)[0] == 3 and plan(2 * CU * B, B)[0] == 2
    assert plan((2 * 64 - 1) * B, B, 64)[0] == 3 and plan(2 * 64 * B, B, 64)[0] == 2
    # B just below and at the split minimum
    for m in (1, 2, 3):
        assert plan(m * (SPLIT_MIN - 1), SPLIT_MIN - 1)[0] == 2
        assert plan(m * SPLIT_MIN, SPLIT_MIN)[0] == 3 and plan(m * SPLIT_MIN, SPLIT_MIN)[1] == 2


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_splits_pieces_and_grids(capi, dt):
    N = 16 // np.dtype(dt).itemsize
    seen = set()
    for B in (1, 2, 3, 100, 1024, 1025, 4096, SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1, 2 * SPLIT_MIN + 5, 3 * SPLIT_MIN, 1 << 20, (1 << 25) + 3):
        for m in (1, 2, 3, 5, 2 * CU - 1, 2 * CU, 1000):
            regime, splits, workgroups = capi.psum_blocks_plan(dt, m * B, B, CU)
            seen.add(regime)
            assert 0 <= regime <= 3 and workgroups > 0, (B, m, regime, workgroups)
            assert (splits >= 2) == (regime == 3) and (regime == 3 or splits == 1), (B, m, regime, splits)
            if regime == 3:
                assert m < 2 * CU and B >= SPLIT_MIN and workgroups == m * splits
                # the pieces the plan can have made: ceil(B / S) rounded up to the vector width for some S >= splits; all of them
                # leave the last piece at least one entry
                pieces = {-(-(-(-B // S)) // N) * N for S in range(splits, 1025)}
                ok = [p for p in pieces if -(-B // p) == splits]
                assert ok and all((splits - 1) * p < B for p in ok), (B, m, splits)
                assert splits <= 1024 and splits * m < 6 * CU
    assert seen == {0, 1, 2, 3}


def test_default_compute_units_and_arguments(capi):
    for B in (1 << 22, 1 << 16, 128):
        assert capi.psum_blocks_plan(np.float32, 1 << 24, B) == capi.psum_blocks_plan(np.float32, 1 << 24, B, 256)
    # fewer compute units: no more pieces
    assert capi.psum_blocks_plan(np.float32, 1 << 24, 1 << 22, 64)[1] <= capi.psum_blocks_plan(np.float32, 1 << 24, 1 << 22, 256)[1]
    assert capi.psum_blocks_plan(np.float64, 0, 5) == (0, 1, 0)
    for bad in ((10, 0), (10, 3)):
        with pytest.raises(capi.EnokiHipError):
            capi.psum_blocks_plan(np.float32, *bad)
    r, s, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    call = lambda t: capi.lib.ek_hip_psum_blocks_plan(t, ctypes.c_size_t(8), ctypes.c_size_t(2), 0, ctypes.byref(r), ctypes.byref(s), ctypes.byref(w))
    assert call(0) == -2 and call(99) == -2
