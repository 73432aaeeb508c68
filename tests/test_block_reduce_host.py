"""ek_hip_reduce_blocks_plan, the host-only report of the route ek_hip_reduce_blocks takes (csrc/block_reduce.hip), no GPU needed.

What is checked is the SHAPE of the plan, not where its thresholds lie: for n entries in blocks of B on 256 compute units the regime
is 0 (copy) exactly at B = 1, 1 (whole-array reduction) exactly at B = n, and otherwise walks 2 (packed) -> 3 (one workgroup per
block) -> 4 (split) monotonically as B grows; splits is 1 outside regime 4 and at least 2 inside it.

Bound on the split: the pieces exist to fill the machine, not to flood it.  The plan aims at 4 workgroups per compute unit, and it
splits only when there are fewer blocks than 2 per compute unit, so  splits * (n / B) < 6 * compute_units  (4 CU from the target
rounded up per block, under 2 CU from the rounding)."""
import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
CU = 256
# every B in the scan divides n: powers of two, and 3 / 5 / 7 times a power of two
SIZES = [1 << 22, 3 << 20, 5 << 20, 7 << 20, 15 << 18]


def divisors_up_to(n, limit):
    return [b for b in range(1, limit + 1) if n % b == 0] if n <= 1 << 16 else sorted(
        {o << s for o in (1, 3, 5, 7, 15, 21, 35, 105) for s in range(0, 23) if (o << s) <= limit and n % (o << s) == 0})


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_plan_over_block_sizes(capi, dt):
    seen = set()
    for n in SIZES + [60060, 4096]:
        last = 2
        for B in divisors_up_to(n, min(n, 1 << 20)) + [n]:
            regime, splits, workgroups = capi.reduce_blocks_plan(dt, n, B, CU)
            m = n // B
            assert 0 <= regime <= 4, (n, B, regime)
            assert (regime == 0) == (B == 1), (n, B, regime)
            assert (regime == 1) == (B == n and B != 1), (n, B, regime)
            assert workgroups >= 1, (n, B, workgroups)
            if regime == 4:
                assert splits >= 2 and splits * m < 6 * CU, (n, B, splits)
            else:
                assert splits == 1, (n, B, regime, splits)
            if regime >= 2:
                assert regime >= last, (n, B, regime, last)          # 2 -> 3 -> 4, never back
                last = regime
            seen.add(regime)
    assert seen == {0, 1, 2, 3, 4}


def test_default_compute_units_and_arguments(capi):
    assert capi.reduce_blocks_plan(np.float32, 1 << 24, 1 << 22) == capi.reduce_blocks_plan(np.float32, 1 << 24, 1 << 22, 256)
    # fewer compute units: no more pieces
    assert capi.reduce_blocks_plan(np.float32, 1 << 24, 1 << 22, 64)[1] <= capi.reduce_blocks_plan(np.float32, 1 << 24, 1 << 22, 256)[1]
    assert capi.reduce_blocks_plan(np.float64, 0, 5) == (0, 1, 0)
    for bad in ((10, 0), (10, 3)):
        with pytest.raises(capi.EnokiHipError):
            capi.reduce_blocks_plan(np.float32, *bad)
    import ctypes
    r, s, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert capi.lib.ek_hip_reduce_blocks_plan(0, ctypes.c_size_t(8), ctypes.c_size_t(2), 0, ctypes.byref(r), ctypes.byref(s), ctypes.byref(w)) == -2
    assert capi.lib.ek_hip_reduce_blocks_plan(99, ctypes.c_size_t(8), ctypes.c_size_t(2), 0, ctypes.byref(r), ctypes.byref(s), ctypes.byref(w)) == -2
