"""ek_hip_sort_plan, the host-only report of what ek_hip_sort does (csrc/sort.hip), no GPU needed.

Route 0 for n <= 1; route 1 forwards to ek_hip_sort_blocks with block == n; route 2 is the radix route: as many 8-bit passes as the key
has bytes, tiles of `tile` entries, `tiles_per_workgroup` consecutive tiles per workgroup.  The tuning "sort_radix" picks between 1
and 2: 0 never radix, 1 from ONE threshold per element size on (at least block_sort's chunk + 1, so that a sort of one launch stays
one launch), 2 from n = 2.  Every refusal of the entry's shape checks is a refusal of the plan."""
import ctypes

import numpy as np
import pytest

DTYPES = [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64]
TRIVIAL, FORWARDED, RADIX = range(3)
SZ = ctypes.c_size_t
TOP = 2 ** 32 - 1


@pytest.fixture(scope="module")
def capi():
    from enoki_amd import capi as c        # (loading the library and asking for a plan needs no device)
    return c


@pytest.fixture
def tuning(capi):
    def set_(mode):
        capi.set_tuning("sort_radix", mode)
    try:
        yield set_
    finally:
        capi.set_tuning("sort_radix", 1)


def name(dt):
    return np.dtype(dt).name


def threshold(capi, dt, cu=0, want_index=True):
    """the first n of the radix route under tuning 1, by bisection on the plan"""
    lo, hi = 2, TOP
    assert capi.sort_plan(dt, lo, want_index, cu)[0] == FORWARDED and capi.sort_plan(dt, hi, want_index, cu)[0] == RADIX
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if capi.sort_plan(dt, mid, want_index, cu)[0] == FORWARDED:
            lo = mid
        else:
            hi = mid
    return hi


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_trivial_for_at_most_one_entry(capi, tuning, dt):
    assert sorted(capi.SORT_ROUTES) == [TRIVIAL, FORWARDED, RADIX]
    for mode in (0, 1, 2):
        tuning(mode)
        for n in (0, 1):
            route, passes, _, _, _, launches, scratch = capi.sort_plan(dt, n)
            assert (route, passes, scratch) == (TRIVIAL, 0, 0) and launches == 0


def test_one_threshold_per_element_size(capi, tuning):
    tuning(1)
    seen = {}
    for dt in DTYPES:
        t = threshold(capi, dt)
        chunk = capi.sort_blocks_plan(dt, 4, 2)[2]
        assert t >= chunk + 1, (name(dt), t)
        seen.setdefault(np.dtype(dt).itemsize, set()).add(t)
        # forwarded below, radix from there up: the bisection's premise, spot-checked
        for n in (2, 3, chunk, chunk + 1, t - 1):
            if n < t:
                assert capi.sort_plan(dt, n)[0] == FORWARDED, (name(dt), n)
        for n in (t, t + 1, 2 * t, 3 * t + 7, 1 << 26, TOP):
            assert capi.sort_plan(dt, n)[0] == RADIX, (name(dt), n)
        # neither the CU count nor the index request moves it
        for cu in (0, 64, 256, 304):
            for want_index in (False, True):
                assert threshold(capi, dt, cu, want_index) == t
    assert sorted(seen) == [4, 8] and all(len(v) == 1 for v in seen.values())


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_the_radix_route(capi, tuning, dt):
    tuning(2)
    itemsize = np.dtype(dt).itemsize
    T = capi.sort_plan(dt, 2)[2]
    assert T in (4096, 8192) and T % 512 == 0
    for cu in (0, 64, 256, 304):
        groups = 2 * (cu or 256)
        for n in (2, 3, 64, T - 1, T, T + 1, 3 * T + 7, groups * T, groups * T + 1, 2 * groups * T, 2 * groups * T + 1, (1 << 26) + 5, TOP):
            route, passes, tile, per, wgs, launches, scratch = capi.sort_plan(dt, n, True, cu)
            assert route == RADIX and passes == itemsize and tile == T
            tiles = -(-n // T)
            assert per == -(-tiles // min(tiles, groups)) and wgs == -(-tiles // per) and 1 <= wgs <= groups
            assert per * wgs * tile >= n and (wgs - 1) * per * tile < n                   # every entry is covered, no workgroup is idle
            assert launches == 4 * passes
            # two buffers of keys and two of positions, and the counters of every (digit, workgroup)
            assert scratch >= 2 * n * (itemsize + 4) + 4 * 256 * wgs
            assert capi.sort_plan(dt, n, False, cu) == (route, passes, tile, per, wgs, launches, scratch)
    # the smallest n of two tiles per workgroup
    assert capi.sort_plan(dt, 512 * T, True, 256)[3] == 1 and capi.sort_plan(dt, 512 * T + 1, True, 256)[3] == 2


@pytest.mark.parametrize("dt", DTYPES, ids=name)
def test_the_tuning_picks_the_route(capi, tuning, dt):
    chunk = capi.sort_blocks_plan(dt, 4, 2)[2]
    sizes = (0, 1, 2, 3, 2048, 2049, chunk, chunk + 1, 1 << 20, 1 << 26, TOP)
    tuning(0)
    for n in sizes:
        route, passes, _, _, _, launches, scratch = capi.sort_plan(dt, n)
        assert route <= FORWARDED and route == (FORWARDED if n >= 2 else TRIVIAL) and passes == 0
        if n >= 2:
            # what ek_hip_sort_blocks does for one row of n entries
            b_route, _, _, merges, wgs = capi.sort_blocks_plan(dt, n, n)
            assert launches == 1 + merges and capi.sort_plan(dt, n)[4] == wgs
            assert (scratch > 0) == (b_route == 3)
    tuning(2)
    for n in sizes:
        assert capi.sort_plan(dt, n)[0] == (RADIX if n >= 2 else TRIVIAL)
    tuning(1)
    assert capi.sort_plan(dt, chunk)[0] == FORWARDED and capi.sort_plan(dt, chunk)[5] == 1        # one launch stays one launch


def test_refusals(capi, tuning):
    lib = capi.lib
    outs = [ctypes.c_int(), ctypes.c_int(), SZ(), SZ(), SZ(), ctypes.c_int(), SZ()]
    refs = [ctypes.byref(o) for o in outs]
    pl = lambda ty, n, cu=0: lib.ek_hip_sort_plan(ty, SZ(n), 1, cu, *refs)
    for mode in (0, 1, 2):
        tuning(mode)
        assert pl(capi.BOOL, 12) == -2 and b"ek_hip_sort_plan" in lib.ek_hip_last_error()
        assert pl(99, 12) == -2 and pl(-1, 12) == -2
        assert pl(capi.F32, 12, -1) == -1
        # 2^32 - 1 entries are the most; one more is refused as unsupported
        assert pl(capi.F32, TOP) == 0 and pl(capi.F64, TOP) == 0
        assert pl(capi.F32, 2 ** 32) == -2 and b"2^32 - 1" in lib.ek_hip_last_error()
        assert pl(capi.U64, 2 ** 32) == -2 and pl(capi.I32, 2 ** 40) == -2
        # null result pointers are allowed
        assert lib.ek_hip_sort_plan(capi.F32, SZ(12), 0, 0, None, None, None, None, None, None, None) == 0
    with pytest.raises(capi.EnokiHipError):
        capi.sort_plan(np.bool_, 10)
    # an unknown value of the tuning is refused and changes nothing
    tuning(2)
    assert lib.ek_hip_set_tuning(b"sort_radix", 3) == -1 and lib.ek_hip_set_tuning(b"sort_radix", -1) == -1
    assert capi.sort_plan(np.float32, 2)[0] == RADIX
