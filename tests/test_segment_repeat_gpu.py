"""ek_hip_repeat_segments through the C ABI (csrc/block_segments.hip): out[i] = in[j] for the last j with starts[j] <= i, 0 in
front of starts[0] -- the transpose of the segment sum over `size` entries.

Expected values are numpy's: gather(v, searchsorted(starts, arange(size), side="right") - 1) with 0 where there is no such j.  The
call moves values and never computes with them, so every comparison is bit for bit.  Every output is written into a window of a
larger buffer that is filled with a value no entry has: nothing in front of or behind the window may change, at any alignment."""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

SZ = ctypes.c_size_t
BASE = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
MARK = 0x7FFFFFF7                                   # (no entry has this value)


def name(dt):
    return np.dtype(dt).name


def starts_of(lengths, gap=0):
    lengths = np.asarray(lengths, np.int64)
    ends = gap + np.cumsum(lengths)
    return (ends - lengths).astype(np.uint32), int(ends[-1]) if lengths.size else gap


def length_mixes():
    """the mixes of tests/test_segment_reduce_gpu.py: every length of BASE in front of, between and behind the others, one long
    segment among single entries, nothing but empty segments, one segment, entries in front of the first start, trailing starts at n"""
    mixes = [(BASE[r:] + BASE[:r], 0) for r in range(len(BASE))]
    mixes += [([1] * 5 + [20000] + [1] * 7, 0), ([20000] + [1] * 300, 0), ([1] * 300 + [20000], 0)]
    mixes += [([0] * 37, 0), ([0] * 300, 11), ([0], 0), ([1], 0), ([5000], 0), ([777], 5)]
    mixes += [(BASE, 7), (BASE[1:] + [0] * 9, 0), ([3, 0, 1, 2] * 3000, 1), ([0] * 6000 + [9000] + [0] * 6000, 0)]
    return mixes


def expected(v, starts, size):
    j = np.searchsorted(starts, np.arange(size, dtype=np.int64), side="right")
    out = np.zeros(size, v.dtype)
    out[j > 0] = v[j[j > 0] - 1]
    return out


def values(rng, dt, m):
    return rng.integers(1, 1 << 30, m).astype(dt)               # (never 0: a missing segment shows)


def run(capi, v, starts, size, offset=0, pad=8):
    """repeat_segments into a window `offset` entries into a buffer of MARKs; checks that nothing outside the window changed"""
    dt = v.dtype
    out = capi.Buf.from_numpy(np.full(size + 2 * pad, MARK, dt))
    capi.repeat_segments(capi.Buf.from_numpy(v), capi.Buf.from_numpy(starts.astype(np.uint32)), size, out=out.view(offset, size))
    got = out.numpy()
    assert np.all(got[:offset] == dt.type(MARK)) and np.all(got[offset + size:] == dt.type(MARK)), (name(dt), size, offset, "written outside out")
    return got[offset:offset + size]


@pytest.mark.parametrize("dt", [np.float32, np.uint32, np.float64, np.int64], ids=name)
def test_length_mixes_at_every_alignment(capi, dt):
    rng = np.random.default_rng(5)
    dt = np.dtype(dt)
    for lengths, gap in length_mixes():
        starts, n = starts_of(lengths, gap)
        v = values(rng, dt, starts.size)
        want = expected(v, starts, n)
        for offset in ((0, 1, 2, 3, 4) if dt.itemsize == 4 else (0, 1, 2)):
            assert bits_equal(run(capi, v, starts, n, offset), want), (name(dt), lengths[:6], gap, offset)
        assert bits_equal(capi.repeat_segments(capi.Buf.from_numpy(v), capi.Buf.from_numpy(starts), n).numpy(), want)


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_size_smaller_and_larger_than_the_last_start(capi, dt):
    rng = np.random.default_rng(6)
    dt = np.dtype(dt)
    for lengths, gap in ((BASE, 3), ([1] * 5 + [20000] + [1] * 7, 0), ([7] * 5000, 0)):
        starts, n = starts_of(lengths, gap)
        v = values(rng, dt, starts.size)
        last = int(starts[-1])
        for size in (1, 2, gap + 1, last // 2, last - 1, last, last + 1, n, n + 1, n + 1000, 2 * n + 3):
            if size > 0:
                for offset in (0, 1):
                    assert bits_equal(run(capi, v, starts, size, offset), expected(v, starts, size)), (name(dt), lengths[:4], size, offset)
    # size == 0: nothing is launched, nothing is written; no segment at all: zeros
    l0 = capi.lib.ek_hip_launch_count()
    assert run(capi, values(rng, dt, 3), np.array([0, 1, 2], np.uint32), 0).size == 0 and capi.lib.ek_hip_launch_count() == l0
    assert bits_equal(run(capi, np.zeros(0, dt), np.zeros(0, np.uint32), 1000, 1), np.zeros(1000, dt))


@pytest.mark.parametrize("dt", [np.uint32, np.float64], ids=name)
def test_more_than_one_trip_of_the_grid(capi, dt):
    """the grid is capped at 6 workgroups per CU and a workgroup writes 4 KiB per trip: 2 Mi entries are more than one trip of both
    element sizes on up to 341 (4-byte) / 682 (8-byte) CUs; many short segments (the starts of a tile fit in LDS), long ones, and
    so many empty ones that a tile's starts do not fit and are searched in global memory"""
    import torch
    rng = np.random.default_rng(8)
    dt = np.dtype(dt)
    size = (2 << 20) - 5
    per_trip = torch.cuda.get_device_properties(0).multi_processor_count * 6 * (4096 // dt.itemsize)
    assert size > per_trip
    for lengths in (rng.integers(0, 8, size // 3), rng.integers(0, 40000, 105), np.concatenate([np.zeros(200000, np.int64), rng.integers(0, 7, 500000)])):
        starts, n = starts_of(lengths, 2)
        starts = starts[starts < size]
        v = values(rng, dt, starts.size)
        got = run(capi, v, starts, size, 1)
        assert bits_equal(got, expected(v, starts, size)), (name(dt), starts.size)


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int32, np.uint64], ids=name)
def test_transpose_identity(capi, dt):
    """sum_i w[i] * segment_repeat(v)[i] == sum_j v[j] * segment_sum(w)[j] on small integers, where both sides are exact"""
    rng = np.random.default_rng(9)
    dt = np.dtype(dt)
    for lengths, gap in length_mixes()[::2] + [([5000, 500000], 3), (rng.integers(0, 3000, 300), 0)]:
        starts, n = starts_of(lengths, gap)
        if n == 0:
            continue
        m = starts.size
        w, v = rng.integers(0, 8, n).astype(dt), rng.integers(0, 8, m).astype(dt)
        st = capi.Buf.from_numpy(starts)
        rep = capi.repeat_segments(capi.Buf.from_numpy(v), st, n).numpy()
        sums = capi.reduce_segments("hsum", capi.Buf.from_numpy(w), st).numpy()
        lhs = int((w.astype(np.int64) * rep.astype(np.int64)).sum())
        rhs = int((v.astype(np.int64) * sums.astype(np.int64)).sum())
        assert lhs == rhs, (name(dt), n, m, lhs, rhs)


def test_arguments(capi):
    lib = capi.lib
    v = capi.Buf.from_numpy(np.arange(1, 5, dtype=np.float32))
    st = capi.Buf.from_numpy(np.array([0, 3, 3, 10], np.uint32))
    out = capi.Buf.from_numpy(np.full(12, 7, np.float32))
    p = lambda b: ctypes.c_void_p(b.ptr)
    rp = lib.ek_hip_repeat_segments
    l0 = lib.ek_hip_launch_count()
    assert rp(capi.F32, None, p(v), p(st), SZ(4), SZ(12)) == -1 and b"ek_hip_repeat_segments" in lib.ek_hip_last_error()
    assert rp(capi.F32, p(out), None, p(st), SZ(4), SZ(12)) == -1 and rp(capi.F32, p(out), p(v), None, SZ(4), SZ(12)) == -1
    assert rp(capi.F32, ctypes.c_void_p(out.ptr + 2), p(v), p(st), SZ(4), SZ(8)) == -1
    assert rp(capi.F32, p(out), ctypes.c_void_p(v.ptr + 1), p(st), SZ(3), SZ(12)) == -1
    assert rp(capi.F32, p(out), p(v), ctypes.c_void_p(st.ptr + 2), SZ(3), SZ(12)) == -1
    assert rp(capi.BOOL, p(out), p(v), p(st), SZ(4), SZ(12)) == -2 and rp(99, p(out), p(v), p(st), SZ(4), SZ(12)) == -2
    assert rp(capi.F32, p(out), p(v), p(st), SZ(4), SZ(1 << 32)) == -2 and b"2^32" in lib.ek_hip_last_error()
    assert rp(capi.F32, p(out), p(v), p(st), SZ(1 << 32), SZ(12)) == -2
    assert rp(capi.F32, None, None, None, SZ(0), SZ(0)) == 0 and rp(capi.F32, None, p(v), p(st), SZ(4), SZ(0)) == 0
    with pytest.raises(ValueError):
        capi.repeat_segments(v, capi.Buf.from_numpy(np.array([0, 3], np.uint32)), 12)          # len(v) != len(starts)
    assert lib.ek_hip_launch_count() == l0
    assert np.array_equal(out.numpy(), np.full(12, 7, np.float32))
    # the calls after refused ones work
    assert rp(capi.F32, p(out), p(v), p(st), SZ(4), SZ(12)) == 0
    assert np.array_equal(out.numpy(), [1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 4, 4])


@pytest.mark.parametrize("dt", [np.float32, np.int64], ids=name)
def test_bad_starts_stay_inside(capi, dt):
    """starts that decrease or exceed the size: values unspecified (as defined for non-decreasing ones), but every output entry is
    written with an entry of `in` or 0, and nothing around `in`, `starts` and `out` is touched.  `in` is a window of a buffer whose
    other entries hold a poison value, so an entry read from outside the window shows in the output."""
    rng = np.random.default_rng(31)
    dt = np.dtype(dt)
    pad, poison = 64, 0x5A5A5A5A
    cases = []
    for size, m in ((5000, 40), (5000, 3), (100000, 25000), (300000, 5), (2000, 9000)):
        cases.append((size, np.sort(rng.integers(0, size + 300, m)).astype(np.uint32), True))      # in order, some above the size
        cases.append((size, rng.integers(0, size + 300, m).astype(np.uint32), False))             # no order at all
        cases.append((size, np.sort(rng.integers(0, size, m))[::-1].astype(np.uint32), False))    # the wrong way round
    for size, starts, ordered in cases:
        v = values(rng, dt, starts.size)
        base = capi.Buf.from_numpy(np.concatenate([np.full(pad, poison, dt), v, np.full(pad, poison, dt)]))
        out = capi.Buf.from_numpy(np.full(size + 2 * pad, MARK, dt))
        capi.repeat_segments(base.view(pad, v.size), capi.Buf.from_numpy(starts), size, out=out.view(pad + 1, size))
        got = out.numpy()
        assert np.all(got[:pad + 1] == dt.type(MARK)) and np.all(got[pad + 1 + size:] == dt.type(MARK))
        body = got[pad + 1:pad + 1 + size]
        assert not np.any(body == dt.type(MARK)) and not np.any(body == dt.type(poison)), (name(dt), size, starts.size)
        assert np.all(np.isin(body, np.concatenate([v, np.zeros(1, dt)]))), (name(dt), size, starts.size)
        if ordered:
            assert bits_equal(body, expected(v, starts, size)), (name(dt), size, starts.size)
