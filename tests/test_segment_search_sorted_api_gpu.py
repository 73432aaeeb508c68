"""segment_search_sorted in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`): keywords, error types, the
UInt32 result for every flat arithmetic type, nothing recorded on differentiable arrays, and the README pipeline end to end.

Every comparison is exact equality with numpy.searchsorted per segment."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TYPES = [("Float32", np.float32), ("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 0, 0, 257, 1025, 5, 9000, 1, 0]
COUNTS = [5, 0, 1, 64, 300, 7, 0, 3, 0, 2500, 9, 1, 4000, 2, 6]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]           # (right, flat)


@pytest.fixture(scope="module")
def ekc():
    import enoki_amd.hip as m
    m.hip_init(0)
    return m


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


def starts_of(lengths, gap=0):
    lengths = np.asarray(lengths, np.int64)
    ends = gap + np.cumsum(lengths)
    return (ends - lengths).astype(np.uint32), int(ends[-1])


def searched(table, table_starts, needles, seg, right, flat):
    """numpy.searchsorted per segment; seg: the segment of every needle, -1 for none"""
    nt = table.size
    lo = np.minimum(table_starts.astype(np.int64), nt)
    hi = np.maximum(lo, np.concatenate([lo[1:], [nt]]))
    out = np.zeros(needles.size, np.int64)
    for j in range(table_starts.size):
        idx = np.flatnonzero(seg == j)
        if idx.size:
            out[idx] = np.searchsorted(table[lo[j]:hi[j]], needles[idx], "right" if right else "left") + (lo[j] if flat else 0)
    return out.astype(np.uint32)


def test_every_flat_type_of_both_modules(ekc, ad):
    import enoki as ek
    rng = np.random.default_rng(1)
    table_starts, nt = starts_of(LENGTHS)
    needle_starts, n = starts_of(COUNTS, 4)
    m = table_starts.size
    seg = np.searchsorted(needle_starts, np.arange(n), side="right") - 1
    rows = rng.integers(0, m + 4, n).astype(np.uint32)
    for mod in (ekc, ad):
        ts, ns, rw = mod.UInt32(table_starts), mod.UInt32(needle_starts), mod.UInt32(rows)
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            ht = rng.integers(0, 200, nt).astype(dt)
            order = np.lexsort((ht, np.repeat(np.arange(m), LENGTHS)))
            ht = ht[order]                                                      # sorted inside every segment, with repeats
            hn = rng.integers(0, 201, n).astype(dt)
            table, needles = A(ht), A(hn)
            for right, flat in FLAGS:
                want = searched(ht, table_starts, hn, seg, right, flat)
                got = mod.segment_search_sorted(table, ts, needles, needle_starts=ns, right=right, flat=flat)
                assert type(got) is mod.UInt32 and len(got) == n and np.array_equal(got.numpy(), want), (cls, right, flat)
                assert np.array_equal(ek.segment_search_sorted(table=table, table_starts=ts, needles=needles, needle_starts=ns,
                                                               right=right, flat=flat).numpy(), want)
                want = searched(ht, table_starts, hn, np.minimum(rows.astype(np.int64), m - 1), right, flat)
                got = mod.segment_search_sorted(table, ts, needles, rows=rw, right=right, flat=flat)
                assert type(got) is mod.UInt32 and np.array_equal(got.numpy(), want), (cls, right, flat, "rows")
            assert np.array_equal(mod.segment_search_sorted(table, ts, needles, ns).numpy(), searched(ht, table_starts, hn, seg, False, False))
            # exactly one owner; starts and rows are UInt32 arrays; their lengths match
            with pytest.raises(ValueError):
                mod.segment_search_sorted(table, ts, needles)
            with pytest.raises(ValueError):
                mod.segment_search_sorted(table, ts, needles, needle_starts=ns, rows=rw)
            if cls != "UInt32":
                with pytest.raises(TypeError):
                    mod.segment_search_sorted(table, table, needles, needle_starts=ns)
                with pytest.raises(TypeError):
                    mod.segment_search_sorted(table, ts, needles, rows=needles)
                with pytest.raises(TypeError):
                    mod.segment_search_sorted(table, ts, rw, needle_starts=ns)           # needles of another type than the table
            with pytest.raises(RuntimeError):
                mod.segment_search_sorted(table, ts, needles, needle_starts=mod.UInt32(needle_starts[:-1]))
            with pytest.raises(RuntimeError):
                mod.segment_search_sorted(table, ts, needles, rows=mod.UInt32(rows[:-1]))
            none = mod.UInt32(np.zeros(0, np.uint32))
            with pytest.raises(RuntimeError):
                mod.segment_search_sorted(table, none, needles, rows=rw)      # a row per needle and no segment
            assert np.array_equal(mod.segment_search_sorted(table, none, needles, needle_starts=none, flat=True).numpy(), np.zeros(n, np.uint32))
            assert np.array_equal(mod.segment_search_sorted(A(ht[:0]), ts, needles, needle_starts=ns, flat=True).numpy(), np.zeros(n, np.uint32))
            assert len(mod.segment_search_sorted(table, ts, A(hn[:0]), needle_starts=ns)) == 0


def test_differentiable_operands_record_nothing(ad):
    table_starts, nt = starts_of([3, 0, 64, 1000])
    needle_starts, n = starts_of([10, 5, 100, 3000], 2)
    rng = np.random.default_rng(2)
    ht = np.sort(rng.random(nt)).astype(np.float32)
    ht = ht[np.lexsort((ht, np.repeat(np.arange(4), [3, 0, 64, 1000])))]
    hn = rng.random(n).astype(np.float32)
    table, needles = ad.Float32(ht), ad.Float32(hn)
    ad.set_requires_gradient(table)
    ad.set_requires_gradient(needles)
    k = ad.segment_search_sorted(table, ad.UInt32(table_starts), needles, needle_starts=ad.UInt32(needle_starts), flat=True)
    assert type(k) is ad.UInt32 and k.index == 0 and not ad.requires_gradient(k)
    seg = np.searchsorted(needle_starts, np.arange(n), side="right") - 1
    assert np.array_equal(k.numpy(), searched(ht, table_starts, hn, seg, False, True))
    # ... and the positions gather from the differentiable table as any index array does
    picked = ad.gather(table, ad.UInt32(np.minimum(k.numpy(), nt - 1)))
    assert ad.requires_gradient(picked)


@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9])
def test_draw_new_samples_from_the_cdf_of_every_compressed_ray(ekc, keep):
    """the README pipeline: compress() drops the culled samples of every ray, the counts per ray become starts through an exclusive
    block_psum, segment_psum of the kept weights is a CDF per ray, segment_search_sorted(..., flat=True) finds the sample every new
    random number falls into and gather picks it -- nothing is read back on the way.  The weights are multiples of 1/8 below 2^10:
    with such weights every float32 prefix sum of up to 64 of them is exact (below 2^16 in steps of 1/8: 19 bits), whatever the
    order of the additions, so the CDF ascends strictly and equals numpy's cumsum bit for bit.  segment_psum does NOT promise an
    ascending result in general (float prefix sums are sums in a fixed tree order); a CDF that a search is going to read wants this
    care, or a running maximum."""
    rng = np.random.default_rng(int(keep * 10))
    rays, S, M = 2001, 64, 6
    hw = (rng.integers(1, 8 << 10, rays * S) / 8.0).astype(np.float32)
    hm = rng.random(rays * S) < keep
    hm.reshape(rays, S)[[5, rays - 2]] = False                     # two rays lose every sample (not the last: its position is nt)
    w, mask = ekc.Float32(hw), ekc.Mask(hm)
    kept = ekc.compress(w, mask)
    where = ekc.compress(ekc.UInt32.arange(rays * S), mask)       # the original position of every kept sample
    counts = ekc.block_sum(ekc.select(mask, ekc.UInt32.full(1, rays * S), ekc.UInt32.zero(rays * S)), S)
    starts = ekc.block_psum(counts, len(counts), exclusive=True)
    cdf = ekc.segment_psum(kept, starts)
    new_starts = ekc.UInt32.arange(rays) * ekc.UInt32.full(M, rays)
    total = ekc.segment_sum(kept, starts)
    xi = (rng.random(rays * M) * 0.999).astype(np.float32)
    u = ekc.Float32(xi) * ekc.segment_repeat(total, new_starts, rays * M)
    at = ekc.segment_search_sorted(cdf, starts, u, needle_starts=new_starts, right=True, flat=True)
    picked = ekc.gather(where, at)
    # numpy, ray by ray
    hu, hat = u.numpy(), at.numpy()
    per_ray = hm.reshape(rays, S).sum(axis=1)
    hstarts = np.concatenate([[0], np.cumsum(per_ray)[:-1]])
    assert np.array_equal(starts.numpy(), hstarts) and len(kept) == int(hm.sum()) and hat.max() < len(kept)
    hcdf, want = cdf.numpy(), np.zeros(rays * M, np.int64)
    for r in range(rays):
        v = hw[r * S:(r + 1) * S][hm[r * S:(r + 1) * S]]
        c = np.cumsum(v.astype(np.float64)).astype(np.float32)    # exact: see above
        assert np.array_equal(hcdf[hstarts[r]:hstarts[r] + v.size], c) and np.all(np.diff(c) > 0)
        k = np.searchsorted(c, hu[r * M:(r + 1) * M], "right")
        assert v.size == 0 or np.all(k < v.size)                   # xi < 1: inside the ray
        want[r * M:(r + 1) * M] = hstarts[r] + k
    assert np.array_equal(hat, want.astype(np.uint32))
    assert np.array_equal(picked.numpy(), np.flatnonzero(hm)[want].astype(np.uint32))
