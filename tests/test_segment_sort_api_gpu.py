"""segment_sort / segment_argsort in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`): all six flat types
against numpy's stable argsort per clamped segment, keyword names, docstrings, and the tape node.  The adjoint of a sort is a scatter
through its permutation and the forward derivative a gather: both move bits, so the gradient identities below are compared bit for
bit, no tolerance.  Then the pipeline the call is for: segment_psum made ascending on the device and searched by
segment_search_sorted, and another array reordered along by gather(.., segment_argsort(.., flat=True))."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

TYPES = [("Float32", np.float32), ("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)]


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


def host_data(dt, n, seed, ties=False):
    rng = np.random.default_rng(seed)
    if ties:
        return rng.integers(0, 5, n).astype(dt)
    if np.dtype(dt).kind == "f":
        return rng.standard_normal(n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def ragged(n, seed, longest=90):
    """ascending starts with a prefix, empty segments, one segment of several thousand entries and starts above n"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest, n // 30)
    lens[::7] = 0
    lens[5] = 5000
    s = 13 + np.concatenate([[0], np.cumsum(lens)])
    return s[s < n + 200].astype(np.uint32)


def reference(h, starts, descending=False):
    """(segment-local permutation, flat permutation, sorted values) by numpy's stable argsort per clamped segment"""
    n = h.size
    flat = np.arange(n, dtype=np.int64)
    local = np.arange(n, dtype=np.int64)
    lo = np.minimum(starts.astype(np.int64), n)
    hi = np.maximum(lo, np.append(lo[1:], n))
    key = h if not descending else (-h if h.dtype.kind == "f" else ~h)
    for a, b in zip(lo, hi):
        if b > a:
            p = np.argsort(key[a:b], kind="stable")
            flat[a:b] = a + p
            local[a:b] = p
    return local.astype(np.uint32), flat.astype(np.uint32), h[flat]


def test_every_flat_type_of_both_modules(ekc, ad):
    import enoki as ek
    n = 12011
    hs = ragged(n, 1)
    assert hs[0] > 0 and (hs > n).any() and (np.diff(hs.astype(np.int64)) > 4096).any()
    for mod in (ekc, ad):
        starts = mod.UInt32(hs)
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            for ties in (False, True):
                h = host_data(dt, n, 3, ties)
                if np.dtype(dt).kind == "f":
                    h[::11] = np.nan
                    h[5::13] = -0.0
                x = A(h)
                for desc in (False, True):
                    p, flat, vals = reference(h, hs, desc)
                    s = mod.segment_sort(x, starts, descending=desc)
                    assert type(s) is A and bits_equal(s.numpy(), vals), (cls, desc)
                    q = mod.segment_argsort(x, starts, descending=desc)
                    assert type(q) is mod.UInt32 and np.array_equal(q.numpy(), p), (cls, desc)
                    assert np.array_equal(mod.segment_argsort(x, starts, descending=desc, flat=True).numpy(), flat), (cls, desc)
                    assert np.array_equal(mod.segment_argsort(x, starts, desc, True).numpy(), flat), (cls, desc)
                    assert bits_equal(ek.segment_sort(array=x, starts=starts, descending=desc).numpy(), vals), (cls, desc)
                    assert np.array_equal(ek.segment_argsort(array=x, starts=starts, descending=desc, flat=False).numpy(), p), (cls, desc)
                assert bits_equal(mod.segment_sort(x, starts).numpy(), reference(h, hs)[2]), cls
            with pytest.raises(TypeError):
                mod.segment_sort(x, starts, reverse=True)
            with pytest.raises(TypeError):
                mod.segment_argsort(x, starts, local=True)
            with pytest.raises(TypeError):
                mod.segment_sort(x)                                              # the starts are not optional
            assert "stable" in mod.segment_sort.__doc__.lower() and "flat" in mod.segment_argsort.__doc__


@pytest.mark.parametrize("cls,dt", TYPES[:2])
def test_the_adjoint_is_a_scatter_through_the_permutation(ekc, ad, cls, dt):
    n = 12011
    hs = ragged(n, 2)
    A = getattr(ad, cls)
    hx, hw, hv = host_data(dt, n, 4), host_data(dt, n, 5), host_data(dt, n, 6)
    hx[::7] = hx[3]                                                     # ties: stability decides the permutation
    starts = ad.UInt32(hs)
    for desc in (False, True):
        p = reference(hx, hs, desc)[1]
        x, w = A(hx), A(hw)
        ad.set_requires_gradient(x)
        s = ad.segment_sort(x, starts, descending=desc)
        assert ad.requires_gradient(s) and len(s) == n
        assert bits_equal(ad.detach(s).numpy(), hx[p])
        ad.backward(ad.hsum(w * s))
        want = np.zeros(n, dt)
        want[p] = hw                                                    # the scatter of w through the permutation
        assert bits_equal(ad.gradient(x).numpy(), want), desc
        # forward mode with a seed array: seed[p]
        x = A(hx)
        ad.set_requires_gradient(x)
        s = ad.segment_sort(x, starts, descending=desc)
        ad.set_gradient(x, getattr(ekc, cls)(hv), False)
        A.forward()
        assert bits_equal(ad.gradient(s).numpy(), hv[p]), desc


def test_what_records_no_node(ad):
    n = 5000
    hs = ragged(n, 3, longest=40)[:60]
    hx = host_data(np.float32, n, 9)
    x, starts = ad.Float32(hx), ad.UInt32(hs)
    s = ad.segment_sort(x, starts)                                      # x does not require a gradient
    assert not ad.requires_gradient(s) and bits_equal(s.numpy(), reference(hx, hs)[2])
    ad.set_requires_gradient(x)
    q = ad.segment_argsort(x, starts, flat=True)
    assert type(q) is ad.UInt32 and not ad.requires_gradient(q)
    assert np.array_equal(q.numpy(), reference(hx, hs)[1])


def test_sorted_prefix_sums_are_searchable(ekc):
    """segment_psum -> segment_sort -> segment_search_sorted, all on the device.  Whether the raw float32 prefix sums already ascend
    on this machine does not matter: the sorted ones must, they must be a permutation of the raw ones inside every segment, and the
    search in them must equal numpy.searchsorted on the same sorted segments."""
    rng = np.random.default_rng(5)
    m = 300
    lens = rng.integers(1, 200, m)
    lens[7] = 6000
    hs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32)
    n = int(lens.sum())
    w = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    starts = ekc.UInt32(hs)
    cdf = ekc.segment_psum(ekc.Float32(w), starts)
    srt = ekc.segment_sort(cdf, starts)
    c, s = cdf.numpy(), srt.numpy()
    per = 8
    needle_starts = (np.arange(m) * per).astype(np.uint32)
    needles = np.empty(m * per, np.float32)
    for j in range(m):
        a, b = int(hs[j]), int(hs[j]) + int(lens[j])
        assert np.all(np.diff(s[a:b]) >= 0) and bits_equal(np.sort(c[a:b]), s[a:b])
        needles[j * per:(j + 1) * per] = rng.random(per).astype(np.float32) * s[b - 1]
        needles[j * per] = s[(a + b) // 2]                              # a needle that hits an entry: left and right differ
    for right in (False, True):
        got = ekc.segment_search_sorted(srt, starts, ekc.Float32(needles), needle_starts=ekc.UInt32(needle_starts), right=right).numpy()
        want = np.concatenate([np.searchsorted(s[int(hs[j]):int(hs[j]) + int(lens[j])], needles[j * per:(j + 1) * per],
                                               side="right" if right else "left") for j in range(m)])
        assert np.array_equal(got, want), right


def test_another_array_follows_the_sorted_depths(ekc):
    n = 9001
    hs = ragged(n, 6)
    rng = np.random.default_rng(6)
    t = rng.uniform(0.0, 10.0, n).astype(np.float32)
    t[::5] = t[1]                                                       # ties
    sigma = rng.uniform(0.0, 2.0, n).astype(np.float32)
    starts = ekc.UInt32(hs)
    p = ekc.segment_argsort(ekc.Float32(t), starts, flat=True)
    flat = reference(t, hs)[1]
    assert bits_equal(ekc.gather(ekc.Float32(sigma), p).numpy(), sigma[flat])
    assert bits_equal(ekc.gather(ekc.Float32(t), p).numpy(), ekc.segment_sort(ekc.Float32(t), starts).numpy())
