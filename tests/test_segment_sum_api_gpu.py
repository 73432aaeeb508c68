"""segment_sum / segment_prod / segment_min / segment_max / segment_repeat in the python modules (enoki_amd.hip,
enoki_amd.hip_autodiff, `import enoki`): every flat arithmetic type, the refusal of values that do not match the starts, and the two
tape nodes -- segment_sum and segment_repeat over the same starts are each other's transpose, so the gradients below are exact
copies of the weights and compared bit for bit.

Float sums are compared with float64 sums under the order-independent bound gamma_(L-1) * sum |x_i| per segment of L entries,
gamma_k = k u / (1 - k u), u = 2^-24 or 2^-53 (any order of L - 1 additions)."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

TYPES = [("Float32", np.float32), ("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 0, 0, 257, 1025, 5, 3000, 1, 0]


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


def segments(h, starts, fn, empty):
    """fn over every segment of h in numpy, `empty` for an empty one"""
    n = h.size
    s = np.minimum(starts.astype(np.int64), n)
    e = np.maximum(s, np.concatenate([s[1:], [n]]))
    return np.array([fn(h[a:b]) if b > a else empty for a, b in zip(s, e)], h.dtype)


def repeated(v, starts, size):
    j = np.searchsorted(starts, np.arange(size, dtype=np.int64), side="right")
    out = np.zeros(size, v.dtype)
    out[j > 0] = v[j[j > 0] - 1]
    return out


def gamma_bounds(h, starts):
    u = 2.0 ** -24 if h.dtype == np.float32 else 2.0 ** -53
    k = np.maximum(segments(np.ones(h.size, np.float64), starts, np.sum, 0.0) - 1, 0)
    return k * u / (1 - k * u) * segments(np.abs(h.astype(np.float64)), starts, np.sum, 0.0)


def test_every_flat_type_of_both_modules(ekc, ad):
    import enoki as ek
    rng = np.random.default_rng(1)
    starts, n = starts_of(LENGTHS, 4)
    m = starts.size
    for mod in (ekc, ad):
        st = mod.UInt32(starts)
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            unsigned = np.dtype(dt).kind == "u"
            h = rng.integers(0, 17, n).astype(dt) if unsigned else rng.integers(-8, 9, n).astype(dt)
            x = A(h)
            if np.dtype(dt).kind == "f":
                lowest, highest = np.nan, np.nan
            else:
                lowest, highest = np.iinfo(dt).min, np.iinfo(dt).max
            for fn, want in (("segment_sum", segments(h, starts, lambda s: s.sum(dtype=dt), 0)),
                             ("segment_min", segments(h, starts, np.min, highest)), ("segment_max", segments(h, starts, np.max, lowest))):
                got = getattr(mod, fn)(x, st)
                assert type(got) is A and len(got) == m and bits_equal(got.numpy(), want), (cls, fn)
                assert bits_equal(getattr(ek, fn)(x, starts=st).numpy(), want), (cls, fn)
            ones_h = (h % 3 + 1).astype(dt) if unsigned else np.where(h % 2 == 0, 1, -1).astype(dt)
            want = segments(ones_h, starts, lambda s: np.multiply.reduce(s, dtype=dt), 1)
            assert bits_equal(mod.segment_prod(A(ones_h), st).numpy(), want), cls
            assert bits_equal(ek.segment_prod(A(ones_h), st).numpy(), want), cls
            v = h[:m]
            for size in (n, n - 100, n + 9):
                rep = mod.segment_repeat(A(v), st, size)
                assert type(rep) is A and bits_equal(rep.numpy(), repeated(v, starts, size)), (cls, size)
            assert bits_equal(ek.segment_repeat(A(v), starts=st, size=n).numpy(), repeated(v, starts, n)), cls
            with pytest.raises(Exception, match="do not match"):
                mod.segment_repeat(x, st, n)                      # n values, m starts
            if cls != "UInt32":
                with pytest.raises(TypeError):
                    mod.segment_sum(x, x)                         # the starts are a UInt32 array
            assert len(mod.segment_sum(x, mod.UInt32(np.zeros(0, np.uint32)))) == 0


@pytest.mark.parametrize("cls,dt", TYPES[:2])
@pytest.mark.parametrize("shape", ["short", "mixed", "long"])
def test_segment_sum_and_segment_repeat_are_transposes_on_the_tape(ekc, ad, cls, dt, shape):
    rng = np.random.default_rng(len(shape))
    lengths = {"short": rng.integers(0, 9, 3000), "mixed": LENGTHS * 5, "long": [70000, 3, 0, 40000]}[shape]
    starts, n = starts_of(lengths, 3)
    m = starts.size
    A, P = getattr(ad, cls), getattr(ekc, cls)
    st, pst = ad.UInt32(starts), ekc.UInt32(starts)
    hx, hw, hv = rng.standard_normal(n).astype(dt), rng.standard_normal(m).astype(dt), rng.standard_normal(n).astype(dt)
    # backward through segment_sum: gradient(x) == segment_repeat(w, starts, n)
    x, w = A(hx), A(hw)
    ad.set_requires_gradient(x)
    s = ad.segment_sum(x, st)
    assert ad.requires_gradient(s) and len(s) == m
    want = segments(hx.astype(np.float64), starts, np.sum, 0.0)
    assert np.all(np.abs(ad.detach(s).numpy().astype(np.float64) - want) <= gamma_bounds(hx, starts))
    ad.backward(ad.hsum(s * w))
    assert bits_equal(ad.gradient(x).numpy(), ekc.segment_repeat(P(hw), pst, n).numpy())
    assert bits_equal(ad.gradient(x).numpy(), repeated(hw, starts, n))
    # backward through segment_repeat: gradient(a) == segment_sum(v) of the plain module
    a, v = A(hw), A(hv)
    ad.set_requires_gradient(a)
    r = ad.segment_repeat(a, st, n)
    assert ad.requires_gradient(r) and len(r) == n and bits_equal(ad.detach(r).numpy(), repeated(hw, starts, n))
    ad.backward(ad.hsum(r * v))
    assert bits_equal(ad.gradient(a).numpy(), ekc.segment_sum(P(hv), pst).numpy())
    # forward through segment_sum: the seed of forward(x) stands for n ones (a size-1 seed), so every segment gets its length
    x = A(hx)
    ad.set_requires_gradient(x)
    s = ad.segment_sum(x, st)
    ad.forward(x)
    assert bits_equal(ad.gradient(s).numpy(), segments(np.ones(n, dt), starts, np.sum, 0))
    # ... and through segment_repeat: one wherever there is a segment, zero in front of the first start
    a = A(hw)
    ad.set_requires_gradient(a)
    r = ad.segment_repeat(a, st, n)
    ad.forward(a)
    assert bits_equal(ad.gradient(r).numpy(), repeated(np.ones(m, dt), starts, n))
    # the size-1 seed of backward(hsum(segment_sum(x))): the same ones
    x = A(hx)
    ad.set_requires_gradient(x)
    ad.backward(ad.hsum(ad.segment_sum(x, st)))
    assert bits_equal(ad.gradient(x).numpy(), repeated(np.ones(m, dt), starts, n))


def test_the_other_three_have_no_gradient(ad):
    h = np.random.default_rng(2).standard_normal(640).astype(np.float32)
    starts = np.array([0, 10, 10, 300, 639], np.uint32)
    x, st = ad.Float32(h), ad.UInt32(starts)
    for fn, np_fn in (("segment_max", np.max), ("segment_min", np.min), ("segment_prod", None)):
        got = getattr(ad, fn)(x, st)                                 # untracked: computes
        assert not ad.requires_gradient(got) and len(got) == 5
        if np_fn is not None:
            assert bits_equal(got.numpy(), segments(h, starts, np_fn, np.float32(np.nan))), fn
    ad.set_requires_gradient(x)
    for fn in ("segment_max", "segment_min", "segment_prod"):
        with pytest.raises(Exception, match="gradients not implemented"):
            getattr(ad, fn)(x, st)


@pytest.mark.parametrize("cls,dt", [("Float32", np.float32), ("Int32", np.int32)])
@pytest.mark.parametrize("keep", [0.0, 0.3, 1.0])
def test_culled_samples_per_ray_end_to_end(ekc, cls, dt, keep):
    """the README pipeline: compress() drops the culled samples of every ray, the counts per ray become starts through an exclusive
    block_psum, segment_sum sums what is left per ray -- next to scatter_add over search_sorted(starts, arange(n), right) - 1"""
    rng = np.random.default_rng(int(keep * 10) + 1)
    rays, S = 3001, 64
    A = getattr(ekc, cls)
    h = rng.standard_normal(rays * S).astype(dt) if np.dtype(dt).kind == "f" else rng.integers(-1000, 1000, rays * S).astype(dt)
    hm = rng.random(rays * S) < keep
    x, mask = A(h), ekc.Mask(hm)
    kept = ekc.compress(x, mask)
    counts = ekc.block_sum(ekc.select(mask, ekc.UInt32.full(1, rays * S), ekc.UInt32.zero(rays * S)), S)
    starts = ekc.block_psum(counts, len(counts), exclusive=True)
    assert np.array_equal(starts.numpy(), np.concatenate([[0], np.cumsum(hm.reshape(rays, S).sum(axis=1))[:-1]]))
    got = ekc.segment_sum(kept, starts).numpy()
    assert len(kept) == int(hm.sum()) and got.size == rays
    # the spelling it replaces
    target = A.zero(rays)
    if len(kept):
        seg_id = ekc.search_sorted(starts, ekc.UInt32.arange(len(kept)), right=True) - ekc.UInt32.full(1, len(kept))
        ekc.scatter_add(target, kept, seg_id)
    old = target.numpy()
    h2 = np.where(hm, h, 0).reshape(rays, S)
    if np.dtype(dt).kind != "f":
        assert np.array_equal(got, h2.sum(axis=1, dtype=dt)) and np.array_equal(old, got)
    else:
        u = 2.0 ** -24
        k = np.maximum(hm.reshape(rays, S).sum(axis=1) - 1, 0)
        truth, bound = h2.astype(np.float64).sum(axis=1), k * u / (1 - k * u) * np.abs(h2.astype(np.float64)).sum(axis=1)
        assert np.all(np.abs(got.astype(np.float64) - truth) <= bound) and np.all(np.abs(old.astype(np.float64) - truth) <= bound)
    # and back: every kept sample gets its ray's value
    w = A(np.arange(1, rays + 1).astype(dt))
    back = ekc.segment_repeat(w, starts, len(kept)).numpy()
    assert np.array_equal(back, np.repeat(np.arange(1, rays + 1), hm.reshape(rays, S).sum(axis=1)).astype(dt))
