"""block_sum / block_prod / block_min / block_max / repeat in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`):
every flat arithmetic type, the refusal of a size that is no multiple of the block, and the two tape nodes -- block_sum and repeat
are each other's transpose, so the gradients below are exact copies of the weights and compared bit for bit.

Float sums are compared with float64 sums under the order-independent bound gamma_(B-1) * sum |x_i|, gamma_k = k u / (1 - k u)
(one more rounding, gamma_B, where the sum is multiplied by a factor afterwards)."""
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


def gamma(k, dt):
    u = 2.0 ** -24 if np.dtype(dt) == np.float32 else 2.0 ** -53
    return k * u / (1 - k * u)


def test_every_flat_type_of_both_modules(ekc, ad):
    import enoki as ek
    rng = np.random.default_rng(1)
    B, m = 5, 1001
    for mod in (ekc, ad):
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            h = rng.integers(-8, 9, m * B).astype(dt) if np.dtype(dt).kind != "u" else rng.integers(0, 17, m * B).astype(dt)
            x, h2 = A(h), h.reshape(m, B)
            for fn, want in (("block_sum", h2.sum(axis=1, dtype=dt)), ("block_min", h2.min(axis=1)), ("block_max", h2.max(axis=1))):
                got = getattr(mod, fn)(x, B)
                assert type(got) is A and bits_equal(got.numpy(), want), (cls, fn)
                assert bits_equal(getattr(ek, fn)(x, block=B).numpy(), want), (cls, fn)
            ones = A(np.where(h % 2 == 0, 1, -1).astype(dt) if np.dtype(dt).kind != "u" else (h % 3 + 1).astype(dt))
            assert bits_equal(mod.block_prod(ones, B).numpy(), np.multiply.reduce(ones.numpy().reshape(m, B), axis=1, dtype=dt)), cls
            rep = mod.repeat(A(h[:m]), B)
            assert type(rep) is A and bits_equal(rep.numpy(), np.repeat(h[:m], B)), cls
            assert bits_equal(ek.repeat(A(h[:m]), B).numpy(), np.repeat(h[:m], B)), cls
            for bad in (0, 8, m * B + 1):                           # (m * B = 5005 = 5 * 7 * 11 * 13)
                with pytest.raises(Exception):
                    mod.block_sum(x, bad)
            with pytest.raises(Exception):
                mod.repeat(x, 0)


@pytest.mark.parametrize("cls,dt", TYPES[:2])
@pytest.mark.parametrize("B", [3, 64, 1000])
def test_block_sum_and_repeat_are_transposes_on_the_tape(ekc, ad, cls, dt, B):
    rng = np.random.default_rng(B)
    m = 257
    n = m * B
    A, P = getattr(ad, cls), getattr(ekc, cls)
    hx, hw, hv = rng.standard_normal(n).astype(dt), rng.standard_normal(m).astype(dt), rng.standard_normal(n).astype(dt)
    # backward through block_sum: gradient(x) == repeat(w)
    x, w = A(hx), A(hw)
    ad.set_requires_gradient(x)
    s = ad.block_sum(x, B)
    assert ad.requires_gradient(s) and len(s) == m
    want = hx.reshape(m, B).astype(np.float64).sum(axis=1)
    assert np.all(np.abs(ad.detach(s).numpy().astype(np.float64) - want) <= gamma(B - 1, dt) * np.abs(hx.reshape(m, B).astype(np.float64)).sum(axis=1))
    ad.backward(ad.hsum(s * w))
    assert bits_equal(ad.gradient(x).numpy(), ekc.repeat(P(hw), B).numpy())
    assert bits_equal(ad.gradient(x).numpy(), np.repeat(hw, B))
    # backward through repeat: gradient(a) == block_sum(v) of the plain module
    a, v = A(hw), A(hv)
    ad.set_requires_gradient(a)
    r = ad.repeat(a, B)
    assert ad.requires_gradient(r) and len(r) == n and bits_equal(ad.detach(r).numpy(), np.repeat(hw, B))
    ad.backward(ad.hsum(r * v))
    assert bits_equal(ad.gradient(a).numpy(), ekc.block_sum(P(hv), B).numpy())
    # forward through block_sum: the seed of forward(x) stands for n ones, B of them per block
    x = A(hx)
    ad.set_requires_gradient(x)
    s = ad.block_sum(x, B)
    ad.forward(x)
    assert bits_equal(ad.gradient(s).numpy(), np.full(m, B, dt))
    # ... and through repeat: ones
    a = A(hw)
    ad.set_requires_gradient(a)
    r = ad.repeat(a, B)
    ad.forward(a)
    assert bits_equal(ad.gradient(r).numpy(), np.ones(n, dt))


def test_the_other_three_have_no_gradient(ad):
    h = np.random.default_rng(2).standard_normal(640).astype(np.float32)
    x = ad.Float32(h)
    for fn, want in (("block_max", h.reshape(10, 64).max(axis=1)), ("block_min", h.reshape(10, 64).min(axis=1)),
                     ("block_prod", None)):
        got = getattr(ad, fn)(x, 64)                                 # untracked: computes
        assert not ad.requires_gradient(got) and len(got) == 10
        if want is not None:
            assert bits_equal(got.numpy(), want), fn
    ad.set_requires_gradient(x)
    for fn in ("block_max", "block_min", "block_prod"):
        with pytest.raises(Exception, match="gradients not implemented"):
            getattr(ad, fn)(x, 64)


@pytest.mark.parametrize("spp", [3, 64, 1000])
def test_samples_per_pixel_end_to_end(ad, spp):
    """img = block_sum(sin(s * t), spp) / spp and the gradient of hsum(img^2) w.r.t. t, next to the scatter_add / gather spelling"""
    rng = np.random.default_rng(spp)
    pixels = 1025
    n = pixels * spp
    hs, ht = rng.uniform(0.5, 2.0, n).astype(np.float32), rng.uniform(-1.0, 1.0, n).astype(np.float32)
    idx = ad.UInt32((np.arange(n) // spp).astype(np.uint32))
    inv = np.float32(1.0 / spp)

    def program(spelling):
        s, t = ad.Float32(hs), ad.Float32(ht)
        ad.set_requires_gradient(t)
        x = ad.sin(s * t)
        if spelling == "block_sum":
            img = ad.block_sum(x, spp) * float(inv)
        else:
            img = ad.Float32(np.zeros(pixels, np.float32))
            ad.scatter_add(img, x, idx)
            img = img * float(inv)
        ad.backward(ad.hsum(img * img))
        return ad.detach(x).numpy(), ad.detach(img).numpy(), ad.gradient(t).numpy()

    x1, img1, g1 = program("block_sum")
    x2, img2, g2 = program("scatter_add")
    assert bits_equal(x1, x2)
    # values: both within gamma_spp * sum |x| * inv of the float64 sum of the same float32 terms (spp - 1 additions, one product)
    x64 = x1.reshape(pixels, spp).astype(np.float64)
    truth, bound = x64.sum(axis=1) * float(inv), gamma(spp, np.float32) * np.abs(x64).sum(axis=1) * float(inv)
    assert np.all(np.abs(img1.astype(np.float64) - truth) <= bound)
    assert np.all(np.abs(img2.astype(np.float64) - truth) <= bound)
    # gradients: each is the exact broadcast of 2 * img * inv times the same factors cos(s t) * s -- bit for bit wherever the two
    # images agree bit for bit.  A pixel whose sums differ (another summation order: at most 2 * bound apart) hands a different
    # factor to its samples; those gradients then differ by that much times |d x / d t| <= |s|, plus the roundings of the three
    # products behind each (gamma_3 of either value).
    same = np.repeat(img1.view(np.uint32) == img2.view(np.uint32), spp)
    assert bits_equal(g1[same], g2[same])
    if not same.all():
        slack = np.repeat(2.0 * float(inv) * 2.0 * bound, spp) * np.abs(hs.astype(np.float64)) + gamma(3, np.float32) * (np.abs(g1) + np.abs(g2))
        assert np.all(np.abs(g1.astype(np.float64) - g2.astype(np.float64))[~same] <= slack[~same])
    want = np.repeat(2.0 * img1.astype(np.float64) * float(inv), spp) * np.cos(hs.astype(np.float64) * ht.astype(np.float64)) * hs
    assert np.allclose(g1, want, rtol=1e-4, atol=1e-6)
