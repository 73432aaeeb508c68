"""segment_psum in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`): every flat arithmetic type, the
tape node -- the adjoint of a prefix sum inside ragged segments is the same scan from the other end with `exclusive` kept, so
gradient(x) of hsum(w * segment_psum(x, starts)) IS segment_psum(w, starts, reverse flipped) and compared bit for bit -- and the
README example, the transmittance in front of every sample that compress() left of a ray.

Float prefix sums are compared with float64 prefix sums under the order-independent bound gamma_k * sum |x_i| over the k + 1 terms
of a prefix, gamma_k = k u / (1 - k u), u = 2^-24 or 2^-53 (any order of k additions)."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

TYPES = [("Float32", np.float32), ("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 0, 0, 257, 1025, 5, 9000, 1, 0]
MODES = [(False, False), (True, False), (False, True), (True, True)]          # (exclusive, reverse)


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


def prefix_sums(h, starts, excl, rev, acc=None):
    """np.cumsum per clamped segment (reversed for `rev`, shifted for `excl`), +0 outside the segments"""
    n = h.size
    out = np.zeros(n, acc or h.dtype)
    s = np.minimum(starts.astype(np.int64), n)
    e = np.maximum(s, np.concatenate([s[1:], [n]]))
    for a, b in zip(s, e):
        if b > a:
            seg = h[a:b].astype(out.dtype)
            c = np.cumsum(seg[::-1] if rev else seg, dtype=out.dtype)
            if excl:
                c = np.concatenate([np.zeros(1, out.dtype), c[:-1]])
            out[a:b] = c[::-1] if rev else c
    return out


def gamma_bounds(h, starts, excl, rev):
    u = 2.0 ** -24 if h.dtype == np.float32 else 2.0 ** -53
    k = np.maximum(prefix_sums(np.ones(h.size, np.float64), starts, excl, rev) - 1, 0)
    return k * u / (1 - k * u) * prefix_sums(np.abs(h.astype(np.float64)), starts, excl, rev)


def test_every_flat_type_of_both_modules(ekc, ad):
    import enoki as ek
    rng = np.random.default_rng(1)
    starts, n = starts_of(LENGTHS, 4)
    for mod in (ekc, ad):
        st = mod.UInt32(starts)
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            h = rng.integers(0, 17, n).astype(dt) if np.dtype(dt).kind == "u" else rng.integers(-8, 9, n).astype(dt)
            x = A(h)
            for excl, rev in MODES:
                want = prefix_sums(h, starts, excl, rev)
                got = mod.segment_psum(x, st, exclusive=excl, reverse=rev)
                assert type(got) is A and len(got) == n and bits_equal(got.numpy(), want), (cls, excl, rev)
                assert bits_equal(ek.segment_psum(x, starts=st, exclusive=excl, reverse=rev).numpy(), want), (cls, excl, rev)
            assert bits_equal(mod.segment_psum(x, st).numpy(), prefix_sums(h, starts, False, False)), cls      # the defaults
            if cls != "UInt32":
                with pytest.raises(TypeError):
                    mod.segment_psum(x, x)                        # the starts are a UInt32 array
            assert bits_equal(mod.segment_psum(x, mod.UInt32(np.zeros(0, np.uint32))).numpy(), np.zeros(n, dt))      # no segment
            assert len(mod.segment_psum(A(h[:0]), st)) == 0


@pytest.mark.parametrize("cls,dt", TYPES[:2])
@pytest.mark.parametrize("shape", ["short", "mixed", "long"])
def test_the_adjoint_is_the_scan_from_the_other_end(ekc, ad, cls, dt, shape):
    rng = np.random.default_rng(len(shape))
    lengths = {"short": rng.integers(0, 9, 3000), "mixed": LENGTHS * 3, "long": [70000, 3, 0, 40000]}[shape]
    starts, n = starts_of(lengths, 3)                             # a gap in front, empty segments in between
    A, P = getattr(ad, cls), getattr(ekc, cls)
    st, pst = ad.UInt32(starts), ekc.UInt32(starts)
    hx, hw, hv = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    for excl, rev in MODES:
        # backward: gradient(x) == segment_psum(w, starts, reverse flipped, exclusive kept) of the plain module
        x, w = A(hx), A(hw)
        ad.set_requires_gradient(x)
        p = ad.segment_psum(x, st, exclusive=excl, reverse=rev)
        assert ad.requires_gradient(p) and len(p) == n
        err = np.abs(ad.detach(p).numpy().astype(np.float64) - prefix_sums(hx, starts, excl, rev, acc=np.float64))
        assert np.all(err <= gamma_bounds(hx, starts, excl, rev))
        ad.backward(ad.hsum(p * w))
        g = ad.gradient(x).numpy()
        assert bits_equal(g, ekc.segment_psum(P(hw), pst, exclusive=excl, reverse=not rev).numpy()), (excl, rev)
        assert np.all(g[:3] == 0) and not np.any(np.signbit(g[:3]))          # in front of every segment
        assert not ad.requires_gradient(st)
        # forward: the node's own scan of what reaches its source -- v, as the derivative of x = v * t by the one-entry t
        t = A(np.ones(1, dt))
        ad.set_requires_gradient(t)
        p = ad.segment_psum(A(hv) * t, st, exclusive=excl, reverse=rev)
        ad.forward(t)
        assert bits_equal(ad.gradient(p).numpy(), ekc.segment_psum(P(hv), pst, exclusive=excl, reverse=rev).numpy()), (excl, rev)
        # the size-1 seeds of backward(hsum(..)) and forward(x) stand for n ones: the number of terms on either side, exactly
        x = A(hx)
        ad.set_requires_gradient(x)
        ad.backward(ad.hsum(ad.segment_psum(x, st, exclusive=excl, reverse=rev)))
        assert bits_equal(ad.gradient(x).numpy(), prefix_sums(np.ones(n, dt), starts, excl, not rev)), (excl, rev)
        x = A(hx)
        ad.set_requires_gradient(x)
        p = ad.segment_psum(x, st, exclusive=excl, reverse=rev)
        ad.forward(x)
        assert bits_equal(ad.gradient(p).numpy(), prefix_sums(np.ones(n, dt), starts, excl, rev)), (excl, rev)


@pytest.mark.parametrize("keep", [0.0, 0.3, 1.0])
def test_transmittance_after_compress_end_to_end(ekc, keep):
    """the README example: compress() drops the culled samples of every ray, the counts per ray become starts through an exclusive
    block_psum, and T = exp(-segment_psum(sigma * dt of the kept samples, starts, exclusive=True)) is the transmittance in front of
    every kept sample -- against a numpy loop over the rays.  With tau the float64 optical depth and |tau_hat - tau| <= b (the gamma
    bound of the prefix), exp(-tau_hat) = exp(-tau) * exp(tau - tau_hat), so |T_hat - T| <= T * (exp(b) - 1) before the rounding
    of float32 exp itself, which is given 4 ulp of T here (the library's exp is within 2 ulp, numpy's float64 exp is the truth)."""
    rng = np.random.default_rng(int(keep * 10) + 1)
    rays, S = 3001, 64
    h = (rng.random(rays * S) * 0.1).astype(np.float32)           # sigma * dt per sample
    hm = rng.random(rays * S) < keep
    x, mask = ekc.Float32(h), ekc.Mask(hm)
    kept = ekc.compress(x, mask)
    counts = ekc.block_sum(ekc.select(mask, ekc.UInt32.full(1, rays * S), ekc.UInt32.zero(rays * S)), S)
    starts = ekc.block_psum(counts, len(counts), exclusive=True)
    per_ray = hm.reshape(rays, S).sum(axis=1)
    assert np.array_equal(starts.numpy(), np.concatenate([[0], np.cumsum(per_ray)[:-1]]))
    tau = ekc.segment_psum(kept, starts, exclusive=True)
    assert len(tau) == len(kept) == int(hm.sum())
    if len(kept) == 0:
        return                                                    # (nothing kept: an empty array, as from block_psum; no arithmetic on it)
    T = ekc.exp(-tau).numpy()
    want, bound = np.zeros(T.size), np.zeros(T.size)
    u, at = 2.0 ** -24, 0
    for r in range(rays):
        v = h[r * S:(r + 1) * S][hm[r * S:(r + 1) * S]].astype(np.float64)
        if v.size:
            tau = np.concatenate([[0.0], np.cumsum(v)[:-1]])
            k = np.maximum(np.arange(v.size) - 1, 0)
            b = k * u / (1 - k * u) * tau                         # (all terms are positive: sum |x| is tau itself)
            want[at:at + v.size] = np.exp(-tau)
            bound[at:at + v.size] = np.exp(-tau) * np.expm1(b) + 4 * u * np.exp(-tau)
            at += v.size
    assert at == T.size and np.all(np.abs(T.astype(np.float64) - want) <= bound)
    if T.size:
        first = starts.numpy()[per_ray > 0]
        assert np.all(T[first] == 1.0)                            # nothing in front of a ray's first kept sample
