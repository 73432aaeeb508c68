"""block_psum in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`): values against the C-ABI call, the
refusal of a size that is no multiple of the block, keyword names, and the tape node.  The adjoint of a per-block prefix sum is the
same scan from the other end of each block (`exclusive` kept), computed by the same kernel on the same data: the gradients below are
compared with a direct block_psum of the weights bit for bit, no tolerance."""
import itertools

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

TYPES = [("Float32", np.float32), ("Float64", np.float64), ("Int32", np.int32), ("UInt32", np.uint32), ("Int64", np.int64), ("UInt64", np.uint64)]
FLAGS = list(itertools.product((False, True), (False, True)))          # (exclusive, reverse)


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


def host_data(dt, n, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dt).kind == "f":
        return rng.standard_normal(n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def test_values_match_the_c_abi(capi, ekc, ad):
    import enoki as ek
    B, m = 100, 173
    for mod, classes in ((ekc, ("Float32", "Float64", "Int32", "UInt64")), (ad, ("Float32", "Float64", "Int32", "UInt64"))):
        for cls in classes:
            dt = dict(TYPES)[cls]
            A = getattr(mod, cls)
            h = host_data(dt, m * B, 3)
            x = A(h)
            for excl, rev in FLAGS:
                want = capi.psum_blocks(capi.Buf.from_numpy(h), B, excl, rev).numpy()
                got = mod.block_psum(x, B, exclusive=excl, reverse=rev)
                assert type(got) is A and bits_equal(got.numpy(), want), (cls, excl, rev)
                assert bits_equal(ek.block_psum(array=x, block=B, exclusive=excl, reverse=rev).numpy(), want), (cls, excl, rev)
            assert bits_equal(mod.block_psum(x, B).numpy(), capi.psum_blocks(capi.Buf.from_numpy(h), B).numpy()), cls
            assert bits_equal(mod.block_psum(x, B, True).numpy(), capi.psum_blocks(capi.Buf.from_numpy(h), B, True).numpy()), cls


def test_every_flat_type_of_both_modules(ekc, ad):
    B, m = 5, 1001
    for mod in (ekc, ad):
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            h = np.random.default_rng(1).integers(0, 9, m * B).astype(dt)
            want = np.cumsum(h.reshape(m, B), axis=1, dtype=dt)
            assert bits_equal(mod.block_psum(A(h), B).numpy(), want.reshape(-1)), cls
            rwant = np.cumsum(h.reshape(m, B)[:, ::-1], axis=1, dtype=dt)[:, ::-1]
            assert bits_equal(mod.block_psum(A(h), B, reverse=True).numpy(), rwant.reshape(-1)), cls
            for bad in (0, 8, m * B + 1):                           # (m * B = 5005 = 5 * 7 * 11 * 13)
                with pytest.raises(Exception):
                    mod.block_psum(A(h), bad)
            with pytest.raises(TypeError):
                mod.block_psum(A(h), B, inclusive=True)


@pytest.mark.parametrize("cls,dt", TYPES[:2])
@pytest.mark.parametrize("B", [100, 1025 + 4096 * 2])
def test_the_adjoint_is_the_scan_from_the_other_end(ekc, ad, cls, dt, B):
    m = 37 if B < 1024 else 3
    n = m * B
    A, P = getattr(ad, cls), getattr(ekc, cls)
    hx, hw = host_data(dt, n, B), host_data(dt, n, B + 1)
    for excl, rev in FLAGS:
        x, w = A(hx), A(hw)
        ad.set_requires_gradient(x)
        s = ad.block_psum(x, B, exclusive=excl, reverse=rev)
        assert ad.requires_gradient(s) and len(s) == n
        assert bits_equal(ad.detach(s).numpy(), ekc.block_psum(P(hx), B, exclusive=excl, reverse=rev).numpy())
        ad.backward(ad.hsum(w * s))
        assert bits_equal(ad.gradient(x).numpy(), ekc.block_psum(P(hw), B, exclusive=excl, reverse=not rev).numpy()), (excl, rev)
        # forward mode: the seed of forward(x) stands for n ones
        x = A(hx)
        ad.set_requires_gradient(x)
        s = ad.block_psum(x, B, exclusive=excl, reverse=rev)
        ad.forward(x)
        assert bits_equal(ad.gradient(s).numpy(), ekc.block_psum(P(np.ones(n, dt)), B, exclusive=excl, reverse=rev).numpy()), (excl, rev)


def test_transmittance_end_to_end(ekc, ad):
    """T = exp(-block_psum(sigma * dt, S, exclusive=True)): the first sample of every ray sees T = 1, and the gradient of hsum(T)
    with respect to sigma is -dt * (sum of T over the samples behind), the reverse exclusive scan"""
    rays, S = 257, 64
    rng = np.random.default_rng(4)
    hs = rng.uniform(0.1, 2.0, rays * S).astype(np.float32)
    step = 0.03125                                           # (a power of two: sigma * dt and its adjoint are exact products)
    sigma = ad.Float32(hs)
    ad.set_requires_gradient(sigma)
    T = ad.exp(-ad.block_psum(sigma * step, S, exclusive=True))
    t = ad.detach(T).numpy().reshape(rays, S)
    assert np.all(t[:, 0] == 1.0) and np.all(np.diff(t, axis=1) < 0)
    ad.backward(ad.hsum(T))
    # d hsum(T) / d tau = -T, scanned from the other end, times dt.  The terms of every sum have one sign, so a relative error of
    # delta in the terms is one of delta in the sum: 2^-20 leaves the adjoint of exp eight roundings of its own
    want = ekc.block_psum(ekc.Float32(-t.reshape(-1)), S, exclusive=True, reverse=True).numpy().astype(np.float64) * step
    got = ad.gradient(sigma).numpy().astype(np.float64)
    assert np.all(want.reshape(rays, S)[:, -1] == 0) and np.all(got.reshape(rays, S)[:, -1] == 0)
    assert np.all(np.abs(got - want) <= 2.0 ** -20 * np.abs(want))
