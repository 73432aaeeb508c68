"""block_sort / block_argsort in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`): all six flat types
against numpy's stable argsort per row, keyword names, the refusal of a length that does not fit, and the tape node.  The adjoint of
a sort is a scatter through its permutation and the forward derivative a gather: both move bits, so the gradient identities below
are compared bit for bit, no tolerance.  Then the pipeline the call is for: block_psum rows made ascending on the device and searched
by block_search_sorted, and another array reordered along by gather(.., block_argsort(.., flat=True))."""
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


def reference(h, B, descending=False):
    """(row-local permutation, flat permutation, sorted values) by numpy's stable argsort per row"""
    x2 = h.reshape(-1, B)
    key = x2 if not descending else (-x2 if x2.dtype.kind == "f" else ~x2)
    p = np.argsort(key, axis=1, kind="stable")
    flat = p + np.arange(x2.shape[0])[:, None] * B
    return p.reshape(-1).astype(np.uint32), flat.reshape(-1).astype(np.uint32), np.take_along_axis(x2, p, axis=1).reshape(-1)


def route3_block(capi, dt):
    chunk = capi.sort_blocks_plan(dt, 4, 2)[2]
    B = 2 * chunk + 5
    assert capi.sort_blocks_plan(dt, 3 * B, B)[0] == 3
    return B


def test_every_flat_type_of_both_modules(ekc, ad):
    import enoki as ek
    B, m = 37, 301
    for mod in (ekc, ad):
        for cls, dt in TYPES:
            A = getattr(mod, cls)
            for ties in (False, True):
                h = host_data(dt, m * B, 3, ties)
                if np.dtype(dt).kind == "f":
                    h[::11] = np.nan
                    h[5::13] = -0.0
                x = A(h)
                for desc in (False, True):
                    p, flat, vals = reference(h, B, desc)
                    s = mod.block_sort(x, B, descending=desc)
                    assert type(s) is A and bits_equal(s.numpy(), vals), (cls, desc)
                    q = mod.block_argsort(x, B, descending=desc)
                    assert type(q) is mod.UInt32 and np.array_equal(q.numpy(), p), (cls, desc)
                    assert np.array_equal(mod.block_argsort(x, B, descending=desc, flat=True).numpy(), flat), (cls, desc)
                    assert np.array_equal(mod.block_argsort(x, B, desc, True).numpy(), flat), (cls, desc)
                    assert bits_equal(ek.block_sort(array=x, block=B, descending=desc).numpy(), vals), (cls, desc)
                    assert np.array_equal(ek.block_argsort(array=x, block=B, descending=desc, flat=False).numpy(), p), (cls, desc)
                assert bits_equal(mod.block_sort(x, B).numpy(), reference(h, B)[2]), cls
            for bad in (0, 8, m * B + 1):                           # (m * B = 11137 = 7 * 37 * 43)
                with pytest.raises(Exception):
                    mod.block_sort(x, bad)
                with pytest.raises(Exception):
                    mod.block_argsort(x, bad)
            with pytest.raises(TypeError):
                mod.block_sort(x, B, reverse=True)
            with pytest.raises(TypeError):
                mod.block_argsort(x, B, local=True)
            assert "stable" in mod.block_sort.__doc__.lower() and "flat" in mod.block_argsort.__doc__


@pytest.mark.parametrize("cls,dt", TYPES[:2])
@pytest.mark.parametrize("long_rows", [False, True], ids=["route1", "route3"])
def test_the_adjoint_is_a_scatter_through_the_permutation(capi, ekc, ad, cls, dt, long_rows):
    B = route3_block(capi, dt) if long_rows else 100
    m = 3 if long_rows else 37
    n = m * B
    A = getattr(ad, cls)
    hx, hw, hv = host_data(dt, n, B), host_data(dt, n, B + 1), host_data(dt, n, B + 2)
    hx[::7] = hx[3]                                                     # ties: stability decides the permutation
    for desc in (False, True):
        p = reference(hx, B, desc)[1]
        x, w = A(hx), A(hw)
        ad.set_requires_gradient(x)
        s = ad.block_sort(x, B, descending=desc)
        assert ad.requires_gradient(s) and len(s) == n
        assert bits_equal(ad.detach(s).numpy(), hx[p])
        ad.backward(ad.hsum(w * s))
        assert bits_equal(ad.gradient(x).numpy()[p], hw), desc          # gradient(x)[p] == w, bit for bit
        # forward mode with a seed array: seed[p]
        x = A(hx)
        ad.set_requires_gradient(x)
        s = ad.block_sort(x, B, descending=desc)
        ad.set_gradient(x, getattr(ekc, cls)(hv), False)
        A.forward()
        assert bits_equal(ad.gradient(s).numpy(), hv[p]), desc


def test_what_records_no_node(ad):
    B, m = 64, 50
    hx = host_data(np.float32, m * B, 9)
    x = ad.Float32(hx)
    s = ad.block_sort(x, B)                                             # x does not require a gradient
    assert not ad.requires_gradient(s) and bits_equal(s.numpy(), reference(hx, B)[2])
    ad.set_requires_gradient(x)
    q = ad.block_argsort(x, B, flat=True)
    assert type(q) is ad.UInt32 and not ad.requires_gradient(q)
    assert np.array_equal(q.numpy(), reference(hx, B)[1])


def test_sorted_prefix_sums_are_searchable(ekc):
    """block_psum -> block_sort -> block_search_sorted, all on the device.  Whether the raw float32 prefix sums already ascend on
    this machine does not matter: the sorted ones must, they must be a permutation of the raw ones, and the search in them must
    equal numpy.searchsorted on the same sorted rows."""
    rows, B, M = 64, 4096, 32
    rng = np.random.default_rng(5)
    w = rng.uniform(1e-3, 1.0, rows * B).astype(np.float32)
    cdf = ekc.block_psum(ekc.Float32(w), B)
    srt = ekc.block_sort(cdf, B)
    c2, s2 = cdf.numpy().reshape(rows, B), srt.numpy().reshape(rows, B)
    assert np.all(np.diff(s2, axis=1) >= 0)
    assert bits_equal(np.sort(c2, axis=1).reshape(-1), s2.reshape(-1))
    needles = (rng.random((rows, M)) * s2[:, -1:]).astype(np.float32)
    needles[:, 0] = s2[:, B // 2]                                       # a needle that hits an entry: left and right differ
    for right in (False, True):
        got = ekc.block_search_sorted(srt, ekc.Float32(needles.reshape(-1)), B, right=right).numpy().reshape(rows, M)
        want = np.stack([np.searchsorted(s2[r], needles[r], side="right" if right else "left") for r in range(rows)])
        assert np.array_equal(got, want), right


def test_another_array_follows_the_sorted_depths(ekc):
    rays, S = 129, 48
    rng = np.random.default_rng(6)
    t = rng.uniform(0.0, 10.0, rays * S).astype(np.float32)
    t[::5] = t[1]                                                       # ties
    sigma = rng.uniform(0.0, 2.0, rays * S).astype(np.float32)
    p = ekc.block_argsort(ekc.Float32(t), S, flat=True)
    got = ekc.gather(ekc.Float32(sigma), p).numpy()
    order = np.argsort(t.reshape(rays, S), axis=1, kind="stable")
    assert bits_equal(got, np.take_along_axis(sigma.reshape(rays, S), order, axis=1).reshape(-1))
    assert bits_equal(ekc.gather(ekc.Float32(t), p).numpy(), ekc.block_sort(ekc.Float32(t), S).numpy())
