"""sort / argsort in the python modules (enoki_amd.hip, enoki_amd.hip_autodiff, `import enoki`): all six flat types against numpy's
stable argsort at 3 T + 7 entries (T: the radix route's tile), on the radix route and on the automatic one; keyword names and
docstrings; the tape node.  The adjoint of a sort is a scatter through its permutation and the forward derivative a gather: both
move bits, so the gradient identities below are compared bit for bit, no tolerance.  Then the pipeline the call is for: hits
grouped by ray id with argsort and gather, the groups' starts from search_sorted, and segment_sum over them."""
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


@pytest.fixture
def radix(ekc):
    """every n >= 2 takes the radix route; the automatic mode comes back afterwards"""
    ekc.hip_set_tuning("sort_radix", 2)
    try:
        yield
    finally:
        ekc.hip_set_tuning("sort_radix", 1)


def size_of(dt):
    """3 T + 7: several workgroups and a partial last tile on the radix route"""
    from enoki_amd import capi
    return 3 * capi.sort_plan(dt, 2)[2] + 7


def host_data(dt, n, seed, ties=False):
    rng = np.random.default_rng(seed)
    if ties:
        return rng.integers(0, 5, n).astype(dt)
    if np.dtype(dt).kind == "f":
        return rng.standard_normal(n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def reference(h, descending=False):
    key = h if not descending else (-h if h.dtype.kind == "f" else ~h)
    return np.argsort(key, kind="stable").astype(np.uint32)


@pytest.mark.parametrize("mode", [2, 1], ids=["radix", "automatic"])
def test_every_flat_type_of_both_modules(ekc, ad, mode):
    import enoki as ek
    from enoki_amd import capi
    ekc.hip_set_tuning("sort_radix", mode)
    try:
        for mod in (ekc, ad):
            for cls, dt in TYPES:
                n = size_of(dt)
                assert capi.sort_plan(dt, n)[0] == 2 or mode == 1
                A = getattr(mod, cls)
                for ties in (False, True):
                    h = host_data(dt, n, 3, ties)
                    if np.dtype(dt).kind == "f":
                        h[::11] = np.nan
                        h[5::13] = -0.0
                    x = A(h)
                    for desc in (False, True):
                        p = reference(h, desc)
                        s = mod.sort(x, descending=desc)
                        assert type(s) is A and bits_equal(s.numpy(), h[p]), (cls, desc)
                        q = mod.argsort(x, descending=desc)
                        assert type(q) is mod.UInt32 and np.array_equal(q.numpy(), p), (cls, desc)
                        assert np.array_equal(mod.argsort(x, desc).numpy(), p), (cls, desc)
                        assert bits_equal(ek.sort(array=x, descending=desc).numpy(), h[p]), (cls, desc)
                        assert np.array_equal(ek.argsort(array=x, descending=desc).numpy(), p), (cls, desc)
                    assert bits_equal(mod.sort(x).numpy(), h[reference(h)]), cls
                    # the whole-array sort is block_sort of one row, bit for bit
                    assert bits_equal(mod.sort(x).numpy(), mod.block_sort(x, n).numpy()), cls
                    assert np.array_equal(mod.argsort(x, True).numpy(), mod.block_argsort(x, n, True).numpy()), cls
                with pytest.raises(TypeError):
                    mod.sort(x, reverse=True)
                with pytest.raises(TypeError):
                    mod.argsort(x, flat=True)
                assert len(mod.sort(A())) == 0 and len(mod.argsort(A())) == 0
            assert "stable" in mod.sort.__doc__.lower() and "gather" in mod.argsort.__doc__
    finally:
        ekc.hip_set_tuning("sort_radix", 1)


def test_grouping_hits_by_ray(ekc, radix):
    """argsort -> gather -> search_sorted(sorted_keys, arange(m)) yields the starts for which segment_sum is numpy.bincount.  The
    weights are multiples of 1/8 below 2^10, so every float32 sum of a few hundred of them is exact in any order."""
    rng = np.random.default_rng(7)
    n, m = size_of(np.uint32), 300
    keys = rng.integers(0, m, n).astype(np.uint32)
    keys[keys == 17] = 18                                               # a ray without hits: an empty segment
    weights = (rng.integers(0, 8192, n) / 8).astype(np.float32)
    k, w = ekc.UInt32(keys), ekc.Float32(weights)
    p = ekc.argsort(k)
    sorted_keys, grouped = ekc.gather(k, p), ekc.gather(w, p)
    assert np.array_equal(sorted_keys.numpy(), np.sort(keys)) and bits_equal(sorted_keys.numpy(), ekc.sort(k).numpy())
    starts = ekc.search_sorted(sorted_keys, ekc.UInt32.arange(m))
    assert np.array_equal(starts.numpy(), np.searchsorted(np.sort(keys), np.arange(m)))
    sums = ekc.segment_sum(grouped, starts).numpy()
    want = np.bincount(keys, weights=weights.astype(np.float64), minlength=m)
    assert want[17] == 0 and want.max() < 2 ** 21 and np.array_equal(sums.astype(np.float64), want)
    # stable: inside every ray the hits keep their input order
    hp = p.numpy().astype(np.int64)
    same = keys[hp][1:] == keys[hp][:-1]
    assert np.all(hp[1:][same] > hp[:-1][same])


@pytest.mark.parametrize("cls,dt", TYPES[:2])
def test_the_adjoint_is_a_scatter_through_the_permutation(ekc, ad, radix, cls, dt):
    n = size_of(dt)
    A = getattr(ad, cls)
    hx, hw, hv = host_data(dt, n, 4), host_data(dt, n, 5), host_data(dt, n, 6)
    hx[::7] = hx[3]                                                     # ties: stability decides the permutation
    for desc in (False, True):
        p = reference(hx, desc)
        x, w = A(hx), A(hw)
        ad.set_requires_gradient(x)
        s = ad.sort(x, descending=desc)
        assert ad.requires_gradient(s) and len(s) == n
        assert bits_equal(ad.detach(s).numpy(), hx[p])
        ad.backward(ad.hsum(w * s))
        assert bits_equal(ad.gradient(x).numpy()[p], hw), desc          # gradient(x)[p] == w
        # forward mode with a seed array: seed[p]
        x = A(hx)
        ad.set_requires_gradient(x)
        s = ad.sort(x, descending=desc)
        ad.set_gradient(x, getattr(ekc, cls)(hv), False)
        A.forward()
        assert bits_equal(ad.gradient(s).numpy(), hv[p]), desc


def test_what_records_no_node(ad, radix):
    n = size_of(np.float32)
    hx = host_data(np.float32, n, 9)
    x = ad.Float32(hx)
    s = ad.sort(x)                                                      # x does not require a gradient
    assert not ad.requires_gradient(s) and bits_equal(s.numpy(), hx[reference(hx)])
    ad.set_requires_gradient(x)
    nodes = len(ad.Float32.whos().splitlines())                         # (one line per node of the tape)
    q = ad.argsort(x, descending=True)
    assert len(ad.Float32.whos().splitlines()) == nodes                 # no node was recorded
    s = ad.sort(x)
    assert len(ad.Float32.whos().splitlines()) == nodes + 1 and ad.requires_gradient(s)      # ... where sort records one
    assert type(q) is ad.UInt32 and not ad.requires_gradient(q)
    assert np.array_equal(q.numpy(), reference(hx, True))
