"""Direct gradient tables (csrc/bucketed_early.hip, ek_hip_bucketed_take_tables; DESIGN sections 3 and 6): on a kept partition whose
buckets are ONE piece each the forward + adjoint kernel writes its two planes of sums in table layout, finished as the fold would
finish them in a fresh table at scale 1, and backward() hands those tables to the fresh gradient arrays -- no fold is launched.
Nothing may change: every result here is compared BITWISE between the tuning `direct_tables` = 0 (slots + fold) and 2 (direct
tables whenever the shape is covered; the default 1 starts at tables of 256 Ki entries, larger than a quick test wants).

Protocol: n = 2^18 lookups, float32 -- the smallest n that is evaluated in bucket order at all (ek_hip_bucketed_applicable); three
steps over the same (index, x[, mask]) arrays, so that steps 2 and 3 stand on the kept partition; y, gA, gB of step 3 are compared,
and the launch record of step 3 shows no `scatter_add_fold` where the tables are taken over and exactly one where they are not.

What the library does with a shape is asked of the library itself, not assumed.  Bucket order starts above 16 Ki table entries
(ek_hip_bucketed_applicable), so K = 4096 (one bucket), K = 3 * 4096 + 5 and the empty-bucket shape K = 3 * 4096 run in ELEMENT
order -- no early sums, float atomics, nothing of this change on their path: those cases stay, say so, and compare within the
reordering bound of their sums.  Next to them stand the smallest shapes that do reach the kernel with one-piece buckets (the
partition aims at one piece per 32 Ki lookups, 8 at this n): K = 8 * 4096 + 5 for the clamp of the last, partial bucket (9 buckets,
the last of 5 entries), K = 5 * 4096 for empty buckets, K = 65536 (16 buckets) for everything else.  Every bucket-order case
first asks ek_hip_bucketed_piece_counts whether its buckets are one piece each."""
import gc
import json

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

N = 1 << 18


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


@pytest.fixture(autouse=True)
def tunings(ad):
    yield
    ad.hip_set_tuning("direct_tables", 1)
    ad.hip_set_tuning("partition_refine", 1)
    ad.hip_set_tuning("partition_cache", 1)


_HOST = {}


def host(K, n=N, kind="uniform"):
    """inputs of one shape, made once and read-only"""
    key = (K, n, kind)
    if key not in _HOST:
        rng = np.random.default_rng(K * 7 + n + len(kind))
        if kind == "uniform":
            idx = rng.integers(0, K, n)
        elif kind == "first_bucket":            # every lookup below 4096: the buckets behind the first stay empty
            idx = rng.integers(0, 4096, n)
        elif kind == "log_uniform":             # as the benchmark's cfg3b_zipf, scaled to K: floor(K^v), v uniform in [0, 1)
            idx = np.minimum(np.floor(K ** rng.uniform(0.0, 1.0, n)), K - 1)
        else:                                   # "sparse_last": exactly two lookups per entry of the last bucket (see the test)
            first = (K - 1) // 4096 * 4096
            tail = np.repeat(np.arange(first, K), 2)
            idx = np.concatenate([rng.integers(0, first, n - tail.size), tail])
            rng.shuffle(idx)
        h = dict(A=rng.uniform(-1, 1, K).astype(np.float32), B=rng.uniform(-1, 1, K).astype(np.float32),
                 x=rng.uniform(-2, 2, n).astype(np.float32), idx=idx.astype(np.uint32), mask=(rng.integers(0, 4, n) != 0))
        for a in h.values():
            a.setflags(write=False)
        _HOST[key] = h
    return _HOST[key]


def counted(ad, fn):
    ad.hip_profile_begin()
    r = fn()
    prof = json.loads(ad.hip_profile_end())
    return r, {k["kernel"]: k["launches"] for k in prof if k["launches"]}


def forward(ad, A, B, x, idx, mask, form):
    a = ad.gather(A, idx, mask) if mask is not None else ad.gather(A, idx)
    if form in ("scalar", "product"):
        b = None
    elif form == "same":
        b = ad.gather(A, idx, mask) if mask is not None else ad.gather(A, idx)
    else:
        b = ad.gather(B, idx, mask) if mask is not None else ad.gather(B, idx)
    if form == "a*x+b":
        u = a * x + b
    elif form == "b-a*x":
        u = b - a * x
    elif form == "product":
        u = a * x
    elif form == "scalar":
        u = ad.fmadd(a, x, ad.Float32(0.5))
    else:
        u = ad.fmadd(a, x, b)
    return ad.hsum(ad.cos(u) if form == "cos" else ad.sin(u))


def step(ad, hA, hB, x, idx, mask=None, form="fmadd", seed=1.0, twice=False, keep=None):
    """one step on FRESH leaves; -> (y, gA, gB) on the host.  twice: a second forward + backward() into the same leaves"""
    A, B = ad.Float32(hA), ad.Float32(hB)
    ad.set_requires_gradient(A); ad.set_requires_gradient(B)
    y = forward(ad, A, B, x, idx, mask, form)
    ad.backward(y * seed if seed != 1.0 else y)
    if twice:
        y = forward(ad, A, B, x, idx, mask, form)
        ad.backward(y)
    with_b = form not in ("scalar", "product", "same")
    if keep is not None:
        keep.update(A=A, B=B, gA=ad.gradient(A), gB=ad.gradient(B))
    return ad.detach(y).numpy().copy(), ad.gradient(A).numpy().copy(), (ad.gradient(B).numpy().copy() if with_b else None)


def three_steps(ad, mode, h, hA=None, masked=False, idx64=False, refine=1, covered=True, **kw):
    """three steps over one set of (x, idx, mask) arrays under direct_tables = mode; -> step 3's results and launch record"""
    if mode is not None:                    # (None: the defaults of the library, whatever they are)
        ad.hip_set_tuning("direct_tables", mode)
        ad.hip_set_tuning("partition_refine", refine)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    if idx64:
        idx = ad.UInt64(idx)
    mask = ad.Mask(h["mask"]) if masked else None
    out = [counted(ad, lambda: step(ad, h["A"] if hA is None else hA, h["B"], x, idx, mask, **kw)) for _ in range(3)]
    (r, ks) = out[2]
    if covered and mode is not None and refine != 1:          # (1: automatic, by the lookups per entry)
        # which walk ran: the refined stream is built at the first hit (step 2) under partition_refine = 2 and never under 0 --
        # the launch record has one name for the forward + adjoint kernel of both walks, the refinement's kernels tell them apart
        assert (out[1][1].get("bucket_refine", 0) >= 1) == (refine == 2), (refine, out[1][1])
    if covered:
        assert ks.get("bucket_partition", 0) == 0 and ks.get("bucket_pair_fma_reduce_adjoint") == covered, ks      # on the kept partition
    else:
        assert "bucket_partition" not in ks and "bucket_pair_fma_reduce_adjoint" not in ks, ks                     # element order
    return r, ks


def one_piece_buckets(capi, h, K, masked=False):
    """does the partition of (idx, x[, mask]) into K entries give EVERY bucket exactly one piece?  (asked of the library)"""
    dA, dx, di = capi.Buf.from_numpy(h["A"]), capi.Buf.from_numpy(h["x"]), capi.Buf.from_numpy(h["idx"])
    dm = capi.Buf.from_numpy(h["mask"].astype(np.uint8)) if masked else None
    b = capi.Bucketed("fmadd", dA, dx, dA, di, hints=capi.Bucketed.HINT_ADJOINT | capi.Bucketed.HINT_BOUNDED, mask=dm)
    total, largest = b.piece_counts()
    b.destroy()
    return largest == 1 and total == (K + 4095) // 4096, (total, largest)


def launches_of(capi, fn):
    capi.profile_begin()
    fn()
    return {k["kernel"]: k["launches"] for k in capi.profile_end() if k["launches"]}


def same_bits(r, s):
    return all(bits_equal(a, b) for a, b in zip(r, s) if a is not None)


def folds(ks):
    return ks.get("scatter_add_fold", 0)


def check(ad, capi, K, n=N, kind="uniform", take=True, hA=None, **kw):
    """direct_tables 0 against 2: the same bits; the fold is gone exactly where the tables are taken over (take = None: the shape
    is not evaluated in bucket order, there is no fold either way)"""
    h = host(K, n, kind)
    backwards = 2 if kw.get("twice") else 1
    r0, k0 = three_steps(ad, 0, h, hA, covered=backwards if take is not None else 0, **kw)
    r2, k2 = three_steps(ad, 2, h, hA, covered=backwards if take is not None else 0, **kw)
    print(f"K={K} n={n} {kind} {kw}: direct_tables=0 {k0}  direct_tables=2 {k2}")
    if take is None or take == "element":
        # The adjoint runs in element order: scatter_add with float atomics, whose sums differ from run to run of ONE setting.
        # Nothing of this change is on that path; the two runs launch the same kernels and agree within what reordering a sum
        # of m terms of magnitude <= max |x| can do, m * 2^-24 * m * max |x| per entry, m = the entry's lookups (twice that
        # when both tables are one array).  y is a fixed tree: the same bits.
        m = np.bincount(h["idx"], minlength=K).astype(np.float64) * (2 if kw.get("form") == "same" else 1)
        bound = m * m * float(np.abs(h["x"]).max()) * 2.0 ** -24
        assert bits_equal(r0[0], r2[0])
        assert all(np.all(np.abs(a.astype(np.float64) - b) <= bound) for a, b in zip(r0[1:], r2[1:]) if a is not None)
        assert k0 == k2 and ("scatter_add_accumulate" in k0 or "scatter_add_lds" in k0), (k0, k2)
        return r2
    assert same_bits(r0, r2), [int(np.sum(a.view(np.uint32) != b.view(np.uint32))) for a, b in zip(r0, r2) if a is not None]
    assert folds(k0) == (0 if take is None else backwards), k0
    assert folds(k2) == (backwards if take is False else 0), (take, k2)
    assert set(k2) - {"scatter_add_fold"} == set(k0) - {"scatter_add_fold"}, (k0, k2)      # nothing else came or went
    return r2


# ---- the tables are taken over -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("K", [4096, 3 * 4096 + 5, 8 * 4096 + 5, 65536])
def test_shapes_under_both_walks(ad, capi, K, refine):
    """one bucket; a last bucket of 5 entries (the clamp); 16 buckets -- on the kept partition's pages and on its refined stream.
    What the clamp case covers: the last bucket's 5 entries arrive at the right place with the right bits.  It would NOT notice a
    missing clamp -- 4091 floats written behind the table land in the allocator's pool and the first K entries still match; the
    bound `j < min(Bins, table_size - bucket * Bins)` is in the kernel's epilogue to be read, not tested here."""
    if not capi.Bucketed.applicable(np.float32, np.uint32, K, N):
        assert K < 16384                                      # (module docstring: element order)
        check(ad, capi, K, take=None, refine=refine)
        return
    one, counts = one_piece_buckets(capi, host(K), K)
    assert one, (K, counts)
    check(ad, capi, K, take=True, refine=refine)


@pytest.mark.parametrize("K,take", [((1 << 18) - 4096, False), (1 << 18, True)])
def test_default_setting_takes_tables_over_from_256_Ki_entries(ad, capi, K, take):
    """no tuning is touched: `direct_tables` = 1 hands the tables over at K = 256 Ki (64 one-piece buckets) and folds one bucket
    below that bound; either way the bits are those of `direct_tables` = 0"""
    h = host(K)
    one, counts = one_piece_buckets(capi, h, K)
    assert one, (K, counts)
    r1, k1 = three_steps(ad, None, h)
    r0, k0 = three_steps(ad, 0, h)
    print(f"K={K} default setting {k1}  direct_tables=0 {k0}")
    assert same_bits(r0, r1) and folds(k0) == 1 and folds(k1) == (0 if take else 1), (k0, k1)


@pytest.mark.parametrize("form", ["fmadd", "a*x+b", "b-a*x", "product"])
def test_spellings(ad, capi, form):
    """sin over the fma, the operator spellings, and the product alone (count 1, the weighted plane).  `b - a*x` records the factor
    -1 on the stream of A (d/da = -x cos u): not every factor is 1, the fold stays and applies it to the direct tables"""
    check(ad, capi, 65536, take=form != "b-a*x", form=form)


def test_index_64_bit(ad, capi):
    check(ad, capi, 65536, idx64=True)


def test_mask_of_the_benchmark(ad, capi):
    one, counts = one_piece_buckets(capi, host(65536), 65536, masked=True)
    assert one, counts
    check(ad, capi, 65536, masked=True)


def test_infinite_table_entry_runs_under_locks_and_still_writes_the_table(ad, capi):
    """An infinite entry of A sends its bucket's piece down the lock path (float sums); a one-piece bucket writes floats either way.
    The lock path adds in the order the lanes arrive, so the bucket with the infinite entry receives exactly two lookups per entry
    here: sums of two terms do not depend on the order, and the bits -- NaNs included -- can be compared."""
    K = 65536
    h = host(K, N, "sparse_last")
    hA = h["A"].copy()
    hA[K - 7] = np.inf
    y, gA, gB = check(ad, capi, K, kind="sparse_last", hA=hA)
    assert np.isnan(y[0]) and np.isnan(gA[K - 7]) and np.isnan(gB[K - 7])
    assert np.all(np.isfinite(gA[:K - 4096])) and np.all(np.isfinite(gB[:K - 4096]))


PAIRS = [("sin", "cos"), ("cos", "sin"), ("sin", "sin")]


@pytest.mark.parametrize("half,other", PAIRS)
def test_function_pairs_through_the_c_abi(ad, capi, half, other):
    """reduce(hsum, half) keeping `other`, on an object that stands on a kept partition: take_tables against scatter_add into
    fresh tables (the tape asks for cos / sin with the factor -1 of d cos = -sin, which folds: test_cosine_folds_with_its_sign)"""
    import ctypes
    K = 65536
    h = host(K)
    lib = capi.lib
    dA, dB, dx, di = (capi.Buf.from_numpy(h[k]) for k in ("A", "B", "x", "idx"))
    H = capi.Bucketed.HINT_ADJOINT | capi.Bucketed.HINT_BOUNDED
    first = capi.Bucketed("fmadd", dA, dx, dB, di, hints=H)
    part = ctypes.c_void_p()
    capi.check(lib.ek_hip_bucketed_partition_retain(first.handle, ctypes.byref(part)))

    def on_kept():
        hnd = ctypes.c_void_p()
        capi.check(lib.ek_hip_bucketed_pair_create_on(part, dA.ek, di.ek, capi.TERNARY["fmadd"], ctypes.c_void_p(dA.ptr), ctypes.c_void_p(dB.ptr),
                                                      None, None, ctypes.c_size_t(K), ctypes.c_size_t(N), ctypes.c_uint(H), 0, ctypes.byref(hnd)))
        b = capi.Bucketed.__new__(capi.Bucketed)
        b.A, b.C, b.dtype, b.K, b.handle = dA, dB, dA.dtype, K, hnd
        return b

    streams = [(other, 0, False), (other, 0, True)]
    try:
        capi.set_tuning("direct_tables", 0)
        b = on_kept()
        y0 = b.reduce("hsum", half, keep=True, keep_op=other).numpy().copy()
        assert b.take_tables(streams) is None
        g = [capi.Buf(np.float32, K), capi.Buf(np.float32, K)]
        b.scatter_add(g, streams, fresh=[1, 1])
        ref = [t.numpy().copy() for t in g]
        held = [capi.Buf.from_numpy(h["B"]), capi.Buf.from_numpy(h["A"])]      # targets that hold data, one factor other than 1
        b.scatter_add(held, streams, fresh=[0, 0], scales=[1.0, -2.5])
        ref_held = [t.numpy().copy() for t in held]
        b.destroy()
        capi.set_tuning("direct_tables", 2)
        b = on_kept()
        b.reduce("hsum", half, keep=True, keep_op=other)
        held = [capi.Buf.from_numpy(h["B"]), capi.Buf.from_numpy(h["A"])]
        ks = launches_of(capi, lambda: b.scatter_add(held, streams, fresh=[0, 0], scales=[1.0, -2.5]))     # the fold reads the direct tables
        assert ks == {"scatter_add_fold": 1}, ks
        assert all(bits_equal(r, t.numpy()) for r, t in zip(ref_held, held))
        b.destroy()
        capi.set_tuning("direct_tables", 2)
        b = on_kept()
        y2 = b.reduce("hsum", half, keep=True, keep_op=other).numpy().copy()
        assert b.take_tables(streams, scales=[1.0, 3.0]) is None            # a factor: not taken, nothing changed
        capi.profile_begin()
        got = b.take_tables(list(reversed(streams)))                       # (the streams in the other order: weighted first)
        ks = {k["kernel"]: k["launches"] for k in capi.profile_end() if k["launches"]}
        assert got is not None and ks == {}, ks
        assert b.take_tables(streams) is None                               # the tables have left
        b.scatter_add(g, streams, fresh=[1, 1])                             # ... and a second request evaluates the streams on the lists
        b.destroy()
        b = on_kept()                                                       # ONE plane taken: the other is still folded from its table
        b.reduce("hsum", half, keep=True, keep_op=other)
        plain = b.take_tables(streams[:1])
        assert plain is not None and bits_equal(ref[0], plain[0].numpy()) and b.take_tables(streams[:1]) is None
        w = [capi.Buf(np.float32, K)]
        ks = launches_of(capi, lambda: b.scatter_add(w, streams[1:], fresh=[1]))
        assert ks == {"scatter_add_fold": 1} and bits_equal(ref[1], w[0].numpy()), ks
        b.destroy()
        assert bits_equal(y0, y2) and bits_equal(ref[0], got[1].numpy()) and bits_equal(ref[1], got[0].numpy())
        assert np.allclose(g[0].numpy(), ref[0], rtol=1e-4, atol=1e-4)
    finally:
        capi.set_tuning("direct_tables", 1)
        first.destroy()
        capi.check(lib.ek_hip_bucket_partition_release(part))


# ---- the fold stays ----------------------------------------------------------------------------------------------------------------
def test_seed_3_folds(ad, capi):
    check(ad, capi, 65536, take=False, seed=3.0)


def test_cosine_folds_with_its_sign(ad, capi):
    """hsum(cos(u)): the tape's streams are -sin(u) and -x sin(u), a factor of -1 -- the fold applies it to the direct tables"""
    check(ad, capi, 65536, take=False, form="cos")


def test_second_backward_into_the_same_leaves(ad, capi):
    """The tape sums a gather's adjoint in a fresh buffer of its own and adds that to what the leaf's gradient holds: the second
    backward() meets fresh targets like the first and takes its tables over; the leaf's sum of the two is the tape's, with the
    same bits.  (A TARGET that holds data is folded into: test_function_pairs_through_the_c_abi.)"""
    check(ad, capi, 65536, take=True, twice=True)


def test_one_array_for_both_tables(ad, capi):
    """fmadd(gather(A, i), x, gather(A, i)): two streams into ONE gradient -- the tape sends this adjoint down in element order
    (the forward pass still forms its early sums; nobody asks for them)"""
    check(ad, capi, 65536, take="element", form="same")


def test_scalar_addend_keeps_its_slots(ad, capi):
    check(ad, capi, 65536, take=False, form="scalar")


def test_a_bucket_of_several_pieces_folds(ad, capi):
    """a log-uniform index array: three quarters of the lookups fall into the first of 16 buckets, which is cut into pieces"""
    K = 65536
    one, (total, largest) = one_piece_buckets(capi, host(K, N, "log_uniform"), K)
    assert largest > 1, (total, largest)
    check(ad, capi, K, kind="log_uniform", take=False)


@pytest.mark.parametrize("K", [3 * 4096, 5 * 4096])
def test_empty_buckets_come_out_as_positive_zero(ad, capi, K):
    """every index below 4096: the buckets behind the first have no piece, nobody would write their range of a direct table -- such
    a partition answers "no" and folds, and the fold writes +0.0 there.  (K = 3 * 4096 is below bucket order: module docstring.)"""
    covered = capi.Bucketed.applicable(np.float32, np.uint32, K, N)
    assert covered == (K == 5 * 4096)
    y, gA, gB = check(ad, capi, K, kind="first_bucket", take=False if covered else None)
    for g in (gA, gB):
        assert np.array_equal(g[4096:].view(np.uint32), np.zeros(K - 4096, np.uint32))
        assert np.any(g[:4096] != 0)


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------
def test_taken_tables_outlive_everything_they_came_from(ad, capi):
    K = 65536
    h = host(K)
    ref, _ = three_steps(ad, 0, h)
    ad.hip_set_tuning("direct_tables", 2)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    keep = {}
    step(ad, h["A"], h["B"], x, idx)
    step(ad, h["A"], h["B"], x, idx)
    r, ks = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, keep=keep))
    assert folds(ks) == 0 and same_bits(ref, r), ks
    gA, gB = keep.pop("gA"), keep.pop("gB")
    keep.clear()                                          # the leaves
    del x, idx                                            # ... the index and x arrays (and with them the kept partition's entry)
    gc.collect()
    first = (gA.numpy().copy(), gB.numpy().copy())
    ad.hip_set_tuning("partition_cache", 0)               # (eviction)
    ad.hip_set_tuning("partition_cache", 1)
    h2 = host(K, N, "sparse_last")
    x2, idx2 = ad.Float32(h2["x"]), ad.UInt32(h2["idx"])
    for _ in range(10):                                   # the pool hands memory out again
        step(ad, h2["B"], h2["A"], x2, idx2)
    assert bits_equal(first[0], ref[1]) and bits_equal(first[1], ref[2])
    assert bits_equal(gA.numpy(), first[0]) and bits_equal(gB.numpy(), first[1])
