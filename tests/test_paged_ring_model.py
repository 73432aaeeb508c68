"""Host model of the placement phase of the single-pass page partition (csrc/ek_paged.h: k_page_partition): is a ring of
`cap` records per bucket deep enough for pages of `page` elements?

A workgroup walks its chunk in tiles of 4096 elements.  Per tile every bucket's fill grows by its arrivals; a tile in which some
bucket's fill exceeds the ring takes the OVERFLOW ROUND (a third barrier, elements written straight from registers); then the
complete pages leave and `fill mod page` stays.  Value partitions of more than 128 buckets stage two planes in rings of 96
records = 1.5 pages of 64 (kPgPlaneCap): the headline input (64 Mi lookups, K = 1 Mi, 256 buckets of 4 Ki entries, 256 workgroups
of 64 tiles each) must stay out of the overflow round -- at most 1 % of its tiles may take it.  (The model gives 1 tile of the
first 4096 at a ring of 96 with 64-element pages, 3 at the earlier ring of 64 with 32-element pages; rings of 88 and 80 with
64-element pages overflow in 10 % and 92 % of the tiles.)
"""
import numpy as np

from conftest import hash_u32

TILE = 4096


def overflow_tiles(buckets_of_tile, n_chunks, tiles_per_chunk, n_buckets, cap, page, n_real=None):
    """number of tiles that take the overflow round; buckets_of_tile(t) -> [n_chunks, <= TILE] bucket numbers of tile t of every
    chunk (buckets from n_real on, if given, collect lanes the partition drops: their fill is not looked at)"""
    fill = np.zeros((n_chunks, n_buckets), np.int64)
    rows = np.arange(n_chunks, dtype=np.int64)[:, None] * n_buckets
    over = 0
    for t in range(tiles_per_chunk):
        b = buckets_of_tile(t).astype(np.int64)
        fill += np.bincount((rows + b).ravel(), minlength=n_chunks * n_buckets).reshape(n_chunks, n_buckets)
        over += int((fill[:, :n_real] > cap).any(axis=1).sum())
        fill %= page
    return over


def overflow_tiles_of(idx, shift, n_buckets, cap, page, chunk):
    """the same for an index array cut into chunks of `chunk` elements (a multiple of TILE; len(idx) a multiple of chunk)"""
    b = (idx.astype(np.int64) >> shift).reshape(-1, chunk // TILE, TILE)
    return overflow_tiles(lambda t: b[:, t, :], b.shape[0], b.shape[1], n_buckets, cap, page)


def headline_buckets(n_chunks, chunk):
    lane = np.arange(TILE, dtype=np.uint64)[None, :]
    first = (np.arange(n_chunks, dtype=np.uint64) * np.uint64(chunk))[:, None]
    return lambda t: ((hash_u32(first + np.uint64(t * TILE) + lane, 4) % np.uint32(1 << 20)) >> np.uint32(12))


def test_ring_of_96_keeps_the_headline_input_out_of_the_overflow_round():
    W, tiles = 256, 64                                  # 64 Mi elements over 256 workgroups
    over = overflow_tiles(headline_buckets(W, tiles * TILE), W, tiles, 256, cap=96, page=64)
    print(f"ring 96, page 64: {over} of {W * tiles} tiles take the overflow round")
    assert over <= 0.01 * W * tiles, over


def test_model_sees_skew():
    """what the GPU tests of the overflow round rely on: all-equal and one-bucket indices overflow in EVERY tile"""
    n, chunk = 1 << 18, 1 << 16
    assert overflow_tiles_of(np.full(n, 12345, np.uint32), 12, 256, 96, 64, chunk) == n // TILE
    spread = np.random.default_rng(1).integers(7 << 12, 8 << 12, n).astype(np.uint32)
    assert overflow_tiles_of(spread, 12, 256, 96, 64, chunk) == n // TILE
    uniform = np.random.default_rng(2).integers(0, 1 << 20, n).astype(np.uint32)
    assert overflow_tiles_of(uniform, 12, 256, 96, 64, chunk) <= 1
