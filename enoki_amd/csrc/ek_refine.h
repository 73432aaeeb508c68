// The refined stream of a kept bucket partition (ek_bucketed.h, bucket_refine.hip, bucketed_early.hip): where sorted group j of a
// piece sits, and how much storage the host sets aside.  No device-only code: tests/cpp/partition_refine_host.cpp includes this
// file as it is.
//
// A piece's elements, ordered by local entry, are cut into GROUPS of four that never span two entries (an entry's run is padded
// to whole groups).  A TILE is 64 lanes x R groups, stored lane-transposed: lane i owns the R consecutive groups
// [t 64 R + i R, t 64 R + (i + 1) R) of the sorted order and finds its g-th one at slot t 64 R + g 64 + i -- so the 64 lanes'
// loads of step g are one contiguous 1 KiB of x (16 B per slot) and 128 B of headers (2 B per slot: local entry in the low
// 12 bits, element count 0..4 above).  A piece's stream is a whole number of tiles; its tail is filled with count-0 groups.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EK_REFINE_HD __host__ __device__
#else
#define EK_REFINE_HD
#endif

namespace ek {

#ifndef EK_REFINE_R
#define EK_REFINE_R 8
#endif
constexpr uint32_t kRefineR = EK_REFINE_R;                    // groups per lane and tile: 4, 8 or 16 (profiles/probe_partition_refine_r14.txt)
constexpr uint32_t kRefineTileGroups = 64u * kRefineR;
constexpr uint32_t kRefineEntryBits = 12;                     // buckets of at most 4 Ki entries (kFixedRecBytes)
static_assert(kRefineR == 4 || kRefineR == 8 || kRefineR == 16, "R is 4, 8 or 16");

/// groups that hold a run of `count` elements of one entry
EK_REFINE_HD inline uint32_t refine_groups_of(uint32_t count) { return (count + 3u) / 4u; }
/// tiles that hold `groups` groups
EK_REFINE_HD inline uint32_t refine_tiles_of(uint64_t groups) { return (uint32_t) ((groups + kRefineTileGroups - 1u) / kRefineTileGroups); }
/// slot (within the piece's stream, in groups) of sorted group j of a piece
EK_REFINE_HD inline uint64_t refine_slot(uint64_t j) {
    const uint64_t t = j / kRefineTileGroups, r = j % kRefineTileGroups;
    return t * kRefineTileGroups + (r % kRefineR) * 64u + r / kRefineR;
}
EK_REFINE_HD inline uint16_t refine_header(uint32_t entry, uint32_t count) { return (uint16_t) (entry | (count << kRefineEntryBits)); }

/// Upper bound of the tiles of ALL pieces, from what the host knows without a read-back: n elements in at most `max_pieces`
/// pieces of buckets of `bins` entries.  An entry with c elements takes ceil(c / 4) <= (c + 3) / 4 groups, and a piece has at most
/// min(its elements, bins) entries that are not empty: groups <= (n + 3 min(n, max_pieces bins)) / 4; every piece then rounds up to
/// whole tiles: one more tile per piece.
inline uint64_t refine_tiles_bound(uint64_t n, uint64_t max_pieces, uint64_t bins) {
    const uint64_t entries = n < max_pieces * bins ? n : max_pieces * bins;
    const uint64_t groups = (n + 3u * entries + 3u) / 4u;
    return groups / kRefineTileGroups + max_pieces;
}
/// bytes of the two streams for `tiles` tiles
inline uint64_t refine_x_bytes(uint64_t tiles) { return tiles * kRefineTileGroups * 16u; }
inline uint64_t refine_header_bytes(uint64_t tiles) { return tiles * kRefineTileGroups * 2u; }

} // namespace ek
