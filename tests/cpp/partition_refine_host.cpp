// Host model of the refined stream's layout (enoki_amd/csrc/ek_refine.h: the slot mapping and the host's size bound, the very
// header the kernels include).  A stand-alone program with its own main; tests/test_partition_refine_host.py builds it with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DEK_REFINE_R={4,8,16} tests/cpp/partition_refine_host.cpp -o ...
// and runs it.  For every piece shape it lays the piece out the way k_bucket_refine_reorder does (entry by entry, runs padded to
// groups of four, the tail of the last tile filled) into buffers of exactly the size the host's bound gives -- a slot beyond them is
// a heap overflow under AddressSanitizer -- and checks that
//   * the mapping is a bijection from the piece's padded sorted groups onto the slots of its tiles,
//   * lane i of tile t owns the R consecutive groups t 64 R + i R ..: group g of the lane at slot t 64 R + g 64 + i, and the four
//     elements of a group lie in ONE 16-byte slot (a group never straddles),
//   * headers carry the entry and the count, pad and tail lanes are zero, every element appears exactly once,
//   * the tiles of the pieces of a partition never exceed refine_tiles_bound(n, pieces, bins).
#include "../../enoki_amd/csrc/ek_refine.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace ek;

static long g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "partition_refine_host: %s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Piece { std::vector<uint32_t> counts; };          // elements per local entry (bins entries)

static uint64_t groups_of(const Piece &p) {
    uint64_t g = 0;
    for (uint32_t c : p.counts) g += refine_groups_of(c);
    return g;
}

/// lays the pieces out one after the other, as the three launches do; returns the tiles used
static uint64_t lay_out(const std::vector<Piece> &pieces, uint32_t bins) {
    uint64_t n = 0;
    for (const Piece &p : pieces) for (uint32_t c : p.counts) n += c;
    const uint64_t cap_tiles = refine_tiles_bound(n, pieces.size(), bins);
    // exactly the bytes the host sets aside (x: float values numbered from 1, 0 = never written; headers: 0xFFFF = never written)
    std::vector<float> x(refine_x_bytes(cap_tiles) / sizeof(float), -1.f);
    std::vector<uint16_t> hdr(refine_header_bytes(cap_tiles) / sizeof(uint16_t), 0xFFFFu);
    CHECK(x.size() == cap_tiles * kRefineTileGroups * 4u && hdr.size() == cap_tiles * kRefineTileGroups);
    uint64_t tile0 = 0, element = 0;
    for (const Piece &p : pieces) {
        CHECK(p.counts.size() == bins);
        const uint64_t groups = groups_of(p), tiles = refine_tiles_of(groups);
        CHECK(tiles * kRefineTileGroups >= groups && (tiles == 0 || (tiles - 1) * kRefineTileGroups < groups));
        CHECK(tile0 + tiles <= cap_tiles);
        const uint64_t slot0 = tile0 * kRefineTileGroups, padded = tiles * kRefineTileGroups;
        std::vector<uint8_t> seen(padded, 0);
        uint64_t j = 0;
        for (uint32_t e = 0; e < bins; ++e) {
            for (uint32_t r = 0; r < p.counts[e]; r += 4, ++j) {
                const uint64_t s = refine_slot(j);
                CHECK(s < padded && !seen[s]);
                seen[s] = 1;
                // lane-transposed: group g of lane i of tile t
                const uint64_t t = j / kRefineTileGroups, i = (j % kRefineTileGroups) / kRefineR, g = j % kRefineR;
                CHECK(s == t * kRefineTileGroups + g * 64u + i);
                const uint32_t count = p.counts[e] - r < 4u ? p.counts[e] - r : 4u;
                hdr.at(slot0 + s) = refine_header(e, count);
                for (uint32_t k = 0; k < 4; ++k) x.at((slot0 + s) * 4u + k) = k < count ? (float) ++element : 0.f;
            }
        }
        CHECK(j == groups);
        for (; j < padded; ++j) {                                 // the tail of the last tile
            const uint64_t s = refine_slot(j);
            CHECK(s < padded && !seen[s]);
            seen[s] = 1;
            hdr.at(slot0 + s) = refine_header(0u, 0u);
            for (uint32_t k = 0; k < 4; ++k) x.at((slot0 + s) * 4u + k) = 0.f;
        }
        for (uint64_t s = 0; s < padded; ++s) CHECK(seen[s]);     // onto: every slot of the piece's tiles
        // a lane's R groups are consecutive groups of the sorted order: entries never decrease along a lane, then along the lanes
        for (uint64_t t = 0; t < tiles; ++t) {
            int64_t last = -1;
            bool tail = false;
            for (uint32_t i = 0; i < 64; ++i)
                for (uint32_t g = 0; g < kRefineR; ++g) {
                    const uint16_t h = hdr.at(slot0 + t * kRefineTileGroups + g * 64u + i);
                    const uint32_t count = h >> kRefineEntryBits, e = h & ((1u << kRefineEntryBits) - 1u);
                    CHECK(h != 0xFFFFu && count <= 4u);
                    if (count == 0) { tail = true; continue; }
                    CHECK(!tail && (int64_t) e >= last);
                    last = e;
                }
        }
        tile0 += tiles;
    }
    // every element exactly once, pads zero, nothing of the pieces' tiles left unwritten
    std::vector<uint8_t> got(element + 1, 0);
    for (uint64_t s = 0; s < tile0 * kRefineTileGroups; ++s) {
        const uint32_t count = hdr[s] >> kRefineEntryBits;
        for (uint32_t k = 0; k < 4; ++k) {
            const float v = x[s * 4u + k];
            if (k < count) { CHECK(v >= 1.f && v <= (float) element && !got[(size_t) v]); got[(size_t) v] = 1; }
            else CHECK(v == 0.f);
        }
    }
    for (uint64_t v = 1; v <= element; ++v) CHECK(got[v]);
    CHECK(element == n);
    return tile0;
}

static Piece piece(uint32_t bins) { Piece p; p.counts.assign(bins, 0u); return p; }

int main() {
    const uint32_t TG = kRefineTileGroups;
    for (uint32_t bins : { 4096u, 2048u, 64u }) {
        std::vector<Piece> shapes;
        shapes.push_back(piece(bins));                                              // empty
        { Piece p = piece(bins); p.counts[bins / 3] = 1; shapes.push_back(p); }     // one element
        for (uint32_t run : { 1u, 3u, 4u, 5u, 4u * TG - 1u, 4u * TG, 4u * TG + 1u }) {
            Piece a = piece(bins); a.counts[7] = run; shapes.push_back(a);          // one run of that length
            if (run <= 5u) { Piece b = piece(bins); for (uint32_t e = 0; e < bins; ++e) b.counts[e] = run; shapes.push_back(b); }   // ... in every entry
        }
        { Piece p = piece(bins); p.counts[bins - 1] = 300007u; shapes.push_back(p); }                     // one entry holds everything
        { Piece p = piece(bins); for (uint32_t e = 0; e < bins; ++e) p.counts[e] = 1u; shapes.push_back(p); }  // every entry exactly one
        { Piece p = piece(bins); uint32_t s = 12345u; for (uint32_t e = 0; e < bins; ++e) { s = s * 1664525u + 1013904223u; p.counts[e] = (s >> 24) % 23u; } shapes.push_back(p); }
        { Piece p = piece(bins); for (uint32_t e = 0; e < bins; e += 2) p.counts[e] = 64u; shapes.push_back(p); }
        for (const Piece &p : shapes) (void) lay_out({ p }, bins);                  // each alone: the bound for ONE piece
        (void) lay_out(shapes, bins);                                               // ... and all of them as the pieces of one partition
        std::vector<Piece> twice(shapes);
        twice.insert(twice.end(), shapes.rbegin(), shapes.rend());
        (void) lay_out(twice, bins);
    }
    // the bound is tight where it should be: n elements in runs of one need n groups
    CHECK(refine_tiles_bound(4096, 1, 4096) >= refine_tiles_of(4096));
    CHECK(refine_tiles_bound(0, 1, 4096) == 1 && refine_tiles_bound(0, 0, 4096) == 0);
    printf("partition_refine_host: R = %u, %ld checks passed\n", kRefineR, g_checks);
    return 0;
}
