// What the sorts share (block_sort.hip: a stable sort inside every block of B entries; segment_sort.hip: the same inside ragged
// segments): the order-preserving composites, their storage in LDS or scratch, the bitonic network over an LDS tile, and the two
// searches of a merge -- merge path over two sorted runs and the rank of a composite in the other piece.
//
// COMPOSITES.  No kernel sorts values: every entry becomes (key, position) with an order-preserving unsigned key
//     floats     u = bits, -0.0 -> +0.0;  key = u ^ (sign ? all ones : sign bit);  NaN -> all ones (no number maps there)
//     signed     key = bits ^ sign bit                    unsigned   key = bits
//     descending key = ~key, NaN still all ones
// and a 32-bit position.  4-byte types: one 64-bit word key << 32 | position, one compare.  8-byte types: a 64-bit key and a 32-bit
// position in two arrays, compared lexicographically.  Padding slots hold all ones in both parts.
#pragma once

#include "ek_block.h"

namespace ek {

enum { kSortUnsigned = 0, kSortSigned = 1, kSortFloat = 2 };

// ---- composites --------------------------------------------------------------------------------------------------------------
template <int ES> struct SortComp;
template <> struct SortComp<4> { uint64_t w; };
template <> struct SortComp<8> { uint64_t key; uint32_t pos; };

__device__ __forceinline__ bool comp_less(const SortComp<4> &a, const SortComp<4> &b) { return a.w < b.w; }
__device__ __forceinline__ bool comp_less(const SortComp<8> &a, const SortComp<8> &b) {
    return a.key < b.key || (a.key == b.key && a.pos < b.pos);
}
__device__ __forceinline__ uint32_t comp_pos(const SortComp<4> &c) { return (uint32_t) c.w; }
__device__ __forceinline__ uint32_t comp_pos(const SortComp<8> &c) { return c.pos; }

template <int ES> __device__ __forceinline__ SortComp<ES> comp_padding() {
    if constexpr (ES == 4) return SortComp<4>{ ~0ull };
    else return SortComp<8>{ ~0ull, ~0u };
}

/// the order-preserving unsigned key of an entry's bits (the table at the top); sort.hip's radix passes sort by it byte by byte
template <int ES, int KIND, typename U> __device__ __forceinline__ U sort_key(U u, bool desc) {
    static_assert(sizeof(U) == ES, "sort_key(): the bits of one entry");
    constexpr U kSign = U(1) << (ES * 8 - 1), kOnes = ~U(0);
    U key;
    if constexpr (KIND == kSortFloat) {
        constexpr U kInf = ES == 4 ? U(0x7F800000u) : U(0x7FF0000000000000ull);
        if ((u & ~kSign) > kInf) {
            key = kOnes;
        } else {
            if (u == kSign) u = 0;
            key = u ^ ((u & kSign) ? kOnes : kSign);
            if (desc) key = ~key;
        }
    } else {
        key = KIND == kSortSigned ? U(u ^ kSign) : u;
        if (desc) key = ~key;
    }
    return key;
}

template <int ES, int KIND, typename U> __device__ __forceinline__ SortComp<ES> comp_make(U u, uint32_t pos, bool desc) {
    const U key = sort_key<ES, KIND, U>(u, desc);
    if constexpr (ES == 4) return SortComp<4>{ ((uint64_t) key << 32) | pos };
    else return SortComp<8>{ key, pos };
}

/// `count` composites in LDS or in scratch: 4-byte types one array of words, 8-byte types the keys followed by the positions
template <int ES> struct CompStore {
    uint64_t *a;
    uint32_t *b;
    __device__ __forceinline__ SortComp<ES> get(size_t i) const {
        if constexpr (ES == 4) return SortComp<4>{ a[i] };
        else return SortComp<8>{ a[i], b[i] };
    }
    __device__ __forceinline__ void set(size_t i, const SortComp<ES> &c) const {
        if constexpr (ES == 4) a[i] = c.w;
        else { a[i] = c.key; b[i] = c.pos; }
    }
};
template <int ES> __host__ __device__ __forceinline__ CompStore<ES> comp_store(void *base, size_t count) {
    uint64_t *a = (uint64_t *) base;
    return CompStore<ES>{ a, (uint32_t *) (a + count) };
}
constexpr size_t comp_bytes(int es) { return es == 4 ? 8 : 12; }

/// Bitonic network over `slots` composites in LDS, a multiple of P = 2^k: every aligned run of P slots ends ascending.  A pair is
/// (lo, lo | j) with j < P: it never crosses a run.  All lanes of the workgroup call this; the slots are written and a barrier
/// has passed; it ends with a barrier.
/// (The stages with j <= 64 exchange inside one wave's 128 slots and could do with a wavefront-scope fence instead of the barrier:
/// tried, and it changed no time -- the stages are bound by their LDS traffic, not by the barriers.)
template <int ES> __device__ __forceinline__ void sort_bitonic(const CompStore<ES> &s, uint32_t slots, uint32_t P) {
    const uint32_t half = slots >> 1;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < half; t += blockDim.x) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const bool up = ((lo & (P - 1)) & k) == 0;
                const SortComp<ES> x = s.get(lo), y = s.get(hi);
                if (comp_less(y, x) == up) { s.set(lo, y); s.set(hi, x); }
            }
            __syncthreads();
        }
    }
}

/// how many of the first d entries of the merge of A (la entries) and B (lb entries) come from A; d <= la + lb
template <int ES>
__device__ __forceinline__ uint32_t sort_merge_path(const CompStore<ES> &s, size_t a, uint32_t la, size_t b, uint32_t lb, uint32_t d) {
    uint32_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);          // mid < la; 0 <= d - 1 - mid < lb
        if (comp_less(s.get(a + mid), s.get(b + (d - 1 - mid)))) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/// number of the `count` ascending composites from slot `first` on that are less than c
template <int ES> __device__ __forceinline__ uint32_t sort_rank(const CompStore<ES> &s, uint32_t first, uint32_t count, const SortComp<ES> &c) {
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (comp_less(s.get(first + mid), c)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/// do the `na` bytes at a and the `nb` bytes at b overlap (a null pointer overlaps nothing)
inline bool sort_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

} // namespace ek
