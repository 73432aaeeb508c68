// What the per-block primitives share (block_reduce.hip, block_scan.hip, block_search.hip, block_sort.hip: one result per block
// of B consecutive entries, or one per entry of every block; block_segments.hip: the same for ragged segments): the handling of a
// pointer that is only element-aligned, the way of an LDS tile out to such a pointer, the sum of a piece of a block or segment,
// the rule that splits few long blocks into pieces, the bounds of a ragged segment, and the argument checks.  The routes
// themselves are described at the top of each of the five files.
#pragma once

#include <cstdint>

// The one rule of this header that a plain host compiler can take as well (tests/cpp/segment_sum_host.cpp checks it there);
// everything behind it needs the HIP compiler.
#if defined(__HIPCC__)
#  define EK_BLOCK_RULE __host__ __device__ inline __attribute__((always_inline))
#else
#  define EK_BLOCK_RULE inline
#endif

namespace ek {

/// Ragged segments (block_segments.hip): segment j of an array of n entries is [lo, hi) with lo = min(start, n) and
/// hi = max(lo, min(next, n)), where `start` is starts[j] and `next` is starts[j + 1] (n behind the last start).  Whatever the two
/// values are -- above n, decreasing -- lo <= hi <= n.
EK_BLOCK_RULE void segment_clamp(uint32_t start, uint32_t next, uint32_t n, uint32_t &lo, uint32_t &hi) {
    lo = start < n ? start : n;
    const uint32_t e = next < n ? next : n;
    hi = e > lo ? e : lo;
}

} // namespace ek

#if defined(__HIPCC__)

#include "ek_reduce.h"

#include <algorithm>

namespace ek {

// ---- shapes (host) -----------------------------------------------------------------------------------------------------------
constexpr size_t kBlockTileBytes = 16 * 1024;     // a packed tile: whole blocks, staged in LDS
constexpr size_t kBlockPackedMax = 1024;          // entries: at least one vector width of blocks per tile for 4- and 8-byte types
constexpr size_t kBlockSplitMinPiece = 8192;      // entries: a block is split only from 16 Ki entries up
constexpr size_t kBlockSplitMaxPieces = kBlockPackedMax;   // (the pieces' partials are a block of the packed route)
constexpr size_t kBlockMaxGrid = 0x7FFFFFFFull;

/// blocks of B entries per packed tile: a multiple of the vector width, so that every tile starts at the base pointer's alignment;
/// `workgroups`: the capped grid over m blocks
inline uint32_t tile_blocks(size_t elem, size_t m, size_t B, size_t &workgroups) {
    const size_t N = 16 / elem, E = kBlockTileBytes / elem, t = std::max<size_t>(N, E / B / N * N);
    workgroups = std::min<size_t>((m + t - 1) / t, kBlockMaxGrid);
    return (uint32_t) t;
}

/// Fewer than 2 x #CU blocks of at least 16 Ki entries are cut into `splits` pieces of `piece` entries (a multiple of the vector
/// width: the pieces of a block share its alignment; the last may be shorter) so that about 4 x #CU workgroups run.
/// Returns whether the m blocks of B > kBlockPackedMax entries are split; splits = 1 and piece = B where they are not.
inline bool split_shape(size_t elem, size_t m, size_t B, size_t cu, size_t &splits, size_t &piece) {
    const size_t N = 16 / elem;
    splits = 1;
    piece = B;
    if (m >= 2 * cu) return false;
    const size_t S = std::min(std::min((4 * cu + m - 1) / m, B / kBlockSplitMinPiece), kBlockSplitMaxPieces);
    if (S < 2) return false;
    const size_t P = ((B + S - 1) / S + N - 1) / N * N, count = (B + P - 1) / P;        // (every piece holds at least one entry)
    if (count < 2) return false;
    splits = count;
    piece = P;
    return true;
}

// ---- argument checks (host): `what` is the entry point's name, which every message begins with -------------------------------
inline int numeric_type_check(const char *what, int type) {
    switch (type) {
        case EK_I32: case EK_U32: case EK_I64: case EK_U64: case EK_F32: case EK_F64: return EK_OK;
        default: return fail(EK_ERR_UNSUPPORTED, "%s: unsupported type %d", what, type);
    }
}

inline int blocks_shape_check(const char *what, size_t n, size_t block) {
    if (block == 0 || n % block != 0) return fail(EK_ERR_INVALID, "%s: %zu entries are no whole number of blocks of %zu", what, n, block);
    return EK_OK;
}

/// every pointer that is there is a multiple of `elem`, a power of two
template <typename... P> int alignment_check(const char *what, size_t elem, const P *...p) {
    if ((... | reinterpret_cast<uintptr_t>(p)) & (elem - 1)) return fail(EK_ERR_INVALID, "%s: pointer not aligned to the element size", what);
    return EK_OK;
}

/// ... and none is missing
template <typename... P> int pointers_check(const char *what, size_t elem, const P *...p) {
    if ((... || !p)) return fail(EK_ERR_INVALID, "%s: null pointer", what);
    return alignment_check(what, elem, p...);
}

/// f(ctype<type>{}) for the six numeric types (numeric_type_check has passed): `typename decltype(tag)::type` is the element type
template <typename F> __forceinline__ int dispatch_numeric(int type, F &&f) {
    switch (type) {
        case EK_I32: return f(ctype<EK_I32>{});
        case EK_U32: return f(ctype<EK_U32>{});
        case EK_I64: return f(ctype<EK_I64>{});
        case EK_U64: return f(ctype<EK_U64>{});
        case EK_F32: return f(ctype<EK_F32>{});
        default: return f(ctype<EK_F64>{});
    }
}

// ---- misaligned views (device; head_of also on the host) ---------------------------------------------------------------------
/// entries of `p` in front of its first 16-byte boundary (p is a multiple of sizeof(T)); R: the type it is computed and returned in
/// (the kernels that take it as a size_t keep their 64-bit arithmetic)
template <typename R = uint32_t, typename T> __host__ __device__ __forceinline__ R head_of(const T *p) {
    return (R) (((R(16) - (R) (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T));
}

/// All 256 lanes: `len` entries of the LDS tile (entry e at tile[e], tile + head on a 16-byte boundary of LDS) to dst, whose first
/// 16-byte boundary has `head` <= len entries in front: 16-byte non-temporal stores between those and the entries behind the last
template <typename T> __device__ __forceinline__ void tile_out(T *dst, const T *tile, uint32_t len, uint32_t head) {
    constexpr uint32_t N = 16 / sizeof(T);
    const uint32_t nvec = (len - head) / N, tail = len - head - nvec * N;
    if (threadIdx.x < head) dst[threadIdx.x] = tile[threadIdx.x];
#pragma unroll 4
    for (uint32_t v = threadIdx.x; v < nvec; v += 256)
        pack_store<T, N, true>(dst + head + v * N, *reinterpret_cast<const Pack<T, N> *>(tile + head + v * N));
    if (threadIdx.x < tail) dst[head + nvec * N + threadIdx.x] = tile[head + nvec * N + threadIdx.x];
}

/// All 256 lanes: the reduction of the `len` entries at src (a multiple of sizeof(T)), in thread 0.  The entries are streamed as
/// k_reduce_stage1 streams an array (16-byte non-temporal loads, four in flight per lane, four accumulators, the 256-thread fold);
/// those in front of the first 16-byte boundary and behind the last are taken one per lane.  len == 0: the identity.
template <typename R, typename T> __device__ __forceinline__ T reduce_piece(const T *__restrict__ src, size_t len) {
    constexpr uint32_t N = 16 / sizeof(T), U = 4;
    size_t head = head_of(src);
    if (head > len) head = len;
    const size_t nvec = (len - head) / N, tail = len - head - nvec * N;
    const T *vsrc = src + head;
    T acc[U];
#pragma unroll
    for (uint32_t k = 0; k < U; ++k) acc[k] = R::identity();
    for (size_t v0 = threadIdx.x; v0 < nvec; v0 += 256 * U) {
        Pack<T, N> p[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k)
            if (v0 + k * 256 < nvec) p[k] = pack_load<T, N, true>(vsrc + (v0 + k * 256) * N);
#pragma unroll
        for (uint32_t k = 0; k < U; ++k) {
            if (v0 + k * 256 < nvec) {
#pragma unroll
                for (uint32_t i = 0; i < N; ++i) acc[k] = R::combine(acc[k], p[k].v[i]);
            }
        }
    }
    if (threadIdx.x < head) acc[0] = R::combine(acc[0], src[threadIdx.x]);
    if (threadIdx.x < tail) acc[1] = R::combine(acc[1], vsrc[nvec * N + threadIdx.x]);
    const T v = R::combine(R::combine(acc[0], acc[1]), R::combine(acc[2], acc[3]));
    return block_reduce<R>(v);
}

/// segment = piece s of block j (S pieces of `piece` entries per block; S == 1: the whole block), one workgroup each
template <typename R, typename T>
__global__ __launch_bounds__(256) void k_reduce_segments(T *__restrict__ out, const T *__restrict__ in, size_t B, size_t piece, uint32_t S,
                                                         size_t segments) {
    for (size_t seg = blockIdx.x; seg < segments; seg += gridDim.x) {
        size_t j = seg, off = 0;
        if (S > 1) { j = seg / S; off = (seg - j * S) * piece; }
        const size_t len = B - off < piece ? B - off : piece;
        const T v = reduce_piece<R, T>(in + j * B + off, len);
        if (threadIdx.x == 0) out[seg] = v;
        __syncthreads();                                  // (block_reduce's LDS words are written again by the next segment)
    }
}

// ---- what block_segments.hip takes from block_reduce.hip --------------------------------------------------------------------
/// the packed block kernel over m blocks of B <= kBlockPackedMax entries: the fold of the m x B partials of a split route
int reduce_blocks_packed(int op, int type, void *out, const void *in, size_t m, size_t B);

} // namespace ek

#endif // __HIPCC__
