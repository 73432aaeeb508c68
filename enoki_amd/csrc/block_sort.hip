// Stable sort inside every block: for the n / B rows of B consecutive entries (the samples of a ray, a row of a row-major table)
//     perm[j * B + k] = the row-local position of the entry of row j that comes k-th in the order      (+ j * B with EK_SORT_FLAT_INDEX)
//     vals[j * B + k] = in[j * B + perm]                                                                 (the entry's own bits)
// The order is ascending by `<` (descending by `>` with EK_SORT_DESCENDING); entries that compare equal keep their input order;
// -0.0 == +0.0; every NaN, whatever its sign or payload, comes after all numbers in BOTH directions.  Per row this is exactly
// numpy.argsort(row, kind="stable"), and argsort(-row) / argsort(~row) for descending floats / integers.
//
// COMPOSITES.  No kernel sorts values: every entry becomes (key, position) with an order-preserving unsigned key
//     floats     u = bits, -0.0 -> +0.0;  key = u ^ (sign ? all ones : sign bit);  NaN -> all ones (no number maps there)
//     signed     key = bits ^ sign bit                    unsigned   key = bits
//     descending key = ~key, NaN still all ones
// and its 32-bit row-local position.  4-byte types: one 64-bit word key << 32 | position, one compare.  8-byte types: a 64-bit key
// and a 32-bit position in two arrays, compared lexicographically.  Composites of a row are distinct, so ANY correct network or
// merge yields the one stable order: the result is a function of the input alone, bit-identical from run to run.  Padding slots
// hold all ones in both parts, larger than any real composite (a position is at most 2^32 - 2).  Values leave as the ORIGINAL bits
// fetched through the sorted position, never rebuilt from a key.
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP: no ticket, no polling loop, no atomics.  What one workgroup needs from another is a later
// launch on the stream, so the call is capturable and no kernel of this file can spin.  No read-back, no host wait.
//
// sort_plan() picks the route (ek_hip_sort_blocks_plan reports it):
//   0 trivial            B == 1: a copy for values, zeros for row-local positions, 0, 1, 2, .. for flat positions.
//   1 packed             B <= 2048.  A workgroup of 256 lanes stages tile_rows = 2048 / P whole rows (P = B rounded up to a power
//                        of two) in LDS with 16-byte non-temporal loads; head / shift / tail as in k_reduce_packed, so a view that
//                        starts off a 16-byte boundary costs no more.  Row r of the tile owns composite slots [r * P, (r + 1) * P).
//                        One bitonic network runs over ALL slots at once: stage (k, j) pairs slot lo with lo | j, j < P, so a pair
//                        never leaves its row, and the direction comes from the ROW-LOCAL slot number (lo & (P - 1)) & k, so every
//                        row ends ascending.  log2(P) (log2(P) + 1) / 2 stages, one barrier each.  Then every lane takes its 8 result
//                        slots into registers (value from the staged row, position), and the composite area is REUSED as the two
//                        output tiles, which leave with 16-byte stores (tile_out, ek_block.h), each shifted for its own pointer's alignment.
//                        LDS: 2048 staged entries + 2048 composites: 24 KiB (4-byte types), 40 KiB (8-byte).  Rows of 1025 .. 2048
//                        entries are a tile of one row: the same 2048-slot network takes 2.2 ms here for 64 Mi float32 entries
//                        at B = 1025 and took 3.3 ms with the 1024 lanes of route 2.
//   2 one workgroup per row, 2048 < B <= chunk.  chunk = 8192 entries for 4-byte types, 4096 for 8-byte types: 64 and 48 KiB of
//                        composites, the most that still lets TWO workgroups of 1024 lanes share a CU, i.e. all 32 wave slots
//                        (DESIGN section 3).  The network has P = B rounded up to a power of two slots, not `chunk`, and the
//                        launch asks for P slots of LDS, so a row of 2049 .. 4096 entries runs a 4096-slot network.  Values are
//                        fetched from the row in global memory (at most 32 KiB, cache resident).
//   3 chunks and merges, B > chunk.  Launch 1 sorts every chunk of `chunk` entries of a row (the last may be shorter) with the
//                        route-2 kernel and writes its composites, positions already row-local, to scratch.  Then
//                        merge_passes = ceil(log2(ceil(B / chunk))) launches: pass p merges the adjacent runs 2q and 2q + 1 of
//                        chunk << p entries of the same row, from one scratch buffer to the other; a run without a partner is
//                        copied through by the same code (its partner has length 0).  A workgroup owns a FIXED tile of 2048 outputs;
//                        2048 divides every run length, so a tile lies in one pair.  Two lanes find where the tile's first and last
//                        diagonal cut the two runs (merge path: a binary search over global memory, bounded by the run lengths),
//                        the two pieces -- 2048 composites together -- go to LDS, every composite finds its rank in the OTHER piece
//                        by a binary search in LDS (composites are distinct: no tie rule), is written to its slot of a second LDS
//                        tile, and the tile leaves in order.  The last pass writes values (a divergent fetch from `in`) and
//                        positions in the caller's layout instead of composites.  1 + merge_passes launches, no fill launch.
//                        Scratch: one or two buffers of n composites from ek_hip_malloc, freed stream-ordered.
// Grids are capped; every kernel walks its tiles / segments in a grid-stride loop.  Positions are 32-bit (n < 2^32), global offsets
// size_t.  An output that was not asked for is neither computed into memory nor allocated.
// (The composites, the network and the two searches of a merge live in ek_sort.h, which segment_sort.hip shares.)
#include "ek_sort.h"

namespace ek {

constexpr uint32_t kSortTileSlots = 2048;          // route 1: composite slots (and staged entries) of a tile
constexpr size_t kSortPackedMaxBlock = kSortTileSlots;   // route 1: a tile holds one row at least
constexpr uint32_t kSortChunk4 = 8192, kSortChunk8 = 4096;   // routes 2, 3: entries of a row or chunk sorted by one workgroup
constexpr uint32_t kSortMergeTile = 2048;          // route 3: outputs per merge tile; divides both chunk sizes
constexpr size_t kSortMaxGrid = 0x7FFFFFFFull;
constexpr size_t kSortMaxEntries = 0xFFFFFFFFull;

struct SortPlan {
    int route, merge_passes;
    size_t tile_rows, chunk, workgroups;
    uint32_t P;                                   // 1, 2: slots of a row's network
};

static inline size_t sort_pow2_ceil(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }

static SortPlan sort_plan(size_t elem, size_t n, size_t B) {
    SortPlan p = { 0, 0, 1, elem == 4 ? kSortChunk4 : kSortChunk8, 0, 1 };
    if (n == 0 || B <= 1) return p;
    const size_t m = n / B;
    if (B <= kSortPackedMaxBlock) {
        p.route = 1;
        p.P = (uint32_t) sort_pow2_ceil(B);
        p.tile_rows = kSortTileSlots / p.P;
        p.workgroups = std::min((m + p.tile_rows - 1) / p.tile_rows, kSortMaxGrid);
    } else if (B <= p.chunk) {
        p.route = 2;
        p.P = (uint32_t) sort_pow2_ceil(B);
        p.workgroups = std::min(m, kSortMaxGrid);
    } else {
        p.route = 3;
        p.P = (uint32_t) p.chunk;
        const size_t runs = (B + p.chunk - 1) / p.chunk;
        while (((size_t) 1 << p.merge_passes) < runs) p.merge_passes++;
        p.workgroups = std::min(m * runs, kSortMaxGrid);
    }
    return p;
}

// ---- route 1: packed ---------------------------------------------------------------------------------------------------------
template <typename U, int KIND>
__global__ __launch_bounds__(256) void k_sort_packed(U *outv, uint32_t *outi, const U *in, size_t m, uint32_t B, uint32_t plog,
                                                     uint32_t tile_rows, size_t tiles, int flags) {
    constexpr int ES = sizeof(U);
    constexpr uint32_t N = 16 / ES, C = kSortTileSlots, PER = C / 256;
    __shared__ __attribute__((aligned(16))) U tile_in[C + N];
    // C composites; afterwards the value tile (C + N entries) and, from the next 16-byte boundary, the index tile (C + 4 entries)
    __shared__ __attribute__((aligned(16))) unsigned char area[C * (ES + 4) + 32];
    const CompStore<ES> comps = comp_store<ES>(area, C);
    U *const tile_v = reinterpret_cast<U *>(area);
    uint32_t *const tile_i = reinterpret_cast<uint32_t *>(area + (C + N) * ES);
    const bool desc = flags & EK_SORT_DESCENDING, flat = flags & EK_SORT_FLAT_INDEX;
    const uint32_t P = 1u << plog;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t r0 = t * tile_rows;
        const uint32_t nr = (uint32_t) (m - r0 < tile_rows ? m - r0 : tile_rows), len = nr * B;        // len <= C
        const U *src = in + r0 * B;
        uint32_t head = head_of(src);
        if (head > len) head = len;
        // entry e of the tile lives at tile_in[shift + e]: the first whole vector lands on a 16-byte boundary of LDS
        const uint32_t shift = (N - head) % N, nvec = (len - head) / N, tail = len - head - nvec * N;
        U *ti = tile_in + shift;
        if (threadIdx.x < head) ti[threadIdx.x] = src[threadIdx.x];
#pragma unroll 4
        for (uint32_t v = threadIdx.x; v < nvec; v += 256)
            *reinterpret_cast<Pack<U, N> *>(ti + head + v * N) = pack_load<U, N, true>(src + head + v * N);
        if (threadIdx.x < tail) ti[head + nvec * N + threadIdx.x] = src[head + nvec * N + threadIdx.x];
        __syncthreads();       // (also: the last tile's stores out of `area` are done)
        const uint32_t slots = nr << plog;
        for (uint32_t s = threadIdx.x; s < slots; s += 256) {
            const uint32_t r = s >> plog, k = s & (P - 1);
            comps.set(s, k < B ? comp_make<ES, KIND, U>(ti[r * B + k], k, desc) : comp_padding<ES>());
        }
        __syncthreads();
        sort_bitonic<ES>(comps, slots, P);
        // every lane takes its results into registers: `area` becomes the output tiles
        U val[PER];
        uint32_t idx[PER];
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t e = i * 256 + threadIdx.x;
            if (e < len) {
                const uint32_t r = e / B, k = e - r * B, pos = comp_pos(comps.get((r << plog) + k));
                val[i] = ti[r * B + pos];
                idx[i] = flat ? (uint32_t) (r0 * B) + r * B + pos : pos;
            }
        }
        __syncthreads();
        uint32_t vhead = 0, ihead = 0;
        if (outv) {
            vhead = head_of(outv + r0 * B);
            if (vhead > len) vhead = len;
        }
        if (outi) {
            ihead = head_of(outi + r0 * B);
            if (ihead > len) ihead = len;
        }
        U *tv = tile_v + (N - vhead) % N;
        uint32_t *tx = tile_i + (4 - ihead) % 4;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t e = i * 256 + threadIdx.x;
            if (e < len) {
                if (outv) tv[e] = val[i];
                if (outi) tx[e] = idx[i];
            }
        }
        __syncthreads();
        if (outv) tile_out<U>(outv + r0 * B, tv, len, vhead);
        if (outi) tile_out<uint32_t>(outi + r0 * B, tx, len, ihead);
    }
}

// ---- routes 2 and 3, launch 1: a workgroup sorts a row, or chunk c of a row ----------------------------------------------------
// `scratch.a` set: the sorted composites go to scratch (route 3); else values and positions go to the caller (route 2)
template <typename U, int KIND>
__global__ __launch_bounds__(1024) void k_sort_chunks(U *outv, uint32_t *outi, CompStore<sizeof(U)> scratch, const U *in, size_t B,
                                                      uint32_t chunk, size_t full_per_row, size_t full_segments, size_t segments, uint32_t capacity,
                                                      int flags) {
    constexpr int ES = sizeof(U);
    extern __shared__ __attribute__((aligned(16))) unsigned char sort_lds[];
    const CompStore<ES> comps = comp_store<ES>(sort_lds, capacity);
    const bool desc = flags & EK_SORT_DESCENDING, flat = flags & EK_SORT_FLAT_INDEX;
    for (size_t seg = blockIdx.x; seg < segments; seg += gridDim.x) {
        // the full chunks of all rows first, then the rows' shorter last chunks: consecutive workgroups go to different XCDs, and
        // numbering the chunks row by row would hand every short chunk of rows of chunk + 1 entries to the same half of them
        const bool whole = seg < full_segments;
        const size_t row = whole ? seg / full_per_row : seg - full_segments;
        const size_t off = (whole ? seg - row * full_per_row : full_per_row) * chunk;
        const uint32_t len = (uint32_t) (B - off < chunk ? B - off : chunk);
        const uint32_t P = len <= 1 ? 1u : 1u << (32 - __clz(len - 1));              // <= capacity
        const U *src = in + row * B;
        for (uint32_t k = threadIdx.x; k < P; k += 1024)
            comps.set(k, k < len ? comp_make<ES, KIND, U>(src[off + k], (uint32_t) off + k, desc) : comp_padding<ES>());
        __syncthreads();
        sort_bitonic<ES>(comps, P, P);
        const size_t g0 = row * B + off;
        if (scratch.a) {
            for (uint32_t k = threadIdx.x; k < len; k += 1024) scratch.set(g0 + k, comps.get(k));
        } else {
            for (uint32_t k = threadIdx.x; k < len; k += 1024) {
                const uint32_t pos = comp_pos(comps.get(k));
                if (outv) outv[g0 + k] = src[pos];
                if (outi) outi[g0 + k] = flat ? (uint32_t) (row * B) + pos : pos;
            }
        }
        __syncthreads();        // (the next segment writes the slots again)
    }
}

// ---- route 3, launches 2 ..: merge the adjacent runs of `run` entries of every row --------------------------------------------
template <typename U>
__global__ __launch_bounds__(256) void k_sort_merge(U *outv, uint32_t *outi, CompStore<sizeof(U)> dst, CompStore<sizeof(U)> src, const U *in,
                                                    size_t B, size_t run, size_t tiles_per_row, size_t tiles, int flags) {
    constexpr int ES = sizeof(U);
    constexpr uint32_t TM = kSortMergeTile;
    __shared__ __attribute__((aligned(16))) unsigned char lds_in[TM * comp_bytes(ES)];
    __shared__ __attribute__((aligned(16))) unsigned char lds_out[TM * comp_bytes(ES)];
    __shared__ uint32_t s_cut[2];
    const CompStore<ES> pieces = comp_store<ES>(lds_in, TM), merged = comp_store<ES>(lds_out, TM);
    const bool flat = flags & EK_SORT_FLAT_INDEX;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t row = t / tiles_per_row, o0 = (t - row * tiles_per_row) * TM;       // the tile's first output, row-local
        const uint32_t tl = (uint32_t) (B - o0 < TM ? B - o0 : TM);
        const size_t pair = o0 / (2 * run) * (2 * run);                                  // the pair's first entry, row-local
        const uint32_t la = (uint32_t) (B - pair < run ? B - pair : run);
        const uint32_t lb = (uint32_t) (B - pair - la < run ? B - pair - la : run);      // 0: a run without a partner
        const size_t ga = row * B + pair, gb = ga + la;
        const uint32_t d0 = (uint32_t) (o0 - pair), d1 = d0 + tl;                        // d1 <= la + lb: TM divides 2 * run
        if (threadIdx.x == 0) s_cut[0] = sort_merge_path<ES>(src, ga, la, gb, lb, d0);
        if (threadIdx.x == 64) s_cut[1] = sort_merge_path<ES>(src, ga, la, gb, lb, d1);
        __syncthreads();
        const uint32_t a0 = s_cut[0], a1 = s_cut[1], b0 = d0 - a0, na = a1 - a0, nb = tl - na;
        for (uint32_t i = threadIdx.x; i < tl; i += 256)
            pieces.set(i, i < na ? src.get(ga + a0 + i) : src.get(gb + b0 + (i - na)));
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < tl; i += 256) {
            const SortComp<ES> c = pieces.get(i);
            const uint32_t slot = i < na ? i + sort_rank<ES>(pieces, na, nb, c) : (i - na) + sort_rank<ES>(pieces, 0, na, c);
            merged.set(slot, c);
        }
        __syncthreads();
        const size_t g0 = row * B + o0;
        if (dst.a) {
            for (uint32_t i = threadIdx.x; i < tl; i += 256) dst.set(g0 + i, merged.get(i));
        } else {
            for (uint32_t i = threadIdx.x; i < tl; i += 256) {
                const uint32_t pos = comp_pos(merged.get(i));
                if (outv) outv[g0 + i] = in[row * B + pos];
                if (outi) outi[g0 + i] = flat ? (uint32_t) (row * B) + pos : pos;
            }
        }
        // (no barrier here: the next tile writes s_cut and `pieces` after everybody passed the barrier above, and `merged` only
        //  after its own two barriers)
    }
}

__global__ __launch_bounds__(256) void k_sort_iota(uint32_t *out, size_t n) {
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t) gridDim.x * 256) out[i] = (uint32_t) i;
}

template <typename U, int KIND>
static int sort_blocks_typed(void *outv_, uint32_t *outi, const void *in_, size_t n, size_t B, const SortPlan &p, int flags) {
    RoctxRange range("enoki-hip: block sort");
    constexpr int ES = sizeof(U);
    Context &c = ctx();
    U *outv = (U *) outv_;
    const U *in = (const U *) in_;
    const size_t m = n / B, out_bytes = n * ((outv ? ES : 0) + (outi ? 4 : 0));
    if (p.route == 1) {
        uint32_t plog = 0;
        while ((1u << plog) < p.P) plog++;
        const size_t tiles = (m + p.tile_rows - 1) / p.tile_rows;
        hipLaunchKernelGGL((k_sort_packed<U, KIND>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, outv, outi, in, m, (uint32_t) B, plog,
                           (uint32_t) p.tile_rows, tiles, flags);
        EK_LAUNCH_CHECK("sort_blocks_packed", n, n * ES + out_bytes);
        return EK_OK;
    }
    if (p.route == 2) {
        hipLaunchKernelGGL((k_sort_chunks<U, KIND>), dim3((unsigned) p.workgroups), dim3(1024), p.P * comp_bytes(ES), c.stream, outv, outi,
                           CompStore<ES>{ nullptr, nullptr }, in, B, (uint32_t) B, (size_t) 1, m, m, p.P, flags);
        EK_LAUNCH_CHECK("sort_blocks_rows", n, n * ES + out_bytes);
        return EK_OK;
    }
    const size_t runs = (B + p.chunk - 1) / p.chunk, cb = comp_bytes(ES), buf_bytes = (n * cb + 15) / 16 * 16;
    void *scratch = nullptr;
    if (int rc = ek_hip_malloc(buf_bytes * (p.merge_passes > 1 ? 2 : 1), &scratch)) return rc;
    CompStore<ES> bufs[2] = { comp_store<ES>(scratch, n), comp_store<ES>((unsigned char *) scratch + buf_bytes, n) };
    int rc = EK_OK;
    do {
        hipLaunchKernelGGL((k_sort_chunks<U, KIND>), dim3((unsigned) p.workgroups), dim3(1024), p.chunk * cb, c.stream, (U *) nullptr,
                           (uint32_t *) nullptr, bufs[0], in, B, (uint32_t) p.chunk, B / p.chunk, m * (B / p.chunk), m * runs,
                           (uint32_t) p.chunk, flags);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort_blocks(): the chunk launch failed"); break; }
        note_launch("sort_blocks_chunks", n, n * (ES + cb));
        const size_t tiles_per_row = (B + kSortMergeTile - 1) / kSortMergeTile, tiles = m * tiles_per_row;
        const unsigned grid = (unsigned) std::min(tiles, kSortMaxGrid);
        for (int pass = 0; pass < p.merge_passes; ++pass) {
            const bool last = pass + 1 == p.merge_passes;
            hipLaunchKernelGGL((k_sort_merge<U>), dim3(grid), dim3(256), 0, c.stream, outv, outi,
                               last ? CompStore<ES>{ nullptr, nullptr } : bufs[(pass + 1) & 1], bufs[pass & 1], in, B, p.chunk << pass, tiles_per_row,
                               tiles, flags);
            if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort_blocks(): a merge launch failed"); break; }
            note_launch("sort_blocks_merge", n, n * cb + (last ? n * ES + out_bytes : n * cb));
        }
    } while (false);
    ek_hip_free(scratch);   // stream-ordered reuse
    return rc;
}

static int sort_shape_check(const char *what, size_t n, size_t block) {
    if (int rc = blocks_shape_check(what, n, block)) return rc;
    if (n > kSortMaxEntries) return fail(EK_ERR_UNSUPPORTED, "%s: %zu entries, more than 2^32 - 1", what, n);
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_sort_blocks_plan(int type, size_t n, size_t block, int want_index, int compute_units, int *route, size_t *tile_rows,
                            size_t *chunk, int *merge_passes, size_t *workgroups) {
    (void) want_index;          // the index travels inside the composite either way: it changes no route
    if (int rc = numeric_type_check("ek_hip_sort_blocks_plan()", type)) return rc;
    if (int rc = sort_shape_check("ek_hip_sort_blocks_plan()", n, block)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_sort_blocks_plan(): %d compute units", compute_units);
    const SortPlan p = sort_plan(type_size(type), n, block);
    if (route) *route = p.route;
    if (tile_rows) *tile_rows = p.tile_rows;
    if (chunk) *chunk = p.chunk;
    if (merge_passes) *merge_passes = p.merge_passes;
    if (workgroups) *workgroups = p.workgroups;
    return EK_OK;
}

int ek_hip_sort_blocks(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, size_t block, int flags) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_sort_blocks()", type)) return rc;
    if (flags & ~(EK_SORT_DESCENDING | EK_SORT_FLAT_INDEX)) return fail(EK_ERR_INVALID, "ek_hip_sort_blocks(): unknown flags %d", flags);
    if (int rc = sort_shape_check("ek_hip_sort_blocks()", n, block)) return rc;
    if (!out_values && !out_index) return fail(EK_ERR_INVALID, "ek_hip_sort_blocks(): no output");
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_sort_blocks()", elem, in)) return rc;
    // (an output that was not asked for is a null pointer: aligned)
    if (int rc = alignment_check("ek_hip_sort_blocks()", elem, out_values)) return rc;
    if (int rc = alignment_check("ek_hip_sort_blocks()", 4, out_index)) return rc;
    if (sort_overlap(in, n * elem, out_values, n * elem) || sort_overlap(in, n * elem, out_index, n * 4) ||
        sort_overlap(out_values, n * elem, out_index, n * 4))
        return fail(EK_ERR_INVALID, "ek_hip_sort_blocks(): in and the outputs overlap");
    const SortPlan p = sort_plan(elem, n, block);
    if (p.route == 0) {
        if (out_values)
            if (int rc = ek_hip_memcpy_device(out_values, in, n * elem)) return rc;
        if (out_index) {
            if (!(flags & EK_SORT_FLAT_INDEX)) return ek_hip_memset(out_index, 0, n * 4);
            hipLaunchKernelGGL(k_sort_iota, dim3(stream_grid(n, ctx().tuning.blocks_per_cu)), dim3(256), 0, ctx().stream, out_index, n);
            EK_LAUNCH_CHECK("sort_blocks_iota", n, n * 4);
        }
        return EK_OK;
    }
    switch (type) {
        case EK_I32: return sort_blocks_typed<uint32_t, kSortSigned>(out_values, out_index, in, n, block, p, flags);
        case EK_U32: return sort_blocks_typed<uint32_t, kSortUnsigned>(out_values, out_index, in, n, block, p, flags);
        case EK_I64: return sort_blocks_typed<uint64_t, kSortSigned>(out_values, out_index, in, n, block, p, flags);
        case EK_U64: return sort_blocks_typed<uint64_t, kSortUnsigned>(out_values, out_index, in, n, block, p, flags);
        case EK_F32: return sort_blocks_typed<uint32_t, kSortFloat>(out_values, out_index, in, n, block, p, flags);
        default: return sort_blocks_typed<uint64_t, kSortFloat>(out_values, out_index, in, n, block, p, flags);
    }
}

}
