// segment_search_sorted: every needle is searched in ITS OWN ragged segment of a flat table; the result is the segment-local count
// of entries t with t < v (right: t <= v), or with EK_SEARCH_FLAT that count plus the segment's clamped start, in ONE launch.  The
// counterpart of block_search.hip for what compress(), a per-ray sample count or a mesh leave behind: segment j of the table is
// [lo_j, hi_j) = segment_clamp(table_starts[j], table_starts[j + 1], nt) (ek_block.h; table_starts[m] := nt), and the segment of a
// needle is named either by needle_starts (needle e belongs to the last j with needle_starts[j] <= e, the rule of
// ek_hip_repeat_segments; no segment in front of needle_starts[0]) or by a row per needle (clamped to m - 1).
//
// The spelling this replaces builds an n-entry row array with repeat_segments, gathers table_starts twice and runs
// log2(longest segment) + 1 rounds of min / add / gather+compare / select / select over n-element arrays -- and needs the longest
// segment, which lives on the device, for its trip count.
//
// Everything below the routes is ek_search.h: 512-thread workgroups, 64 KiB of LDS (two workgroups per CU), 4 needles per lane as
// independent chains in lockstep, the branch-free step with every read clamped, 16-byte non-temporal needle loads and index
// stores, the per-job peel and tail of search_range.  The routes are chosen from (type, nt, m, n, #CU) alone:
//
//   1 paired tiles    needle_starts given.  Needle-driven: a workgroup owns a run of consecutive tiles of 2048 needles, so the work
//                     is balanced whatever the starts hold.  For its first tile it finds j0 = #(needle_starts <= first needle) by
//                     an upper-bound search in global memory; later tiles take it from the window of the tile before.  A tile
//                     stages a WINDOW of needle_starts from j0 - 1 on, 512 at a time until one lies behind the tile (at most
//                     kSegSearchWindow), and the same range of table_starts plus the one behind it (or nt).  The table entries of
//                     the tile's segments are then one contiguous SPAN (the starts are expected to ascend), of which the first
//                     kSegSearchSpanBytes are staged with 16-byte loads.  Each needle finds its segment by an upper bound in the
//                     staged needle starts and clamps its [lo, hi).  A needle whose clamped segment lies inside the staged span is
//                     searched there; any other -- a span too long, decreasing starts -- is searched in global memory with the same
//                     steps, reads clamped to nt - 1.  A needle at or behind the last staged start of a window that did not reach
//                     the tile's end finds its segment in needle_starts itself.  These per-needle tests are what makes the
//                     bad-input contract hold without a second code path: slow but correct.
//   2 indexed, LDS    rows given, nt * sizeof(T) <= 64 KiB: the table is staged whole once per workgroup.
//   3 indexed, global rows given, larger table: every step reads global memory.  What this route saves over the loop is launches and
//                     index traffic, not bandwidth.
//                     In both, lo / hi come from two clamped reads of table_starts per needle.
//
// The first step of a lane's searches is the largest power of two <= the longest clamped segment among ITS chains: a lane whose
// segments are short leaves the loop early (its reads are not issued at all), and a 64-entry segment pays 7 steps wherever it lies.
//
// LDS: the staged searches read 4 or 8 bytes per lane at data-dependent addresses.  The first steps of the needles of one segment
// read the same word (a broadcast); the last steps spread over the segment's entries, where conflicts are what a binary search
// costs.  64 KiB per workgroup of 512 lanes: two workgroups, 16 waves, per CU.
//
// Whatever the three index arrays hold: every read of the table is clamped into [0, nt), every read of a starts array lies below
// m, every output entry is written once by the lane that owns it, every loop has a trip count bounded by a constant, log2(nt) or
// log2(m).  No atomics, no scratch memory, nothing read back, no kernel waits for another workgroup: capturable, and bit-identical
// from run to run.
#include "ek_search.h"

namespace ek {

constexpr uint32_t kSegSearchTile = kSearchBlock * kSearchLane;        // needles per tile: one item per lane
constexpr uint32_t kSegSearchWindow = kSegSearchTile + 4;              // starts per window: a tile of one-needle segments, the
                                                                       // start in front and the one behind
constexpr size_t kSegSearchSpanBytes = 48 * 1024 - 256;                // table entries a tile stages (the window takes 16.1 KiB)

enum { kSegRouteNone = 0, kSegRoutePaired = 1, kSegRouteIndexedLds = 2, kSegRouteIndexedGlobal = 3 };

struct SegmentSearchPlan {
    int route;
    size_t tiles_per_workgroup, workgroups;
    size_t lds_entries;          // 1: entries of a tile's span that are staged; 2, 3: the largest table that is staged whole
    size_t window;               // 1: starts a tile stages; 2, 3: 0
};

static SegmentSearchPlan segment_search_plan(size_t elem_size, size_t nt, size_t n, bool indexed, int num_cu) {
    SegmentSearchPlan p = { kSegRouteNone, 0, 0, 0, 0 };
    p.lds_entries = (indexed ? kSearchLdsBytes : kSegSearchSpanBytes) / elem_size;
    p.window = indexed ? 0 : kSegSearchWindow;
    if (n == 0) return p;
    const size_t cap = (size_t) (num_cu > 0 ? num_cu : 256) * kSearchBlocksPerCu, tiles = (n + kSegSearchTile - 1) / kSegSearchTile;
    p.route = !indexed ? kSegRoutePaired : nt <= p.lds_entries ? kSegRouteIndexedLds : kSegRouteIndexedGlobal;
    p.tiles_per_workgroup = (tiles + std::min(cap, tiles) - 1) / std::min(cap, tiles);
    p.workgroups = (tiles + p.tiles_per_workgroup - 1) / p.tiles_per_workgroup;
    return p;
}

/// the largest power of two <= x (0 for 0)
__device__ __forceinline__ uint32_t floor_pow2(uint32_t x) { return x ? 1u << (31 - __clz(x)) : 0u; }

/// route 1: workgroup w owns the tiles [w * per_workgroup, (w + 1) * per_workgroup) of kSegSearchTile needles
template <typename T, bool Right>
__global__ __launch_bounds__(kSearchBlock) void k_segment_search_paired(uint32_t *__restrict__ out, const T *__restrict__ table, uint32_t nt,
                                                                        const uint32_t *__restrict__ table_starts, uint32_t m,
                                                                        const T *__restrict__ needles, uint32_t n,
                                                                        const uint32_t *__restrict__ needle_starts, uint32_t top_m,
                                                                        uint32_t tiles, uint32_t per_workgroup, uint32_t flat) {
    constexpr uint32_t W = kSegSearchWindow, E = (uint32_t) (kSegSearchSpanBytes / sizeof(T));
    __shared__ __attribute__((aligned(16))) T lds[E];
    __shared__ uint32_t nwin[W];             // needle_starts[ws .. ws + cnt)
    __shared__ uint32_t twin[W + 4];         // table_starts[ws .. ws + cnt], nt behind the last start
    const uint32_t t0 = blockIdx.x * per_workgroup, t1 = tiles - t0 < per_workgroup ? tiles : t0 + per_workgroup;   // (t0 < tiles)
    uint32_t j0 = 0;                         // the number of needle starts <= the tile's first needle
    bool known = false;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t e0 = t * kSegSearchTile, e1 = n - e0 < kSegSearchTile ? n : e0 + kSegSearchTile;             // e0 < e1 <= n
        if (!known) {
            const uint32_t at[1] = { e0 }, zero[1] = { 0 }, all[1] = { m };
            uint32_t pos[1] = { 0 };
            search_steps<uint32_t, true, 1>(needle_starts, zero, zero, all, m - 1, top_m, at, pos);
            j0 = pos[0];                                                                          // <= m
        }
        // the window begins at the segment of the tile's first needle
        const uint32_t ws = j0 ? j0 - 1 : 0u, room = m - ws < W ? m - ws : W;                     // ws <= m
        uint32_t cnt = 0;
        bool reached = room == 0;
        while (cnt < room) {
            const uint32_t step = room - cnt < (uint32_t) kSearchBlock ? room - cnt : (uint32_t) kSearchBlock;
            if (threadIdx.x < step) {
                nwin[cnt + threadIdx.x] = needle_starts[ws + cnt + threadIdx.x];                  // ws + cnt + step <= ws + room <= m
                twin[cnt + threadIdx.x] = table_starts[ws + cnt + threadIdx.x];
            }
            __syncthreads();
            cnt += step;
            reached = ws + cnt == m || nwin[cnt - 1] >= e1;
            if (reached) break;
        }
        if (threadIdx.x == 0) twin[cnt] = ws + cnt < m ? table_starts[ws + cnt] : nt;             // cnt <= W
        __syncthreads();
        const uint32_t wtop = floor_pow2(cnt), behind = cnt ? nwin[cnt - 1] : 0u;
        // q: the staged starts <= the tile's last needle; the span of the segments ws .. ws + q - 1, cut to what LDS takes
        uint32_t q = 0;
        if (cnt) {
            const uint32_t at[1] = { e1 - 1 }, zero[1] = { 0 }, all[1] = { cnt };
            uint32_t pos[1] = { 0 };
            search_steps<uint32_t, true, 1>(nwin, zero, zero, all, cnt - 1, wtop, at, pos);
            q = pos[0];                                                                           // <= cnt
        }
        uint32_t span_lo = 0, span_hi = 0;
        if (q) {
            segment_clamp(twin[0], twin[q], nt, span_lo, span_hi);
            if (span_hi - span_lo > E) span_hi = span_lo + E;
        }
        const uint32_t span = span_hi - span_lo;                                                  // span_lo + span <= nt
        stage_entries<T>(lds, table + span_lo, span);
        __syncthreads();
        search_range<T>(out, needles, e0, e1, [&](const auto &v, size_t j, auto &r) {
            constexpr int K = (int) (sizeof(v) / sizeof(T));
            uint32_t e[K], p[K], zero[K], all[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { e[k] = e0 + (uint32_t) j + k; p[k] = 0; zero[k] = 0; all[k] = cnt; }
            if (cnt) search_steps<uint32_t, true, K>(nwin, zero, zero, all, cnt - 1, wtop, e, p);
            uint32_t lo[K], len[K];
            bool far = false;                                       // a needle of this lane lies behind what the window covers
#pragma unroll
            for (int k = 0; k < K; ++k) {
                lo[k] = 0; len[k] = 0;
                if (p[k]) {                                         // twin[p] exists: p <= cnt
                    uint32_t hi;
                    segment_clamp(twin[p[k] - 1], twin[p[k]], nt, lo[k], hi);
                    len[k] = hi - lo[k];
                }
                far |= !reached && e[k] >= behind;
            }
            if (far) {                                              // (not reached: m > ws + cnt >= 1)
                uint32_t g[K];
#pragma unroll
                for (int k = 0; k < K; ++k) { g[k] = 0; all[k] = m; }
                search_steps<uint32_t, true, K>(needle_starts, zero, zero, all, m - 1, top_m, e, g);                 // <= m
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (e[k] >= behind) {
                        lo[k] = 0; len[k] = 0;
                        if (g[k]) {
                            uint32_t hi;
                            segment_clamp(table_starts[g[k] - 1], g[k] < m ? table_starts[g[k]] : nt, nt, lo[k], hi);
                            len[k] = hi - lo[k];
                        }
                    }
                }
            }
            // staged or not, per needle; a segment of no entries is searched nowhere
            uint32_t first[K], count[K], longest = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool inside = lo[k] >= span_lo && lo[k] + len[k] <= span_hi;                // lo + len <= nt: no wrap
                first[k] = inside ? lo[k] - span_lo : 0u;
                count[k] = inside ? len[k] : 0u;
                longest = max(longest, count[k]);
                r[k] = 0;
            }
            if (longest) search_steps<T, Right, K>(lds, zero, first, count, span - 1, floor_pow2(longest), v, r);    // span >= longest
            longest = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                count[k] = count[k] ? 0u : len[k];
                longest = max(longest, count[k]);
            }
            if (longest) search_steps<T, Right, K>(table, zero, lo, count, nt - 1, floor_pow2(longest), v, r);       // nt >= longest
            if (flat) {
#pragma unroll
                for (int k = 0; k < K; ++k) r[k] += lo[k];                                       // <= hi <= nt
            }
        });
        known = reached;
        if (reached && cnt) {                                       // the next tile begins at e1
            const uint32_t at[1] = { e1 }, zero[1] = { 0 }, all[1] = { cnt };
            uint32_t pos[1] = { 0 };
            search_steps<uint32_t, true, 1>(nwin, zero, zero, all, cnt - 1, wtop, at, pos);
            j0 = ws + pos[0];                                                                     // <= ws + cnt <= m
        }
        __syncthreads();                                            // the searches are done with the window and the span
    }
}

/// routes 2 and 3: the segment of every needle comes from `rows`, clamped to m - 1 (m >= 1)
template <typename T, bool Right, bool Resident>
__global__ __launch_bounds__(kSearchBlock) void k_segment_search_indexed(uint32_t *__restrict__ out, const T *__restrict__ table, uint32_t nt,
                                                                         const uint32_t *__restrict__ table_starts, uint32_t m,
                                                                         const T *__restrict__ needles, const uint32_t *__restrict__ rows,
                                                                         size_t n, uint32_t peel, int needles_vec, int rows_vec,
                                                                         uint32_t flat) {
    constexpr int N = kSearchLane;
    __shared__ __attribute__((aligned(16))) T lds[Resident ? kSearchLdsBytes / sizeof(T) : 1];
    if constexpr (Resident) {
        stage_entries<T>(lds, table, nt);
        __syncthreads();
    }
    const T *mem = Resident ? lds : table;
    auto search = [&](const auto &v, const auto &row, auto &r) {
        constexpr int K = (int) (sizeof(v) / sizeof(T));
        uint32_t zero[K], lo[K], count[K], longest = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t j = min(row[k], m - 1);
            uint32_t hi;
            segment_clamp(table_starts[j], j + 1 < m ? table_starts[j + 1] : nt, nt, lo[k], hi);
            count[k] = hi - lo[k];
            longest = max(longest, count[k]);
            zero[k] = 0; r[k] = 0;
        }
        if (longest) search_steps<T, Right, K>(mem, zero, lo, count, nt - 1, floor_pow2(longest), v, r);             // nt >= longest
        if (flat) {
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] += lo[k];
        }
    };
    const size_t items = (n - peel) / N;
    for (size_t item = (size_t) blockIdx.x * kSearchBlock + threadIdx.x; item < items; item += (size_t) gridDim.x * kSearchBlock) {
        const size_t e = peel + item * N;
        T v[N];
        uint32_t row[N];
        search_load<T, N>(needles + e, needles_vec, v);
        search_load<uint32_t, N>(rows + e, rows_vec, row);
        Pack<uint32_t, N> r;
        search(v, row, r.v);
        pack_store<uint32_t, N, true>(out + e, r);
    }
    const uint32_t rest = peel + (uint32_t) ((n - peel) - items * N);
    if (blockIdx.x == 0 && threadIdx.x < rest) {
        const size_t e = threadIdx.x < peel ? threadIdx.x : peel + items * N + (threadIdx.x - peel);
        const T v[1] = { needles[e] };
        const uint32_t row[1] = { rows[e] };
        uint32_t r[1];
        search(v, row, r);
        out[e] = r[0];
    }
}

/// one launch on the context's stream; the arguments are converted to the kernel's parameter types
template <typename... Params, typename... Args>
static void segment_search_launch(void (*kernel)(Params...), size_t grid, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned) grid), dim3(kSearchBlock), 0, ctx().stream, (Params) args...);
}

template <typename T>
static int segment_search_sorted(uint32_t *out, const void *table_, size_t nt, const uint32_t *table_starts, size_t m, const void *needles_,
                                 size_t n, const uint32_t *needle_starts, const uint32_t *rows, int flags) {
    RoctxRange range("enoki-hip: segment_search_sorted");
    const T *table = (const T *) table_, *needles = (const T *) needles_;
    const SegmentSearchPlan p = segment_search_plan(sizeof(T), nt, n, rows != nullptr, ctx().num_cu);
    const bool right = (flags & EK_SEARCH_RIGHT) != 0;
    const uint32_t flat = (flags & EK_SEARCH_FLAT) ? 1u : 0u;
    if (p.route == kSegRoutePaired) {
        const size_t tiles = (n + kSegSearchTile - 1) / kSegSearchTile;
        segment_search_launch(right ? k_segment_search_paired<T, true> : k_segment_search_paired<T, false>, p.workgroups, out, table, nt,
                              table_starts, m, needles, n, needle_starts, search_top(m), tiles, p.tiles_per_workgroup, flat);
    } else {
        size_t peel = head_of(out);
        if (peel > n) peel = n;
        const bool lds = p.route == kSegRouteIndexedLds;
        segment_search_launch(lds ? (right ? k_segment_search_indexed<T, true, true> : k_segment_search_indexed<T, false, true>)
                                  : (right ? k_segment_search_indexed<T, true, false> : k_segment_search_indexed<T, false, false>),
                              p.workgroups, out, table, nt, table_starts, m, needles, rows, n, peel, aligned16(needles + peel),
                              aligned16(rows + peel), flat);
    }
    // the table once (route 3 reads what the needles point at, counted as the table all the same), needle in, index out, both
    // starts once or a row per needle and its two starts
    EK_LAUNCH_CHECK("segment_search_sorted", n, nt * sizeof(T) + n * (sizeof(T) + sizeof(uint32_t)) + (rows ? n * 4 + m * 4 : m * 8));
    return EK_OK;
}

/// everything ek_hip_search_sorted_segments and its plan refuse from the sizes alone
static int segment_search_check(const char *what, int type, size_t nt, size_t m, size_t n) {
    if (int rc = numeric_type_check(what, type)) return rc;
    if (nt > 0xFFFFFFFFull || m > 0xFFFFFFFFull || n > 0xFFFFFFFFull)
        return fail(EK_ERR_UNSUPPORTED, "%s: 2^32 entries, segments or needles or more are unsupported (%zu, %zu, %zu)", what, nt, m, n);
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_search_sorted_segments_plan(int type, size_t nt, size_t m, size_t n, int indexed, int compute_units, int *route,
                                       size_t *tile_needles, size_t *tiles_per_workgroup, size_t *workgroups, size_t *lds_entries,
                                       size_t *window) {
    const char *what = "ek_hip_search_sorted_segments_plan()";
    if (int rc = segment_search_check(what, type, nt, m, n)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "%s: %d compute units", what, compute_units);
    if (indexed && m == 0 && n != 0) return fail(EK_ERR_INVALID, "%s: %zu needles and no segment to search", what, n);
    const SegmentSearchPlan p = segment_search_plan(type_size(type), nt, n, indexed != 0, compute_units);
    if (route) *route = p.route;
    if (tile_needles) *tile_needles = kSegSearchTile;
    if (tiles_per_workgroup) *tiles_per_workgroup = p.tiles_per_workgroup;
    if (workgroups) *workgroups = p.workgroups;
    if (lds_entries) *lds_entries = p.lds_entries;
    if (window) *window = p.window;
    return EK_OK;
}

int ek_hip_search_sorted_segments(int type, uint32_t *out, const void *table, size_t nt, const uint32_t *table_starts, size_t m,
                                  const void *needles, size_t n, const uint32_t *needle_starts, const uint32_t *row_index, int flags) {
    const char *what = "ek_hip_search_sorted_segments()";
    if (int rc = ensure_init()) return rc;
    if (int rc = segment_search_check(what, type, nt, m, n)) return rc;
    if (flags & ~(EK_SEARCH_RIGHT | EK_SEARCH_FLAT)) return fail(EK_ERR_INVALID, "%s: unknown flags 0x%x", what, (unsigned) flags);
    if (needle_starts && row_index) return fail(EK_ERR_INVALID, "%s: needle_starts and row_index are both given", what);
    // (no segments: there is no needle_starts array to point at, and every needle is in front of every segment)
    if (!needle_starts && !row_index && m != 0) return fail(EK_ERR_INVALID, "%s: neither needle_starts nor row_index is given", what);
    if (row_index && m == 0 && n != 0) return fail(EK_ERR_INVALID, "%s: %zu needles and no segment to search", what, n);
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check(what, sizeof(uint32_t), out)) return rc;
    if (int rc = pointers_check(what, elem, needles)) return rc;
    if (int rc = nt ? pointers_check(what, elem, table) : alignment_check(what, elem, table)) return rc;
    if (int rc = m ? pointers_check(what, sizeof(uint32_t), table_starts) : alignment_check(what, sizeof(uint32_t), table_starts)) return rc;
    if (int rc = alignment_check(what, sizeof(uint32_t), needle_starts, row_index)) return rc;
    if (m == 0 || nt == 0) {                              // every count is 0, and so is every clamped start
        RoctxRange range("enoki-hip: segment_search_sorted");
        EK_HIP_CHECK(hipMemsetAsync(out, 0, n * sizeof(uint32_t), ctx().stream));
        note_launch("segment_search_sorted_zero", n, n * sizeof(uint32_t));
        return EK_OK;
    }
    return dispatch_numeric(type, [&](auto t) {
        return segment_search_sorted<typename decltype(t)::type>(out, table, nt, table_starts, m, needles, n, needle_starts, row_index, flags);
    });
}

}
