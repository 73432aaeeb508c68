// block_search_sorted: every needle is searched in ITS OWN sorted row of a row-major table of R rows of B entries; the result is
// the row-local count of entries t with t < v (right: t <= v), in ONE launch.
//
// The spelling this replaces, binary_search(0, B, [&](i) { return gather(T, row * B + min(i, B - 1)) < v; }), runs log2(B) + 1
// rounds of min / multiply-add / gather+compare / select / select over n-element arrays and needs the index array `row`.
//
// Everything below the routes is ek_search.h: 512-thread workgroups, 64 KiB of LDS (two workgroups per CU), 4 needles per lane as
// independent chains in lockstep, the branch-free fixed-trip step, 16-byte non-temporal needle loads and index stores.
//
//   1 tile of rows   blocked needles (needle e belongs to row e / M), B * sizeof(T) <= 64 KiB.  A job is a tile of t consecutive
//                    rows: t * B consecutive entries, staged into LDS with 16-byte loads, and t * M consecutive needles, each
//                    searched at lds + local_row * B.  local_row = j / M is one multiply by a host-computed reciprocal (t > 1
//                    implies t * M <= 65536, for which it is exact; t == 1 needs none).  With few rows and many needles per row
//                    (t == 1) a row is split: s workgroups stage the same row and take one piece of its needles each.  The
//                    workgroups walk the t-tiles x s-pieces jobs grid-stride.  Bytes: the table once, sizeof(T) + 4 per needle.
//   2 sampled row    blocked needles, B * sizeof(T) > 64 KiB: per (row, piece of its needles) the two-level search of search.hip on
//                    table + r * B -- every stride-th entry of the row in LDS, then log2(stride) steps inside one window in global
//                    memory.  A piece with few needles stages fewer samples (at least one per lane): a sample is a strided read.
//   3 indexed, LDS   rows given per needle (clamped to R - 1), whole table <= 64 KiB: staged whole, searched at lds + row * B.
//   4 indexed, global rows given per needle, larger table: every step reads global memory at table + row * B, nothing is staged.
//                    What this route saves over the loop is launches and index traffic, not bandwidth.
//   5 one row        blocked needles, R == 1: this IS search_sorted, and is forwarded to it (same bits, same kernel name).
//
// Needles and outputs of a job start wherever the job starts, so the peel to the first 16-byte aligned store and the tail are found
// per job in the kernel (at most 6 elements, one per lane).  No scratch, no atomics, nothing read back: capturable.
#include "ek_search.h"

namespace ek {

constexpr uint32_t kBlockSearchTileNeedles = 65536;   // needles of a tile of more than one row (keeps j * M below 2^32)
constexpr size_t kBlockSearchPieceNeedles = 8192;     // a row is not split into pieces of fewer needles than this

enum { kRouteNone = 0, kRouteTile = 1, kRouteSampled = 2, kRouteIndexedLds = 3, kRouteIndexedGlobal = 4, kRouteOneRow = 5 };

struct BlockSearchPlan {
    int route;
    uint32_t rows_per_tile;      // t (routes 1 and 2; 2: always 1)
    uint32_t pieces;             // s: workgroups per row (routes 1 and 2)
    size_t jobs;                 // tiles * pieces
    size_t workgroups;           // the grid
    SearchPlan sp;               // the search inside one row
};

static BlockSearchPlan block_search_plan(size_t elem_size, size_t R, size_t B, size_t n, bool indexed, int num_cu) {
    BlockSearchPlan p = { kRouteNone, 0, 0, 0, 0, { 0, 1, 0, 0 } };
    if (n == 0 || R == 0) return p;
    const size_t cap_entries = kSearchLdsBytes / elem_size, cap = (size_t) num_cu * kSearchBlocksPerCu;
    if (indexed) {
        p.route = R * B <= cap_entries ? kRouteIndexedLds : kRouteIndexedGlobal;
        p.sp = { (uint32_t) B, 1, search_top(B), 0 };            // route 4 takes the same steps, in global memory
        const size_t items = n / kSearchLane;
        p.workgroups = std::min(cap, std::max<size_t>(1, (items + kSearchBlock - 1) / kSearchBlock));
        return p;
    }
    if (R == 1) {
        p.route = kRouteOneRow;
        p.sp = search_plan(elem_size, B);
        return p;
    }
    const size_t M = n / R;
    size_t t = 1, s = 1;
    if (B <= cap_entries) {
        p.route = kRouteTile;
        t = std::min(cap_entries / B, std::max<size_t>(1, kBlockSearchTileNeedles / M));
        // no more rows than fill the grid once, but enough for one item per lane
        const size_t spread = (R + cap - 1) / cap, fill = (kSearchBlock * kSearchLane + M - 1) / M;
        t = std::max<size_t>(1, std::min({ t, std::max(spread, fill), R }));
        p.sp = { (uint32_t) B, 1, search_top(B), 0 };
    } else {
        p.route = kRouteSampled;
    }
    const size_t tiles = (R + t - 1) / t;
    if (t == 1 && tiles < cap)
        s = std::max<size_t>(1, std::min((cap + tiles - 1) / tiles, M / kBlockSearchPieceNeedles));
    if (p.route == kRouteSampled) {
        // samples: four per needle of a piece, at least one per lane, at most the 64 KiB
        const size_t piece = (M + s - 1) / s;
        size_t samples = kSearchBlock;
        while (samples < cap_entries && samples < 4 * piece) samples <<= 1;
        p.sp = search_plan(elem_size, B, std::min(samples, cap_entries));
    }
    p.rows_per_tile = (uint32_t) t;
    p.pieces = (uint32_t) s;
    p.jobs = tiles * s;
    p.workgroups = std::min(cap, p.jobs);
    return p;
}

/// piece `piece` of `pieces` of `count` needles
__device__ __forceinline__ size_t piece_begin(size_t count, uint32_t piece, uint32_t pieces) {
    return count / pieces * piece + min((size_t) piece, count % pieces);
}

/// route 1: a job is (tile of t rows, piece of its needles)
template <typename T, bool Right>
__global__ __launch_bounds__(kSearchBlock) void k_block_search_tiles(uint32_t *__restrict__ out, const T *__restrict__ table,
                                                                     const T *__restrict__ needles, uint32_t R, uint32_t B, size_t M,
                                                                     uint32_t t, uint32_t pieces, size_t jobs, uint64_t rcp_m,
                                                                     SearchPlan p) {
    __shared__ __attribute__((aligned(16))) T lds[kSearchLdsBytes / sizeof(T)];
    for (size_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const uint32_t tile = (uint32_t) (job / pieces), piece = (uint32_t) (job - (size_t) tile * pieces);
        const uint32_t row0 = tile * t, rows = min(t, R - row0);   // tile < ceil(R / t): row0 < R
        __syncthreads();                                           // the previous job's searches are done with the LDS
        stage_entries<T>(lds, table + (size_t) row0 * B, rows * B);
        __syncthreads();
        const size_t first = (size_t) row0 * M, count = (size_t) rows * M;
        const size_t j0 = piece_begin(count, piece, pieces), j1 = piece_begin(count, piece + 1, pieces);
        search_range<T>(out, needles, first + j0, first + j1, [&](const auto &v, size_t j, auto &r) {
            constexpr int N = (int) (sizeof(v) / sizeof(T));
            uint32_t base[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                // t > 1: one piece, j + k < t * M <= 65536 and M <= 32768, where the multiply is the exact quotient
                const uint32_t local = t > 1 ? (uint32_t) (((uint64_t) ((uint32_t) j + k) * rcp_m) >> 32) : 0u;
                base[k] = min(local, rows - 1) * B;
            }
            search_run<T, Right, N>(lds, base, table, B, p, v, r);
        });
    }
}

/// route 2: a job is (row, piece of its needles); the row's samples are staged, its windows are read in global memory
template <typename T, bool Right>
__global__ __launch_bounds__(kSearchBlock) void k_block_search_rows(uint32_t *__restrict__ out, const T *__restrict__ table,
                                                                    const T *__restrict__ needles, uint32_t B, size_t M,
                                                                    uint32_t pieces, size_t jobs, SearchPlan p) {
    __shared__ T lds[kSearchLdsBytes / sizeof(T)];
    for (size_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const uint32_t row = (uint32_t) (job / pieces), piece = (uint32_t) (job - (size_t) row * pieces);
        const T *__restrict__ entries = table + (size_t) row * B;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < p.resident; i += kSearchBlock) lds[i] = entries[i * p.stride + (p.stride - 1)];
        __syncthreads();
        const size_t first = (size_t) row * M;
        const size_t j0 = piece_begin(M, piece, pieces), j1 = piece_begin(M, piece + 1, pieces);
        search_range<T>(out, needles, first + j0, first + j1, [&](const auto &v, size_t, auto &r) {
            constexpr int N = (int) (sizeof(v) / sizeof(T));
            const uint32_t base[N] = { };
            search_run<T, Right, N>(lds, base, entries, B, p, v, r);
        });
    }
}

/// routes 3 and 4: the row of every needle comes from `rows`, clamped to R - 1
template <typename T, bool Right, bool Resident>
__global__ __launch_bounds__(kSearchBlock) void k_block_search_indexed(uint32_t *__restrict__ out, const T *__restrict__ table,
                                                                       const T *__restrict__ needles, const uint32_t *__restrict__ rows,
                                                                       size_t n, uint32_t R, uint32_t B, uint32_t top, uint32_t peel,
                                                                       int needles_vec, int rows_vec) {
    constexpr int N = kSearchLane;
    __shared__ __attribute__((aligned(16))) T lds[Resident ? kSearchLdsBytes / sizeof(T) : 1];
    if constexpr (Resident) {
        stage_entries<T>(lds, table, R * B);
        __syncthreads();
    }
    const T *mem = Resident ? lds : table;
    auto search = [&](const auto &v, const auto &row, auto &r) {
        constexpr int K = (int) (sizeof(v) / sizeof(T));
        uint32_t base[K], zero[K], count[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { base[k] = min(row[k], R - 1) * B; zero[k] = 0; count[k] = B; r[k] = 0; }
        search_steps<T, Right, K>(mem, base, zero, count, B - 1, top, v, r);
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
static void block_search_launch(void (*kernel)(Params...), size_t grid, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned) grid), dim3(kSearchBlock), 0, ctx().stream, (Params) args...);
}

template <typename T>
static int block_search_sorted(uint32_t *out, const void *table_, size_t R, size_t B, const void *needles_, size_t n,
                               const uint32_t *rows, int right) {
    RoctxRange range("enoki-hip: block_search_sorted");
    const T *table = (const T *) table_, *needles = (const T *) needles_;
    const BlockSearchPlan p = block_search_plan(sizeof(T), R, B, n, rows != nullptr, ctx().num_cu);
    const size_t M = rows ? 0 : n / R;
    switch (p.route) {
        case kRouteTile:
            block_search_launch(right ? k_block_search_tiles<T, true> : k_block_search_tiles<T, false>, p.workgroups, out, table, needles,
                                R, B, M, p.rows_per_tile, p.pieces, p.jobs, (1ull << 32) / M + 1, p.sp);
            break;
        case kRouteSampled:
            block_search_launch(right ? k_block_search_rows<T, true> : k_block_search_rows<T, false>, p.workgroups, out, table, needles,
                                B, M, p.pieces, p.jobs, p.sp);
            break;
        default: {
            size_t peel = head_of(out);
            if (peel > n) peel = n;
            const bool lds = p.route == kRouteIndexedLds;
            block_search_launch(lds ? (right ? k_block_search_indexed<T, true, true> : k_block_search_indexed<T, false, true>)
                                    : (right ? k_block_search_indexed<T, true, false> : k_block_search_indexed<T, false, false>),
                                p.workgroups, out, table, needles, rows, n, R, B, p.sp.lds_top, peel, aligned16(needles + peel),
                                aligned16(rows + peel));
        }
    }
    // the table once (route 4 reads what the needles point at, counted as the table all the same), needle in, index out, row in
    EK_LAUNCH_CHECK("block_search_sorted", n, R * B * sizeof(T) + n * (sizeof(T) + sizeof(uint32_t) + (rows ? sizeof(uint32_t) : 0)));
    return EK_OK;
}

/// everything ek_hip_search_sorted_blocks and its plan refuse, before any memory is touched
static int block_search_check(const char *what, int type, size_t R, size_t B, size_t n, bool indexed) {
    if (int rc = search_type_check(what, type, 0)) return rc;
    if (B == 0) return fail(EK_ERR_INVALID, "%s: rows of 0 entries", what);
    if (R > 0xFFFFFFFFull / B) return fail(EK_ERR_UNSUPPORTED, "%s: tables of 2^32 entries or more are unsupported (%zu x %zu)", what, R, B);
    if (R == 0 && n != 0) return fail(EK_ERR_INVALID, "%s: %zu needles and no row to search", what, n);
    if (!indexed && R != 0 && n % R != 0)
        return fail(EK_ERR_INVALID, "%s: %zu needles are no whole number per row of %zu rows", what, n, R);
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_search_sorted_blocks_plan(int type, size_t rows, size_t block, size_t n, int indexed, int compute_units, int *route,
                                     int *rows_per_tile, int *workgroups_per_row, int *resident, int *stride, int *global_steps) {
    if (int rc = block_search_check("ek_hip_search_sorted_blocks_plan()", type, rows, block, n, indexed != 0)) return rc;
    const BlockSearchPlan p = block_search_plan(type_size(type), rows, block, n, indexed != 0, compute_units > 0 ? compute_units : 256);
    if (route) *route = p.route;
    if (rows_per_tile) *rows_per_tile = (int) p.rows_per_tile;
    if (workgroups_per_row) *workgroups_per_row = (int) p.pieces;
    if (resident) *resident = (int) p.sp.resident;
    if (stride) *stride = (int) p.sp.stride;
    if (global_steps) *global_steps = (int) p.sp.global_steps;
    return EK_OK;
}

int ek_hip_search_sorted_blocks(int type, uint32_t *out, const void *table, size_t rows, size_t block, const void *needles, size_t n,
                                const uint32_t *row_index, int right) {
    if (int rc = ensure_init()) return rc;
    if (int rc = block_search_check("ek_hip_search_sorted_blocks()", type, rows, block, n, row_index != nullptr)) return rc;
    if (n == 0) return EK_OK;
    if (!out || !needles || !table) return fail(EK_ERR_INVALID, "ek_hip_search_sorted_blocks(): null pointer");
    if (rows == 1 && !row_index) return ek_hip_search_sorted(type, out, table, block, needles, n, right);
    return dispatch_numeric(type, [&](auto t) {
        return block_search_sorted<typename decltype(t)::type>(out, table, rows, block, needles, n, row_index, right);
    });
}

}
