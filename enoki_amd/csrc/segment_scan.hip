// Prefix sums inside ragged segments: for the m segments [lo_j, hi_j) of a flat array of n entries that a device array of start
// positions gives (starts[m] := n; segment_clamp in ek_block.h), and entry i of segment j,
//     out[i] = in[lo_j] + .. + in[i]              flags 0
//              in[lo_j] + .. + in[i - 1]          EK_SCAN_EXCLUSIVE
//              in[i] + .. + in[hi_j - 1]          EK_SCAN_REVERSE
//              in[i + 1] + .. + in[hi_j - 1]      both                          (the empty sum is +0)
// and out[i] = +0 for the entries in front of min(starts[0], n), which belong to no segment.  The counterpart of block_scan.hip for
// what compress() leaves behind; the spelling it replaces, psum(x) - segment_repeat(gather(psum(x), starts), starts, n), takes four
// passes and subtracts two large running sums to get a small one.  The promises of block_scan.hip hold word for word: every output
// is a sum of its own segment's terms only, an inclusive entry with one term is its input bit for bit (-0.0 included: running
// sums start from -0.0), an exclusive entry IS the neighbouring inclusive entry (moved, never recomputed), nothing of one segment
// reaches another, the shape of every sum is fixed by (type, flags, n, m, pointer alignment, #CU) and the contents of `starts`,
// and NO KERNEL WAITS FOR ANOTHER WORKGROUP: no ticket, no descriptor, no look-back, no polling loop, no global atomics.
//
// ONE route, output-driven, so that the work is balanced whatever `starts` holds.  segscan_plan() (what ek_hip_psum_segments_plan
// reports), from host-known numbers only:
//     tile                = 16 KiB / sizeof(T) consecutive entries: tile t is the entries [t * tile, min((t + 1) * tile, n))
//     tiles               = ceil(n / tile)
//     tiles_per_workgroup = ceil(tiles / min(tiles, 4 x #CU))          a workgroup owns a RANGE of consecutive tiles
//     workgroups          = ceil(tiles / tiles_per_workgroup)
//     launches            = 1 for one workgroup, 3 otherwise; all of them 0 for n == 0 or m == 0 (m == 0: out is zero-filled)
// Everything below is told in SCAN ORDER: ascending entries, or descending ones for REVERSE (tiles, lanes and starts mirrored).
// A HEAD is an entry that takes nothing from the entry before it: entry s for every start s (REVERSE: entry s - 1, and n - 1).
//
// The scan launch, per tile:
//   * the tile is staged in LDS with 16-byte non-temporal loads (head / tail by element for a view that is only element-aligned).
//     Entry e lives at word e + e / R of LDS, R = tile / 256 being the entries a lane owns: the lanes' runs then sit R + 1 words
//     apart, an odd number, and fall into different banks.
//   * heads: the workgroup knows j, the number of starts in front of the tile (one search_steps in `starts` for its first tile
//     only), and streams the starts from there on, 256 at a time: every start that falls into the tile ORs a bit into its lane's
//     flag word in LDS (idempotent: the equal starts of empty segments cost nothing but the loop), and a barrier that counts the
//     starts that lie in or before the tile both ends the loop (fewer than 256) and moves j on for the next tile.  A scatter of
//     (starts in the tile) flags, not a search per entry.
//   * every lane scans its run of R entries in registers with the (value, flag) operator -- a flagged entry takes its own value
//     and nothing from before --, the run totals are scanned by 6 __shfl_up steps per wave, the four wave totals go through LDS,
//     and the lane adds what arrives from before to its entries in front of its first head.
//   * EXCLUSIVE moves every inclusive value one position on (inside a lane in registers, between lanes and tiles through LDS)
//     and writes +0 at every head.  Entries in front of min(starts[0], n) are written as +0.
//   * the results go back to the LDS tile (every lane has its inputs in registers by then) and leave with 16-byte non-temporal
//     stores shifted for the alignment of `out`, which need not be that of `in`.
// The carry between the tiles of a workgroup is a register of that workgroup.  Between workgroups it comes from EARLIER LAUNCHES:
//   1 totals   workgroup w, for its range [a, b) in scan order: the sum of the entries from the range's last head on (from a if it
//              holds none), and whether it holds a head.  One search_steps and reduce_piece (ek_block.h): where segments are short
//              against a range, this reads a few entries, not the array; a range in front of all segments reads nothing.
//   2 carries  one workgroup: the inclusive scan of the (total, head) pairs in scan order with the same operator: c[w].
//   3 scan     workgroup w starts from c[w - 1].  c[w] IS, by definition, the inclusive result at the last entry of range w: the
//              scan launch writes it there (inclusive) or at the first entry of range w + 1 (EXCLUSIVE, unless that is a head) --
//              the same bits in both modes, with no seam launch.  It is a sum of that segment's own terms in another fixed order.
// Whatever `starts` holds: every read of `in` lies in [0, n), every read of `starts` in [0, m), every entry of out[0, n) is
// written exactly once by the workgroup whose tile holds it, and every loop is bounded by n / tile, m / 256 + 1 or a constant.
// Starts above n are clamped to n.  Where `starts` decreases only the values are unspecified.  out == in is allowed: a workgroup
// reads a tile before it writes it, and launch 1 has read what it needs before launch 3 writes.  The scratch of launches 1 and 2
// (one value and one word per workgroup) comes from ek_hip_malloc and is freed stream-ordered: capturable.
#include "ek_search.h"

namespace ek {

constexpr size_t kSegScanBlocksPerCu = 4;

struct SegScanPlan {
    size_t tile, tiles, per_workgroup, workgroups;
    int launches;
};

static SegScanPlan segscan_plan(size_t elem, size_t n, size_t m, int num_cu) {
    SegScanPlan p = { kBlockTileBytes / elem, 0, 0, 0, 0 };
    if (n == 0 || m == 0) return p;
    const size_t cu = num_cu > 0 ? (size_t) num_cu : 256;
    p.tiles = (n + p.tile - 1) / p.tile;
    const size_t cap = std::min(p.tiles, cu * kSegScanBlocksPerCu);
    p.per_workgroup = (p.tiles + cap - 1) / cap;
    p.workgroups = (p.tiles + p.per_workgroup - 1) / p.per_workgroup;
    p.launches = p.workgroups > 1 ? 3 : 1;
    return p;
}

template <typename T> __device__ __forceinline__ T seg_add(T a, T b) {
    using W = wrap_t<T>;                                    // unsigned arithmetic for integers: wrap-around, no UB
    return (T) ((W) a + (W) b);
}

/// the sum that starts from -0.0, for reduce_piece: one term stays that term bit for bit
template <typename T> struct SegSum {
    static __device__ __forceinline__ T identity() { return sum_identity<T>; }
    static __device__ __forceinline__ T combine(T a, T b) { return seg_add(a, b); }
};

template <typename T> __device__ __forceinline__ T seg_shfl_up(T v, int delta) {
    if constexpr (sizeof(T) == 8) {
        uint64_t u;
        __builtin_memcpy(&u, &v, 8);
        uint32_t lo = __shfl_up((uint32_t) u, delta, 64), hi = __shfl_up((uint32_t) (u >> 32), delta, 64);
        u = ((uint64_t) hi << 32) | lo;
        __builtin_memcpy(&v, &u, 8);
        return v;
    } else {
        return __shfl_up(v, delta, 64);
    }
}

/// All 256 lanes, lane order = scan order: (v, f) is the lane's total and whether it holds a head.  Returns what reaches the
/// lane's first entry from before it -- `carry` included, which is what reaches lane 0 -- and moves `carry` behind lane 255.
/// One barrier; s_v and s_f (4 words each) are free again after the caller's next one.
template <typename T> __device__ __forceinline__ T segscan_lanes(T v, uint32_t f, T &carry, T *s_v, uint32_t *s_f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T uv = seg_shfl_up(v, d);
        const uint32_t uf = __shfl_up(f, d, 64);
        if (lane >= d) {
            if (!f) v = seg_add(uv, v);
            f |= uf;
        }
    }
    T pv = seg_shfl_up(v, 1);
    uint32_t pf = __shfl_up(f, 1, 64);
    if (lane == 0) { pv = sum_identity<T>; pf = 0; }
    if (lane == 63) { s_v[wave] = v; s_f[wave] = f; }
    __syncthreads();
    T before = carry, run = carry;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        run = s_f[w] ? s_v[w] : seg_add(run, s_v[w]);
        if (w < wave) before = run;
    }
    carry = run;
    return pf ? pv : seg_add(before, pv);
}

/// the tiles [t0, t1) of workgroup w and the entries [a, b) they cover
__device__ __forceinline__ void segscan_range(uint32_t w, uint32_t tiles, uint32_t per_workgroup, uint32_t E, uint32_t n, uint32_t &t0,
                                              uint32_t &t1, uint32_t &a, uint32_t &b) {
    t0 = w * per_workgroup;                                                                       // < tiles
    t1 = tiles - t0 < per_workgroup ? tiles : t0 + per_workgroup;
    a = t0 * E;                                                                                   // < n
    b = t1 == tiles ? n : t1 * E;
}

// ---- launch 1: the total behind the last head of every range -----------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_psum_segments_totals(T *__restrict__ agg_v, uint32_t *__restrict__ agg_f, const T *__restrict__ in,
                                                              uint32_t n, const uint32_t *__restrict__ starts, uint32_t m, uint32_t top,
                                                              uint32_t tiles, uint32_t per_workgroup, int rev) {
    constexpr uint32_t E = kBlockTileBytes / sizeof(T);
    uint32_t t0, t1, a, b;
    segscan_range(blockIdx.x, tiles, per_workgroup, E, n, t0, t1, a, b);                          // a < b <= n
    // c: the number of starts <= the range's last entry in scan order
    const uint32_t at[1] = { rev ? a : b - 1 }, zero[1] = { 0 }, all[1] = { m };
    uint32_t pos[1] = { 0 };
    search_steps<uint32_t, true, 1>(starts, zero, zero, all, m - 1, top, at, pos);
    const uint32_t c = pos[0];                                                                    // <= m
    uint32_t lo = a, hi = b, head = 0;
    if (!rev) {
        if (c == 0) lo = b;                               // in front of all segments: nothing of it is ever used
        else {
            const uint32_t s = starts[c - 1], h = s < n ? s : n;
            head = h >= a;
            lo = h > a ? h : a;
            if (lo > b) lo = b;                           // (decreasing starts)
        }
    } else {
        // the last head in scan order is the entry in front of the smallest start > a (starts[m] := n)
        const uint32_t s = c < m ? starts[c] : n, h = s < n ? s : n;
        head = h <= b;
        hi = h < b ? h : b;
        if (hi < a || c == 0) hi = a;                     // (decreasing starts); c == 0: [a, h) lies in front of all segments
    }
    const T v = reduce_piece<SegSum<T>, T>(in + lo, (size_t) (hi - lo));
    if (threadIdx.x == 0) { agg_v[blockIdx.x] = v; agg_f[blockIdx.x] = head; }
}

// ---- launch 2: the inclusive scan of the W (total, head) pairs, in place ------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void k_psum_segments_carries(T *agg_v, const uint32_t *__restrict__ agg_f, uint32_t W, int rev) {
    __shared__ T s_v[4];
    __shared__ uint32_t s_f[4];
    const uint32_t K = (W + 255) / 256, p0 = threadIdx.x * K;            // the lane's K consecutive ranges in scan order
    T acc = sum_identity<T>;
    uint32_t f = 0;
    for (uint32_t k = 0; k < K; ++k) {
        if (p0 + k < W) {
            const uint32_t w = rev ? W - 1 - (p0 + k) : p0 + k;
            const uint32_t g = agg_f[w];
            acc = g ? agg_v[w] : seg_add(acc, agg_v[w]);
            f |= g;
        }
    }
    T carry = sum_identity<T>;
    acc = segscan_lanes<T>(acc, f, carry, s_v, s_f);
    for (uint32_t k = 0; k < K; ++k) {
        if (p0 + k < W) {
            const uint32_t w = rev ? W - 1 - (p0 + k) : p0 + k;
            acc = agg_f[w] ? agg_v[w] : seg_add(acc, agg_v[w]);
            agg_v[w] = acc;
        }
    }
}

// ---- launch 3 (the only one for a single workgroup): the scan ------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_psum_segments(T *out, const T *in, uint32_t n, const uint32_t *__restrict__ starts, uint32_t m,
                                                       uint32_t top, uint32_t tiles, uint32_t per_workgroup, const T *__restrict__ carries,
                                                       int flags) {
    constexpr uint32_t N = 16 / sizeof(T), E = kBlockTileBytes / sizeof(T), R = E / 256;
    constexpr T kId = sum_identity<T>;
    __shared__ T tile[E + E / R];                         // entry e at tile[e + e / R]
    __shared__ uint32_t s_flag[256];                      // bit i of word l: scan position l * R + i of the tile is a head
    __shared__ T s_last[257];                             // EXCLUSIVE: lane l's last inclusive value at [l + 1]
    __shared__ T s_v[4];
    __shared__ uint32_t s_f[4];
    const bool excl = flags & EK_SCAN_EXCLUSIVE, rev = flags & EK_SCAN_REVERSE;
    const uint32_t tid = threadIdx.x, W = gridDim.x, w = blockIdx.x;
    uint32_t t0, t1, a, b;
    segscan_range(w, tiles, per_workgroup, E, n, t0, t1, a, b);
    const uint32_t s0 = starts[0], first = s0 < n ? s0 : n;                                       // (m >= 1)
    // what reaches the range from before it; for EXCLUSIVE also the inclusive result of the entry before it, the same bits
    T carry = kId, prev = T(0);
    if (rev ? w + 1 < W : w > 0) carry = prev = carries[rev ? w + 1 : w - 1];
    const T closing = W > 1 ? carries[w] : T(0);          // the inclusive result at the range's last entry in scan order
    uint32_t j = 0;                                       // the number of starts in front of (REVERSE: up to the end of) the tile
    bool known = false;
    for (uint32_t q = 0; q < t1 - t0; ++q) {
        const uint32_t t = rev ? t1 - 1 - q : t0 + q, base = t * E, len = n - base < E ? n - base : E;
        s_flag[tid] = 0;
        __syncthreads();                                  // (the tile has left; the flag words are clear before anybody ORs)
        // ---- stage
        {
            const T *src = in + base;
            uint32_t head = head_of(src);
            if (head > len) head = len;
            const uint32_t nvec = (len - head) / N, tail = len - head - nvec * N;
            if (tid < head) tile[tid + tid / R] = src[tid];
#pragma unroll 4
            for (uint32_t v = tid; v < nvec; v += 256) {
                const Pack<T, N> p = pack_load<T, N, true>(src + head + v * N);
#pragma unroll
                for (uint32_t k = 0; k < N; ++k) {
                    const uint32_t e = head + v * N + k;
                    tile[e + e / R] = p.v[k];
                }
            }
            if (tid < tail) {
                const uint32_t e = head + nvec * N + tid;
                tile[e + e / R] = src[e];
            }
        }
        // ---- heads
        if (!known) {
            uint32_t pos[1] = { 0 };
            const uint32_t at[1] = { rev ? base + len : base }, zero[1] = { 0 }, all[1] = { m };
            if (rev) search_steps<uint32_t, true, 1>(starts, zero, zero, all, m - 1, top, at, pos);       // starts <= base + len
            else search_steps<uint32_t, false, 1>(starts, zero, zero, all, m - 1, top, at, pos);          // starts < base
            j = pos[0];                                                                           // <= m
            known = true;
        }
        if (rev && base + len == n && tid == 0) {         // entry n - 1, where the whole scan begins
            const uint32_t sp = E - len;
            atomicOr(&s_flag[sp / R], 1u << (sp % R));
        }
        {
            const uint32_t j0 = j, room = rev ? j0 : m - j0;                                      // starts left to walk
            for (uint64_t cnt = 0;; cnt += 256) {
                const uint64_t k = cnt + tid;
                const bool valid = k < room;
                uint32_t s = valid ? starts[rev ? j0 - 1 - (uint32_t) k : j0 + (uint32_t) k] : 0u;
                if (s > n) s = n;
                // used: the start lies in or before the tile (scan order); inside: its head lies in the tile, at entry base + e
                bool used, inside;
                uint32_t e;
                if (!rev) { used = valid && s < base + len; inside = used && s >= base; e = s - base; }
                else { used = valid && s > base; inside = used && s <= base + len; e = s - 1 - base; }
                if (inside) {
                    const uint32_t sp = rev ? E - 1 - e : e;
                    atomicOr(&s_flag[sp / R], 1u << (sp % R));
                }
                const uint32_t c = (uint32_t) __syncthreads_count(used);
                j = rev ? j - c : j + c;
                if (c < 256) break;                       // a start behind the tile, or no start left
            }
        }
        // (the loop above ran at least one barrier: the tile and the flags are complete)
        // ---- the lane's run, in scan order
        const uint32_t fw = s_flag[tid];
        T x[R];
        T acc = kId;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
            const uint32_t sp = tid * R + i, e = rev ? E - 1 - sp : sp;
            const T v = e < len ? tile[e + e / R] : kId;
            acc = (fw >> i) & 1u ? v : seg_add(acc, v);
            x[i] = acc;
        }
        const T pre = segscan_lanes<T>(acc, fw != 0, carry, s_v, s_f);
        {
            bool open = true;
#pragma unroll
            for (uint32_t i = 0; i < R; ++i) {
                if ((fw >> i) & 1u) open = false;
                if (open) x[i] = seg_add(pre, x[i]);
            }
        }
        if (excl) {
            // every entry takes the inclusive value of the entry before it -- moved, never recomputed -- and a head takes +0
            s_last[tid + 1] = x[R - 1];
            __syncthreads();
            const T left = tid ? s_last[tid] : prev;
            prev = s_last[256];
#pragma unroll
            for (uint32_t i = R - 1; i > 0; --i) x[i] = x[i - 1];
            x[0] = left;
#pragma unroll
            for (uint32_t i = 0; i < R; ++i)
                if ((fw >> i) & 1u) x[i] = T(0);
        }
        // the range's last entry in scan order (inclusive results only: an exclusive one lands in the next range)
        const uint32_t closing_at = !excl && W > 1 && q + 1 == t1 - t0 ? (rev ? E - 1 : len - 1) : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i) {
            const uint32_t sp = tid * R + i, e = rev ? E - 1 - sp : sp;
            if (e < len) {
                T v = sp == closing_at ? closing : x[i];
                if (base + e < first) v = T(0);
                tile[e + e / R] = v;
            }
        }
        __syncthreads();
        // ---- out
        {
            T *dst = out + base;
            uint32_t head = head_of(dst);
            if (head > len) head = len;
            const uint32_t nvec = (len - head) / N, tail = len - head - nvec * N;
            if (tid < head) dst[tid] = tile[tid + tid / R];
#pragma unroll 4
            for (uint32_t v = tid; v < nvec; v += 256) {
                Pack<T, N> p;
#pragma unroll
                for (uint32_t k = 0; k < N; ++k) {
                    const uint32_t e = head + v * N + k;
                    p.v[k] = tile[e + e / R];
                }
                pack_store<T, N, true>(dst + head + v * N, p);
            }
            if (tid < tail) {
                const uint32_t e = head + nvec * N + tid;
                dst[e] = tile[e + e / R];
            }
        }
    }
}

template <typename T>
static int psum_segments_launch(T *out, const T *in, size_t n, const uint32_t *starts, size_t m, const SegScanPlan &p, int flags, T *agg_v) {
    Context &c = ctx();
    const uint32_t top = search_top(m), W = (uint32_t) p.workgroups;
    const int rev = flags & EK_SCAN_REVERSE;
    if (W > 1) {
        uint32_t *agg_f = (uint32_t *) (agg_v + W);
        hipLaunchKernelGGL((k_psum_segments_totals<T>), dim3(W), dim3(256), 0, c.stream, agg_v, agg_f, in, (uint32_t) n, starts, (uint32_t) m, top,
                           (uint32_t) p.tiles, (uint32_t) p.per_workgroup, rev);
        EK_LAUNCH_CHECK("psum_segments_totals", n, n * sizeof(T) + m * 4 + W * (sizeof(T) + 4));
        hipLaunchKernelGGL((k_psum_segments_carries<T>), dim3(1), dim3(256), 0, c.stream, agg_v, (const uint32_t *) agg_f, W, rev);
        EK_LAUNCH_CHECK("psum_segments_carries", W, W * (2 * sizeof(T) + 4));
    }
    hipLaunchKernelGGL((k_psum_segments<T>), dim3(W), dim3(256), 0, c.stream, out, in, (uint32_t) n, starts, (uint32_t) m, top, (uint32_t) p.tiles,
                       (uint32_t) p.per_workgroup, (const T *) agg_v, flags);
    EK_LAUNCH_CHECK("psum_segments", n, 2 * n * sizeof(T) + m * 4);
    return EK_OK;
}

template <typename T>
static int psum_segments_typed(void *out, const void *in, size_t n, const uint32_t *starts, size_t m, const SegScanPlan &p, int flags) {
    RoctxRange range("enoki-hip: segment prefix sum");
    void *scratch = nullptr;
    if (p.workgroups > 1)
        if (int rc = ek_hip_malloc(p.workgroups * (sizeof(T) + sizeof(uint32_t)), &scratch)) return rc;
    const int rc = psum_segments_launch<T>((T *) out, (const T *) in, n, starts, m, p, flags, (T *) scratch);
    if (scratch) ek_hip_free(scratch);   // stream-ordered reuse
    return rc;
}

static int segscan_size_check(const char *what, size_t n, size_t m) {
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull)
        return fail(EK_ERR_UNSUPPORTED, "%s: 2^32 entries or segments or more are unsupported (%zu, %zu)", what, n, m);
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_psum_segments_plan(int type, size_t n, size_t m, int compute_units, size_t *tile, size_t *tiles_per_workgroup, size_t *workgroups,
                              int *launches) {
    if (int rc = numeric_type_check("ek_hip_psum_segments_plan()", type)) return rc;
    if (int rc = segscan_size_check("ek_hip_psum_segments_plan()", n, m)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_psum_segments_plan(): %d compute units", compute_units);
    const SegScanPlan p = segscan_plan(type_size(type), n, m, compute_units);
    if (tile) *tile = p.tile;
    if (tiles_per_workgroup) *tiles_per_workgroup = p.per_workgroup;
    if (workgroups) *workgroups = p.workgroups;
    if (launches) *launches = p.launches;
    return EK_OK;
}

int ek_hip_psum_segments(int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m, int flags) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_psum_segments()", type)) return rc;
    if (flags & ~(EK_SCAN_EXCLUSIVE | EK_SCAN_REVERSE)) return fail(EK_ERR_INVALID, "ek_hip_psum_segments(): unknown flags %d", flags);
    if (int rc = segscan_size_check("ek_hip_psum_segments()", n, m)) return rc;
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_psum_segments()", elem, out, in)) return rc;
    if (m == 0) return ek_hip_memset(out, 0, n * elem);   // no segment: +0 everywhere (all bits clear in every type)
    if (int rc = pointers_check("ek_hip_psum_segments()", sizeof(uint32_t), starts)) return rc;
    const SegScanPlan p = segscan_plan(elem, n, m, ctx().num_cu);
    return dispatch_numeric(type, [&](auto t) { return psum_segments_typed<typename decltype(t)::type>(out, in, n, starts, m, p, flags); });
}

}
