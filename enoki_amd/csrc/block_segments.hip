// Ragged segments: out[j] = reduce(in[lo_j .. hi_j)) for m segments of a flat array of n entries that are given by a device array
// of start positions (starts[m] := n; lo_j = min(starts[j], n), hi_j = max(lo_j, min(starts[j + 1], n)): segment_clamp in
// ek_block.h), and the transpose  repeat_segments: out[i] = in[j] for the last j with starts[j] <= i, 0 in front of starts[0].
// The counterpart of block_reduce.hip for what compress(), block_search_sorted and a mesh leave behind: the samples of ray j are
// still consecutive, but there are count[j] of them.  starts = exclusive block_psum of the counts.
//
// The spellings these replace, scatter_add(zero(m), x, seg_id) and gather(v, seg_id), need the n-entry seg_id array built first
// (search_sorted(starts, arange(n), right) - 1) and stream it through the generic kernels.
//
// ek_hip_reduce_segments takes one of three routes, chosen by segment_plan() (what ek_hip_reduce_segments_plan reports) from the
// MEAN length ceil(n / m) -- never from what `starts` holds, which the host does not know:
//   1 grouped  n <= 1024 m.  A workgroup owns W consecutive segments (W = the segments that fill one 16 KiB tile at the mean
//              length, a multiple of the groups per workgroup, at most 2048).  Their clamped starts go to LDS once.  The entries
//              of the W segments are one contiguous range, walked in chunks of one LDS tile that is staged exactly as
//              k_reduce_packed stages its tile.  Inside a chunk every segment gets a group of G = 2^ceil(log2(clamp(mean, 1, 64)))
//              adjacent lanes, which combine the part of the segment that lies in the chunk and finish with log2(G) shuffle steps.
//              A segment that continues in the next chunk leaves its value in an LDS word (NOT a register: W / groups values per
//              lane would be indexed dynamically), which the next chunk's value is combined onto, in chunk order.  A segment far
//              longer than the mean costs its workgroup more chunks; the chunks that lie inside it whole are streamed by all 256
//              lanes at once, as in route 2, but by this ONE workgroup: slow but correct.
//   2 one workgroup per segment, n > 1024 m: reduce_piece (ek_block.h) from the segment's clamped bounds.
//   3 split    fewer than 2 x #CU segments of mean >= 16 Ki: S pieces per segment with S = split_shape(mean); the piece length of
//              segment j is ceil(len_j / S) rounded up to the vector width, computed on the device; pieces behind the segment's
//              end yield the identity.  The m x S partials are folded by the packed block kernel with B = S.  Two launches.
// ek_hip_repeat_segments is output-driven: a workgroup takes a run of consecutive tiles of 4 KiB of output (one 16-byte store per
// lane; at most 6 workgroups per CU).  It finds the segment of its first entry by binary search in `starts` (search_steps of
// ek_search.h: every read clamped to the array), stages the starts from there on in LDS, 256 at a time until one lies behind the
// tile (at most 4096), and searches every entry of the tile in that window (in `starts` itself if the window did not reach).  The
// window also tells where the next tile's window begins, so only a workgroup's first tile pays the search in global memory.
//
// Whatever `starts` holds: every read of `in` lies inside a clamped segment or at an index below m, every output entry is written
// once by the lane that owns it, every loop has a trip count that is bounded by n, m or a constant.  No atomics, no read-back, no
// host wait, no kernel waits for another workgroup; the partials of 3 come from the caching allocator (capturable).  The shape of
// every sum is a function of (type, op, n, m, alignment, #CU) and of `starts`: run-to-run identical.
#include "ek_search.h"

namespace ek {

constexpr uint32_t kSegPerWorkgroupMax = 2048;    // segments a workgroup of the grouped route owns (their starts and carries: LDS)
constexpr uint32_t kSegWindow = 4096;             // starts of a repeat tile that are searched in LDS
constexpr uint32_t kSegRepeatVectors = 1;         // 16-byte stores per lane and repeat tile
constexpr size_t kSegRepeatBlocksPerCu = 6;

struct SegmentPlan {
    int route;                     // 0: m == 0
    uint32_t glog, per_workgroup;  // 1: log2(lanes per segment), segments per workgroup
    size_t splits;                 // 3: pieces per segment
    size_t workgroups;             // grid of the first launch
};

static SegmentPlan segment_plan(size_t elem, size_t n, size_t m, int num_cu) {
    SegmentPlan p = { 0, 0, 0, 1, 0 };
    if (m == 0) return p;
    const size_t cu = num_cu > 0 ? (size_t) num_cu : 256, mean = (n + m - 1) / m, E = kBlockTileBytes / elem;
    if (n <= kBlockPackedMax * m) {
        p.route = 1;
        while ((1u << p.glog) < mean && p.glog < 6) p.glog++;
        const size_t groups = 256u >> p.glog, fill = E / std::max<size_t>(mean, 1) / groups * groups;
        p.per_workgroup = (uint32_t) std::min<size_t>(std::max(fill, groups), kSegPerWorkgroupMax);
        p.workgroups = std::min<size_t>((m + p.per_workgroup - 1) / p.per_workgroup, kBlockMaxGrid);
        return p;
    }
    size_t piece;
    p.route = split_shape(elem, m, mean, cu, p.splits, piece) ? 3 : 2;
    p.workgroups = std::min<size_t>(m * p.splits, kBlockMaxGrid);
    return p;
}

template <typename R, typename T>
__global__ __launch_bounds__(256) void k_reduce_grouped(T *__restrict__ out, const T *__restrict__ in, uint32_t n,
                                                        const uint32_t *__restrict__ starts, size_t m, uint32_t W, uint32_t glog,
                                                        size_t workgroups) {
    constexpr uint32_t N = 16 / sizeof(T), E = kBlockTileBytes / sizeof(T);
    __shared__ __attribute__((aligned(16))) T tile[E + N];
    __shared__ T carry[kSegPerWorkgroupMax];
    __shared__ uint32_t bound[kSegPerWorkgroupMax + 1];
    const uint32_t G = 1u << glog, group = threadIdx.x >> glog, l = threadIdx.x & (G - 1), groups = 256u >> glog;
    for (size_t w = blockIdx.x; w < workgroups; w += gridDim.x) {
        const size_t s0 = w * W;
        const uint32_t ns = (uint32_t) (m - s0 < W ? m - s0 : W);
        for (uint32_t k = threadIdx.x; k <= ns; k += 256) {
            const uint32_t s = s0 + k < m ? starts[s0 + k] : n;
            bound[k] = s < n ? s : n;
            if (k < ns) carry[k] = R::identity();
        }
        __syncthreads();
        // the workgroup's range [r0, r1) (uniform); with decreasing starts a segment may lie outside it and is then not read at all
        const uint32_t r0 = bound[0], r1 = bound[ns] > r0 ? bound[ns] : r0;
        // chunks >= 1 (an empty range still takes the one trip that writes the results); no sum here can pass 2^32 - 1
        const uint32_t chunks = r1 > r0 ? (r1 - r0) / E + ((r1 - r0) % E != 0) : 1u, trips = (ns + groups - 1) / groups;
        const uint32_t stop = 1u << (31 - __clz(ns));                                              // (ns >= 1)
        for (uint32_t c = 0; c < chunks;) {
            const uint32_t c0 = r0 + c * E, len = r1 - c0 < E ? r1 - c0 : E;                      // c0 + len <= r1 <= n
            // Chunks that lie inside ONE segment (a segment far longer than the mean) are not staged: the segment that holds the
            // chunk's first entry is looked up in the staged starts, and if it also holds the chunk's last entry all 256 lanes
            // stream its whole chunks from memory, like a workgroup of route 2, onto its carry.  Never the workgroup's last chunk,
            // which writes the results.  (All of this is uniform: the starts are in LDS.)
            if (c + 1 < chunks) {
                const uint32_t at[1] = { c0 }, zero[1] = { 0 }, count[1] = { ns };
                uint32_t pos[1] = { 0 };
                search_steps<uint32_t, true, 1>(bound, zero, zero, count, ns - 1, stop, at, pos);
                if (pos[0]) {
                    const uint32_t k = pos[0] - 1;
                    uint32_t lo, hi;
                    segment_clamp(bound[k], bound[k + 1], n, lo, hi);
                    if (lo <= c0 && hi - c0 >= E && hi > c0) {
                        uint32_t whole = (hi - c0) / E;                                           // >= 1
                        if (whole > chunks - 1 - c) whole = chunks - 1 - c;                       // >= 1: inside [r0, r1) whatever hi is
                        const T v = reduce_piece<R, T>(in + c0, (size_t) whole * E);
                        if (threadIdx.x == 0) carry[k] = R::combine(carry[k], v);
                        __syncthreads();
                        c += whole;
                        continue;
                    }
                }
            }
            const T *src = in + c0;
            uint32_t head = head_of(src);
            if (head > len) head = len;
            // entry c0 + e lives at tile[shift + e]: the first whole vector lands on a 16-byte boundary of LDS
            const uint32_t shift = (N - head) % N, nvec = (len - head) / N, tail = len - head - nvec * N;
            T *dst = tile + shift;
            if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
#pragma unroll 4
            for (uint32_t v = threadIdx.x; v < nvec; v += 256)
                *reinterpret_cast<Pack<T, N> *>(dst + head + v * N) = pack_load<T, N, true>(src + head + v * N);
            if (threadIdx.x < tail) dst[head + nvec * N + threadIdx.x] = src[head + nvec * N + threadIdx.x];
            __syncthreads();
            // (the same trip count for every lane: the shuffles below are executed by whole waves)
            for (uint32_t it = 0; it < trips; ++it) {
                const uint32_t k = it * groups + group;
                T acc = R::identity();
                if (k < ns) {
                    uint32_t lo, hi;
                    segment_clamp(bound[k], bound[k + 1], n, lo, hi);
                    if (lo < c0) lo = c0;
                    if (hi > c0 + len) hi = c0 + len;
                    if (hi > lo) {
                        const uint32_t b = hi - c0;                                               // <= len <= E
                        for (uint32_t e = lo - c0 + l; e < b; e += G) acc = R::combine(acc, dst[e]);
                    }
                }
                for (uint32_t d = G >> 1; d; d >>= 1) acc = R::combine(acc, shfl_down(acc, (int) d));
                if (l == 0 && k < ns) {
                    acc = R::combine(carry[k], acc);
                    if (c + 1 == chunks) out[s0 + k] = acc;
                    else carry[k] = acc;
                }
            }
            __syncthreads();
            ++c;
        }
    }
}

/// piece = piece s of segment j (S pieces per segment; S == 1: the whole segment), one workgroup each
template <typename R, typename T>
__global__ __launch_bounds__(256) void k_reduce_ragged(T *__restrict__ out, const T *__restrict__ in, uint32_t n,
                                                       const uint32_t *__restrict__ starts, size_t m, uint32_t S, size_t pieces) {
    constexpr uint32_t N = 16 / sizeof(T);
    for (size_t p = blockIdx.x; p < pieces; p += gridDim.x) {
        const size_t j = S > 1 ? p / S : p, s = p - j * S;
        uint32_t lo, hi;
        segment_clamp(starts[j], j + 1 < m ? starts[j + 1] : n, n, lo, hi);
        size_t off = 0, len = hi - lo;
        if (S > 1) {
            const size_t L = len, P = ((L + S - 1) / S + N - 1) / N * N;
            off = s * P < L ? s * P : L;
            len = L - off < P ? L - off : P;
        }
        const T v = reduce_piece<R, T>(in + lo + off, len);
        if (threadIdx.x == 0) out[p] = v;
        __syncthreads();                                  // (block_reduce's LDS words are written again by the next piece)
    }
}

template <int Op, typename T>
static int reduce_segments_op(int type, T *out, const T *in, size_t n, const uint32_t *starts, size_t m, const SegmentPlan &p) {
    using R = Reducer<Op, T>;
    RoctxRange range("enoki-hip: segment reduction");
    Context &c = ctx();
    if (p.route == 1) {
        const size_t workgroups = (m + p.per_workgroup - 1) / p.per_workgroup;
        hipLaunchKernelGGL((k_reduce_grouped<R, T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, out, in, (uint32_t) n, starts, m,
                           p.per_workgroup, p.glog, workgroups);
        EK_LAUNCH_CHECK("reduce_segments_grouped", n, (n + m) * sizeof(T) + m * 4);
        return EK_OK;
    }
    if (p.route == 2) {
        hipLaunchKernelGGL((k_reduce_ragged<R, T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, out, in, (uint32_t) n, starts, m, 1u, m);
        EK_LAUNCH_CHECK("reduce_segments", n, (n + m) * sizeof(T) + m * 4);
        return EK_OK;
    }
    const size_t pieces = m * p.splits;
    void *partials = nullptr;
    if (int rc = ek_hip_malloc(pieces * sizeof(T), &partials)) return rc;
    hipLaunchKernelGGL((k_reduce_ragged<R, T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, (T *) partials, in, (uint32_t) n, starts, m,
                       (uint32_t) p.splits, pieces);
    int rc = EK_OK;
    if (hipError_t err = hipGetLastError(); err != hipSuccess) rc = hip_fail(err, "reduce_segments_split", __FILE__, __LINE__);
    else {
        note_launch("reduce_segments_split", n, (n + pieces) * sizeof(T) + m * 4);
        rc = reduce_blocks_packed(Op, type, out, partials, m, p.splits);
    }
    ek_hip_free(partials);   // stream-ordered reuse
    return rc;
}

template <typename T>
static int reduce_segments_typed(int op, int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m, const SegmentPlan &p) {
    switch (op) {
        case EK_HSUM: return reduce_segments_op<EK_HSUM, T>(type, (T *) out, (const T *) in, n, starts, m, p);
        case EK_HPROD: return reduce_segments_op<EK_HPROD, T>(type, (T *) out, (const T *) in, n, starts, m, p);
        case EK_HMIN: return reduce_segments_op<EK_HMIN, T>(type, (T *) out, (const T *) in, n, starts, m, p);
        default: return reduce_segments_op<EK_HMAX, T>(type, (T *) out, (const T *) in, n, starts, m, p);
    }
}

// ---- repeat --------------------------------------------------------------------------------------------------------------
// Tile t is the output entries [peel + t * TE, peel + (t + 1) * TE), `peel` being the entries in front of the first 16-byte boundary
// of `out`; tile 0 takes those as well and the last tile the entries behind the last whole vector.  j = the number of starts <= i
// (upper bound); the entry is in[j - 1], or 0 for j == 0.
template <typename T, int K>
__device__ __forceinline__ void segment_lookup(const T *__restrict__ in, const uint32_t *__restrict__ starts, const uint32_t *win, uint32_t m,
                                               uint32_t top, uint32_t j0, uint32_t cnt, uint32_t wtop, bool resident, const uint32_t (&i)[K],
                                               T (&v)[K]) {
    uint32_t pos[K], zero[K], count[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { pos[k] = 0; zero[k] = 0; }
    if (resident) {
#pragma unroll
        for (int k = 0; k < K; ++k) count[k] = cnt;
        search_steps<uint32_t, true, K>(win, zero, zero, count, cnt - 1, wtop, i, pos);
#pragma unroll
        for (int k = 0; k < K; ++k) pos[k] += j0;                                                 // <= j0 + cnt <= m
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) count[k] = m;
        search_steps<uint32_t, true, K>(starts, zero, zero, count, m - 1, top, i, pos);           // <= m
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = pos[k] ? in[pos[k] - 1] : T(0);
}

template <typename T>
__global__ __launch_bounds__(256) void k_repeat_segments(T *__restrict__ out, const T *__restrict__ in, const uint32_t *__restrict__ starts,
                                                         uint32_t m, uint32_t top, uint32_t size, uint32_t peel, uint32_t tiles,
                                                         uint32_t per_workgroup) {
    constexpr uint32_t N = 16 / sizeof(T), TE = 256 * N * kSegRepeatVectors;
    __shared__ uint32_t win[kSegWindow];
    const uint32_t t0 = blockIdx.x * per_workgroup, t1 = tiles - t0 < per_workgroup ? tiles : t0 + per_workgroup;   // (t0 < tiles)
    // j0: the number of starts <= the tile's first entry.  A workgroup's tiles are consecutive, so only its first tile searches
    // `starts` for it; every later one takes it from the window of the tile before (unless that window did not reach).
    uint32_t j0 = 0;
    bool known = false;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t b0 = (uint64_t) peel + (uint64_t) t * TE;
        const uint32_t a0 = (uint32_t) b0, e0 = t ? a0 : 0u, e1 = b0 + TE < size ? (uint32_t) (b0 + TE) : size;      // e0 < e1 <= size
        if (!known) {
            const uint32_t at[1] = { e0 }, zero[1] = { 0 }, all[1] = { m };
            uint32_t pos[1] = { 0 };
            search_steps<uint32_t, true, 1>(starts, zero, zero, all, m - 1, top, at, pos);
            j0 = pos[0];                                                                          // <= m
        }
        // the window: starts[j0 .. j0 + cnt), 256 at a time until it holds a start behind the tile or `starts` ends
        const uint32_t room = m - j0 < kSegWindow ? m - j0 : kSegWindow;
        uint32_t cnt = 0;
        bool resident = room == 0;
        while (cnt < room) {
            const uint32_t step = room - cnt < 256u ? room - cnt : 256u;
            if (threadIdx.x < step) win[cnt + threadIdx.x] = starts[j0 + cnt + threadIdx.x];
            __syncthreads();
            cnt += step;
            resident = j0 + cnt == m || win[cnt - 1] > e1;
            if (resident) break;
        }
        const uint32_t wtop = cnt ? 1u << (31 - __clz(cnt)) : 0u;
        const uint32_t nvec = (e1 - a0) / N, rest = e1 - a0 - nvec * N;
        for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
            uint32_t i[N];
            Pack<T, N> p;
#pragma unroll
            for (uint32_t k = 0; k < N; ++k) i[k] = a0 + v * N + k;
            segment_lookup<T, N>(in, starts, win, m, top, j0, cnt, wtop, resident, i, p.v);
            pack_store<T, N, true>(out + a0 + v * N, p);
        }
        // by element: behind the last whole vector (the last tile only) and in front of the first (tile 0 only)
        if (threadIdx.x < rest || (t == 0 && threadIdx.x >= 64 && threadIdx.x - 64 < peel)) {
            const uint32_t i[1] = { threadIdx.x < rest ? a0 + nvec * N + threadIdx.x : threadIdx.x - 64 };
            T v[1];
            segment_lookup<T, 1>(in, starts, win, m, top, j0, cnt, wtop, resident, i, v);
            out[i[0]] = v[0];
        }
        known = resident;
        if (resident) {                                   // the next tile begins at e1
            const uint32_t at[1] = { e1 }, zero[1] = { 0 }, all[1] = { cnt };
            uint32_t pos[1] = { 0 };
            search_steps<uint32_t, true, 1>(win, zero, zero, all, cnt - 1, wtop, at, pos);
            j0 += pos[0];                                                                         // <= j0 + cnt <= m
        }
        __syncthreads();
    }
}

template <typename T> static int repeat_segments_typed(void *out, const void *in, const uint32_t *starts, size_t m, size_t size) {
    Context &c = ctx();
    constexpr size_t N = 16 / sizeof(T), TE = 256 * N * kSegRepeatVectors;
    size_t peel = head_of((const T *) out);
    if (peel > size) peel = size;
    const size_t tiles = std::max<size_t>((size - peel + TE - 1) / TE, 1);
    const size_t cap = std::min(tiles, (size_t) c.num_cu * kSegRepeatBlocksPerCu), per_workgroup = (tiles + cap - 1) / cap;
    const size_t grid = (tiles + per_workgroup - 1) / per_workgroup;
    hipLaunchKernelGGL((k_repeat_segments<T>), dim3((unsigned) grid), dim3(256), 0, c.stream, (T *) out, (const T *) in, starts, (uint32_t) m,
                       search_top(m), (uint32_t) size, (uint32_t) peel, (uint32_t) tiles, (uint32_t) per_workgroup);
    EK_LAUNCH_CHECK("repeat_segments", size, (size + m) * sizeof(T) + m * 4);
    return EK_OK;
}

static int segments_size_check(const char *what, size_t n, size_t m) {
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull)
        return fail(EK_ERR_UNSUPPORTED, "%s: 2^32 entries or segments or more are unsupported (%zu, %zu)", what, n, m);
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_reduce_segments_plan(int type, size_t n, size_t m, int compute_units, int *route, int *group_lanes, int *splits, size_t *workgroups) {
    if (int rc = numeric_type_check("ek_hip_reduce_segments_plan()", type)) return rc;
    if (int rc = segments_size_check("ek_hip_reduce_segments_plan()", n, m)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_reduce_segments_plan(): %d compute units", compute_units);
    const SegmentPlan p = segment_plan(type_size(type), n, m, compute_units);
    if (route) *route = p.route;
    if (group_lanes) *group_lanes = p.route == 1 ? 1 << p.glog : 0;
    if (splits) *splits = (int) p.splits;
    if (workgroups) *workgroups = p.workgroups;
    return EK_OK;
}

int ek_hip_reduce_segments(int op, int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m) {
    if (int rc = ensure_init()) return rc;
    if (op < 0 || op >= EK_REDUCE_COUNT) return fail(EK_ERR_INVALID, "ek_hip_reduce_segments(): unknown op %d", op);
    if (int rc = numeric_type_check("ek_hip_reduce_segments()", type)) return rc;
    if (int rc = segments_size_check("ek_hip_reduce_segments()", n, m)) return rc;
    if (m == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_reduce_segments()", elem, out)) return rc;
    if (int rc = pointers_check("ek_hip_reduce_segments()", sizeof(uint32_t), starts)) return rc;
    if (int rc = n ? pointers_check("ek_hip_reduce_segments()", elem, in) : alignment_check("ek_hip_reduce_segments()", elem, in)) return rc;
    const SegmentPlan p = segment_plan(elem, n, m, ctx().num_cu);
    return dispatch_numeric(type, [&](auto t) { return reduce_segments_typed<typename decltype(t)::type>(op, type, out, in, n, starts, m, p); });
}

int ek_hip_repeat_segments(int type, void *out, const void *in, const uint32_t *starts, size_t m, size_t n) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_repeat_segments()", type)) return rc;
    if (int rc = segments_size_check("ek_hip_repeat_segments()", n, m)) return rc;
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_repeat_segments()", elem, out)) return rc;
    if (m) {
        if (int rc = pointers_check("ek_hip_repeat_segments()", elem, in)) return rc;
        if (int rc = pointers_check("ek_hip_repeat_segments()", sizeof(uint32_t), starts)) return rc;
    }
    return elem == 4 ? repeat_segments_typed<uint32_t>(out, in, starts, m, n) : repeat_segments_typed<uint64_t>(out, in, starts, m, n);
}

}
