// Per-block prefix sums: for the n / B blocks of B consecutive entries (the samples of a ray, a row of a row-major table)
//     out[j * B + k] = x[0] + .. + x[k]          flags 0                       x = in + j * B
//                      x[0] + .. + x[k - 1]      EK_SCAN_EXCLUSIVE
//                      x[k] + .. + x[B - 1]      EK_SCAN_REVERSE
//                      x[k + 1] + .. + x[B - 1]  both                          (the empty sum is +0)
// The whole-array spelling, psum(x) - repeat(gather(psum(x), block starts), B), is three more passes, subtracts two large sums to
// get a small one, and inherits the run-to-run variation of the look-back scan (scan.hip).  Here a block belongs to one workgroup or
// is cut into pieces in a fixed way, so:
//   * every output is a sum of its own terms only; nothing is ever subtracted, and an exclusive result is not "inclusive minus x";
//   * an inclusive entry with one term is that input bit for bit (-0.0 included): running sums start from -0.0, the identity;
//   * an exclusive entry k IS the inclusive entry k - 1 (k + 1 for REVERSE) of the same call, bit for bit: every kernel computes
//     inclusive values and MOVES them by one position (in LDS, through LDS between lanes, or by the seam launch of route 3);
//   * no value of one block reaches another block's output;
//   * the shape of every sum is fixed by (type, n, B, flags, pointer alignment, #CU): bit-identical from run to run;
//   * NO KERNEL WAITS FOR ANOTHER WORKGROUP: no ticket, no descriptor, no look-back, no polling loop, no atomics.  Where one
//     workgroup needs another's result it is a later launch on the stream.  That is what makes the result reproducible and the call
//     capturable, and a kernel that never waits cannot spin.
//
// scan_plan() picks the route (ek_hip_psum_blocks_plan reports it):
//   0 copy / zero fill   B == 1.
//   1 packed             B <= 1024.  A workgroup stages a tile of whole blocks (at most 16 KiB, a multiple of the vector width in
//                        blocks) in LDS with 16-byte non-temporal loads; head / shift / tail as in k_reduce_packed, so a misaligned
//                        view costs no more than an aligned one.  Every block gets a group of G = 2^glog ADJACENT lanes, G about B / 4
//                        and at most 64; lane l owns the CONTIGUOUS run [l * run, (l + 1) * run) of its block with
//                        run = ceil(B / G) | 1, an ODD number: the lanes of a group then read words l * run + i, which fall into
//                        G different banks for any power-of-two bank count (an even run would put them gcd(run, 64) to a bank).
//                        Groups of one wave sit B words apart and still meet in a bank for a power-of-two B up to 128 (B = 64:
//                        four groups 64 words apart, 4-way): see DESIGN section 3.  A lane adds its run up, the run totals are scanned inside the group by
//                        glog __shfl_up steps masked at the group's edge (all lanes of a wave execute every shuffle: the trip count
//                        is uniform), then the lane walks its run again from its offset and writes the running sums to a SECOND LDS
//                        tile, one position further on for EXCLUSIVE, at the mirrored index for REVERSE.  That tile leaves with
//                        16-byte stores, shifted for the alignment of `out`, which need not be that of `in`.
//   2 one workgroup per block, B > 1024: the block is walked in chunks of 256 lanes x one 16-byte vector x kScanBlockRows rows with
//                        a carry kept by the workgroup; inside a chunk the register scan of k_scan_lookback (vector-local scan, wave
//                        __shfl_up scan, four wave totals through LDS).  Entries in front of the block's first 16-byte boundary and
//                        behind its last go by element.  REVERSE walks the chunks from the block's end, mirrors the lane order and
//                        reverses every vector in registers.  EXCLUSIVE hands every lane its left neighbour's last running sum
//                        through LDS.  Stores are 16-byte stores where `out` shares the alignment of `in`, by element otherwise.
//   3 split              fewer than 2 x #CU blocks of at least 16 Ki entries: (1) the totals of S pieces per block (multiples of the
//                        vector width, the last may be shorter; split_shape and k_reduce_segments of ek_block.h), (2) the packed kernel, exclusive, same direction, over the m x S
//                        totals with B = S, (3) the chunk kernel over every piece with its carry-in; for EXCLUSIVE (4) a seam launch
//                        that writes every piece's first entry: the last running sum of the piece before it, bit for bit.  12 bytes
//                        per 4-byte entry instead of 8.  Scratch from ek_hip_malloc, freed stream-ordered.
#include "ek_block.h"

namespace ek {

constexpr int kScanBlockRows = 4;                  // a chunk: 256 lanes x 16 bytes x 4 rows = 16 KiB

struct ScanPlan {
    int regime;
    size_t splits, piece;                // 3: pieces per block and entries per piece (the last piece of a block may be shorter)
    uint32_t tile_blocks, glog, run;     // 1: blocks per tile, log2(lanes per block), entries per lane (odd)
    size_t workgroups;                   // grid of the first launch
};

static void packed_shape(size_t elem, size_t m, size_t B, ScanPlan &p) {
    p.tile_blocks = tile_blocks(elem, m, B, p.workgroups);
    p.glog = 0;
    while ((4u << p.glog) < B && p.glog < 6) p.glog++;
    p.run = (uint32_t) ((B + (1u << p.glog) - 1) >> p.glog) | 1u;
}

static ScanPlan scan_plan(size_t elem, size_t n, size_t B, int num_cu) {
    ScanPlan p = { 0, 1, B, 0, 0, 0, 1 };
    const size_t m = n / B, cu = num_cu > 0 ? (size_t) num_cu : 256;
    if (B == 1) return p;
    if (B <= kBlockPackedMax) {
        p.regime = 1;
        packed_shape(elem, m, B, p);
        return p;
    }
    p.regime = split_shape(elem, m, B, cu, p.splits, p.piece) ? 3 : 2;
    p.workgroups = std::min<size_t>(m * p.splits, kBlockMaxGrid);
    return p;
}

template <typename T> __device__ __forceinline__ T scan_add(T a, T b) {
    using W = wrap_t<T>;                                    // unsigned arithmetic for integers: wrap-around, no UB
    return (T) ((W) a + (W) b);
}

template <typename T> __device__ __forceinline__ T block_scan_shfl_up(T v, int delta) {
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

// ---- route 1: packed ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_scan_packed(T *out, const T *in, size_t m, uint32_t B, uint32_t tile_blocks, uint32_t glog,
                                                     uint32_t run, size_t tiles, int flags) {
    constexpr uint32_t N = 16 / sizeof(T), E = kBlockTileBytes / sizeof(T);
    constexpr T kId = sum_identity<T>;
    __shared__ __attribute__((aligned(16))) T tile_in[E + N];
    __shared__ __attribute__((aligned(16))) T tile_out[E + N];
    const bool excl = flags & EK_SCAN_EXCLUSIVE, rev = flags & EK_SCAN_REVERSE;
    const uint32_t G = 1u << glog, group = threadIdx.x >> glog, l = threadIdx.x & (G - 1), groups = 256u >> glog;
    // this lane's run of its block, in scan order (entry k of the scan is entry B - 1 - k of the block for REVERSE)
    const uint32_t k0 = l * run < B ? l * run : B, k1 = k0 + run < B ? k0 + run : B;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t b0 = t * tile_blocks;
        const uint32_t nb = (uint32_t) (m - b0 < tile_blocks ? m - b0 : tile_blocks), len = nb * B;       // len <= E
        const T *src = in + b0 * B;
        uint32_t head = head_of(src);
        if (head > len) head = len;
        // element e of the tile lives at tile_in[shift + e]: the first whole vector lands on a 16-byte boundary of LDS
        const uint32_t shift = (N - head) % N, nvec = (len - head) / N, tail = len - head - nvec * N;
        T *ti = tile_in + shift;
        if (threadIdx.x < head) ti[threadIdx.x] = src[threadIdx.x];
#pragma unroll 4
        for (uint32_t v = threadIdx.x; v < nvec; v += 256)
            *reinterpret_cast<Pack<T, N> *>(ti + head + v * N) = pack_load<T, N, true>(src + head + v * N);
        if (threadIdx.x < tail) ti[head + nvec * N + threadIdx.x] = src[head + nvec * N + threadIdx.x];
        // ... and element e of the result at tile_out[oshift + e], by the alignment of `out`
        T *dst = out + b0 * B;
        uint32_t ohead = head_of(dst);
        if (ohead > len) ohead = len;
        const uint32_t oshift = (N - ohead) % N, onvec = (len - ohead) / N, otail = len - ohead - onvec * N;
        T *to = tile_out + oshift;
        __syncthreads();
        // (the same trip count for every lane: the shuffles below are executed by whole waves)
        const uint32_t trips = (nb + groups - 1) / groups;
        for (uint32_t it = 0; it < trips; ++it) {
            const uint32_t blk = it * groups + group;
            const bool valid = blk < nb;
            const T *b = ti + blk * B;
            T *o = to + blk * B;
            T s = kId;
            if (valid)
                for (uint32_t k = k0; k < k1; ++k) s = scan_add(s, b[rev ? B - 1 - k : k]);
            for (uint32_t d = 1; d < G; d <<= 1) {
                const T up = block_scan_shfl_up(s, (int) d);
                if (l >= d) s = scan_add(s, up);
            }
            T p = block_scan_shfl_up(s, 1);                      // the sum of the runs in front of this lane's
            if (l == 0) p = kId;
            if (valid) {
                if (excl && l == 0) o[rev ? B - 1 : 0] = T(0);
                for (uint32_t k = k0; k < k1; ++k) {
                    p = scan_add(p, b[rev ? B - 1 - k : k]);
                    const uint32_t w = excl ? k + 1 : k;
                    if (w < B) o[rev ? B - 1 - w : w] = p;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < ohead) dst[threadIdx.x] = to[threadIdx.x];
#pragma unroll 4
        for (uint32_t v = threadIdx.x; v < onvec; v += 256)
            pack_store<T, N, true>(dst + ohead + v * N, *reinterpret_cast<const Pack<T, N> *>(to + ohead + v * N));
        if (threadIdx.x < otail) dst[ohead + onvec * N + threadIdx.x] = to[ohead + onvec * N + threadIdx.x];
        // (no barrier here: the next tile's loads write tile_in, which nobody reads any more, and its barrier after the loads
        //  comes before anybody writes tile_out again)
    }
}

// ---- routes 2 and 3: a workgroup walks a block, or piece s of block j (S pieces of `piece` entries per block) ----------------
template <typename T> __device__ __forceinline__ void pack_reverse(Pack<T, 16 / sizeof(T)> &p) {
    constexpr int V = 16 / sizeof(T);
#pragma unroll
    for (int j = 0; j < V / 2; ++j) { const T t = p.v[j]; p.v[j] = p.v[V - 1 - j]; p.v[V - 1 - j] = t; }
}

template <typename T>
__global__ __launch_bounds__(256) void k_scan_segments(T *out, const T *in, size_t B, size_t piece, uint32_t S, size_t segments,
                                                       const T *__restrict__ carries, T *__restrict__ lasts, int flags) {
    constexpr int V = 16 / sizeof(T), R = kScanBlockRows;
    constexpr T kId = sum_identity<T>;                    // -0.0 for floating point: padding must not turn -0.0 into +0.0
    __shared__ T s_wave[2][R][4];                         // (by chunk parity: a chunk's totals are read while the next one's are written)
    __shared__ T s_last[R][256];                          // EXCLUSIVE: every lane's last running sum of a row
    const bool excl = flags & EK_SCAN_EXCLUSIVE, rev = flags & EK_SCAN_REVERSE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t seg = blockIdx.x; seg < segments; seg += gridDim.x) {
        size_t j = seg, s = 0, off = 0;
        if (S > 1) { j = seg / S; s = seg - j * S; off = s * piece; }
        const size_t len = B - off < piece ? B - off : piece;
        const T *src = in + j * B + off;
        T *dst = out + j * B + off;
        const bool first = S == 1 || (rev ? s == S - 1 : s == 0);          // the piece the scan of this block starts with
        size_t head = head_of(src);
        if (head > len) head = len;
        const size_t nvec = (len - head) / V;
        const uint32_t tail = (uint32_t) (len - head - nvec * V);
        const T *vsrc = src + head;
        T *vdst = dst + head;
        const bool store_vec = (reinterpret_cast<uintptr_t>(vdst) & 15u) == 0;
        // In scan order: `npre` entries by element, nvec vectors, `npost` entries by element; entry g of the scan is entry g of
        // the segment, or entry len - 1 - g for REVERSE.
        const uint32_t npre = rev ? tail : (uint32_t) head, npost = rev ? (uint32_t) head : tail;
        T pre[V - 1], post[V - 1];
#pragma unroll
        for (uint32_t i = 0; i < V - 1; ++i) {
            pre[i] = i < npre ? src[rev ? len - 1 - i : i] : kId;
            const size_t g = npre + nvec * V + i;
            post[i] = i < npost ? src[rev ? len - 1 - g : g] : kId;
        }
        __syncthreads();                                   // (out may be in: thread 0 overwrites these entries below; s_last is free again)
        T carry = first ? kId : carries[seg];              // the sum of everything in front of the next entry
        T prev = T(0);                                     // EXCLUSIVE: the running sum AT the entry before the next one
        bool have_prev = first;                            // (the first entry of a later piece is written by the seam launch)
#pragma unroll
        for (uint32_t i = 0; i < V - 1; ++i) {
            if (i < npre) {
                carry = scan_add(carry, pre[i]);
                if (threadIdx.x == 0) {
                    if (!excl) dst[rev ? len - 1 - i : i] = carry;
                    else if (have_prev) dst[rev ? len - 1 - i : i] = prev;
                }
                prev = carry;
                have_prev = true;
            }
        }
        uint32_t parity = 0;
        for (size_t q0 = 0; q0 < nvec; q0 += (size_t) R * 256, parity ^= 1u) {
            // rows of this chunk that hold a vector (uniform over the workgroup): the others are skipped whole
            const int rows = nvec - q0 >= (size_t) R * 256 ? R : (int) ((nvec - q0 + 255) >> 8);
            Pack<T, V> v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t q = q0 + (size_t) r * 256 + threadIdx.x;
                if (q < nvec) {
                    v[r] = pack_load<T, V, true>(vsrc + (rev ? nvec - 1 - q : q) * V);
                    if (rev) pack_reverse<T>(v[r]);
                } else {
#pragma unroll
                    for (int i = 0; i < V; ++i) v[r].v[i] = kId;
                }
            }
            T incl[R];             // (exclusive over the lanes: what is added to this lane's vector)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= rows) break;
#pragma unroll
                for (int i = 1; i < V; ++i) v[r].v[i] = scan_add(v[r].v[i], v[r].v[i - 1]);
                T t = v[r].v[V - 1];
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const T up = block_scan_shfl_up(t, d);
                    if (lane >= d) t = scan_add(t, up);
                }
                const T below = block_scan_shfl_up(t, 1);
                incl[r] = lane == 0 ? kId : below;
                if (lane == 63) s_wave[parity][r][wave] = t;
            }
            __syncthreads();
            T running = carry;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= rows) break;
                T before = running;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (w < wave) before = scan_add(before, s_wave[parity][r][w]);
                    running = scan_add(running, s_wave[parity][r][w]);
                }
                const T add = scan_add(before, incl[r]);
#pragma unroll
                for (int i = 0; i < V; ++i) v[r].v[i] = scan_add(v[r].v[i], add);
            }
            carry = running;
            if (excl) {
                // every entry takes the running sum of the entry before it: inside a vector from its neighbour, across lanes,
                // rows and chunks through LDS -- moved, never recomputed
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < rows) s_last[r][threadIdx.x] = v[r].v[V - 1];
                __syncthreads();
                const size_t qe = (nvec - q0 < (size_t) R * 256 ? nvec - q0 : (size_t) R * 256) - 1;     // the chunk's last vector
                const T chunk_last = s_last[qe >> 8][qe & 255];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r >= rows) break;
                    T left = prev;
                    if (threadIdx.x > 0) left = s_last[r][threadIdx.x - 1];
                    else if (r > 0) left = s_last[r - 1][255];
#pragma unroll
                    for (int i = V - 1; i > 0; --i) v[r].v[i] = v[r].v[i - 1];
                    v[r].v[0] = left;
                }
                prev = chunk_last;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t q = q0 + (size_t) r * 256 + threadIdx.x;
                if (q < nvec) {
                    // (EXCLUSIVE, a later piece: scan entry 0 belongs to the seam launch)
                    const bool skip0 = excl && !have_prev && q == 0;
                    if (rev) pack_reverse<T>(v[r]);
                    T *p = vdst + (rev ? nvec - 1 - q : q) * V;
                    if (store_vec && !skip0) {
                        pack_store<T, V, true>(p, v[r]);
                    } else {
#pragma unroll
                        for (int i = 0; i < V; ++i)
                            if (!(skip0 && i == (rev ? V - 1 : 0))) p[i] = v[r].v[i];
                    }
                }
            }
            have_prev = true;
        }
        T last = prev;
#pragma unroll
        for (uint32_t i = 0; i < V - 1; ++i) {
            if (i < npost) {
                const size_t g = npre + nvec * V + i;
                carry = scan_add(carry, post[i]);
                if (threadIdx.x == 0) {
                    if (!excl) dst[rev ? len - 1 - g : g] = carry;
                    else if (have_prev) dst[rev ? len - 1 - g : g] = last;
                }
                last = carry;
                have_prev = true;
            }
        }
        if (lasts && threadIdx.x == 0) lasts[seg] = last;
    }
}

/// route 3, launch 4 (EXCLUSIVE only): the first entry of every piece but the one its block's scan starts with is the last running
/// sum of the piece in front of it
template <typename T>
__global__ __launch_bounds__(256) void k_scan_seams(T *__restrict__ out, const T *__restrict__ lasts, size_t B, size_t piece, uint32_t S,
                                                    size_t segments, int rev) {
    for (size_t seg = (size_t) blockIdx.x * 256 + threadIdx.x; seg < segments; seg += (size_t) gridDim.x * 256) {
        const size_t j = seg / S, s = seg - j * S, off = s * piece;
        const size_t len = B - off < piece ? B - off : piece;
        if (!rev) {
            if (s > 0) out[j * B + off] = lasts[seg - 1];
        } else {
            if (s + 1 < S) out[j * B + off + len - 1] = lasts[seg + 1];
        }
    }
}

template <typename T> static int launch_scan_packed(const char *name, T *out, const T *in, size_t m, size_t B, const ScanPlan &p, int flags) {
    const size_t tiles = (m + p.tile_blocks - 1) / p.tile_blocks;
    hipLaunchKernelGGL((k_scan_packed<T>), dim3((unsigned) p.workgroups), dim3(256), 0, ctx().stream, out, in, m, (uint32_t) B, p.tile_blocks,
                       p.glog, p.run, tiles, flags);
    EK_LAUNCH_CHECK(name, m * B, 2 * m * B * sizeof(T));
    return EK_OK;
}

template <typename T> static int scan_split(T *out, const T *in, size_t n, size_t B, const ScanPlan &p, int flags, T *scratch) {
    Context &c = ctx();
    const size_t m = n / B, segments = m * p.splits;
    T *carries = scratch, *lasts = (flags & EK_SCAN_EXCLUSIVE) ? scratch + segments : nullptr;
    // launch 1: the total of every piece, by the kernel that sums the pieces of block_sum (ek_block.h)
    hipLaunchKernelGGL((k_reduce_segments<Reducer<EK_HSUM, T>, T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, carries, in, B, p.piece,
                       (uint32_t) p.splits, segments);
    EK_LAUNCH_CHECK("psum_blocks_totals", n, (n + segments) * sizeof(T));
    ScanPlan fold = p;
    packed_shape(sizeof(T), m, p.splits, fold);
    if (int rc = launch_scan_packed<T>("psum_blocks_carries", carries, carries, m, p.splits, fold, (flags & EK_SCAN_REVERSE) | EK_SCAN_EXCLUSIVE))
        return rc;
    hipLaunchKernelGGL((k_scan_segments<T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, out, in, B, p.piece, (uint32_t) p.splits,
                       segments, (const T *) carries, lasts, flags);
    EK_LAUNCH_CHECK("psum_blocks_pieces", n, (2 * n + segments) * sizeof(T));
    if (lasts) {
        hipLaunchKernelGGL((k_scan_seams<T>), dim3((unsigned) ((segments + 255) / 256)), dim3(256), 0, c.stream, out, (const T *) lasts, B, p.piece,
                           (uint32_t) p.splits, segments, (int) (flags & EK_SCAN_REVERSE));
        EK_LAUNCH_CHECK("psum_blocks_seams", segments, 2 * segments * sizeof(T));
    }
    return EK_OK;
}

template <typename T> static int psum_blocks_typed(void *out_, const void *in_, size_t n, size_t B, const ScanPlan &p, int flags) {
    RoctxRange range("enoki-hip: block prefix sum");
    T *out = (T *) out_;
    const T *in = (const T *) in_;
    const size_t m = n / B;
    if (p.regime == 1) return launch_scan_packed<T>("psum_blocks_packed", out, in, m, B, p, flags);
    if (p.regime == 2) {
        hipLaunchKernelGGL((k_scan_segments<T>), dim3((unsigned) p.workgroups), dim3(256), 0, ctx().stream, out, in, B, B, 1u, m,
                           (const T *) nullptr, (T *) nullptr, flags);
        EK_LAUNCH_CHECK("psum_blocks", n, 2 * n * sizeof(T));
        return EK_OK;
    }
    void *scratch = nullptr;
    if (int rc = ek_hip_malloc(2 * m * p.splits * sizeof(T), &scratch)) return rc;
    const int rc = scan_split<T>(out, in, n, B, p, flags, (T *) scratch);
    ek_hip_free(scratch);   // stream-ordered reuse
    return rc;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_psum_blocks_plan(int type, size_t n, size_t block, int compute_units, int *regime, int *splits, size_t *workgroups) {
    if (int rc = numeric_type_check("ek_hip_psum_blocks_plan()", type)) return rc;
    if (int rc = blocks_shape_check("ek_hip_psum_blocks_plan()", n, block)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_psum_blocks_plan(): %d compute units", compute_units);
    ScanPlan p = { 0, 1, block, 0, 0, 0, 0 };
    if (n) p = scan_plan(type_size(type), n, block, compute_units);
    if (regime) *regime = p.regime;
    if (splits) *splits = (int) p.splits;
    if (workgroups) *workgroups = p.workgroups;
    return EK_OK;
}

int ek_hip_psum_blocks(int type, void *out, const void *in, size_t n, size_t block, int flags) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_psum_blocks()", type)) return rc;
    if (flags & ~(EK_SCAN_EXCLUSIVE | EK_SCAN_REVERSE)) return fail(EK_ERR_INVALID, "ek_hip_psum_blocks(): unknown flags %d", flags);
    if (int rc = blocks_shape_check("ek_hip_psum_blocks()", n, block)) return rc;
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_psum_blocks()", elem, out, in)) return rc;
    const ScanPlan p = scan_plan(elem, n, block, ctx().num_cu);
    if (p.regime == 0) {
        // one term per sum: the input itself; no term at all: +0 (all bits clear in every type)
        if (flags & EK_SCAN_EXCLUSIVE) return ek_hip_memset(out, 0, n * elem);
        return out == in ? EK_OK : ek_hip_memcpy_device(out, in, n * elem);
    }
    return dispatch_numeric(type, [&](auto t) { return psum_blocks_typed<typename decltype(t)::type>(out, in, n, block, p, flags); });
}

}
