// Block reductions: out[j] = reduce(in[j * B .. (j + 1) * B)) for the n / B blocks of B consecutive entries (the spp samples of a
// pixel, a row of a row-major matrix), and their transpose  repeat: out[i] = in[i / B].
//
// The spellings these replace, scatter_add(zero(n / B), x, arange(n) / B) and gather(v, arange(n) / B), stream an n-entry index
// array that carries no information.  The algorithmic traffic is one pass: sizeof(T) * (1 + 1 / B) bytes per element, both ways.
//
// ek_hip_reduce_blocks takes one of five routes, chosen by block_plan() (what ek_hip_reduce_blocks_plan reports):
//   0 copy    B == 1.
//   1 whole   B == n: ek_hip_reduce, bit for bit.
//   2 packed  B <= 1024.  A workgroup takes a tile of whole blocks, at most 16 KiB and a multiple of the vector width in blocks, so
//             every tile starts at the base pointer's alignment.  The tile goes to LDS with 16-byte non-temporal loads (the few
//             elements in front of the first 16-byte boundary and behind the last one by element, and the tile is shifted in LDS by
//             that many so that the LDS stores are 16-byte stores too): a misaligned view costs no more than an aligned one, and the
//             result does not depend on the alignment.  Then every block gets a group of G = 2^ceil(log2(min(B, 64))) ADJACENT lanes:
//             lane l of the group combines entries l, l + G, .. of its block and the group finishes with log2(G) shuffle steps.
//             Groups, not padding: the lanes of a wave then read (64 / G) * min(B, G) <= 64 consecutive LDS words per access -- no
//             two in one bank for any B, where one lane per block at stride B is gcd(B, 64)-way conflicted and padding would have to
//             change with B -- and a block of 64 entries is 1 read and 6 shuffles per lane instead of 64 dependent reads in one lane.
//   3 one workgroup per block, B > 1024: the block is streamed as k_reduce_stage1 streams an array (16-byte non-temporal loads, four
//             in flight per lane, four accumulators, the 256-thread fold); the entries in front of the block's first 16-byte boundary
//             and behind its last are taken one per lane, so B * sizeof(T) need not be a multiple of 16 and neither need the base.
//   4 split   fewer than 2 x #CU blocks of at least 16 Ki entries: every block is cut into S pieces of P entries (P a multiple of the
//             vector width: the pieces of a block share its alignment) so that about 4 x #CU workgroups run; the same kernel as 3
//             writes m x S partials, which the packed kernel folds with B = S.  Two launches in a fixed order.
// The kernel of 3 and 4 (k_reduce_segments), the tile and split rules (tile_blocks, split_shape) and head_of are shared with the
// other per-block primitives: ek_block.h.  The staging of 2 stays spelled out in k_reduce_packed, k_scan_packed and k_sort_packed:
// as a function of its own it compiles to other code for the 8-byte types.
// No atomics, no read-back, no host wait; the partials of 4 come from the caching allocator (capturable).  Every sum has a fixed
// shape for a given (type, op, n, B, alignment, #CU): run-to-run identical.
#include "ek_block.h"

namespace ek {

struct BlockPlan {
    int regime;
    size_t splits, piece;          // 4: pieces per block and entries per piece (the last piece of a block may be shorter)
    uint32_t tile_blocks, glog;    // 2: blocks per tile, log2(lanes per block)
    size_t workgroups;             // grid of the first launch
};

static void packed_shape(size_t elem, size_t m, size_t B, BlockPlan &p) {
    p.tile_blocks = tile_blocks(elem, m, B, p.workgroups);
    p.glog = 0;
    while ((1u << p.glog) < B && p.glog < 6) p.glog++;
}

static BlockPlan block_plan(size_t elem, size_t n, size_t B, int num_cu) {
    BlockPlan p = { 0, 1, B, 0, 0, 1 };
    const size_t m = n / B, N = 16 / elem, cu = num_cu > 0 ? (size_t) num_cu : 256;
    if (B == 1) return p;
    if (B == n) {
        // (the grid of ek_hip_reduce at its default tuning)
        p.regime = 1;
        p.workgroups = std::min<size_t>(std::min<size_t>((((n / N + 3) / 4 + 1) + 255) / 256, cu * 4), 2048);
        return p;
    }
    if (B <= kBlockPackedMax) {
        p.regime = 2;
        packed_shape(elem, m, B, p);
        return p;
    }
    p.regime = split_shape(elem, m, B, cu, p.splits, p.piece) ? 4 : 3;
    p.workgroups = std::min<size_t>(m * p.splits, kBlockMaxGrid);
    return p;
}

template <typename R, typename T>
__global__ __launch_bounds__(256) void k_reduce_packed(T *__restrict__ out, const T *__restrict__ in, size_t m, uint32_t B, uint32_t tile_blocks,
                                                       uint32_t glog, size_t tiles) {
    constexpr uint32_t N = 16 / sizeof(T), E = kBlockTileBytes / sizeof(T);
    __shared__ __attribute__((aligned(16))) T tile[E + N];
    const uint32_t G = 1u << glog, group = threadIdx.x >> glog, l = threadIdx.x & (G - 1), groups = 256u >> glog;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t b0 = t * tile_blocks;
        const uint32_t nb = (uint32_t) (m - b0 < tile_blocks ? m - b0 : tile_blocks), len = nb * B;       // len <= E
        const T *src = in + b0 * B;
        uint32_t head = head_of(src);
        if (head > len) head = len;
        // element e of the tile lives at tile[shift + e]: the first whole vector lands on a 16-byte boundary of LDS
        const uint32_t shift = (N - head) % N, nvec = (len - head) / N, tail = len - head - nvec * N;
        T *dst = tile + shift;
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
#pragma unroll 4
        for (uint32_t v = threadIdx.x; v < nvec; v += 256)
            *reinterpret_cast<Pack<T, N> *>(dst + head + v * N) = pack_load<T, N, true>(src + head + v * N);
        if (threadIdx.x < tail) dst[head + nvec * N + threadIdx.x] = src[head + nvec * N + threadIdx.x];
        __syncthreads();
        // (the same trip count for every lane: the shuffles below are executed by whole waves)
        const uint32_t trips = (nb + groups - 1) / groups;
        for (uint32_t it = 0; it < trips; ++it) {
            const uint32_t blk = it * groups + group;
            T acc = R::identity();
            if (blk < nb) {
                const T *b = dst + blk * B;
                for (uint32_t k = l; k < B; k += G) acc = R::combine(acc, b[k]);
            }
            for (uint32_t d = G >> 1; d; d >>= 1) acc = R::combine(acc, shfl_down(acc, (int) d));
            if (l == 0 && blk < nb) out[b0 + blk] = acc;
        }
        __syncthreads();
    }
}

template <typename R, typename T> static int launch_packed(const char *name, T *out, const T *in, size_t m, size_t B, const BlockPlan &p) {
    const size_t tiles = (m + p.tile_blocks - 1) / p.tile_blocks;
    hipLaunchKernelGGL((k_reduce_packed<R, T>), dim3((unsigned) p.workgroups), dim3(256), 0, ctx().stream, out, in, m, (uint32_t) B, p.tile_blocks,
                       p.glog, tiles);
    EK_LAUNCH_CHECK(name, m * B, (m * B + m) * sizeof(T));
    return EK_OK;
}

template <int Op, typename T> static int reduce_blocks_op(T *out, const T *in, size_t n, size_t B, const BlockPlan &p) {
    using R = Reducer<Op, T>;
    RoctxRange range("enoki-hip: block reduction");
    Context &c = ctx();
    const size_t m = n / B;
    if (p.regime == 2) return launch_packed<R, T>("reduce_blocks_packed", out, in, m, B, p);
    if (p.regime == 3) {
        hipLaunchKernelGGL((k_reduce_segments<R, T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, out, in, B, B, 1u, m);
        EK_LAUNCH_CHECK("reduce_blocks", n, (n + m) * sizeof(T));
        return EK_OK;
    }
    const size_t segments = m * p.splits;
    void *partials = nullptr;
    if (int rc = ek_hip_malloc(segments * sizeof(T), &partials)) return rc;
    BlockPlan fold = p;
    packed_shape(sizeof(T), m, p.splits, fold);
    hipLaunchKernelGGL((k_reduce_segments<R, T>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, (T *) partials, in, B, p.piece,
                       (uint32_t) p.splits, segments);
    int rc = EK_OK;
    if (hipError_t err = hipGetLastError(); err != hipSuccess) rc = hip_fail(err, "reduce_blocks_split", __FILE__, __LINE__);
    else {
        note_launch("reduce_blocks_split", n, (n + segments) * sizeof(T));
        rc = launch_packed<R, T>("reduce_blocks_fold", out, (const T *) partials, m, p.splits, fold);
    }
    ek_hip_free(partials);   // stream-ordered reuse
    return rc;
}

template <typename T> static int reduce_blocks_typed(int op, void *out, const void *in, size_t n, size_t B, const BlockPlan &p) {
    switch (op) {
        case EK_HSUM: return reduce_blocks_op<EK_HSUM, T>((T *) out, (const T *) in, n, B, p);
        case EK_HPROD: return reduce_blocks_op<EK_HPROD, T>((T *) out, (const T *) in, n, B, p);
        case EK_HMIN: return reduce_blocks_op<EK_HMIN, T>((T *) out, (const T *) in, n, B, p);
        default: return reduce_blocks_op<EK_HMAX, T>((T *) out, (const T *) in, n, B, p);
    }
}

int reduce_blocks_packed(int op, int type, void *out, const void *in, size_t m, size_t B) {
    BlockPlan p = { 2, 1, B, 0, 0, 1 };
    packed_shape(type_size(type), m, B, p);
    return dispatch_numeric(type, [&](auto t) { return reduce_blocks_typed<typename decltype(t)::type>(op, out, in, m * B, B, p); });
}

// ---- repeat --------------------------------------------------------------------------------------------------------------
// One 16-byte non-temporal store per lane and trip.  A lane divides ONCE (its first element / B); every later trip is `threads`
// vectors further on: quotient and remainder advance by the host's (dq, dr) with one conditional carry.  Inside a vector the
// remainder counts up to B.  The host peels the elements in front of the first 16-byte boundary of `out`; they and the elements
// behind the last whole vector (at most 6 together) are written one per lane by workgroup 0.
template <typename T>
__global__ __launch_bounds__(256) void k_repeat(T *__restrict__ out, const T *__restrict__ in, size_t total, size_t B, uint32_t peel, size_t dq, size_t dr) {
    constexpr uint32_t N = 16 / sizeof(T);
    const size_t items = (total - peel) / N, threads = (size_t) gridDim.x * 256;
    size_t item = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (item < items) {
        const size_t e = peel + item * N;
        size_t q = e / B, r = e - q * B;
        for (; item < items; item += threads) {
            Pack<T, N> p;
            size_t qq = q, rr = r;
#pragma unroll
            for (uint32_t i = 0; i < N; ++i) {
                p.v[i] = in[qq];
                if (++rr == B) { rr = 0; ++qq; }
            }
            pack_store<T, N, true>(out + peel + item * N, p);
            q += dq;
            r += dr;
            if (r >= B) { r -= B; ++q; }
        }
    }
    const uint32_t rest = peel + (uint32_t) ((total - peel) - items * N);
    if (blockIdx.x == 0 && threadIdx.x < rest) {
        const size_t e = threadIdx.x < peel ? threadIdx.x : peel + items * N + (threadIdx.x - peel);
        out[e] = in[e / B];
    }
}

template <typename T> static int repeat_typed(void *out, const void *in, size_t m, size_t B) {
    Context &c = ctx();
    constexpr size_t N = 16 / sizeof(T);
    const size_t total = m * B;
    size_t peel = head_of((const T *) out);
    if (peel > total) peel = total;
    const size_t items = (total - peel) / N;
    size_t blocks = (items + 255) / 256, cap = (size_t) c.num_cu * 16;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    const size_t step = blocks * 256 * N;
    hipLaunchKernelGGL((k_repeat<T>), dim3((unsigned) blocks), dim3(256), 0, c.stream, (T *) out, (const T *) in, total, B, (uint32_t) peel,
                       step / B, step % B);
    EK_LAUNCH_CHECK("repeat", total, (total + m) * sizeof(T));
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_reduce_blocks_plan(int type, size_t n, size_t block, int compute_units, int *regime, int *splits, size_t *workgroups) {
    if (int rc = numeric_type_check("ek_hip_reduce_blocks_plan()", type)) return rc;
    if (int rc = blocks_shape_check("ek_hip_reduce_blocks_plan()", n, block)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_reduce_blocks_plan(): %d compute units", compute_units);
    BlockPlan p = { 0, 1, block, 0, 0, 0 };
    if (n) p = block_plan(type_size(type), n, block, compute_units);
    if (regime) *regime = p.regime;
    if (splits) *splits = (int) p.splits;
    if (workgroups) *workgroups = p.workgroups;
    return EK_OK;
}

int ek_hip_reduce_blocks(int op, int type, void *out, const void *in, size_t n, size_t block) {
    if (int rc = ensure_init()) return rc;
    if (op < 0 || op >= EK_REDUCE_COUNT) return fail(EK_ERR_INVALID, "ek_hip_reduce_blocks(): unknown op %d", op);
    if (int rc = numeric_type_check("ek_hip_reduce_blocks()", type)) return rc;
    if (int rc = blocks_shape_check("ek_hip_reduce_blocks()", n, block)) return rc;
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_reduce_blocks()", elem, out, in)) return rc;
    const BlockPlan p = block_plan(elem, n, block, ctx().num_cu);
    if (p.regime == 0) return ek_hip_memcpy_device(out, in, n * elem);
    if (p.regime == 1) return ek_hip_reduce(op, type, out, in, n);
    return dispatch_numeric(type, [&](auto t) { return reduce_blocks_typed<typename decltype(t)::type>(op, out, in, n, block, p); });
}

int ek_hip_repeat(int type, void *out, const void *in, size_t m, size_t block) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_repeat()", type)) return rc;
    if (block == 0) return fail(EK_ERR_INVALID, "ek_hip_repeat(): blocks of 0 entries");
    if (m == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_repeat()", elem, out, in)) return rc;
    if (block == 1) return ek_hip_memcpy_device(out, in, m * elem);
    return elem == 4 ? repeat_typed<uint32_t>(out, in, m, block) : repeat_typed<uint64_t>(out, in, m, block);
}

}
