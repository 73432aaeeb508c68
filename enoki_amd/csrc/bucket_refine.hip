// The refined stream of a kept bucket partition (ek_refine.h): the elements of every piece once more, in the order of their table
// entries, in groups of four that share an entry, lane-transposed for the forward + adjoint kernel of the headline step
// (bucketed_early.hip: one record read and two 64-bit LDS adds per GROUP instead of per element, no 2-byte index per element).
// Built ONCE per partition, at the first launch of an object that stands on a kept one (bucketed_forward_adjoint_launch), by three
// launches on the consumer's grid and piece cut (bucket_piece):
//   count     LDS histogram of the piece over the bucket's entries -> the piece's tiles
//   offsets   exclusive prefix of the tiles over the pieces (one small workgroup)
//   reorder   the histogram again, scanned in the LDS to group-padded offsets; every element goes through an LDS cursor of its
//             entry to its transposed slot, the first element of a group writes the group's header; pads and tail groups are filled
// No atomics between workgroups: a piece belongs to one workgroup.  The kernels may be slow (they run once); the element order
// inside an entry is whatever the cursor dealt -- the consumer's sums are 64-bit integers, their order cannot matter.
#include "ek_bucketed.h"
#include "ek_refine.h"

namespace ek {

constexpr int kRefineBins = 1 << kRefineEntryBits;

/// calls f(position, local entry) for every element of the piece: complete pages, then the partially filled ones up to their count
template <int PS, typename F>
__device__ __forceinline__ void refine_for_each(const BucketLists &bl, const PieceRange &r, const uint16_t *__restrict__ pair_idx,
                                                uint32_t lmask, F f) {
    constexpr uint32_t Page = 1u << PS, PP = kBucketThreads / Page;      // pages per trip of the workgroup
    const uint32_t g = threadIdx.x / Page, e = threadIdx.x % Page;
    const uint32_t nfull = r.f1 - r.f0, total = nfull + (r.p1 - r.p0);
    for (uint32_t q = g; q < total; q += PP) {
        uint32_t page, count;
        if (q < nfull) { page = bl.glist_full[r.f0 + q]; count = Page; }
        else { const uint32_t ev = bl.glist_part[r.p0 + (q - nfull)]; page = ev >> 6; count = (ev & 63u) + 1u; }
        if (e < count) {
            const size_t pos = ((size_t) page << PS) + e;
            f(pos, (uint32_t) pair_idx[pos] & lmask);
        }
    }
}

/// inclusive prefix of one value per thread over the workgroup (kBucketThreads threads); `total` to everybody
__device__ __forceinline__ uint32_t refine_block_scan(uint32_t v, uint32_t *wave_tot /* [kBucketWaves] shared */, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t) __shfl_up((int) s, d, 64);
        if (lane >= d) s += o;
    }
    __syncthreads();                                   // (wave_tot may still be read from the call before)
    if (lane == 63) wave_tot[wave] = s;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBucketWaves; ++w) { const uint32_t t = wave_tot[w]; before += w < wave ? t : 0u; all += t; }
    total = all;
    return s + before;
}

template <int PS>
__global__ __launch_bounds__(kBucketThreads) void k_bucket_refine_count(uint32_t *__restrict__ tiles, const uint16_t *__restrict__ pair_idx,
                                                                        BucketLists bl, int shift) {
    __shared__ uint32_t hist[kRefineBins];
    __shared__ uint32_t wave_tot[kBucketWaves];
    int bucket;
    PieceRange range;
    if (!bucket_piece<PS>(bl, bucket, range)) {
        if (threadIdx.x == 0) tiles[blockIdx.x] = 0u;
        return;
    }
    for (int j = threadIdx.x; j < kRefineBins; j += kBucketThreads) hist[j] = 0u;
    __syncthreads();
    refine_for_each<PS>(bl, range, pair_idx, (1u << shift) - 1u, [&](size_t, uint32_t l) { atomicAdd(&hist[l], 1u); });
    __syncthreads();
    uint32_t groups = 0;
    for (int j = threadIdx.x; j < kRefineBins; j += kBucketThreads) groups += refine_groups_of(hist[j]);
    uint32_t total;
    (void) refine_block_scan(groups, wave_tot, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = refine_tiles_of(total);
}

/// tiles[0 .. pieces) -> their exclusive prefix in place, tiles[pieces] = the sum
__global__ __launch_bounds__(kBucketThreads) void k_bucket_refine_offsets(uint32_t *__restrict__ tiles, unsigned pieces) {
    __shared__ uint32_t wave_tot[kBucketWaves];
    const unsigned per = (pieces + kBucketThreads - 1) / kBucketThreads, p0 = threadIdx.x * per, p1 = p0 + per < pieces ? p0 + per : pieces;
    uint32_t sum = 0;
    for (unsigned p = p0; p < p1; ++p) sum += tiles[p];
    uint32_t total;
    uint32_t run = refine_block_scan(sum, wave_tot, total) - sum;
    for (unsigned p = p0; p < p1; ++p) { const uint32_t t = tiles[p]; tiles[p] = run; run += t; }
    if (threadIdx.x == 0) tiles[pieces] = total;
}

template <int PS>
__global__ __launch_bounds__(kBucketThreads) void k_bucket_refine_reorder(float *__restrict__ xr, uint16_t *__restrict__ hdr,
                                                                          const uint32_t *__restrict__ tiles, uint32_t cap_tiles,
                                                                          const uint16_t *__restrict__ pair_idx, const float *__restrict__ x_b,
                                                                          BucketLists bl, int shift) {
    __shared__ uint32_t hist[kRefineBins], goff[kRefineBins], cursor[kRefineBins];
    __shared__ uint32_t wave_tot[kBucketWaves];
    int bucket;
    PieceRange range;
    if (!bucket_piece<PS>(bl, bucket, range)) return;
    const uint32_t t0 = tiles[blockIdx.x], t1 = tiles[blockIdx.x + 1];
    // (the host's bound covers every partition -- tests/cpp/partition_refine_host.cpp; nothing is written beyond the storage even so)
    const uint64_t slot0 = (uint64_t) t0 * kRefineTileGroups, cap = (uint64_t) cap_tiles * kRefineTileGroups;
    const uint32_t lmask = (1u << shift) - 1u;
    for (int j = threadIdx.x; j < kRefineBins; j += kBucketThreads) { hist[j] = 0u; cursor[j] = 0u; }
    __syncthreads();
    refine_for_each<PS>(bl, range, pair_idx, lmask, [&](size_t, uint32_t l) { atomicAdd(&hist[l], 1u); });
    __syncthreads();
    // thread t owns entries 4 t .. 4 t + 3: their group counts, the exclusive prefix over the piece
    constexpr int kOwn = kRefineBins / kBucketThreads;
    uint32_t cnt[kOwn], sum = 0;
#pragma unroll
    for (int k = 0; k < kOwn; ++k) { cnt[k] = hist[kOwn * threadIdx.x + k]; sum += refine_groups_of(cnt[k]); }
    uint32_t groups;
    uint32_t run = refine_block_scan(sum, wave_tot, groups) - sum;
    auto x_at = [&](uint64_t j) -> uint64_t { return slot0 + refine_slot(j); };
#pragma unroll
    for (int k = 0; k < kOwn; ++k) {
        goff[kOwn * threadIdx.x + k] = run;
        run += refine_groups_of(cnt[k]);
        // the pad lanes of the entry's last group
        if (cnt[k] & 3u) {
            const uint64_t s = x_at(run - 1u);
            if (s < cap)
                for (uint32_t lane = cnt[k] & 3u; lane < 4u; ++lane) xr[s * 4u + lane] = 0.f;
        }
    }
    __syncthreads();
    refine_for_each<PS>(bl, range, pair_idx, lmask, [&](size_t pos, uint32_t l) {
        const uint32_t rank = atomicAdd(&cursor[l], 1u), count = hist[l];
        const uint64_t s = x_at(goff[l] + rank / 4u);
        if (s < cap) {
            xr[s * 4u + (rank & 3u)] = x_b[pos];
            if ((rank & 3u) == 0u) hdr[s] = refine_header(l, count - rank < 4u ? count - rank : 4u);
        }
    });
    // the tail of the piece's last tile: groups without elements
    const uint64_t end = (uint64_t) (t1 - t0) * kRefineTileGroups;
    for (uint64_t j = groups + threadIdx.x; j < end; j += kBucketThreads) {
        const uint64_t s = x_at(j);
        if (s < cap) {
            hdr[s] = refine_header(0u, 0u);
#pragma unroll
            for (int lane = 0; lane < 4; ++lane) xr[s * 4u + lane] = 0.f;
        }
    }
}

static void refine_log(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void refine_log(const char *fmt, ...) {
    if (ctx().log_level < 2) return;
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "enoki-hip: [partition cache] refined stream: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
}

int partition_refine(BucketPartition *p) {
    if (!p || p->refine_state != 0) return EK_OK;
    Context &c = ctx();
    p->refine_state = -1;                                       // decided once per partition, whatever the answer
    const int mode = c.tuning.partition_refine;
    if (mode == 0) { refine_log("skipped (partition_refine = 0)"); return EK_OK; }
    if (p->type != EK_F32 || !p->page_shift || p->shift > (int) kRefineEntryBits || p->evicted) { refine_log("skipped (shape not covered)"); return EK_OK; }
    // the stream pays when it is smaller than the pages: 18 (d / 4 + 0.375) B per entry against 6 d at d lookups per entry -- from
    // d = 4.5 on.  Measured (profiles/probe_partition_refine_r14.txt): the step -10 % at d = 8 and 16, -15 % at 64; at d = 4 it is no
    // slower (-3 %), which does not pay for twice the pinned bytes
    if (mode == 1 && p->n < (size_t) 8 * p->table_size) {
        refine_log("skipped (%zu lookups into %zu entries: fewer than 8 per entry)", p->n, p->table_size);
        return EK_OK;
    }
    const uint64_t cap_tiles = refine_tiles_bound(p->n, p->max_pieces, (uint64_t) 1 << p->shift);
    if (cap_tiles >= ((uint64_t) 1 << 32) / kRefineTileGroups) { refine_log("skipped (too large)"); return EK_OK; }
    const size_t xb = (size_t) refine_x_bytes(cap_tiles), hb = ((size_t) refine_header_bytes(cap_tiles) + 15u) & ~(size_t) 15u;
    const size_t bytes = xb + hb + ((size_t) p->max_pieces + 1u) * sizeof(uint32_t);
    void *mem = nullptr;
    if (ek_hip_malloc(bytes, &mem) != EK_OK || !mem) { refine_log("skipped (no memory for %zu bytes)", bytes); return EK_OK; }
    float *xr = (float *) mem;
    uint16_t *hdr = (uint16_t *) ((char *) mem + xb);
    uint32_t *tiles = (uint32_t *) ((char *) mem + xb + hb);
    const BucketLists bl{ p->bucket_base, p->piece_prefix, p->base_part, p->glist_full, p->glist_part, p->n_buckets };
    const uint16_t *pair_idx = (const uint16_t *) p->pair_idx;
    const float *x_b = (const float *) p->x_b;
    auto launch = [&](auto ps) -> int {
        constexpr int PS = decltype(ps)::value;
        hipLaunchKernelGGL(k_bucket_refine_count<PS>, dim3(p->max_pieces), dim3(kBucketThreads), 0, c.stream, tiles, pair_idx, bl, p->shift);
        EK_LAUNCH_CHECK("bucket_refine", p->n, p->n * sizeof(uint16_t));
        hipLaunchKernelGGL(k_bucket_refine_offsets, dim3(1), dim3(kBucketThreads), 0, c.stream, tiles, p->max_pieces);
        EK_LAUNCH_CHECK("bucket_refine", (size_t) p->max_pieces, (size_t) p->max_pieces * 2 * sizeof(uint32_t));
        hipLaunchKernelGGL(k_bucket_refine_reorder<PS>, dim3(p->max_pieces), dim3(kBucketThreads), 0, c.stream, xr, hdr, tiles, (uint32_t) cap_tiles,
                           pair_idx, x_b, bl, p->shift);
        EK_LAUNCH_CHECK("bucket_refine", p->n, p->n * (2 * sizeof(uint16_t) + 2 * sizeof(float)) + p->n / 2);
        return EK_OK;
    };
    const int rc = p->page_shift == 6 ? launch(std::integral_constant<int, 6>{}) : launch(std::integral_constant<int, 5>{});
    if (rc != EK_OK) { ek_hip_free(mem); return rc; }
    p->refined = mem; p->refined_x = xr; p->refined_hdr = hdr; p->refined_tiles = tiles;
    p->refined_cap_tiles = (uint32_t) cap_tiles; p->refined_bytes = bytes;
    p->refine_state = 1;
    refine_log("built (%zu lookups, %d buckets of %d entries, up to %u pieces, R = %u, %zu bytes)", p->n, p->n_buckets, 1 << p->shift,
               p->max_pieces, kRefineR, bytes);
    return EK_OK;
}

} // namespace ek
