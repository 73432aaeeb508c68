// Stable sort of a WHOLE array: with p the permutation that puts the n entries of `in` in order,
//     out_index[k]  = p[k]          (the position of the entry that lands at slot k: ready for a gather from another array)
//     out_values[k] = in[p[k]]      (the entry's own bits, fetched through the sorted position)
// -- the call that makes the hits of a ray, the fragments of a pixel or the particles of a cell consecutive, which every block_* and
// segment_* call presumes.  Order, ties, -0.0 and NaN are those of ek_sort.h: numpy.argsort(x, kind="stable"), descending
// argsort(-x) / argsort(~x); bit for bit what ek_hip_sort_blocks(x, block = n) returns.
//
// radix_plan() picks the route (ek_hip_sort_plan reports it):
//   0 trivial    n <= 1.
//   1 forwarded  to ek_hip_sort_blocks with block == n: one bitonic launch up to a chunk, chunks and log2 merges beyond it.
//   2 radix      least-significant-digit radix sort of (key, position) pairs, 8 bits per pass: 4 passes for 4-byte types, 8 for 8-byte
//                types, whatever the keys hold (a pass whose digit is the same everywhere is not skipped: the host would have to
//                read something back to know).  The tuning "sort_radix" decides between 1 and 2: 0 never radix, 1 by the measured
//                crossover (kRadixAuto4 / kRadixAuto8 entries), 2 radix from n = 2 on.
//
// THE RADIX ROUTE.  The array is cut into tiles of `tile` entries (8192 for 4-byte types, 4096 for 8-byte types), workgroup w owns
// the consecutive tiles [w * tiles_per_workgroup, ..), and at most 2 x #CU workgroups run: all of them resident at once.  A pass is
// four launches and no kernel waits for another workgroup -- no look-back, no ticket, no global atomics:
//   count    every workgroup counts the 256 digit values of its range in LDS (integer LDS atomics, one per run of equal digits a
//            lane meets) and writes counts[digit][workgroup].
//   2 scans  k_bin_scan_rows turns every digit's row into its exclusive prefix over the workgroups, k_bin_scan_buckets the 256 row
//            totals into the digits' first slots (ek_binned.h: the scans of scatter_add's partition).
//   scatter  every workgroup walks its tiles in order.  A tile is laid out so that (wave, item, lane) order is element order; the
//            lanes of a wave that hold the same digit find each other with 8 ballots, the first of them bumps the wave's own counter
//            of that digit in LDS, and the lane's rank is that counter plus the number of peers in front of it: a stable rank
//            without an atomic.  An exclusive prefix over the 8 waves and over the digits gives every entry its slot in the tile
//            sorted by digit, the pairs are staged there in LDS, and leave in slot order, so the stores of a digit are consecutive.
//            The workgroup's cursor of every digit then moves on by the tile's count.
// Pass 0 reads `in`: the key is sort_key() of the entry's bits and the position is the element number -- no arange buffer.  Middle
// passes move (key, position) between two scratch buffers.  The last pass writes the caller's outputs instead: out_index the
// position, out_values in[position] -- fetched, never rebuilt from the key (the key of every NaN is all ones).  The order is total
// on (key, position), so the result is a function of the input alone.  Every store lands below n: count and scatter derive the
// digit from the same words with the same ranges, so the cursors partition [0, n); positions are element numbers < n.
// LDS: 8 KiB of wave counters, 4 KiB of digit tables, the staged keys and positions: 76 KiB for 4-byte types, 60 KiB for 8-byte
// types -- two workgroups of 512 lanes per CU either way (DESIGN section 3 says why the 8-byte tile is halved, not kept).
// Scratch (ek_hip_malloc, freed stream-ordered): two buffers of n keys, two of n positions, 256 x workgroups + 513 counters.
// The launch sequence is fixed by (type, n, #CU, tuning): the call can be captured and replayed with other contents.
#include "ek_sort.h"
#include "ek_binned.h"

namespace ek {

constexpr uint32_t kRadixThreads = 512, kRadixWaves = kRadixThreads / 64, kRadixDigits = 256;
template <int ES> constexpr uint32_t kRadixPer = ES == 4 ? 16 : 8;                 // entries per lane and tile
template <int ES> constexpr uint32_t kRadixTile = kRadixThreads * kRadixPer<ES>;   // 8192 / 4096 entries
constexpr size_t kRadixGroupsPerCu = 2;
constexpr size_t kRadixMaxEntries = 0xFFFFFFFFull;
// the automatic crossover (tuning "sort_radix" = 1): the smallest measured n from which the radix route is faster than the forwarded
// one at that and every larger measured n (profiles/probe_sort_r22.txt); never below block_sort's chunk + 1
constexpr size_t kRadixAuto4 = 65536, kRadixAuto8 = 262144;
static_assert(kRadixAuto4 >= 8193 && kRadixAuto8 >= 4097, "a one-launch sort stays one launch");

struct RadixPlan {
    int route, passes, launches;
    size_t tile, per_workgroup, workgroups, key_bytes, pos_bytes, count_words, scratch_bytes;
};

static int radix_plan(int type, size_t n, int num_cu, int mode, RadixPlan &p) {
    const size_t elem = type_size(type);
    p = RadixPlan{ 0, 0, 0, elem == 4 ? kRadixTile<4> : kRadixTile<8>, 0, 0, 0, 0, 0, 0 };
    if (n <= 1) return EK_OK;
    const bool radix = mode == 2 || (mode == 1 && n >= (elem == 4 ? kRadixAuto4 : kRadixAuto8));
    if (!radix) {
        int route = 0, merge_passes = 0;
        size_t chunk = 0, workgroups = 0;
        if (int rc = ek_hip_sort_blocks_plan(type, n, n, 1, num_cu, &route, nullptr, &chunk, &merge_passes, &workgroups)) return rc;
        p.route = 1;
        p.launches = 1 + merge_passes;
        p.workgroups = workgroups;
        p.tile = chunk;
        if (route == 3) p.scratch_bytes = (n * comp_bytes((int) elem) + 15) / 16 * 16 * (merge_passes > 1 ? 2 : 1);
        return EK_OK;
    }
    const size_t cu = num_cu > 0 ? (size_t) num_cu : 256, tiles = (n + p.tile - 1) / p.tile, cap = std::min(tiles, cu * kRadixGroupsPerCu);
    p.route = 2;
    p.passes = (int) elem;
    p.per_workgroup = (tiles + cap - 1) / cap;
    p.workgroups = (tiles + p.per_workgroup - 1) / p.per_workgroup;
    p.launches = 4 * p.passes;
    p.key_bytes = (n * elem + 15) / 16 * 16;
    p.pos_bytes = (n * 4 + 15) / 16 * 16;
    p.count_words = kRadixDigits * p.workgroups + 2 * kRadixDigits + 1;
    p.scratch_bytes = 2 * p.key_bytes + 2 * p.pos_bytes + p.count_words * sizeof(uint32_t);
    return EK_OK;
}

template <typename U> __device__ __forceinline__ uint32_t radix_digit(U key, int shift) { return (uint32_t) (key >> shift) & (kRadixDigits - 1); }

// ---- count: counts[digit * workgroups + workgroup] over the workgroup's range [blockIdx.x * chunk, ..) --------------------------
template <typename U, int KIND, bool FIRST>
__global__ __launch_bounds__(kRadixThreads) void k_sort_radix_count(uint32_t *__restrict__ counts, const U *__restrict__ keys, size_t n,
                                                                    size_t chunk, int shift, bool desc) {
    constexpr int ES = sizeof(U);
    constexpr uint32_t LOADS = 8;
    __shared__ uint32_t hist[kRadixDigits];
    for (uint32_t b = threadIdx.x; b < kRadixDigits; b += kRadixThreads) hist[b] = 0;
    __syncthreads();
    const size_t begin = (size_t) blockIdx.x * chunk, end = begin + chunk < n ? begin + chunk : n;
    // a lane adds a RUN of equal digits at once: keys whose upper bytes are all alike (ids, small integers) would otherwise send
    // 64 lanes to one LDS word per instruction
    uint32_t run_digit = 0, run = 0;
    for (size_t i0 = begin + threadIdx.x; i0 < end; i0 += (size_t) kRadixThreads * LOADS) {
        U k[LOADS];
#pragma unroll
        for (uint32_t j = 0; j < LOADS; ++j) {
            const size_t i = i0 + (size_t) j * kRadixThreads;
            k[j] = i < end ? keys[i] : U(0);
        }
#pragma unroll
        for (uint32_t j = 0; j < LOADS; ++j) {
            if (i0 + (size_t) j * kRadixThreads < end) {
                const uint32_t d = radix_digit(FIRST ? sort_key<ES, KIND, U>(k[j], desc) : k[j], shift);
                if (d != run_digit) {
                    if (run) atomicAdd(&hist[run_digit], run);
                    run_digit = d;
                    run = 0;
                }
                run++;
            }
        }
    }
    if (run) atomicAdd(&hist[run_digit], run);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kRadixDigits; b += kRadixThreads) counts[(size_t) b * gridDim.x + blockIdx.x] = hist[b];
}

// ---- scatter: MODE 0 first pass (keys from `in`, positions are element numbers), 1 middle, 2 last (the caller's outputs) ---------
// amdgpu_waves_per_eu(4) = 128 registers: two workgroups per CU, which the LDS allows.  The 4-byte middle and last passes spill 7
// and 2 registers under it (32 and 12 B of scratch per lane); left to itself the compiler takes 138 and one workgroup per CU.
template <typename U, int KIND, int MODE>
__global__ __launch_bounds__(kRadixThreads) __attribute__((amdgpu_waves_per_eu(4))) void
k_sort_radix_scatter(U *__restrict__ out_keys, uint32_t *__restrict__ out_pos, U *__restrict__ outv, uint32_t *__restrict__ outi,
                     const U *__restrict__ in_keys, const uint32_t *__restrict__ in_pos, const U *__restrict__ in,
                     const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ bucket_base, size_t n, size_t chunk, int shift,
                     bool desc) {
    constexpr int ES = sizeof(U);
    constexpr uint32_t PER = kRadixPer<ES>, T = kRadixTile<ES>;
    __shared__ uint32_t wave_count[kRadixWaves][kRadixDigits];      // per-wave digit counters, then exclusive over the waves
    __shared__ uint32_t total[kRadixDigits], tile_off[kRadixDigits], cursor[kRadixDigits], to_global[kRadixDigits];
    __shared__ U stage_key[T];
    __shared__ uint32_t stage_pos[T];

    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    for (uint32_t b = threadIdx.x; b < kRadixDigits; b += kRadixThreads) cursor[b] = bucket_base[b] + offsets[(size_t) b * gridDim.x + blockIdx.x];
    const size_t begin = (size_t) blockIdx.x * chunk, end = begin + chunk < n ? begin + chunk : n;

    for (size_t base = begin; base < end; base += T) {
        for (uint32_t b = threadIdx.x; b < kRadixWaves * kRadixDigits; b += kRadixThreads) (&wave_count[0][0])[b] = 0;
        __syncthreads();        // (also: the cursors are set, and the last tile's reads of the staged pairs are done)

        // striped inside the wave: (wave, item, lane) order == element order; entry (j, lane) of the wave is tile entry first + j * 64
        const uint32_t tile_count = (uint32_t) (end - base < T ? end - base : T), first = wave * (T / kRadixWaves) + lane;
        U key[PER];
        uint32_t pos[MODE == 0 ? 1 : PER], rank[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t e = first + j * 64;
            if constexpr (MODE == 0) {
                key[j] = e < tile_count ? sort_key<ES, KIND, U>(in[base + e], desc) : U(0);
            } else {
                key[j] = e < tile_count ? in_keys[base + e] : U(0);
                pos[j] = e < tile_count ? in_pos[base + e] : 0u;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t d = radix_digit(key[j], shift);
            const bool on = first + j * 64 < tile_count;
            unsigned long long peers = __ballot(on);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool set = (d >> bit) & 1u;
                const unsigned long long m = __ballot(on && set);
                peers &= set ? m : ~m;
            }
            const uint32_t below = (uint32_t) __popcll(peers & lt_mask);
            uint32_t old = 0;
            if (on && below == 0) {                       // the first lane of its digit in this item
                volatile uint32_t *slot = &wave_count[wave][d];
                old = *slot;
                *slot = old + (uint32_t) __popcll(peers);
            }
            const int leader = on ? __ffsll((long long) peers) - 1 : (int) lane;
            old = __shfl(old, leader, 64);
            rank[j] = old + below;
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        // per digit: exclusive prefix over the waves, and the tile's total
        if (threadIdx.x < kRadixDigits) {
            uint32_t run = 0;
            for (uint32_t w = 0; w < kRadixWaves; ++w) {
                const uint32_t c = wave_count[w][threadIdx.x];
                wave_count[w][threadIdx.x] = run;
                run += c;
            }
            total[threadIdx.x] = run;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const uint32_t l = threadIdx.x;
            const uint32_t h0 = total[4 * l], h1 = total[4 * l + 1], h2 = total[4 * l + 2], h3 = total[4 * l + 3];
            const uint32_t sum = h0 + h1 + h2 + h3;
            uint32_t incl = sum;
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint32_t up = __shfl_up(incl, dd, 64);
                if (l >= (uint32_t) dd) incl += up;
            }
            uint32_t o = incl - sum;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                tile_off[4 * l + q] = o;
                to_global[4 * l + q] = cursor[4 * l + q] - o;     // slot s of the sorted tile goes to s + to_global[digit] (mod 2^32)
                o += q == 0 ? h0 : q == 1 ? h1 : q == 2 ? h2 : h3;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            if (first + j * 64 < tile_count) {
                const uint32_t d = radix_digit(key[j], shift), s = tile_off[d] + wave_count[wave][d] + rank[j];     // s < tile_count
                stage_key[s] = key[j];
                stage_pos[s] = MODE == 0 ? (uint32_t) base + first + j * 64 : pos[MODE == 0 ? 0 : j];
            }
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < tile_count; s += kRadixThreads) {
            const U k = stage_key[s];
            const uint32_t ps = stage_pos[s], g = s + to_global[radix_digit(k, shift)];                              // g < n
            if constexpr (MODE == 2) {
                if (outi) outi[g] = ps;
                if (outv) outv[g] = in[ps];
            } else {
                out_keys[g] = k;
                out_pos[g] = ps;
            }
        }
        if (threadIdx.x < kRadixDigits) cursor[threadIdx.x] += total[threadIdx.x];
        // (the barrier at the top of the next tile comes before anybody writes wave_count, and two more before the staged pairs,
        //  `total` and the tables are written again)
    }
}

template <typename U, int KIND>
static int sort_radix_typed(void *outv_, uint32_t *outi, const void *in_, size_t n, const RadixPlan &p, int flags) {
    RoctxRange range("enoki-hip: radix sort");
    constexpr int ES = sizeof(U);
    Context &c = ctx();
    U *outv = (U *) outv_;
    const U *in = (const U *) in_;
    const bool desc = flags & EK_SORT_DESCENDING;
    void *scratch = nullptr;
    if (int rc = ek_hip_malloc(p.scratch_bytes, &scratch)) return rc;
    unsigned char *s = (unsigned char *) scratch;
    U *kbuf[2] = { (U *) s, (U *) (s + p.key_bytes) };
    uint32_t *pbuf[2] = { (uint32_t *) (s + 2 * p.key_bytes), (uint32_t *) (s + 2 * p.key_bytes + p.pos_bytes) };
    uint32_t *counts = (uint32_t *) (s + 2 * p.key_bytes + 2 * p.pos_bytes), *row_total = counts + kRadixDigits * p.workgroups,
             *bucket_base = row_total + kRadixDigits;
    const unsigned grid = (unsigned) p.workgroups;
    const size_t chunk = p.per_workgroup * p.tile, out_bytes = n * ((outv ? 2 * ES : 0) + (outi ? 4 : 0));
    const dim3 threads(kRadixThreads);
    int rc = EK_OK;
    for (int pass = 0; pass < p.passes && rc == EK_OK; ++pass) {
        const int shift = pass * 8;
        const bool first = pass == 0, last = pass + 1 == p.passes;
        const U *src_k = first ? in : kbuf[(pass - 1) & 1];
        const uint32_t *src_p = first ? nullptr : pbuf[(pass - 1) & 1];
        if (first)
            hipLaunchKernelGGL((k_sort_radix_count<U, KIND, true>), dim3(grid), threads, 0, c.stream, counts, src_k, n, chunk, shift, desc);
        else
            hipLaunchKernelGGL((k_sort_radix_count<U, KIND, false>), dim3(grid), threads, 0, c.stream, counts, src_k, n, chunk, shift, desc);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort(): a count launch failed"); break; }
        note_launch("sort_radix_count", n, n * ES);
        hipLaunchKernelGGL(k_bin_scan_rows, dim3(kRadixDigits), dim3(1024), 0, c.stream, counts, row_total, grid);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort(): a scan launch failed"); break; }
        note_launch("sort_radix_scan_rows", kRadixDigits * p.workgroups, 2 * kRadixDigits * p.workgroups * sizeof(uint32_t));
        hipLaunchKernelGGL(k_bin_scan_buckets, dim3(1), dim3(256), 0, c.stream, bucket_base, (uint32_t *) nullptr, (const uint32_t *) row_total,
                           (int) kRadixDigits, 0u);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort(): a scan launch failed"); break; }
        note_launch("sort_radix_scan_digits", kRadixDigits, 2 * kRadixDigits * sizeof(uint32_t));
        if (first)
            hipLaunchKernelGGL((k_sort_radix_scatter<U, KIND, 0>), dim3(grid), threads, 0, c.stream, kbuf[0], pbuf[0], (U *) nullptr,
                               (uint32_t *) nullptr, (const U *) nullptr, (const uint32_t *) nullptr, in, (const uint32_t *) counts,
                               (const uint32_t *) bucket_base, n, chunk, shift, desc);
        else if (!last)
            hipLaunchKernelGGL((k_sort_radix_scatter<U, KIND, 1>), dim3(grid), threads, 0, c.stream, kbuf[pass & 1], pbuf[pass & 1], (U *) nullptr,
                               (uint32_t *) nullptr, src_k, src_p, in, (const uint32_t *) counts, (const uint32_t *) bucket_base, n, chunk, shift,
                               desc);
        else
            hipLaunchKernelGGL((k_sort_radix_scatter<U, KIND, 2>), dim3(grid), threads, 0, c.stream, (U *) nullptr, (uint32_t *) nullptr, outv, outi,
                               src_k, src_p, in, (const uint32_t *) counts, (const uint32_t *) bucket_base, n, chunk, shift, desc);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort(): a scatter launch failed"); break; }
        note_launch("sort_radix_scatter", n, first ? n * (2 * ES + 4) : last ? n * (ES + 4) + out_bytes : 2 * n * (ES + 4));
    }
    ek_hip_free(scratch);   // stream-ordered reuse
    return rc;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_sort_plan(int type, size_t n, int want_index, int compute_units, int *route, int *passes, size_t *tile, size_t *tiles_per_workgroup,
                     size_t *workgroups, int *launches, size_t *scratch_bytes) {
    (void) want_index;          // the position travels with the key either way: it changes neither route nor scratch
    if (int rc = numeric_type_check("ek_hip_sort_plan()", type)) return rc;
    if (n > kRadixMaxEntries) return fail(EK_ERR_UNSUPPORTED, "ek_hip_sort_plan(): %zu entries, more than 2^32 - 1", n);
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_sort_plan(): %d compute units", compute_units);
    RadixPlan p;
    if (int rc = radix_plan(type, n, compute_units, ctx().tuning.sort_radix, p)) return rc;
    if (route) *route = p.route;
    if (passes) *passes = p.passes;
    if (tile) *tile = p.tile;
    if (tiles_per_workgroup) *tiles_per_workgroup = p.per_workgroup;
    if (workgroups) *workgroups = p.workgroups;
    if (launches) *launches = p.launches;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return EK_OK;
}

int ek_hip_sort(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, int flags) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_sort()", type)) return rc;
    if (flags & ~(EK_SORT_DESCENDING | EK_SORT_FLAT_INDEX)) return fail(EK_ERR_INVALID, "ek_hip_sort(): unknown flags %d", flags);
    if (n > kRadixMaxEntries) return fail(EK_ERR_UNSUPPORTED, "ek_hip_sort(): %zu entries, more than 2^32 - 1", n);
    if (!out_values && !out_index) return fail(EK_ERR_INVALID, "ek_hip_sort(): no output");
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_sort()", elem, in)) return rc;
    // (an output that was not asked for is a null pointer: aligned)
    if (int rc = alignment_check("ek_hip_sort()", elem, out_values)) return rc;
    if (int rc = alignment_check("ek_hip_sort()", 4, out_index)) return rc;
    if (sort_overlap(in, n * elem, out_values, n * elem) || sort_overlap(in, n * elem, out_index, n * 4) ||
        sort_overlap(out_values, n * elem, out_index, n * 4))
        return fail(EK_ERR_INVALID, "ek_hip_sort(): in and the outputs overlap");
    RadixPlan p;
    if (int rc = radix_plan(type, n, ctx().num_cu, ctx().tuning.sort_radix, p)) return rc;
    // (one row of n entries: its row-local positions are the flat ones)
    if (p.route != 2) return ek_hip_sort_blocks(type, out_values, out_index, in, n, n, flags & EK_SORT_DESCENDING);
    switch (type) {
        case EK_I32: return sort_radix_typed<uint32_t, kSortSigned>(out_values, out_index, in, n, p, flags);
        case EK_U32: return sort_radix_typed<uint32_t, kSortUnsigned>(out_values, out_index, in, n, p, flags);
        case EK_I64: return sort_radix_typed<uint64_t, kSortSigned>(out_values, out_index, in, n, p, flags);
        case EK_U64: return sort_radix_typed<uint64_t, kSortUnsigned>(out_values, out_index, in, n, p, flags);
        case EK_F32: return sort_radix_typed<uint32_t, kSortFloat>(out_values, out_index, in, n, p, flags);
        default: return sort_radix_typed<uint64_t, kSortFloat>(out_values, out_index, in, n, p, flags);
    }
}

}
