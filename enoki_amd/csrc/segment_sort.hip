// Stable sort inside ragged segments: for the m segments [lo_j, hi_j) of a flat array of n entries that a device array of start
// positions gives (starts[m] := n; segment_clamp in ek_block.h),
//     perm[lo_j + k] = the segment-local position of the entry of segment j that comes k-th in the order  (+ lo_j with EK_SORT_FLAT_INDEX)
//     vals[lo_j + k] = in[lo_j + perm]                                                                       (the entry's own bits)
// and the entries in front of min(starts[0], n), which belong to no segment, stay where they are (their position is i in both
// modes).  The counterpart of block_sort.hip for what compress() leaves behind; order, ties, -0.0, NaN and the composites are the
// ones of ek_sort.h: per segment numpy.argsort(segment, kind="stable"), argsort(-segment) / argsort(~segment) descending.
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP, nothing is read back, there are no global atomics, and the host knows only n and m: the
// launch sequence is fixed by (type, n, m, #CU), so a captured call replays with other contents in `starts`.
//
// ONE route, output-driven, so that the work is balanced whatever `starts` holds.  segsort_plan() (ek_hip_sort_segments_plan):
//     tile                = 2048 consecutive entries: tile t is the entries [t * tile, min((t + 1) * tile, n))
//     tiles               = ceil(n / tile)
//     tiles_per_workgroup = ceil(tiles / min(tiles, 8 x #CU))          a workgroup owns a RANGE of consecutive tiles
//     workgroups          = ceil(tiles / tiles_per_workgroup)
//     merges              = ceil(log2(tiles))                          the only number of merge launches the host can know
//     launches            = 1 for one tile, 2 + merges otherwise; m == 0 is a copy and 0, 1, 2, ..: no kernel of this file
//
// WHO OWNS AN ENTRY is decided by ONE function of (`starts`, a tile boundary x): segsort_at(x) searches the number c of starts
// <= x (bounded, fixed trip count) and tells whether segment c - 1, clamped, holds both entry x - 1 and entry x.  Such a segment
// CROSSES x.  An entry is LONG when the segment that crosses the left or the right boundary of its tile holds it; every other
// entry is SHORT.  The tile launch writes the caller's outputs for short entries, the merge launches for long ones.  Every kernel
// calls the same function on the same words, so for ANY contents of `starts` the kernels agree on every entry.
//
// 1 tiles   Per tile: staged in LDS like k_sort_packed (16-byte non-temporal loads, head / shift / tail).  Heads as in
//           segment_scan.hip: one search in `starts` for the workgroup's first tile, then a stream of starts, 256 at a time, every
//           start inside the tile ORs a flag bit in LDS (idempotent).  A max-scan of the flagged positions gives every entry its
//           RUN: 1 + the tile-local position of the last head at or before it, 0 in front of the tile's first head.  One bitonic
//           network of 66 stages over the 2048 composites ordered by (run, key, tile-local position): 12 + 32 + 11 bits in one 64-bit
//           word for 4-byte types; a 64-bit key plus the word run << 16 | position, the run compared first, for 8-byte types.
//           Padding is all ones.  Entries in front of min(starts[0], n) get key 0: they stay in place.  Slot e of the sorted tile
//           belongs to the run of entry e, so a short slot writes value and position (position - (run - 1), or the flat one; run 0
//           counts from 0), and a long slot writes its composite in block_sort's form, key and FLAT position, to scratch buffer 0.
//           A tile without long entries leaves through the LDS output tiles and tile_out; one with long entries stores from
//           registers.  The tile also writes one word: does a segment cross its left boundary.
// 2 needed  One workgroup folds those words to needed = 1 + max ctz(t) over the crossed boundaries t * tile (0: none).
// 3 merges  Pass p < merges, all launched; every workgroup of pass p reads `needed` and returns at once when p >= needed, so a
//           pass that the data do not need costs no array traffic.  A workgroup owns a fixed tile of 2048 outputs inside the pair
//           [a, b) of two groups of 2^p tiles that meet at mid.  Three lanes call segsort_at(a), (mid), (b).  The segment M that
//           crosses mid is the only one this pass merges: its pieces [max(lo, a), mid) and [mid, min(hi, b)) are sorted runs in
//           buffer p & 1, and the tile's share is produced as in k_sort_merge (merge path on the two diagonals, the pieces into
//           LDS, rank in the other piece).  M CONTINUES when segsort_at(a) or segsort_at(b) names the same segment; then the
//           composites go to buffer (p + 1) & 1, and the pass whose mid is that boundary finds M again.  Otherwise this is M's last
//           pass and the tile writes values and positions in the caller's layout.  The pieces of a segment that crosses a or b
//           but not mid are COPIED THROUGH to the other buffer (the alternative, deriving a piece's buffer from the highest boundary
//           inside it, lets a pass read and write the same range of one buffer).  So every long piece is in buffer p & 1 when pass
//           p begins.  Everything else in the pair was final earlier and is not touched.
//
// BAD STARTS (above n, equal, decreasing, random).  There is no second code path.  Every read of `starts` lies in [0, m) and
// every loop is bounded by m / 256 + 1, tiles, log2 of a run length or a constant.  Runs need not be sorted then: merge-path cuts
// are clamped to the tile, ranks may collide, so the LDS tile of a merge starts out as padding and every position taken from a
// composite is clamped below n before it indexes `in`.  A long entry is always written: the pass where its crossing boundary is
// mid merges it, and it is either final there or continues over a boundary of a higher pass, the last of which has a = 0 and b = n.
// Only values are unspecified.  Scratch: one or two buffers of n composites, tiles + 1 words; ek_hip_malloc, freed stream-ordered.
#include "ek_sort.h"
#include "ek_search.h"

namespace ek {

constexpr uint32_t kSegSortTile = 2048;
constexpr size_t kSegSortBlocksPerCu = 8;
constexpr size_t kSegSortMaxGrid = 0x7FFFFFFFull;

struct SegSortPlan {
    size_t tile, tiles, per_workgroup, workgroups, merge_workgroups, buf_bytes, scratch_bytes;
    int merges, launches;
};

static SegSortPlan segsort_plan(size_t elem, size_t n, size_t m, int num_cu) {
    SegSortPlan p = { kSegSortTile, 0, 0, 0, 0, 0, 0, 0, 0 };
    if (n == 0 || m == 0) return p;
    const size_t cu = num_cu > 0 ? (size_t) num_cu : 256;
    p.tiles = (n + p.tile - 1) / p.tile;
    const size_t cap = std::min(p.tiles, cu * kSegSortBlocksPerCu);
    p.per_workgroup = (p.tiles + cap - 1) / cap;
    p.workgroups = (p.tiles + p.per_workgroup - 1) / p.per_workgroup;
    while (((size_t) 1 << p.merges) < p.tiles) p.merges++;
    p.launches = 1;
    if (p.merges) {
        p.launches = 2 + p.merges;
        p.merge_workgroups = std::min(p.tiles, kSegSortMaxGrid);
        p.buf_bytes = (n * comp_bytes((int) elem) + 15) / 16 * 16;
        p.scratch_bytes = p.buf_bytes * (p.merges > 1 ? 2 : 1) + (p.tiles + 1) * sizeof(uint32_t);
    }
    return p;
}

/// the segment that crosses boundary x, 0 < x < n: `found` when segment c - 1 (c: the number of starts <= x) holds entries x - 1 and x
struct SegAt { uint32_t found, c, lo, hi; };

__device__ __forceinline__ SegAt segsort_at(const uint32_t *starts, uint32_t m, uint32_t top, uint32_t n, uint32_t x) {
    const uint32_t at[1] = { x }, zero[1] = { 0 }, all[1] = { m };
    uint32_t pos[1] = { 0 };
    search_steps<uint32_t, true, 1>(starts, zero, zero, all, m - 1, top, at, pos);
    SegAt s = { 0, pos[0], 0, 0 };                                                                // c <= m
    if (s.c) {
        segment_clamp(starts[s.c - 1], s.c < m ? starts[s.c] : n, n, s.lo, s.hi);
        s.found = s.lo < x && x < s.hi;
    }
    return s;
}

// ---- the tile's composites: (run, key, tile-local position) ---------------------------------------------------------------------
__device__ __forceinline__ SortComp<4> segcomp_make(uint32_t run, const SortComp<4> &k, uint32_t e, bool keyless) {
    return SortComp<4>{ ((uint64_t) run << 43) | (keyless ? 0ull : (k.w >> 32) << 11) | e };
}
__device__ __forceinline__ SortComp<8> segcomp_make(uint32_t run, const SortComp<8> &k, uint32_t e, bool keyless) {
    return SortComp<8>{ keyless ? 0ull : k.key, (run << 16) | e };
}
__device__ __forceinline__ uint32_t segcomp_run(const SortComp<4> &c) { return (uint32_t) (c.w >> 43); }
__device__ __forceinline__ uint32_t segcomp_run(const SortComp<8> &c) { return c.pos >> 16; }
__device__ __forceinline__ uint32_t segcomp_pos(const SortComp<4> &c) { return (uint32_t) c.w & 0x7FFu; }
__device__ __forceinline__ uint32_t segcomp_pos(const SortComp<8> &c) { return c.pos & 0xFFFFu; }
/// block_sort's form: the key and the flat position
__device__ __forceinline__ SortComp<4> segcomp_flat(const SortComp<4> &c, uint32_t flat) {
    return SortComp<4>{ ((c.w >> 11) << 32) | flat };
}
__device__ __forceinline__ SortComp<8> segcomp_flat(const SortComp<8> &c, uint32_t flat) { return SortComp<8>{ c.key, flat }; }

/// the network of sort_bitonic over all C slots; 8-byte types compare the run in front of the key
template <int ES> __device__ __forceinline__ void segsort_network(const CompStore<ES> &s) {
    constexpr uint32_t C = kSegSortTile;
    if constexpr (ES == 4) {
        sort_bitonic<4>(s, C, C);
    } else {
        for (uint32_t k = 2; k <= C; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = threadIdx.x; t < C / 2; t += 256) {
                    const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const bool up = (lo & k) == 0;
                    const SortComp<8> x = s.get(lo), y = s.get(hi);
                    const uint32_t rx = x.pos >> 16, ry = y.pos >> 16;
                    const bool less = ry < rx || (ry == rx && comp_less(y, x));
                    if (less == up) { s.set(lo, y); s.set(hi, x); }
                }
                __syncthreads();
            }
        }
    }
}

// ---- launch 1: the tiles ------------------------------------------------------------------------------------------------------
template <typename U, int KIND>
__global__ __launch_bounds__(256) void k_sort_segments_tiles(U *outv_, uint32_t *outi_, CompStore<sizeof(U)> scratch, uint32_t *edge, const U *in,
                                                             uint32_t n, const uint32_t *starts, uint32_t m, uint32_t top, uint32_t tiles,
                                                             uint32_t per_workgroup, int flags_) {
    constexpr int ES = sizeof(U);
    constexpr uint32_t N = 16 / ES, C = kSegSortTile, PER = C / 256;
    __shared__ __attribute__((aligned(16))) U tile_in[C + N];
    // C composites; afterwards the value tile (C + N entries) and, from the next 16-byte boundary, the index tile (C + 4 entries)
    __shared__ __attribute__((aligned(16))) unsigned char area[C * (ES + 4) + 32];
    __shared__ __attribute__((aligned(16))) uint16_t s_run[C];
    __shared__ uint32_t s_flag[256];                      // bit i of word l: entry l * PER + i of the tile is a head
    __shared__ uint32_t s_wave[4];
    __shared__ SegAt s_edge[2];
    const CompStore<ES> comps = comp_store<ES>(area, C);
    U *const tile_v = reinterpret_cast<U *>(area);
    uint32_t *const tile_i = reinterpret_cast<uint32_t *>(area + (C + N) * ES);
    const uint32_t t0 = blockIdx.x * per_workgroup, t1 = tiles - t0 < per_workgroup ? tiles : t0 + per_workgroup;
    const uint32_t s0 = starts[0], first = s0 < n ? s0 : n;                                       // (m >= 1)
    uint32_t j = 0;                                       // the number of starts in front of the tile
    bool known = false;
    for (uint32_t t = t0; t < t1; ++t) {
        // the lane number, the output pointers and the flags are taken anew for every tile: hoisted out of this loop, the two dozen
        // predicates below (tid < head, lane >= d, outv != null, ..) are 64-bit masks that live in scalar registers across the
        // whole network and spill
        uint32_t tid = threadIdx.x;
        U *outv = outv_;
        uint32_t *outi = outi_;
        int flags = flags_;
        asm volatile("" : "+v"(tid), "+s"(outv), "+s"(outi), "+s"(flags));
        const bool desc = flags & EK_SORT_DESCENDING, flat = flags & EK_SORT_FLAT_INDEX;
        const uint32_t lane = tid & 63, wave = tid >> 6;
        const uint32_t base = t * C, len = n - base < C ? n - base : C;
        s_flag[tid] = 0;
        if ((tid & 63) == 0 && wave < 2) {                // the tile's two boundaries, one lane of two waves each
            const uint32_t x = wave ? base + len : base;
            s_edge[wave] = x > 0 && x < n ? segsort_at(starts, m, top, n, x) : SegAt{ 0, 0, 0, 0 };
        }
        // ---- stage: entry e of the tile lives at tile_in[shift + e], the first whole vector on a 16-byte boundary of LDS
        const U *src = in + base;
        uint32_t head = head_of(src);
        if (head > len) head = len;
        const uint32_t shift = (N - head) % N, nvec = (len - head) / N, tail = len - head - nvec * N;
        U *ti = tile_in + shift;
        if (tid < head) ti[tid] = src[tid];
#pragma unroll 4
        for (uint32_t v = tid; v < nvec; v += 256)
            *reinterpret_cast<Pack<U, N> *>(ti + head + v * N) = pack_load<U, N, true>(src + head + v * N);
        if (tid < tail) ti[head + nvec * N + tid] = src[head + nvec * N + tid];
        __syncthreads();       // (the flag words are clear, the edges known; the last tile's stores out of `area` are done)
        // ---- heads
        if (!known) {
            uint32_t pos[1] = { 0 };
            const uint32_t at[1] = { base }, zero[1] = { 0 }, all[1] = { m };
            search_steps<uint32_t, false, 1>(starts, zero, zero, all, m - 1, top, at, pos);       // starts < base
            j = pos[0];                                                                           // <= m
            known = true;
        }
        {
            const uint32_t j0 = j, room = m - j0;                                                 // starts left to walk
            for (uint64_t cnt = 0;; cnt += 256) {
                const uint64_t k = cnt + tid;
                const bool valid = k < room;
                uint32_t s = valid ? starts[j0 + (uint32_t) k] : 0u;
                if (s > n) s = n;
                const bool used = valid && s < base + len;                                        // in or before the tile
                if (used && s >= base) atomicOr(&s_flag[(s - base) / PER], 1u << ((s - base) % PER));
                const uint32_t c = (uint32_t) __syncthreads_count(used);
                j += c;
                if (c < 256) break;                       // a start behind the tile, or no start left
            }
        }
        // ---- runs: 1 + the position of the last head at or before the entry, by a max-scan over the lanes
        {
            const uint32_t fw = s_flag[tid];
            uint32_t v = fw ? tid * PER + (31 - __clz(fw)) + 1 : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = __shfl_up(v, d, 64);
                if (lane >= (uint32_t) d && u > v) v = u;
            }
            uint32_t run = __shfl_up(v, 1, 64);
            if (lane == 0) run = 0;
            if (lane == 63) s_wave[wave] = v;
            __syncthreads();
            for (uint32_t w = 0; w < wave; ++w) run = s_wave[w] > run ? s_wave[w] : run;
            Pack<uint16_t, PER> r;
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) {
                if ((fw >> i) & 1u) run = tid * PER + i + 1;
                r.v[i] = (uint16_t) run;
            }
            *reinterpret_cast<Pack<uint16_t, PER> *>(s_run + tid * PER) = r;
        }
        __syncthreads();
        for (uint32_t e = tid; e < C; e += 256)
            comps.set(e, e < len ? segcomp_make(s_run[e], comp_make<ES, KIND, U>(ti[e], 0, desc), e, base + e < first) : comp_padding<ES>());
        __syncthreads();
        segsort_network<ES>(comps);
        const SegAt L = s_edge[0], R = s_edge[1];          // (written again only behind the barriers below)
        // every lane takes its results into registers: `area` becomes the output tiles
        U val[PER];
        uint32_t idx[PER];
        SortComp<ES> far[PER];
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t e = i * 256 + tid;
            if (e < len) {
                const SortComp<ES> c = comps.get(e);
                const uint32_t pos = segcomp_pos(c), run = segcomp_run(c);                        // pos < len: a real composite
                val[i] = ti[pos];
                idx[i] = flat || run == 0 ? base + pos : pos - (run - 1);
                far[i] = segcomp_flat(c, base + pos);
            }
        }
        if (edge && tid == 0) edge[t] = L.found;
        if (L.found || R.found) {
            // a tile with long entries: those leave as composites, the short ones element by element
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) {
                const uint32_t e = i * 256 + tid, g = base + e;
                if (e < len) {
                    if ((L.found && g < L.hi) || (R.found && g >= R.lo)) {
                        scratch.set(g, far[i]);
                    } else {
                        if (outv) outv[g] = val[i];
                        if (outi) outi[g] = idx[i];
                    }
                }
            }
            __syncthreads();   // (the next tile writes tile_in)
            continue;
        }
        __syncthreads();
        uint32_t vhead = 0, ihead = 0;
        if (outv) {
            vhead = head_of(outv + base);
            if (vhead > len) vhead = len;
        }
        if (outi) {
            ihead = head_of(outi + base);
            if (ihead > len) ihead = len;
        }
        U *tv = tile_v + (N - vhead) % N;
        uint32_t *tx = tile_i + (4 - ihead) % 4;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t e = i * 256 + tid;
            if (e < len) {
                if (outv) tv[e] = val[i];
                if (outi) tx[e] = idx[i];
            }
        }
        __syncthreads();
        if (outv) tile_out<U>(outv + base, tv, len, vhead);
        if (outi) tile_out<uint32_t>(outi + base, tx, len, ihead);
    }
}

// ---- launch 2: how many merge passes the data need ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sort_segments_needed(uint32_t *needed, const uint32_t *__restrict__ edge, uint32_t tiles) {
    __shared__ uint32_t s_wave[4];
    uint32_t v = 0;
    for (uint32_t t = 1 + threadIdx.x; t < tiles; t += 256)
        if (edge[t]) v = max(v, (uint32_t) __builtin_ctz(t) + 1u);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t) __shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *needed = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));
}

// ---- launches 3 ..: pass p merges the segment that crosses the middle of every pair of groups of 2^p tiles ---------------------
template <typename U>
__global__ __launch_bounds__(256) void k_sort_segments_merge(U *outv, uint32_t *outi, CompStore<sizeof(U)> dst, CompStore<sizeof(U)> src,
                                                             const U *in, uint32_t n, const uint32_t *starts, uint32_t m, uint32_t top,
                                                             uint32_t tiles, uint32_t pass, const uint32_t *__restrict__ needed, int flags) {
    constexpr int ES = sizeof(U);
    constexpr uint32_t TM = kSegSortTile;
    if (pass >= *needed) return;
    __shared__ __attribute__((aligned(16))) unsigned char lds_in[TM * comp_bytes(ES)];
    __shared__ __attribute__((aligned(16))) unsigned char lds_out[TM * comp_bytes(ES)];
    __shared__ uint32_t s_cut[2];
    __shared__ SegAt s_seg[3];
    const CompStore<ES> pieces = comp_store<ES>(lds_in, TM), merged = comp_store<ES>(lds_out, TM);
    const bool flat = flags & EK_SORT_FLAT_INDEX;
    const uint32_t tid = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t o0 = t * TM, o1 = n - o0 < TM ? n : o0 + TM;                               // the tile's outputs
        const uint32_t a = (t >> (pass + 1) << (pass + 1)) * TM;                                  // <= o0
        const uint64_t mid64 = (uint64_t) a + ((uint64_t) TM << pass), b64 = (uint64_t) a + ((uint64_t) TM << (pass + 1));
        const uint32_t mid = mid64 < n ? (uint32_t) mid64 : n, b = b64 < n ? (uint32_t) b64 : n;  // a < mid <= b <= n
        __syncthreads();       // (everybody has the last tile's segments in registers and has left its LDS tiles)
        if ((tid & 63) == 0 && tid < 192) {               // the pair's three boundaries, one lane of three waves each
            const uint32_t x = tid == 0 ? a : tid == 64 ? mid : b;
            s_seg[tid >> 6] = x > 0 && x < n ? segsort_at(starts, m, top, n, x) : SegAt{ 0, 0, 0, 0 };
        }
        __syncthreads();
        const SegAt A = s_seg[0], M = s_seg[1], B = s_seg[2];
        const bool cont_l = M.found && A.found && A.c == M.c, cont_r = M.found && B.found && B.c == M.c;
        // the merged range [r0, r1) (r0 < mid < r1) and the ranges [a, cl) and [cr, b) that are copied through
        uint32_t r0 = mid, r1 = mid, cl = a, cr = b;
        if (M.found) { r0 = M.lo > a ? M.lo : a; r1 = M.hi < b ? M.hi : b; }
        if (A.found && !cont_l) { cl = A.hi < mid ? A.hi : mid; if (cl > r0) cl = r0; }
        if (B.found && !cont_r) { cr = B.lo > mid ? B.lo : mid; if (cr < r1) cr = r1; }
        const uint32_t m0 = o0 > r0 ? o0 : r0, m1 = o1 < r1 ? o1 : r1;                            // the tile's share of the merge
        if (m0 < m1) {
            const uint32_t la = mid - r0, lb = r1 - mid, d0 = m0 - r0, d1 = m1 - r0, cnt = m1 - m0;   // cnt <= TM; d1 <= la + lb
            if (tid == 0) s_cut[0] = sort_merge_path<ES>(src, r0, la, mid, lb, d0);
            if (tid == 64) s_cut[1] = sort_merge_path<ES>(src, r0, la, mid, lb, d1);
            for (uint32_t i = tid; i < cnt; i += 256) merged.set(i, comp_padding<ES>());          // (ranks collide where runs are not sorted)
            __syncthreads();
            // sorted runs: a0 <= a1 <= a0 + cnt.  Anything else is clamped so that both pieces stay inside their runs.
            const uint32_t a0 = s_cut[0], a1 = s_cut[1] > a0 ? s_cut[1] : a0, b0 = d0 - a0;
            const uint32_t na = a1 - a0 < cnt ? a1 - a0 : cnt, nb = cnt - na;
            for (uint32_t i = tid; i < cnt; i += 256)
                pieces.set(i, i < na ? src.get((size_t) r0 + a0 + i) : src.get((size_t) mid + b0 + (i - na)));
            __syncthreads();
            for (uint32_t i = tid; i < cnt; i += 256) {
                const SortComp<ES> c = pieces.get(i);
                const uint32_t slot = i < na ? i + sort_rank<ES>(pieces, na, nb, c) : (i - na) + sort_rank<ES>(pieces, 0, na, c);
                merged.set(slot, c);                                                              // slot < cnt
            }
            __syncthreads();
            if (cont_l || cont_r) {
                for (uint32_t i = tid; i < cnt; i += 256) dst.set((size_t) m0 + i, merged.get(i));
            } else {
                for (uint32_t i = tid; i < cnt; i += 256) {
                    uint32_t pos = comp_pos(merged.get(i));
                    if (pos >= n) pos = n - 1;
                    if (outv) outv[m0 + i] = in[pos];
                    if (outi) outi[m0 + i] = flat ? pos : (pos > M.lo ? pos - M.lo : 0u);
                }
            }
        }
        for (size_t g = (size_t) o0 + tid; g < (o1 < cl ? o1 : cl); g += 256) dst.set(g, src.get(g));            // (a <= o0)
        for (size_t g = (size_t) (o0 > cr ? o0 : cr) + tid; g < (o1 < b ? o1 : b); g += 256) dst.set(g, src.get(g));
    }
}

__global__ __launch_bounds__(256) void k_sort_segments_iota(uint32_t *out, size_t n) {
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t) gridDim.x * 256) out[i] = (uint32_t) i;
}

template <typename U, int KIND>
static int sort_segments_typed(void *outv_, uint32_t *outi, const void *in_, size_t n, const uint32_t *starts, size_t m, const SegSortPlan &p,
                               int flags) {
    RoctxRange range("enoki-hip: segment sort");
    constexpr int ES = sizeof(U);
    Context &c = ctx();
    U *outv = (U *) outv_;
    const U *in = (const U *) in_;
    const size_t cb = comp_bytes(ES), out_bytes = n * ((outv ? ES : 0) + (outi ? 4 : 0));
    const uint32_t top = search_top(m), tiles = (uint32_t) p.tiles;
    void *scratch = nullptr;
    if (p.scratch_bytes)
        if (int rc = ek_hip_malloc(p.scratch_bytes, &scratch)) return rc;
    unsigned char *sb = (unsigned char *) scratch;
    CompStore<ES> none = { nullptr, nullptr }, bufs[2] = { none, none };
    uint32_t *edge = nullptr, *needed = nullptr;
    if (scratch) {
        bufs[0] = comp_store<ES>(sb, n);
        if (p.merges > 1) bufs[1] = comp_store<ES>(sb + p.buf_bytes, n);
        edge = (uint32_t *) (sb + p.buf_bytes * (p.merges > 1 ? 2 : 1));
        needed = edge + tiles;
    }
    int rc = EK_OK;
    do {
        hipLaunchKernelGGL((k_sort_segments_tiles<U, KIND>), dim3((unsigned) p.workgroups), dim3(256), 0, c.stream, outv, outi, bufs[0], edge, in,
                           (uint32_t) n, starts, (uint32_t) m, top, tiles, (uint32_t) p.per_workgroup, flags);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort_segments(): the tile launch failed"); break; }
        note_launch("sort_segments_tiles", n, n * ES + m * 4 + out_bytes);
        if (!p.merges) break;
        hipLaunchKernelGGL(k_sort_segments_needed, dim3(1), dim3(256), 0, c.stream, needed, (const uint32_t *) edge, tiles);
        if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort_segments(): the pass count launch failed"); break; }
        note_launch("sort_segments_needed", tiles, (size_t) tiles * 4);
        for (int pass = 0; pass < p.merges; ++pass) {
            hipLaunchKernelGGL((k_sort_segments_merge<U>), dim3((unsigned) p.merge_workgroups), dim3(256), 0, c.stream, outv, outi,
                               bufs[(pass + 1) & 1], bufs[pass & 1], in, (uint32_t) n, starts, (uint32_t) m, top, tiles, (uint32_t) pass,
                               (const uint32_t *) needed, flags);
            if (hipGetLastError() != hipSuccess) { rc = fail(EK_ERR_HIP, "ek_hip_sort_segments(): a merge launch failed"); break; }
            note_launch("sort_segments_merge", n, 2 * n * cb);
        }
    } while (false);
    if (scratch) ek_hip_free(scratch);   // stream-ordered reuse
    return rc;
}

static int segsort_size_check(const char *what, size_t n, size_t m) {
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull)
        return fail(EK_ERR_UNSUPPORTED, "%s: more than 2^32 - 1 entries or segments are unsupported (%zu, %zu)", what, n, m);
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_sort_segments_plan(int type, size_t n, size_t m, int want_index, int compute_units, size_t *tile, size_t *tiles,
                              size_t *tiles_per_workgroup, size_t *workgroups, int *merges, size_t *merge_workgroups, int *launches,
                              size_t *scratch_bytes) {
    (void) want_index;          // the position travels inside the composite either way: it changes nothing
    if (int rc = numeric_type_check("ek_hip_sort_segments_plan()", type)) return rc;
    if (int rc = segsort_size_check("ek_hip_sort_segments_plan()", n, m)) return rc;
    if (compute_units < 0) return fail(EK_ERR_INVALID, "ek_hip_sort_segments_plan(): %d compute units", compute_units);
    const SegSortPlan p = segsort_plan(type_size(type), n, m, compute_units);
    if (tile) *tile = p.tile;
    if (tiles) *tiles = p.tiles;
    if (tiles_per_workgroup) *tiles_per_workgroup = p.per_workgroup;
    if (workgroups) *workgroups = p.workgroups;
    if (merges) *merges = p.merges;
    if (merge_workgroups) *merge_workgroups = p.merge_workgroups;
    if (launches) *launches = p.launches;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return EK_OK;
}

int ek_hip_sort_segments(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, const uint32_t *starts, size_t m,
                         int flags) {
    if (int rc = ensure_init()) return rc;
    if (int rc = numeric_type_check("ek_hip_sort_segments()", type)) return rc;
    if (flags & ~(EK_SORT_DESCENDING | EK_SORT_FLAT_INDEX)) return fail(EK_ERR_INVALID, "ek_hip_sort_segments(): unknown flags %d", flags);
    if (int rc = segsort_size_check("ek_hip_sort_segments()", n, m)) return rc;
    if (!out_values && !out_index) return fail(EK_ERR_INVALID, "ek_hip_sort_segments(): no output");
    if (n == 0) return EK_OK;
    const size_t elem = type_size(type);
    if (int rc = pointers_check("ek_hip_sort_segments()", elem, in)) return rc;
    // (an output that was not asked for is a null pointer: aligned)
    if (int rc = alignment_check("ek_hip_sort_segments()", elem, out_values)) return rc;
    if (int rc = alignment_check("ek_hip_sort_segments()", 4, out_index)) return rc;
    if (sort_overlap(in, n * elem, out_values, n * elem) || sort_overlap(in, n * elem, out_index, n * 4) ||
        sort_overlap(out_values, n * elem, out_index, n * 4))
        return fail(EK_ERR_INVALID, "ek_hip_sort_segments(): in and the outputs overlap");
    if (m == 0) {
        // no segment: every entry stays where it is
        if (out_values)
            if (int rc = ek_hip_memcpy_device(out_values, in, n * elem)) return rc;
        if (out_index) {
            hipLaunchKernelGGL(k_sort_segments_iota, dim3(stream_grid(n, ctx().tuning.blocks_per_cu)), dim3(256), 0, ctx().stream, out_index, n);
            EK_LAUNCH_CHECK("sort_segments_iota", n, n * 4);
        }
        return EK_OK;
    }
    if (int rc = pointers_check("ek_hip_sort_segments()", sizeof(uint32_t), starts)) return rc;
    const SegSortPlan p = segsort_plan(elem, n, m, ctx().num_cu);
    switch (type) {
        case EK_I32: return sort_segments_typed<uint32_t, kSortSigned>(out_values, out_index, in, n, starts, m, p, flags);
        case EK_U32: return sort_segments_typed<uint32_t, kSortUnsigned>(out_values, out_index, in, n, starts, m, p, flags);
        case EK_I64: return sort_segments_typed<uint64_t, kSortSigned>(out_values, out_index, in, n, starts, m, p, flags);
        case EK_U64: return sort_segments_typed<uint64_t, kSortUnsigned>(out_values, out_index, in, n, starts, m, p, flags);
        case EK_F32: return sort_segments_typed<uint32_t, kSortFloat>(out_values, out_index, in, n, starts, m, p, flags);
        default: return sort_segments_typed<uint64_t, kSortFloat>(out_values, out_index, in, n, starts, m, p, flags);
    }
}

}
