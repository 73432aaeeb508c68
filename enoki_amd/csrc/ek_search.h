// The search that search.hip (one sorted table), block_search.hip (one sorted row per needle) and segment_search.hip (one ragged
// segment per needle) share: the plan of the two-level search, the predicate, the needle loads, N independent searches in lockstep,
// the staging of consecutive entries and the walk of a range of needles between its peel and its tail.
//
// A search is the branch-free fixed-trip form  pos += pred(T[pos + h - 1]) ? h : 0  for h = top, top / 2, .., 1 with the bound
// test in the predicate; the trip count depends on the size of the searched range only, so no lane diverges.  Every read is
// clamped to the range it searches, whatever the needle and whatever the table holds.
#pragma once

#include "ek_block.h"        // head_of, numeric_type_check, dispatch_numeric

namespace ek {

constexpr int kSearchBlock = 512;
constexpr int kSearchLane = 4;                    // needles per lane and item
constexpr size_t kSearchLdsBytes = 64 * 1024;
constexpr int kSearchBlocksPerCu = 2;

struct SearchPlan {
    uint32_t resident;      // entries or samples in LDS
    uint32_t stride;        // sample s is entry (s + 1) * stride - 1; 1: the table is resident whole
    uint32_t lds_top;       // first step of the LDS search: the largest power of two <= resident (0: empty table)
    uint32_t global_steps;  // log2(stride)
};

/// `capacity`: entries of LDS the samples may take (0: all of it)
static SearchPlan search_plan(size_t elem_size, size_t K, size_t capacity = 0) {
    const size_t R = capacity ? capacity : kSearchLdsBytes / elem_size;
    SearchPlan p = { 0, 1, 0, 0 };
    while (K / p.stride > R) { p.stride <<= 1; p.global_steps++; }
    p.resident = (uint32_t) (K / p.stride);
    if (p.resident) {
        p.lds_top = 1;
        while (p.lds_top <= p.resident / 2) p.lds_top <<= 1;
    }
    return p;
}

template <typename T, bool Right> __device__ __forceinline__ bool search_before(T t, T v) {
    if constexpr (Right) return t <= v; else return t < v;
}

/// the N needles of one item: 16-byte non-temporal loads, or element loads for a pointer that is only element-aligned
template <typename T, int N> __device__ __forceinline__ void search_load(const T *__restrict__ src, int vec, T (&v)[N]) {
    if (vec) {
        constexpr int V = 16 / sizeof(T);
#pragma unroll
        for (int j = 0; j < N / V; ++j) {
            const Pack<T, V> pk = pack_load<T, V, true>(src + j * V);
#pragma unroll
            for (int k = 0; k < V; ++k) v[j * V + k] = pk.v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = __builtin_nontemporal_load(src + k);
    }
}

/// N searches in lockstep, chain k over the count[k] entries mem[base[k] + first[k] ..]; every read stays at or below
/// mem[base[k] + last].  pos[k] (0 on entry) becomes the number of those entries before v[k].
template <typename T, bool Right, int N>
__device__ __forceinline__ void search_steps(const T *mem, const uint32_t (&base)[N], const uint32_t (&first)[N],
                                             const uint32_t (&count)[N], uint32_t last, uint32_t top, const T (&v)[N],
                                             uint32_t (&pos)[N]) {
    for (uint32_t h = top; h; h >>= 1) {
        T t[N];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = mem[base[k] + min(first[k] + pos[k] + h - 1, last)];
#pragma unroll
        for (int k = 0; k < N; ++k) pos[k] += (pos[k] + h - 1 < count[k] && search_before<T, Right>(t[k], v[k])) ? h : 0u;
    }
}

/// N independent searches in lockstep over the K entries of `table`: first the p.resident entries or samples that start at
/// lds[lds_base[k]], then, for a sampled table, log2(stride) steps inside one window of `table`
template <typename T, bool Right, int N>
__device__ __forceinline__ void search_run(const T *lds, const uint32_t (&lds_base)[N], const T *__restrict__ table, uint32_t K,
                                           const SearchPlan &p, const T (&v)[N], uint32_t (&result)[N]) {
    uint32_t pos[N], zero[N], count[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { pos[k] = 0; zero[k] = 0; count[k] = p.resident; }
    search_steps<T, Right, N>(lds, lds_base, zero, count, p.resident - 1, p.lds_top, v, pos);
    if (p.stride > 1) {                                            // (uniform) K > resident >= 1 here
        uint32_t lo[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            lo[k] = pos[k] * p.stride;                             // <= resident * stride <= K
            count[k] = min(p.stride - 1, K - lo[k]);
            pos[k] = 0;
        }
        search_steps<T, Right, N>(table, zero, lo, count, K - 1, p.stride >> 1, v, pos);
#pragma unroll
        for (int k = 0; k < N; ++k) pos[k] += lo[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) result[k] = pos[k];
}

/// `count` consecutive entries into LDS: 16-byte loads between an element-wise head and tail
template <typename T> __device__ __forceinline__ void stage_entries(T *lds, const T *__restrict__ src, uint32_t count) {
    constexpr uint32_t V = 16 / sizeof(T);
    uint32_t head = head_of(src);
    if (head > count) head = count;
    if (threadIdx.x < head) lds[threadIdx.x] = src[threadIdx.x];
    const uint32_t vecs = (count - head) / V;
    for (uint32_t i = threadIdx.x; i < vecs; i += kSearchBlock) {
        const Pack<T, V> pk = pack_load<T, V, false>(src + head + i * V);
#pragma unroll
        for (uint32_t k = 0; k < V; ++k) lds[head + i * V + k] = pk.v[k];
    }
    for (uint32_t i = head + vecs * V + threadIdx.x; i < count; i += kSearchBlock) lds[i] = src[i];
}

/// The workgroup searches needles [e0, e1): whole items of N between a peel to the first 16-byte aligned output and a tail.
/// search(v, j, r): the results r of the needles v, the first of which is needle e0 + j.
template <typename T, typename Search>
__device__ __forceinline__ void search_range(uint32_t *__restrict__ out, const T *__restrict__ needles, size_t e0, size_t e1,
                                             const Search &search) {
    constexpr int N = kSearchLane;
    const size_t count = e1 - e0;
    size_t peel = head_of<size_t>(out + e0);
    if (peel > count) peel = count;
    const int vec = (reinterpret_cast<uintptr_t>(needles + e0 + peel) & 15u) == 0;
    const size_t items = (count - peel) / N;
    for (size_t item = threadIdx.x; item < items; item += kSearchBlock) {
        const size_t j = peel + item * N;
        T v[N];
        search_load<T, N>(needles + e0 + j, vec, v);
        Pack<uint32_t, N> r;
        search(v, j, r.v);
        pack_store<uint32_t, N, true>(out + e0 + j, r);
    }
    const uint32_t rest = (uint32_t) (count - items * N);          // peel + tail, at most 6
    if (threadIdx.x < rest) {
        const size_t j = threadIdx.x < peel ? threadIdx.x : items * N + threadIdx.x;
        const T v[1] = { needles[e0 + j] };
        uint32_t r[1];
        search(v, j, r);
        out[e0 + j] = r[0];
    }
}

/// the largest power of two <= count (0 for 0): the first step of a search over `count` entries
static uint32_t search_top(size_t count) {
    uint32_t top = count ? 1 : 0;
    while (top && top <= count / 2) top <<= 1;
    return top;
}

static int search_type_check(const char *what, int type, size_t K) {
    if (int rc = numeric_type_check(what, type)) return rc;
    if (K > 0xFFFFFFFFull) return fail(EK_ERR_UNSUPPORTED, "%s: tables of 2^32 entries or more are unsupported (%zu)", what, K);
    return EK_OK;
}

} // namespace ek
