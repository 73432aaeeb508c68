// search_sorted: per needle v the number of entries t of a sorted table with t < v (right: t <= v), in ONE launch.
//
// The spelling this replaces, binary_search(0, K, [&](i) { return gather(T, min(i, K - 1)) < v; }) (include/enoki/array.h), runs
// log2(K) + 1 rounds of min / gather+compare / select / select over n-element arrays.  The answer is one uint32 per needle, so the
// algorithmic traffic is the needle in and the index out (8 B per 4-byte needle).
//
//   * 512-thread workgroups (8 waves), at most two per CU, grid-stride over items of 4 needles per lane: the needles of an item are
//     read with 16-byte non-temporal loads (two for 8-byte types) and its four indices leave in one 16-byte non-temporal store.  The
//     host peels 0..3 leading elements so that the stores are 16-byte aligned; the needle loads fall back to element loads when the
//     needle pointer is not aligned at the same element.  Peel and tail (at most 6 elements) are searched one per lane by workgroup 0.
//   * The four searches of a lane are independent chains that advance in lockstep, one table read each per step, so four reads are in
//     flight per lane.  A search is the branch-free fixed-trip form  pos += pred(T[pos + h - 1]) ? h : 0  for h = top, top / 2, .., 1
//     with a bound test in the predicate; the trip count depends on K only: no lane diverges.
//   * The workgroup stages the table into 64 KiB of LDS: whole when it has up to R = 64 KiB / sizeof(T) entries, otherwise the LAST
//     entry of every block of `stride` entries (stride the smallest power of two with K / stride <= R).  b = the count over the
//     samples says that blocks 0 .. b-1 lie wholly before the needle and that the last entry of block b does not, so the count is
//     b * stride + (the count over the next min(stride - 1, K - b * stride) entries): log2(stride) steps in global memory inside a
//     window of consecutive entries.  Both levels count with the same predicate over a sorted range, so runs of equal entries that
//     span sample boundaries need no special case.
//   * 64 KiB per workgroup: two workgroups (16 waves) fit the 160 KiB of a CU, and every halving of R would add a global step --
//     those, one request per lane and step, are what bounds large tables.
#include "ek_search.h"

namespace ek {

template <typename T, bool Right>
__global__ __launch_bounds__(kSearchBlock) void k_search_sorted(uint32_t *__restrict__ out, const T *__restrict__ table, uint32_t K,
                                                                const T *__restrict__ needles, size_t n, SearchPlan p, uint32_t peel,
                                                                int needles_vec) {
    constexpr int N = kSearchLane;
    __shared__ T lds[kSearchLdsBytes / sizeof(T)];
    for (uint32_t i = threadIdx.x; i < p.resident; i += kSearchBlock) lds[i] = table[i * p.stride + (p.stride - 1)];
    __syncthreads();
    const uint32_t base[N] = { }, base1[1] = { };                  // the one table starts at lds[0]

    // (requesting a lane's NEXT item before the current one is searched changed no shape of tools/probe_search_sorted.py by more than
    //  2 % in one call on one box, at 4 to 8 more VGPRs: left out)
    const size_t items = (n - peel) / N;
    for (size_t item = (size_t) blockIdx.x * kSearchBlock + threadIdx.x; item < items; item += (size_t) gridDim.x * kSearchBlock) {
        const size_t e = peel + item * N;
        T v[N];
        search_load<T, N>(needles + e, needles_vec, v);
        Pack<uint32_t, N> r;
        search_run<T, Right, N>(lds, base, table, K, p, v, r.v);
        pack_store<uint32_t, N, true>(out + e, r);
    }

    // the elements in front of the first aligned store and behind the last whole item
    const uint32_t rest = peel + (uint32_t) ((n - peel) - items * N);
    if (blockIdx.x == 0 && threadIdx.x < rest) {
        const size_t e = threadIdx.x < peel ? threadIdx.x : peel + items * N + (threadIdx.x - peel);
        const T v[1] = { needles[e] };
        uint32_t r[1];
        search_run<T, Right, 1>(lds, base1, table, K, p, v, r);
        out[e] = r[0];
    }
}

template <typename T>
static int search_sorted(uint32_t *out, const void *table, size_t K, const void *needles, size_t n, int right) {
    RoctxRange range("enoki-hip: search_sorted");
    Context &c = ctx();
    const SearchPlan p = search_plan(sizeof(T), K);
    size_t peel = head_of(out);
    if (peel > n) peel = n;
    const int needles_vec = aligned16((const T *) needles + peel);
    const size_t items = (n - peel) / kSearchLane;
    size_t blocks = (items + kSearchBlock - 1) / kSearchBlock, cap = (size_t) c.num_cu * kSearchBlocksPerCu;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    if (right)
        hipLaunchKernelGGL((k_search_sorted<T, true>), dim3((unsigned) blocks), dim3(kSearchBlock), 0, c.stream, out, (const T *) table,
                           (uint32_t) K, (const T *) needles, n, p, (uint32_t) peel, needles_vec);
    else
        hipLaunchKernelGGL((k_search_sorted<T, false>), dim3((unsigned) blocks), dim3(kSearchBlock), 0, c.stream, out, (const T *) table,
                           (uint32_t) K, (const T *) needles, n, p, (uint32_t) peel, needles_vec);
    EK_LAUNCH_CHECK("search_sorted", n, n * (sizeof(T) + sizeof(uint32_t)));
    return EK_OK;
}

} // namespace ek

using namespace ek;

extern "C" {

int ek_hip_search_sorted_plan(int type, size_t K, int *resident, int *stride, int *global_steps) {
    if (int rc = search_type_check("ek_hip_search_sorted_plan()", type, K)) return rc;
    const SearchPlan p = search_plan(type_size(type), K);
    if (resident) *resident = (int) p.resident;
    if (stride) *stride = (int) p.stride;
    if (global_steps) *global_steps = (int) p.global_steps;
    return EK_OK;
}

int ek_hip_search_sorted(int type, uint32_t *out, const void *table, size_t K, const void *needles, size_t n, int right) {
    if (int rc = ensure_init()) return rc;
    if (int rc = search_type_check("ek_hip_search_sorted()", type, K)) return rc;
    if (n == 0) return EK_OK;
    if (!out || !needles || (!table && K)) return fail(EK_ERR_INVALID, "ek_hip_search_sorted(): null pointer");
    switch (type) {
        case EK_I32: return search_sorted<int32_t>(out, table, K, needles, n, right);
        case EK_U32: return search_sorted<uint32_t>(out, table, K, needles, n, right);
        case EK_I64: return search_sorted<int64_t>(out, table, K, needles, n, right);
        case EK_U64: return search_sorted<uint64_t>(out, table, K, needles, n, right);
        case EK_F32: return search_sorted<float>(out, table, K, needles, n, right);
        default: return search_sorted<double>(out, table, K, needles, n, right);
    }
}

}
