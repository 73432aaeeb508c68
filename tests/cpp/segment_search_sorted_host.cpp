// segment_search_sorted (include/enoki/array.h) down to the C-ABI call, on the host stand-in of the C ABI (host_abi_stub.h),
// without a GPU: a stand-alone program with its own main; tests/test_segment_search_sorted_host.py builds and runs it (also under
// -fsanitize=address,undefined).  The stand-in does not define ek_hip_search_sorted_segments; this file does, as a plain host loop
// over the clamp rule of ek_block.h.
//
//   * unevaluated operands (unary maps of table and needles) are evaluated once each, then the one call is made;
//   * no needles: no call, whatever the other sizes are;
//   * starts or rows that are no UInt32 array are refused before the C ABI is reached (and before an operand is evaluated), and so
//     are needle starts of another length than the table starts, rows of another length than the needles, and rows without a segment;
//   * a differentiable table or needles record no node, the result is a plain UInt32 index array, nothing stays allocated;
//   * -DBARE_TYPE: a flat array type WITHOUT the member compiles and throws at run time.
#include <enoki/hip.h>
#include <enoki/autodiff.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

#ifdef BARE_TYPE
// a second, tiny translation unit: the free functions on an array type that has no segment_search_sorted_ member
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

int main() {
    Bare b, starts;
    int thrown = 0;
    try { (void) enoki::segment_search_sorted(b, starts, b, starts, true, false); }
    catch (const std::runtime_error &e) { thrown += std::string(e.what()) == "segment_search_sorted(): not available for this array type"; }
    try { (void) enoki::segment_search_sorted_indexed(b, starts, b, starts); }
    catch (const std::runtime_error &e) { thrown += std::string(e.what()) == "segment_search_sorted_indexed(): not available for this array type"; }
    CHECK(thrown == 2);
    printf("segment_search_sorted_host: a type without the member compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/csrc/ek_block.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_search_calls = 0;

/// the definition: per needle the count of entries of its clamped segment before it (right: not after it), plus lo with flat
static void search_loop(uint32_t *out, const float *table, size_t nt, const uint32_t *ts, size_t m, const float *needles, size_t n,
                        const uint32_t *ns, const uint32_t *rows, bool right, bool flat) {
    for (size_t e = 0; e < n; ++e) {
        long j = -1;
        if (rows) j = (long) std::min<size_t>(rows[e], m - 1);
        else for (size_t k = 0; k < m; ++k) if (ns[k] <= e) j = (long) k;
        out[e] = 0;
        if (j < 0) continue;
        uint32_t lo, hi, count = 0;
        ek::segment_clamp(ts[j], (size_t) j + 1 < m ? ts[j + 1] : (uint32_t) nt, (uint32_t) nt, lo, hi);
        for (uint32_t i = lo; i < hi; ++i) count += right ? table[i] <= needles[e] : table[i] < needles[e];
        out[e] = count + (flat ? lo : 0u);
    }
}

extern "C" int ek_hip_search_sorted_segments(int type, uint32_t *out, const void *table, size_t nt, const uint32_t *table_starts, size_t m,
                                             const void *needles, size_t n, const uint32_t *needle_starts, const uint32_t *row_index, int flags) {
    ++g_search_calls;
    if (type != EK_F32 || (flags & ~3)) STUB_UNSUPPORTED("search_sorted_segments", type, flags);
    if ((needle_starts && row_index) || (!needle_starts && !row_index && m) || n == 0 || !out || !needles || (nt && !table) || (m && !table_starts))
        STUB_UNSUPPORTED("search_sorted_segments: arguments", (int) m, (int) n);
    search_loop(out, (const float *) table, nt, table_starts, m, (const float *) needles, n, needle_starts, row_index,
                flags & EK_SEARCH_RIGHT, flags & EK_SEARCH_FLAT);
    return EK_OK;
}
extern "C" int ek_hip_search_sorted_segments_plan(int, size_t, size_t, size_t, int, int, int *route, size_t *tile_needles,
                                                  size_t *tiles_per_workgroup, size_t *workgroups, size_t *lds_entries, size_t *window) {
    *route = 1; *tile_needles = 2048; *tiles_per_workgroup = 1; *workgroups = 1; *lds_entries = 1; *window = 1;
    return EK_OK;
}

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using D = DiffArray<F>;
using DU = DiffArray<U>;

template <typename A> static auto host(const A &a) {
    std::vector<std::decay_t<decltype(a.coeff(0))>> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}

static std::vector<uint32_t> searched(const std::vector<float> &table, const std::vector<uint32_t> &ts, const std::vector<float> &needles,
                                      const std::vector<uint32_t> *ns, const std::vector<uint32_t> *rows, bool right, bool flat) {
    std::vector<uint32_t> r(needles.size());
    search_loop(r.data(), table.data(), table.size(), ts.data(), ts.size(), needles.data(), needles.size(), ns ? ns->data() : nullptr,
                rows ? rows->data() : nullptr, right, flat);
    return r;
}

template <typename Fn> static bool throws(Fn &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

// 5 * 16384 + 3 entries and needles (what a unary map needs to stay unevaluated); table segments of 0, 1, 2, .. entries whose
// values ascend (so does sin on [-1.5, 1.5]), the last starts at nt and above it; 0 .. 79 needles per segment behind 3 that belong to none
static constexpr size_t N = 5 * (1 << 14) + 3;
static void ragged(std::vector<uint32_t> &ts, std::vector<uint32_t> &ns) {
    for (size_t at = 0, len = 0; at <= N; at += len, len = (len + 1) % 40) ts.push_back((uint32_t) at);
    ts.push_back((uint32_t) N + 5);
    for (size_t k = 0, at = 3; k < ts.size(); ++k, at += (k * 7) % 80) ns.push_back((uint32_t) std::min(at, N + 9));
}

static void plain() {
    F x = linspace<F>(-1.5f, 1.5f, N), y = linspace<F>(1.4f, -1.4f, N);
    (void) x.data(); (void) y.data();
    std::vector<uint32_t> hts, hns, hrows(N);
    ragged(hts, hns);
    for (size_t i = 0; i < N; ++i) hrows[i] = (uint32_t) ((i * 2654435761u) % (hts.size() + 7));
    U ts = U::copy(hts.data(), hts.size()), ns = U::copy(hns.data(), hns.size()), rows = U::copy(hrows.data(), N);
    hip_set_defer(true);
    // (1) unevaluated operands: one unary launch each, one call -- and nothing again for the second call
    {
        F table = sin(x), needles = sin(y);
        CHECK(table.mapped_() && needles.mapped_());
        const long u0 = g_unary_calls, c0 = g_search_calls;
        U r = segment_search_sorted(table, ts, needles, ns);
        CHECK(g_unary_calls == u0 + 2 && g_search_calls == c0 + 1 && !table.mapped_() && !needles.mapped_() && r.size() == N);
        U r2 = segment_search_sorted_indexed(table, ts, needles, rows, true, true);
        CHECK(g_unary_calls == u0 + 2 && g_search_calls == c0 + 2 && r2.size() == N);
        CHECK(host(r) == searched(host(table), hts, host(needles), &hns, nullptr, false, false));
        CHECK(host(r2) == searched(host(table), hts, host(needles), nullptr, &hrows, true, true));
        CHECK(r.coeff(0) == 0 && r.coeff(2) == 0);                                                          // in front of every segment
        CHECK(host(segment_search_sorted(table, ts, needles, ns, true)) == searched(host(table), hts, host(needles), &hns, nullptr, true, false));
        CHECK(host(segment_search_sorted(table, ts, needles, ns, false, true)) == searched(host(table), hts, host(needles), &hns, nullptr, false, true));
    }
    // (2) starts or rows that are no UInt32 array are refused before the C ABI is reached and before an operand is evaluated
    // (HIPArray converts between element types, so for a type WITH the member array.h refuses other starts when it compiles:
    //  static_assert(is_same<Starts, uint32_array_t<T>>).  A type that cannot be UInt32 starts at all throws at run time.)
    {
        static_assert(std::is_same_v<uint32_array_t<F>, U> && std::is_same_v<uint32_array_t<D>, DU>, "the starts are UInt32");
        static_assert(enoki::detail::has_segment_search_sorted<F, U>::value && enoki::detail::has_segment_search_sorted<D, DU>::value &&
                      !enoki::detail::has_segment_search_sorted<F, std::string>::value, "the member takes UInt32 arrays");
        F table = sin(x), needles = sin(y);
        const std::string not_starts = "0, 3, 7";
        const long u0 = g_unary_calls, c0 = g_search_calls;
        CHECK(throws([&] { (void) segment_search_sorted(table, not_starts, needles, not_starts); }));
        CHECK(throws([&] { (void) segment_search_sorted_indexed(table, not_starts, needles, not_starts, true, true); }));
        // length mismatches, and a row per needle without any segment
        U shorter = U::copy(hns.data(), hns.size() - 1), fewer = U::copy(hrows.data(), N - 1), none;
        CHECK(throws([&] { (void) segment_search_sorted(table, ts, needles, shorter); }));
        CHECK(throws([&] { (void) segment_search_sorted(table, shorter, needles, ns); }));
        CHECK(throws([&] { (void) segment_search_sorted_indexed(table, ts, needles, fewer); }));
        CHECK(throws([&] { (void) segment_search_sorted_indexed(table, none, needles, rows); }));
        // both owners or neither (the member; the free functions cannot spell it)
        CHECK(throws([&] { (void) table.segment_search_sorted_(ts, needles, &ns, &rows, false, false); }));
        CHECK(throws([&] { (void) table.segment_search_sorted_(ts, needles, nullptr, nullptr, false, false); }));
        CHECK(g_unary_calls == u0 && g_search_calls == c0 && table.mapped_() && needles.mapped_());
    }
    // (3) no needles: no call; no segments or no entries: one call each
    {
        const long c0 = g_search_calls;
        U none;
        F nothing, table = sin(x);
        CHECK(segment_search_sorted(table, ts, nothing, ns).size() == 0 && segment_search_sorted(nothing, none, nothing, none, true).size() == 0);
        CHECK(segment_search_sorted_indexed(table, ts, nothing, none).size() == 0 && segment_search_sorted_indexed(table, none, nothing, none).size() == 0);
        CHECK(g_search_calls == c0 && table.mapped_());
        U zeros = segment_search_sorted(x, none, y, none, false, true);
        CHECK(g_search_calls == c0 + 1 && host(zeros) == std::vector<uint32_t>(N, 0u));
        U empty = segment_search_sorted(nothing, ts, y, ns, true, true);
        CHECK(g_search_calls == c0 + 2 && host(empty) == std::vector<uint32_t>(N, 0u));
    }
    hip_set_defer(false);
}

static void on_differentiable_arrays() {
    const std::vector<float> ht = { 1, 2, 3, 10, 20, 5, 6, 7, 8 }, hn = { 2.5f, 0, 15, 99, 6, 6 };
    const std::vector<uint32_t> hts = { 0, 3, 5 }, hns = { 0, 2, 4 }, hrows = { 0, 0, 1, 1, 2, 9 };
    const size_t live = g_live.size();
    {
        D table = D(F::copy(ht.data(), ht.size())), needles = D(F::copy(hn.data(), hn.size()));
        DU ts = DU(U::copy(hts.data(), 3)), ns = DU(U::copy(hns.data(), 3)), rows = DU(U::copy(hrows.data(), 6));
        set_requires_gradient(table);
        set_requires_gradient(needles);
        const size_t nodes = Tape<F>::get()->node_count();
        DU k = segment_search_sorted(table, ts, needles, ns);
        DU f = segment_search_sorted(table, ts, needles, ns, true, true);
        DU r = segment_search_sorted_indexed(table, ts, needles, rows, true);
        static_assert(std::is_same_v<decltype(k), DU>, "a plain index array");
        CHECK(Tape<F>::get()->node_count() == nodes && k.index_() == 0 && f.index_() == 0 && r.index_() == 0);
        CHECK((host(k.value_()) == std::vector<uint32_t>{ 2, 0, 1, 2, 1, 1 }));
        CHECK((host(f.value_()) == std::vector<uint32_t>{ 2, 0, 4, 5, 7, 7 }));
        CHECK((host(r.value_()) == std::vector<uint32_t>{ 2, 0, 1, 2, 2, 2 }));
        // the positions feed a gather of the differentiable table as any index array does
        D picked = gather<D>(table, f);                                      // (every position is below nt here)
        CHECK(picked.index_() != 0 && picked.size() == 6);
    }
    CHECK(g_live.size() == live);
}

int main() {
    plain();
    on_differentiable_arrays();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("segment_search_sorted_host: operands evaluated once, no needles no call, wrong starts and rows types and length mismatches "
           "refused, nothing recorded on differentiable arrays, %ld calls, no block left allocated\n", g_search_calls);
    return 0;
}
#endif
