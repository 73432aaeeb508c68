// segment_sort / segment_argsort (include/enoki/array.h) down to the C-ABI call and through the tape, on the host stand-in of the
// C ABI (host_abi_stub.h), without a GPU: a stand-alone program with its own main; tests/test_segment_sort_host.py builds and runs
// it (also under -fsanitize=address,undefined).  The stand-in does not define ek_hip_sort_segments; this file does, as
// std::stable_sort over the clamp rule of ek_block.h.
//
//   * unevaluated operands (a unary map, deferred starts) are evaluated once, then the one call is made;
//   * no entries: no call; no starts: one call that leaves every entry in place;
//   * starts that are no UInt32 array are refused before the C ABI is reached (and before the operand is evaluated);
//   * one call serves values and permutation: segment_sort of a tracked DiffArray makes ONE call with both outputs, segment_sort of
//     a plain array one call with values only, segment_argsort one call with the index only;
//   * segment_sort of a tracked DiffArray records exactly one node of the source's size, segment_argsort none; backward scatters
//     the weights through the permutation (gradient(x)[p] == w), forward gathers the seed (seed[p]), size-1 seeds included; the
//     two sweeps are each other's transpose; `starts` gets no gradient;
//   * the node releases the permutation it keeps;
//   * -DBARE_TYPE: a flat array type WITHOUT the members compiles and throws at run time;
//   * no block stays allocated.
#include <enoki/hip.h>
#include <enoki/autodiff.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

#ifdef BARE_TYPE
// a second, tiny translation unit: the free functions on an array type that has neither member
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

int main() {
    Bare b, starts;
    bool sort_thrown = false, argsort_thrown = false;
    try { (void) enoki::segment_sort(b, starts, true); }
    catch (const std::runtime_error &e) { sort_thrown = std::string(e.what()) == "segment_sort(): not available for this array type"; }
    try { enoki::segment_argsort(b, starts, false, true); }
    catch (const std::runtime_error &e) { argsort_thrown = std::string(e.what()) == "segment_argsort(): not available for this array type"; }
    CHECK(sort_thrown && argsort_thrown);
    printf("segment_sort_host: a type without the members compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/csrc/ek_block.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

/// the definition: per clamped segment the stable order by < (by > when descending), every NaN last; entries in front of the
/// first segment stay.  Flat positions.
static std::vector<uint32_t> sorted_perm(const std::vector<float> &x, const std::vector<uint32_t> &starts, bool descending) {
    const uint32_t n = (uint32_t) x.size();
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    for (size_t j = 0; j < starts.size(); ++j) {
        uint32_t lo, hi;
        ek::segment_clamp(starts[j], j + 1 < starts.size() ? starts[j + 1] : n, n, lo, hi);
        std::stable_sort(p.begin() + lo, p.begin() + hi, [&](uint32_t a, uint32_t b) {
            if (std::isnan(x[a]) || std::isnan(x[b])) return !std::isnan(x[a]) && std::isnan(x[b]);
            return descending ? x[a] > x[b] : x[a] < x[b];
        });
    }
    return p;
}

/// segment-local positions of a flat permutation (an entry in front of the first segment counts from 0)
static std::vector<uint32_t> local_of(std::vector<uint32_t> p, const std::vector<uint32_t> &starts) {
    const uint32_t n = (uint32_t) p.size();
    for (size_t j = 0; j < starts.size(); ++j) {
        uint32_t lo, hi;
        ek::segment_clamp(starts[j], j + 1 < starts.size() ? starts[j + 1] : n, n, lo, hi);
        for (uint32_t i = lo; i < hi; ++i) p[i] -= lo;
    }
    return p;
}

template <typename V> static std::vector<V> taken(const std::vector<V> &x, const std::vector<uint32_t> &flat) {
    std::vector<V> r(x.size());
    for (size_t i = 0; i < x.size(); ++i) r[i] = x[flat[i]];
    return r;
}

static long g_sort_calls = 0, g_value_outputs = 0, g_index_outputs = 0;

extern "C" int ek_hip_sort_segments(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, const uint32_t *starts, size_t m,
                                    int flags) {
    ++g_sort_calls;
    g_value_outputs += out_values != nullptr;
    g_index_outputs += out_index != nullptr;
    if (type != EK_F32) STUB_UNSUPPORTED("sort_segments", type, flags);
    if (n == 0 || (flags & ~3) || (!out_values && !out_index) || !in || (m && !starts)) {
        fprintf(stderr, "stand-in: no entries, a bad flag or a bad pointer reached the C ABI\n");
        abort();
    }
    const std::vector<float> x((const float *) in, (const float *) in + n);
    const std::vector<uint32_t> s(starts, starts + m), flat = sorted_perm(x, s, flags & EK_SORT_DESCENDING);
    if (out_values) {
        const std::vector<float> v = taken(x, flat);
        memcpy(out_values, v.data(), n * sizeof(float));
    }
    if (out_index) memcpy(out_index, ((flags & EK_SORT_FLAT_INDEX) ? flat : local_of(flat, s)).data(), n * sizeof(uint32_t));
    return EK_OK;
}
extern "C" int ek_hip_sort_segments_plan(int, size_t, size_t, int, int, size_t *tile, size_t *tiles, size_t *tiles_per_workgroup,
                                         size_t *workgroups, int *merges, size_t *merge_workgroups, int *launches, size_t *scratch_bytes) {
    *tile = 2048; *tiles = 1; *tiles_per_workgroup = 1; *workgroups = 1; *merges = 0; *merge_workgroups = 0; *launches = 1; *scratch_bytes = 0;
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

template <typename Fn> static bool throws(Fn &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

// 5 * 16384 + 3 entries (what a unary map needs to stay unevaluated); segments of 0, 1, 2, .. entries, the first behind 3 entries
// that belong to none, the last ones empty at n and above it
static constexpr size_t N = 5 * (1 << 14) + 3;
static std::vector<uint32_t> ragged_starts() {
    std::vector<uint32_t> s;
    for (size_t at = 3, len = 0; at <= N; at += len, len = (len + 1) % 40) s.push_back((uint32_t) at);
    s.push_back((uint32_t) N);
    s.push_back((uint32_t) N + 5);
    return s;
}

static void plain() {
    F x = linspace<F>(-40.f, 40.f, N);
    (void) x.data();
    const std::vector<uint32_t> hs = ragged_starts();
    U starts = U::copy(hs.data(), hs.size());
    hip_set_defer(true);
    // (1) an unevaluated operand: one unary launch, one call -- and nothing again for the second call
    {
        F s = sin(x);
        CHECK(s.mapped_());
        const long u0 = g_unary_calls, c0 = g_sort_calls, v0 = g_value_outputs, i0 = g_index_outputs;
        F r = segment_sort(s, starts);
        CHECK(g_unary_calls == u0 + 1 && g_sort_calls == c0 + 1 && !s.mapped_() && r.size() == N);
        CHECK(g_value_outputs == v0 + 1 && g_index_outputs == i0);                // values only: no index is computed or allocated
        U p = segment_argsort(s, starts, true, true);
        CHECK(g_unary_calls == u0 + 1 && g_sort_calls == c0 + 2 && p.size() == N);
        CHECK(g_value_outputs == v0 + 1 && g_index_outputs == i0 + 1);            // index only
        const std::vector<float> h = host(s);
        CHECK(host(r) == taken(h, sorted_perm(h, hs, false)));
        CHECK(host(p) == sorted_perm(h, hs, true));
        CHECK(host(segment_argsort(s, starts)) == local_of(sorted_perm(h, hs, false), hs));
        CHECK(host(segment_sort(s, starts, true)) == taken(h, sorted_perm(h, hs, true)));
        CHECK(p.coeff(0) == 0u && p.coeff(2) == 2u && r.coeff(1) == s.coeff(1));  // in front of starts[0]: in place
    }
    // (2) starts that are no UInt32 array are refused before the C ABI is reached and before the operand is evaluated
    // (HIPArray converts between element types, so for a type WITH the members array.h refuses other starts when it compiles:
    //  static_assert(is_same<Starts, uint32_array_t<T>>).  A type that cannot take UInt32 starts at all throws at run time.)
    {
        static_assert(std::is_same_v<uint32_array_t<F>, U> && std::is_same_v<uint32_array_t<D>, DU>, "the starts are UInt32");
        static_assert(enoki::detail::has_segment_sort<F, U>::value && enoki::detail::has_segment_sort<D, DU>::value &&
                      !enoki::detail::has_segment_sort<F, std::string>::value, "the member takes a UInt32 array");
        static_assert(enoki::detail::has_segment_argsort<F, U>::value && enoki::detail::has_segment_argsort<D, DU>::value &&
                      !enoki::detail::has_segment_argsort<F, std::string>::value, "the member takes a UInt32 array");
        F s = sin(x);
        const std::string not_starts = "0, 3, 7";
        const long u0 = g_unary_calls, c0 = g_sort_calls;
        CHECK(throws([&] { (void) segment_sort(s, not_starts); }) && throws([&] { (void) segment_sort(s, not_starts, true); }));
        CHECK(throws([&] { segment_argsort(s, not_starts); }) && throws([&] { segment_argsort(s, not_starts, true, true); }));
        CHECK(g_unary_calls == u0 && g_sort_calls == c0 && s.mapped_());
    }
    // (3) no entries: no call; no starts: no segment, one call that leaves everything in place
    {
        const long c0 = g_sort_calls;
        U none;
        F nothing;
        CHECK(segment_sort(nothing, starts).size() == 0 && segment_sort(nothing, none, true).size() == 0 && g_sort_calls == c0);
        CHECK(segment_argsort(nothing, starts).size() == 0 && segment_argsort(nothing, none, true, true).size() == 0 && g_sort_calls == c0);
        F same = segment_sort(x, none, true);
        CHECK(g_sort_calls == c0 + 1 && host(same) == host(x));
        std::vector<uint32_t> iota(N);
        std::iota(iota.begin(), iota.end(), 0u);
        CHECK(host(segment_argsort(x, none)) == iota && host(segment_argsort(x, none, true, true)) == iota && g_sort_calls == c0 + 3);
    }
    // (4) ties keep their input order, NaNs come last in both directions, empty segments own nothing
    {
        const float nan = std::nanf("");
        const float v[10] = { 9.f, 1.f, nan, -0.f, 0.f, 1.f, -nan, -1.f, 0.f, 5.f };
        const uint32_t st[4] = { 1, 1, 9, 9 };
        F t = F::copy(v, 10);
        U ts = U::copy(st, 4);
        CHECK((host(segment_argsort(t, ts)) == std::vector<uint32_t>{ 0, 6, 2, 3, 7, 0, 4, 1, 5, 0 }));
        CHECK((host(segment_argsort(t, ts, true)) == std::vector<uint32_t>{ 0, 0, 4, 2, 3, 7, 6, 1, 5, 0 }));
        CHECK((host(segment_argsort(t, ts, false, true)) == std::vector<uint32_t>{ 0, 7, 3, 4, 8, 1, 5, 2, 6, 9 }));
    }
    hip_set_defer(false);
}

static void on_the_tape() {
    const size_t n = 200;
    const std::vector<uint32_t> hs = { 2, 2, 5, 6, 40, 40, 41, 150, 200, 230 };
    const size_t m = hs.size();
    // (a triangle wave: the segments are not sorted, and every segment has its own order)
    std::vector<float> hx_(n);
    for (size_t i = 0; i < n; ++i) hx_[i] = std::fabs(float((i * 7) % 11) - 5.f) + 0.01f * float(i % 5);
    F hx = F::copy(hx_.data(), n), hw = linspace<F>(1.f, 2.f, n), hv = linspace<F>(2.f, 3.f, n);
    const std::vector<float> ones(n, 1.f);
    const size_t live = g_live.size();
    {
        DU starts = DU(U::copy(hs.data(), m));
        for (int desc = 0; desc < 2; ++desc) {
            const std::vector<uint32_t> p = sorted_perm(hx_, hs, desc);
            // one node of the source's size, made by ONE call that wrote values and permutation; backward scatters the weights
            {
                D x = D(hx);
                set_requires_gradient(x);
                const size_t nodes = Tape<F>::get()->node_count();
                const long c0 = g_sort_calls, v0 = g_value_outputs, i0 = g_index_outputs;
                D s = segment_sort(x, starts, desc);
                CHECK(g_sort_calls == c0 + 1 && g_value_outputs == v0 + 1 && g_index_outputs == i0 + 1);
                CHECK(Tape<F>::get()->node_count() == nodes + 1 && s.index_() != 0 && s.size() == n);
                CHECK(host(detach(s)) == taken(hx_, p));
                D y = hsum(s * D(hw));
                backward(y);
                CHECK(g_sort_calls == c0 + 1);                                  // the sweep sorts nothing again
                CHECK(taken(host(gradient(x)), p) == host(hw));                 // gradient(x)[p] == w, bit for bit
                CHECK(starts.index_() == 0 && throws([&] { (void) gradient(starts); }));   // the starts stay untracked
            }
            // ... and from the size-1 seed of backward(hsum(segment_sort(x))): ones
            {
                D x = D(hx);
                set_requires_gradient(x);
                D y = hsum(segment_sort(x, starts, desc));
                backward(y);
                CHECK(host(gradient(x)) == ones);
            }
            // forward: the size-1 seed of forward(x) stands for n ones; an array seed arrives as seed[p]
            {
                D x = D(hx);
                set_requires_gradient(x);
                D s = segment_sort(x, starts, desc);
                forward(x);
                CHECK(host(gradient(s)) == ones);
            }
            {
                D x = D(hx);
                set_requires_gradient(x);
                D s = segment_sort(x, starts, desc);
                set_gradient(x, hv, false);
                forward<D>();
                CHECK(host(gradient(s)) == taken(host(hv), p));
            }
            // the two sweeps transpose each other: <w, gather(v, p)> == <scatter(w, p), v> on small integers
            {
                std::vector<float> vi(n), wi(n), sc(n, 0.f);
                for (size_t i = 0; i < n; ++i) { vi[i] = (float) ((int) (i * 7 % 13) - 6); wi[i] = (float) ((int) (i * 5 % 7) - 3); }
                double lhs = 0, rhs = 0;
                for (size_t i = 0; i < n; ++i) { lhs += (double) wi[i] * vi[p[i]]; sc[p[i]] += wi[i]; }
                for (size_t i = 0; i < n; ++i) rhs += (double) sc[i] * vi[i];
                CHECK(lhs == rhs);
                D x = D(hx);
                set_requires_gradient(x);
                D s = segment_sort(x, starts, desc);
                set_gradient(x, F::copy(vi.data(), n), false);
                forward<D>();
                const std::vector<float> fwd = host(gradient(s));               // gather(v, p)
                D x2 = D(hx);
                set_requires_gradient(x2);
                D y = hsum(segment_sort(x2, starts, desc) * D(F::copy(wi.data(), n)));
                backward(y);
                const std::vector<float> bwd = host(gradient(x2));              // scatter(w, p)
                double l2 = 0, r2 = 0;
                for (size_t i = 0; i < n; ++i) { l2 += (double) wi[i] * fwd[i]; r2 += (double) bwd[i] * vi[i]; }
                CHECK(l2 == lhs && r2 == lhs && bwd == sc);
            }
            // segment_argsort of a tracked array: an index array, no node, index only
            {
                D x = D(hx);
                set_requires_gradient(x);
                const size_t nodes = Tape<F>::get()->node_count();
                const long c0 = g_sort_calls, v0 = g_value_outputs;
                auto q = segment_argsort(x, starts, desc, true);
                CHECK(Tape<F>::get()->node_count() == nodes && g_sort_calls == c0 + 1 && g_value_outputs == v0);
                CHECK(q.index_() == 0 && host(detach(q)) == p);
                CHECK(host(detach(segment_argsort(x, starts, desc))) == local_of(p, hs));
            }
        }
        // an untracked array records nothing and asks for values only
        {
            D plain_x = D(hx);
            const size_t nodes = Tape<F>::get()->node_count();
            const long i0 = g_index_outputs;
            D s = segment_sort(plain_x, starts);
            CHECK(s.index_() == 0 && Tape<F>::get()->node_count() == nodes && g_index_outputs == i0 && s.size() == n);
        }
    }
    // the node keeps the permutation while it lives (not the starts) and releases it with its edge
    {
        D x = D(hx);
        set_requires_gradient(x);
        const size_t before = g_live.size();
        D s;
        {
            DU starts = DU(U::copy(hs.data(), m));
            s = segment_sort(x, starts, true);
        }
        CHECK(g_live.size() == before + 2);                       // the sorted values and the permutation, which only the node holds
        D y = hsum(s * D(hw));
        backward(y);
        CHECK(taken(host(gradient(x)), sorted_perm(hx_, hs, true)) == host(hw));
        s = D();
        y = D();
    }
    CHECK(g_live.size() == live);
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("segment_sort_host: operands evaluated once, no entries make no call, a wrong starts type refused, one call serves values and "
           "permutation, one tape node for segment_sort and none for segment_argsort, sweeps transpose, permutation released, %ld calls, "
           "no block left allocated\n", g_sort_calls);
    return 0;
}
#endif
