// sort / argsort (include/enoki/array.h) down to the C-ABI call and through the tape, on the host stand-in of the C ABI
// (host_abi_stub.h), without a GPU: a stand-alone program with its own main; tests/test_sort_host.py builds and runs it (also under
// -fsanitize=address,undefined).  The stand-in does not define ek_hip_sort; this file does, as std::stable_sort.
//
//   * an unevaluated operand (a unary map) is evaluated once, then the one call is made;
//   * one call serves values and permutation: sort of a tracked DiffArray makes ONE call with both outputs, sort of a plain array
//     one call with values only, argsort one call with the index only -- an output that was not requested is not passed;
//   * sort of a tracked DiffArray records exactly one node of the source's size, argsort none; backward scatters the weights
//     through the permutation (gradient(x)[p] == w), forward gathers the seed (seed[p]), size-1 seeds included;
//   * more than 2^32 - 1 entries are refused before the C ABI is reached;
//   * an unqualified sort(first, last, cmp) over a std::vector of arrays still means std::sort;
//   * -DNO_ENTRY: without the entry in the C ABI the members throw and say which entry is missing;
//   * -DBARE_TYPE: a flat array type WITHOUT the members compiles and throws at run time;
//   * no block stays allocated.
#include <enoki/hip.h>
#include <enoki/autodiff.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

#ifdef BARE_TYPE
// a second, tiny translation unit: the free functions on an array type that has neither member
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

int main() {
    Bare b;
    bool sort_thrown = false, argsort_thrown = false;
    try { (void) enoki::sort(b, true); }
    catch (const std::runtime_error &e) { sort_thrown = std::string(e.what()) == "sort(): not available for this array type"; }
    try { enoki::argsort(b); }
    catch (const std::runtime_error &e) { argsort_thrown = std::string(e.what()) == "argsort(): not available for this array type"; }
    CHECK(sort_thrown && argsort_thrown);
    printf("sort_host: a type without the members compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

/// the definition: the stable order by < (by > when descending), every NaN last
static std::vector<uint32_t> sorted_perm(const std::vector<float> &x, bool descending) {
    std::vector<uint32_t> p(x.size());
    std::iota(p.begin(), p.end(), 0u);
    std::stable_sort(p.begin(), p.end(), [&](uint32_t a, uint32_t b) {
        if (std::isnan(x[a]) || std::isnan(x[b])) return !std::isnan(x[a]) && std::isnan(x[b]);
        return descending ? x[a] > x[b] : x[a] < x[b];
    });
    return p;
}

template <typename V> static std::vector<V> taken(const std::vector<V> &x, const std::vector<uint32_t> &p) {
    std::vector<V> r(x.size());
    for (size_t i = 0; i < x.size(); ++i) r[i] = x[p[i]];
    return r;
}

#ifndef NO_ENTRY
static long g_sort_calls = 0, g_value_outputs = 0, g_index_outputs = 0;

extern "C" int ek_hip_sort(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, int flags) {
    ++g_sort_calls;
    g_value_outputs += out_values != nullptr;
    g_index_outputs += out_index != nullptr;
    if (type != EK_F32) STUB_UNSUPPORTED("sort", type, flags);
    if (n == 0 || n > 0xFFFFFFFFull || (flags & ~3) || (!out_values && !out_index) || !in) {
        fprintf(stderr, "stand-in: a bad size, flag or pointer reached the C ABI\n");
        abort();
    }
    const std::vector<float> x((const float *) in, (const float *) in + n);
    const std::vector<uint32_t> p = sorted_perm(x, flags & EK_SORT_DESCENDING);
    if (out_values) {
        const std::vector<float> v = taken(x, p);
        memcpy(out_values, v.data(), n * sizeof(float));
    }
    if (out_index) memcpy(out_index, p.data(), n * sizeof(uint32_t));
    return EK_OK;
}
extern "C" int ek_hip_sort_plan(int, size_t, int, int, int *route, int *passes, size_t *tile, size_t *tiles_per_workgroup, size_t *workgroups,
                                int *launches, size_t *scratch_bytes) {
    *route = 1; *passes = 0; *tile = 8192; *tiles_per_workgroup = 0; *workgroups = 1; *launches = 1; *scratch_bytes = 0;
    return EK_OK;
}
#endif

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using D = DiffArray<F>;

static constexpr size_t N = 5 << 14;      // (what a unary map needs to stay unevaluated)

template <typename A> static auto host(const A &a) {
    std::vector<std::decay_t<decltype(a.coeff(0))>> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}

template <typename Fn> static bool throws(Fn &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

/// An unqualified call over iterators into a container of arrays: argument-dependent lookup finds enoki::sort through the
/// iterator's template arguments, and the call must still be std::sort (found the same way through std::vector).
template <typename A> static void std_sort_still_compiles() {
    std::vector<A> v;
    v.push_back(A(linspace<F>(0.f, 1.f, 3)));
    v.push_back(A(linspace<F>(0.f, 1.f, 2)));
    v.push_back(A(linspace<F>(0.f, 1.f, 5)));
    sort(v.begin(), v.end(), [](const A &a, const A &b) { return a.size() < b.size(); });
    CHECK(v[0].size() == 2 && v[1].size() == 3 && v[2].size() == 5);
}

#ifdef NO_ENTRY
int main() {
    F x = linspace<F>(-4.f, 4.f, 12);
    bool named = false, named2 = false;
    try { (void) sort(x); }
    catch (const std::runtime_error &e) { named = std::string(e.what()).find("this C ABI has no entry ek_hip_sort") != std::string::npos; }
    try { (void) argsort(x, true); }
    catch (const std::runtime_error &e) { named2 = std::string(e.what()).find("this C ABI has no entry ek_hip_sort") != std::string::npos; }
    CHECK(named && named2);
    {
        D d = D(x);
        set_requires_gradient(d);
        CHECK(throws([&] { (void) sort(d); }) && throws([&] { (void) argsort(d); }));
    }
    std_sort_still_compiles<F>();
    x = F();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("sort_host: without the entry the members throw and name it\n");
    return 0;
}
#else

static void plain() {
    F x = linspace<F>(-4.f, 4.f, N);
    (void) x.data();
    hip_set_defer(true);
    // (1) an unevaluated operand: one unary launch, one call -- and nothing again for the second call
    {
        F s = sin(x);
        CHECK(s.mapped_());
        const long u0 = g_unary_calls, c0 = g_sort_calls, v0 = g_value_outputs, i0 = g_index_outputs;
        F r = sort(s);
        CHECK(g_unary_calls == u0 + 1 && g_sort_calls == c0 + 1 && !s.mapped_() && r.size() == N);
        CHECK(g_value_outputs == v0 + 1 && g_index_outputs == i0);                // values only: no index is passed or allocated
        U p = argsort(s, true);
        CHECK(g_unary_calls == u0 + 1 && g_sort_calls == c0 + 2 && p.size() == N);
        CHECK(g_value_outputs == v0 + 1 && g_index_outputs == i0 + 1);            // index only
        const std::vector<float> hs = host(s);
        CHECK(host(r) == taken(hs, sorted_perm(hs, false)));
        CHECK(host(p) == sorted_perm(hs, true));
        CHECK(host(argsort(s)) == sorted_perm(hs, false));
        CHECK(host(sort(s, true)) == taken(hs, sorted_perm(hs, true)));
    }
    // (2) a host scalar is an array of one entry; an empty array stays empty without a call
    {
        const long c0 = g_sort_calls;
        F one = sort(F(2.5f));
        CHECK(one.size() == 1 && one.coeff(0) == 2.5f);
        U zero = argsort(F(2.5f), true);
        CHECK(zero.size() == 1 && zero.coeff(0) == 0u);
        F none;
        CHECK(sort(none).size() == 0 && argsort(none).size() == 0 && sort(none, true).size() == 0);
        CHECK(g_sort_calls == c0 + 2);
    }
    // (3) ties keep their input order, NaNs come last in both directions
    {
        const float nan = std::nanf("");
        const float v[8] = { 1.f, nan, -0.f, 0.f, 1.f, -nan, -1.f, 0.f };
        F t = F::copy(v, 8);
        CHECK((host(argsort(t)) == std::vector<uint32_t>{ 6, 2, 3, 7, 0, 4, 1, 5 }));
        CHECK((host(argsort(t, true)) == std::vector<uint32_t>{ 0, 4, 2, 3, 7, 6, 1, 5 }));
        const std::vector<float> sv = host(sort(t));
        CHECK(std::signbit(sv[1]) && !std::signbit(sv[2]) && std::isnan(sv[6]) && !std::signbit(sv[6]) && std::signbit(sv[7]));
    }
    // (4) more than 2^32 - 1 entries: refused by the member before the C ABI is reached.  The array is foreign memory that is never
    //     touched -- the size alone decides
    {
        static float one_entry = 0.f;
        const long c0 = g_sort_calls;
        F huge = F::map(&one_entry, (size_t) 1 << 32);
        bool said = false;
        try { (void) sort(huge); }
        catch (const std::runtime_error &e) { said = std::string(e.what()).find("more than 2^32 - 1") != std::string::npos; }
        CHECK(said && throws([&] { (void) argsort(huge, true); }) && g_sort_calls == c0);
    }
    hip_set_defer(false);
    std_sort_still_compiles<F>();
}

static void on_the_tape() {
    const size_t n = 192;
    // (a triangle wave with ties: not sorted)
    std::vector<float> hx_(n);
    for (size_t i = 0; i < n; ++i) hx_[i] = std::fabs(float((i * 7) % 11) - 5.f) + 0.01f * float(i % 5);
    F hx = F::copy(hx_.data(), n), hw = linspace<F>(1.f, 2.f, n), hv = linspace<F>(2.f, 3.f, n);
    const std::vector<float> ones(n, 1.f);
    for (int desc = 0; desc < 2; ++desc) {
        const std::vector<uint32_t> p = sorted_perm(hx_, desc);
        // one node of the source's size, made by ONE call that wrote values and permutation; backward scatters the weights
        {
            D x = D(hx);
            set_requires_gradient(x);
            const size_t nodes = Tape<F>::get()->node_count();
            const long c0 = g_sort_calls, v0 = g_value_outputs, i0 = g_index_outputs;
            D s = sort(x, desc);
            CHECK(g_sort_calls == c0 + 1 && g_value_outputs == v0 + 1 && g_index_outputs == i0 + 1);
            CHECK(Tape<F>::get()->node_count() == nodes + 1 && s.index_() != 0 && s.size() == n);
            CHECK(host(detach(s)) == taken(hx_, p));
            D y = hsum(s * D(hw));
            backward(y);
            CHECK(g_sort_calls == c0 + 1);                                  // the sweep sorts nothing again
            CHECK(taken(host(gradient(x)), p) == host(hw));                 // gradient(x)[p] == w, bit for bit
        }
        // ... and from the size-1 seed of backward(hsum(sort(x))): ones
        {
            D x = D(hx);
            set_requires_gradient(x);
            D y = hsum(sort(x, desc));
            backward(y);
            CHECK(host(gradient(x)) == ones);
        }
        // forward: the size-1 seed of forward(x) stands for n ones; an array seed arrives as seed[p]
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = sort(x, desc);
            forward(x);
            CHECK(host(gradient(s)) == ones);
        }
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = sort(x, desc);
            set_gradient(x, hv, false);
            forward<D>();
            CHECK(host(gradient(s)) == taken(host(hv), p));
        }
        // argsort of a tracked array: an index array, no node, index only
        {
            D x = D(hx);
            set_requires_gradient(x);
            const size_t nodes = Tape<F>::get()->node_count();
            const long c0 = g_sort_calls, v0 = g_value_outputs;
            auto q = argsort(x, desc);
            CHECK(Tape<F>::get()->node_count() == nodes && g_sort_calls == c0 + 1 && g_value_outputs == v0);
            CHECK(q.index_() == 0 && host(detach(q)) == p);
        }
    }
    // an untracked array records nothing and asks for values only
    {
        D plain_x = D(hx);
        const size_t nodes = Tape<F>::get()->node_count();
        const long i0 = g_index_outputs;
        D s = sort(plain_x);
        CHECK(s.index_() == 0 && Tape<F>::get()->node_count() == nodes && g_index_outputs == i0);
    }
    std_sort_still_compiles<D>();
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("sort_host: operands evaluated once, one call serves values and permutation, an output that was not requested is not passed, "
           "one tape node for sort and none for argsort, gradients permuted, too many entries refused, std::sort still compiles, "
           "%ld calls, no block left allocated\n", g_sort_calls);
    return 0;
}
#endif
#endif
