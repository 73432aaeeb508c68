// block_sort / block_argsort (include/enoki/array.h) down to the C-ABI call and through the tape, on the host stand-in of the C ABI
// (host_abi_stub.h), without a GPU: a stand-alone program with its own main; tests/test_block_sort_host.py builds and runs it (also
// under -fsanitize=address,undefined).  The stand-in does not define ek_hip_sort_blocks; this file does, as std::stable_sort.
//
//   * an unevaluated operand (a unary map) is evaluated once, then the one call is made;
//   * a bad block size throws before the C ABI is reached (and before the operand is evaluated);
//   * one call serves values and permutation: block_sort of a tracked DiffArray makes ONE call with both outputs, block_sort of a
//     plain array one call with values only, block_argsort one call with the index only;
//   * block_sort of a tracked DiffArray records exactly one node of the source's size, block_argsort none; backward scatters the
//     weights through the permutation (gradient(x)[p] == w), forward gathers the seed (seed[p]), size-1 seeds included;
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
    Bare b;
    bool sort_thrown = false, argsort_thrown = false;
    try { (void) enoki::block_sort(b, 2, true); }
    catch (const std::runtime_error &e) { sort_thrown = std::string(e.what()) == "block_sort(): not available for this array type"; }
    try { enoki::block_argsort(b, 2, false, true); }
    catch (const std::runtime_error &e) { argsort_thrown = std::string(e.what()) == "block_argsort(): not available for this array type"; }
    CHECK(sort_thrown && argsort_thrown);
    printf("block_sort_host: a type without the members compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

/// the definition: per row the stable order by < (by > when descending), every NaN last; row-local positions
static std::vector<uint32_t> sorted_perm(const std::vector<float> &x, size_t block, bool descending) {
    std::vector<uint32_t> p(x.size());
    for (size_t j = 0; j < x.size() / block; ++j) {
        const float *row = x.data() + j * block;
        uint32_t *q = p.data() + j * block;
        std::iota(q, q + block, 0u);
        std::stable_sort(q, q + block, [&](uint32_t a, uint32_t b) {
            if (std::isnan(row[a]) || std::isnan(row[b])) return !std::isnan(row[a]) && std::isnan(row[b]);
            return descending ? row[a] > row[b] : row[a] < row[b];
        });
    }
    return p;
}

static std::vector<uint32_t> flat_of(std::vector<uint32_t> p, size_t block) {
    for (size_t i = 0; i < p.size(); ++i) p[i] += (uint32_t) (i / block * block);
    return p;
}

template <typename V> static std::vector<V> taken(const std::vector<V> &x, const std::vector<uint32_t> &flat) {
    std::vector<V> r(x.size());
    for (size_t i = 0; i < x.size(); ++i) r[i] = x[flat[i]];
    return r;
}

#ifndef NO_ENTRY
static long g_sort_calls = 0, g_value_outputs = 0, g_index_outputs = 0;

extern "C" int ek_hip_sort_blocks(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, size_t block, int flags) {
    ++g_sort_calls;
    g_value_outputs += out_values != nullptr;
    g_index_outputs += out_index != nullptr;
    if (type != EK_F32) STUB_UNSUPPORTED("sort_blocks", type, flags);
    if (block == 0 || n % block || (flags & ~3) || (!out_values && !out_index) || !in) {
        fprintf(stderr, "stand-in: a bad block size, flag or pointer reached the C ABI\n");
        abort();
    }
    const std::vector<float> x((const float *) in, (const float *) in + n);
    const std::vector<uint32_t> local = sorted_perm(x, block, flags & EK_SORT_DESCENDING), flat = flat_of(local, block);
    if (out_values) {
        const std::vector<float> v = taken(x, flat);
        memcpy(out_values, v.data(), n * sizeof(float));
    }
    if (out_index) memcpy(out_index, ((flags & EK_SORT_FLAT_INDEX) ? flat : local).data(), n * sizeof(uint32_t));
    return EK_OK;
}
extern "C" int ek_hip_sort_blocks_plan(int, size_t, size_t, int, int, int *route, size_t *tile_rows, size_t *chunk, int *merge_passes,
                                       size_t *workgroups) {
    *route = 1; *tile_rows = 1; *chunk = 8192; *merge_passes = 0; *workgroups = 1;
    return EK_OK;
}
#endif

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using D = DiffArray<F>;

static constexpr size_t B = 5, M = 1 << 14, N = B * M;      // (N: what a unary map needs to stay unevaluated)

template <typename A> static auto host(const A &a) {
    std::vector<std::decay_t<decltype(a.coeff(0))>> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}

template <typename Fn> static bool throws(Fn &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

#ifdef NO_ENTRY
int main() {
    F x = linspace<F>(-4.f, 4.f, 12);
    bool named = false, named2 = false;
    try { (void) block_sort(x, 3); }
    catch (const std::runtime_error &e) { named = std::string(e.what()).find("this C ABI has no entry ek_hip_sort_blocks") != std::string::npos; }
    try { (void) block_argsort(x, 3); }
    catch (const std::runtime_error &e) { named2 = std::string(e.what()).find("this C ABI has no entry ek_hip_sort_blocks") != std::string::npos; }
    CHECK(named && named2);
    // ... but a bad block is refused first
    bool bad = false;
    try { (void) block_sort(x, 5); }
    catch (const std::runtime_error &e) { bad = std::string(e.what()).find("no whole number of blocks") != std::string::npos; }
    CHECK(bad);
    x = F();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("block_sort_host: without the entry the members throw and name it\n");
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
        F r = block_sort(s, B);
        CHECK(g_unary_calls == u0 + 1 && g_sort_calls == c0 + 1 && !s.mapped_() && r.size() == N);
        CHECK(g_value_outputs == v0 + 1 && g_index_outputs == i0);                // values only: no index is computed or allocated
        U p = block_argsort(s, B, true, true);
        CHECK(g_unary_calls == u0 + 1 && g_sort_calls == c0 + 2 && p.size() == N);
        CHECK(g_value_outputs == v0 + 1 && g_index_outputs == i0 + 1);            // index only
        const std::vector<float> hs = host(s);
        CHECK(host(r) == taken(hs, flat_of(sorted_perm(hs, B, false), B)));
        CHECK(host(p) == flat_of(sorted_perm(hs, B, true), B));
        CHECK(host(block_argsort(s, B)) == sorted_perm(hs, B, false));
        CHECK(host(block_sort(s, B, true)) == taken(hs, flat_of(sorted_perm(hs, B, true), B)));
    }
    // (2) a bad block size throws before the C ABI is reached and before the operand is evaluated
    {
        F s = sin(x);
        const long u0 = g_unary_calls, c0 = g_sort_calls;
        CHECK(throws([&] { (void) block_sort(s, 0); }) && throws([&] { (void) block_sort(s, 7, true); }) &&
              throws([&] { (void) block_argsort(s, N + 1, false, true); }) && throws([&] { (void) block_argsort(s, 0); }));
        CHECK(g_unary_calls == u0 && g_sort_calls == c0 && s.mapped_());
    }
    // (3) a host scalar is an array of one entry; an empty array stays empty without a call
    {
        const long c0 = g_sort_calls;
        F one = block_sort(F(2.5f), 1);
        CHECK(one.size() == 1 && one.coeff(0) == 2.5f && throws([&] { (void) block_sort(F(2.5f), 2); }));
        U zero = block_argsort(F(2.5f), 1, false, true);
        CHECK(zero.size() == 1 && zero.coeff(0) == 0u);
        F none;
        CHECK(block_sort(none, 3).size() == 0 && block_argsort(none, 3).size() == 0);
        CHECK(g_sort_calls == c0 + 2);
    }
    // (4) ties keep their input order, NaNs come last in both directions
    {
        const float nan = std::nanf("");
        const float v[8] = { 1.f, nan, -0.f, 0.f, 1.f, -nan, -1.f, 0.f };
        F t = F::copy(v, 8);
        CHECK((host(block_argsort(t, 8)) == std::vector<uint32_t>{ 6, 2, 3, 7, 0, 4, 1, 5 }));
        CHECK((host(block_argsort(t, 8, true)) == std::vector<uint32_t>{ 0, 4, 2, 3, 7, 6, 1, 5 }));
        CHECK((host(block_argsort(t, 4, false, true)) == std::vector<uint32_t>{ 2, 3, 0, 1, 6, 7, 4, 5 }));
    }
    hip_set_defer(false);
}

static void on_the_tape() {
    const size_t m = 64, b = 3, n = m * b;
    // (a triangle wave: the rows are not sorted, and every row has its own order)
    std::vector<float> hx_(n);
    for (size_t i = 0; i < n; ++i) hx_[i] = std::fabs(float((i * 7) % 11) - 5.f) + 0.01f * float(i % 5);
    F hx = F::copy(hx_.data(), n), hw = linspace<F>(1.f, 2.f, n), hv = linspace<F>(2.f, 3.f, n);
    const std::vector<float> ones(n, 1.f);
    for (int desc = 0; desc < 2; ++desc) {
        const std::vector<uint32_t> p = flat_of(sorted_perm(hx_, b, desc), b);
        // one node of the source's size, made by ONE call that wrote values and permutation; backward scatters the weights
        {
            D x = D(hx);
            set_requires_gradient(x);
            const size_t nodes = Tape<F>::get()->node_count();
            const long c0 = g_sort_calls, v0 = g_value_outputs, i0 = g_index_outputs;
            D s = block_sort(x, b, desc);
            CHECK(g_sort_calls == c0 + 1 && g_value_outputs == v0 + 1 && g_index_outputs == i0 + 1);
            CHECK(Tape<F>::get()->node_count() == nodes + 1 && s.index_() != 0 && s.size() == n);
            CHECK(host(detach(s)) == taken(hx_, p));
            D y = hsum(s * D(hw));
            backward(y);
            CHECK(g_sort_calls == c0 + 1);                                  // the sweep sorts nothing again
            CHECK(taken(host(gradient(x)), p) == host(hw));                 // gradient(x)[p] == w, bit for bit
        }
        // ... and from the size-1 seed of backward(hsum(block_sort(x))): ones
        {
            D x = D(hx);
            set_requires_gradient(x);
            D y = hsum(block_sort(x, b, desc));
            backward(y);
            CHECK(host(gradient(x)) == ones);
        }
        // forward: the size-1 seed of forward(x) stands for n ones; an array seed arrives as seed[p]
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = block_sort(x, b, desc);
            forward(x);
            CHECK(host(gradient(s)) == ones);
        }
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = block_sort(x, b, desc);
            set_gradient(x, hv, false);
            forward<D>();
            CHECK(host(gradient(s)) == taken(host(hv), p));
        }
        // block_argsort of a tracked array: an index array, no node, index only
        {
            D x = D(hx);
            set_requires_gradient(x);
            const size_t nodes = Tape<F>::get()->node_count();
            const long c0 = g_sort_calls, v0 = g_value_outputs;
            auto q = block_argsort(x, b, desc, true);
            CHECK(Tape<F>::get()->node_count() == nodes && g_sort_calls == c0 + 1 && g_value_outputs == v0);
            CHECK(q.index_() == 0 && host(detach(q)) == p);
        }
    }
    // an untracked array records nothing and asks for values only; a bad block on a tracked one throws
    {
        D plain_x = D(hx);
        const size_t nodes = Tape<F>::get()->node_count();
        const long i0 = g_index_outputs;
        D s = block_sort(plain_x, b);
        CHECK(s.index_() == 0 && Tape<F>::get()->node_count() == nodes && g_index_outputs == i0);
        D x = D(hx);
        set_requires_gradient(x);
        CHECK(throws([&] { (void) block_sort(x, 7); }) && throws([&] { (void) block_argsort(x, 0); }));
    }
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("block_sort_host: operands evaluated once, bad blocks refused, one call serves values and permutation, one tape node for "
           "block_sort and none for block_argsort, gradients permuted, %ld calls, no block left allocated\n", g_sort_calls);
    return 0;
}
#endif
#endif
