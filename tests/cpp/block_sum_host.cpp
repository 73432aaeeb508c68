// block_sum / block_prod / block_min / block_max / repeat (include/enoki/array.h) down to the C-ABI calls and through the tape, on
// the host stand-in of the C ABI (host_abi_stub.h), without a GPU: a stand-alone program with its own main;
// tests/test_block_sum_host.py builds and runs it (also under -fsanitize=address,undefined).  The stand-in does not define
// ek_hip_reduce_blocks and ek_hip_repeat; this file does, as plain host loops.
//
//   * an unevaluated operand (a unary map) is evaluated once, then the one call is made;
//   * a bad block size throws before the C ABI is reached (and before the operand is evaluated);
//   * block_sum of a tracked DiffArray records one node of n / B entries; backward gives repeat(w), forward block_sum(seed), both
//     also from a size-1 seed; repeat is the mirror image;
//   * block_max of a tracked array throws, of an untracked one computes;
//   * -DBARE_TYPE: a flat array type WITHOUT the members compiles and throws at run time;
//   * no block stays allocated.
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
// a second, tiny translation unit: the free functions on an array type that has no block_sum_ / repeat_ members
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

template <typename F> static bool throws_unavailable(F &&f, const char *name) {
    try { f(); } catch (const std::runtime_error &e) { return std::string(e.what()) == std::string(name) + "(): not available for this array type"; }
    return false;
}

int main() {
    Bare b;
    CHECK(throws_unavailable([&] { (void) enoki::block_sum(b, 2); }, "block_sum"));
    CHECK(throws_unavailable([&] { (void) enoki::block_prod(b, 2); }, "block_prod"));
    CHECK(throws_unavailable([&] { (void) enoki::block_min(b, 2); }, "block_min"));
    CHECK(throws_unavailable([&] { (void) enoki::block_max(b, 2); }, "block_max"));
    CHECK(throws_unavailable([&] { (void) enoki::repeat(b, 2); }, "repeat"));
    printf("block_sum_host: a type without the members compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_block_calls = 0, g_repeat_calls = 0;

extern "C" int ek_hip_reduce_blocks(int op, int type, void *out, const void *in, size_t n, size_t block) {
    ++g_block_calls;
    if (type != EK_F32) STUB_UNSUPPORTED("reduce_blocks", type, op);
    if (block == 0 || n % block) { fprintf(stderr, "stand-in: a bad block size reached the C ABI\n"); abort(); }
    const float *x = (const float *) in;
    for (size_t j = 0; j < n / block; ++j) {
        float acc = x[j * block];
        for (size_t k = 1; k < block; ++k) {
            const float v = x[j * block + k];
            acc = op == EK_HSUM ? acc + v : op == EK_HPROD ? acc * v : op == EK_HMIN ? fminf(acc, v) : fmaxf(acc, v);
        }
        ((float *) out)[j] = acc;
    }
    return EK_OK;
}
extern "C" int ek_hip_repeat(int type, void *out, const void *in, size_t m, size_t block) {
    ++g_repeat_calls;
    if (type != EK_F32) STUB_UNSUPPORTED("repeat", type, 0);
    if (block == 0) { fprintf(stderr, "stand-in: a bad block size reached the C ABI\n"); abort(); }
    for (size_t i = 0; i < m * block; ++i) ((float *) out)[i] = ((const float *) in)[i / block];
    return EK_OK;
}
extern "C" int ek_hip_reduce_blocks_plan(int, size_t, size_t, int, int *regime, int *splits, size_t *workgroups) {
    *regime = 2; *splits = 1; *workgroups = 1;
    return EK_OK;
}

using namespace enoki;
using F = HIPArray<float>;
using D = DiffArray<F>;

static constexpr size_t B = 5, M = 1 << 14, N = B * M;      // (N: what a unary map needs to stay unevaluated)

template <typename A> static std::vector<float> host(const A &a) {
    std::vector<float> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}

static std::vector<float> sums(const std::vector<float> &x, size_t block) {
    std::vector<float> r(x.size() / block);
    for (size_t j = 0; j < r.size(); ++j) {
        float acc = x[j * block];
        for (size_t k = 1; k < block; ++k) acc += x[j * block + k];
        r[j] = acc;
    }
    return r;
}

static std::vector<float> repeated(const std::vector<float> &x, size_t block) {
    std::vector<float> r(x.size() * block);
    for (size_t i = 0; i < r.size(); ++i) r[i] = x[i / block];
    return r;
}

template <typename Fn> static bool throws(Fn &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

static void plain() {
    F x = linspace<F>(-4.f, 4.f, N);
    (void) x.data();
    hip_set_defer(true);
    // (1) an unevaluated operand: one unary launch, one call -- and nothing again for the second call
    {
        F s = sin(x);
        CHECK(s.mapped_());
        const long u0 = g_unary_calls, b0 = g_block_calls;
        F r = block_sum(s, B);
        CHECK(g_unary_calls == u0 + 1 && g_block_calls == b0 + 1 && !s.mapped_() && r.size() == M);
        F r2 = block_max(s, B);
        CHECK(g_unary_calls == u0 + 1 && g_block_calls == b0 + 2);
        CHECK(host(r) == sums(host(s), B));
        F c = cos(x);
        const long r0 = g_repeat_calls, u1 = g_unary_calls;
        F rep = repeat(c, 3);
        CHECK(g_unary_calls == u1 + 1 && g_repeat_calls == r0 + 1 && rep.size() == 3 * N && host(rep) == repeated(host(c), 3));
    }
    // (2) a bad block size throws before the C ABI is reached and before the operand is evaluated
    {
        F s = sin(x);
        const long u0 = g_unary_calls, b0 = g_block_calls, r0 = g_repeat_calls;
        CHECK(throws([&] { (void) block_sum(s, 0); }) && throws([&] { (void) block_sum(s, 7); }) && throws([&] { (void) block_min(s, N + 1); }));
        CHECK(throws([&] { (void) repeat(s, 0); }));
        CHECK(g_unary_calls == u0 && g_block_calls == b0 && g_repeat_calls == r0 && s.mapped_());
    }
    // (3) a host scalar is an array of one entry; an empty array stays empty without a call
    {
        const long b0 = g_block_calls, r0 = g_repeat_calls;
        F one = block_sum(F(2.5f), 1);
        CHECK(one.size() == 1 && one.coeff(0) == 2.5f && throws([&] { (void) block_sum(F(2.5f), 2); }));
        F four = repeat(F(2.5f), 4);
        CHECK(four.size() == 4 && four.coeff(3) == 2.5f);
        F none;
        CHECK(block_sum(none, 3).size() == 0 && repeat(none, 3).size() == 0);
        CHECK(g_block_calls == b0 + 1 && g_repeat_calls == r0 + 1);
    }
    hip_set_defer(false);
}

static void on_the_tape() {
    const size_t m = 64, b = 3, n = m * b;
    F hx = linspace<F>(-1.f, 1.f, n), hw = linspace<F>(1.f, 2.f, m), hv = linspace<F>(2.f, 3.f, n);
    // block_sum: one node of n / b entries; backward gives repeat(w)
    {
        D x = D(hx);
        set_requires_gradient(x);
        const size_t nodes = Tape<F>::get()->node_count();
        D s = block_sum(x, b);
        CHECK(Tape<F>::get()->node_count() == nodes + 1 && s.index_() != 0 && s.size() == m);
        CHECK(host(detach(s)) == sums(host(hx), b));
        D y = hsum(s * D(hw));
        backward(y);
        CHECK(host(gradient(x)) == repeated(host(hw), b));
    }
    // ... and from the size-1 seed of backward(hsum(block_sum(x))): all ones
    {
        D x = D(hx);
        set_requires_gradient(x);
        D y = hsum(block_sum(x, b));
        backward(y);
        CHECK(host(gradient(x)) == std::vector<float>(n, 1.f));
    }
    // forward through block_sum: the size-1 seed of forward(x) gives b per block, an array seed its block sums
    {
        D x = D(hx);
        set_requires_gradient(x);
        D s = block_sum(x, b);
        forward(x);
        CHECK(host(gradient(s)) == std::vector<float>(m, (float) b));
    }
    {
        D x = D(hx);
        set_requires_gradient(x);
        D s = block_sum(x, b);
        set_gradient(x, hv, false);
        forward<D>();
        CHECK(host(gradient(s)) == sums(host(hv), b));
    }
    // repeat is the mirror image: one node of m * b entries, backward gives block_sum(v), forward repeat(seed)
    {
        D a = D(hw);
        set_requires_gradient(a);
        const size_t nodes = Tape<F>::get()->node_count();
        D r = repeat(a, b);
        CHECK(Tape<F>::get()->node_count() == nodes + 1 && r.index_() != 0 && r.size() == n);
        CHECK(host(detach(r)) == repeated(host(hw), b));
        D y = hsum(r * D(hv));
        backward(y);
        CHECK(host(gradient(a)) == sums(host(hv), b));
    }
    {
        D a = D(hw);
        set_requires_gradient(a);
        D y = hsum(repeat(a, b));
        backward(y);
        CHECK(host(gradient(a)) == std::vector<float>(m, (float) b));
    }
    {
        D a = D(hw);
        set_requires_gradient(a);
        D r = repeat(a, b);
        forward(a);
        CHECK(host(gradient(r)) == std::vector<float>(n, 1.f));
    }
    // no gradient for the other three: a tracked array throws, an untracked one computes
    {
        D x = D(hx);
        set_requires_gradient(x);
        CHECK(throws([&] { (void) block_max(x, b); }) && throws([&] { (void) block_min(x, b); }) && throws([&] { (void) block_prod(x, b); }));
        D plain_x = D(hx);
        D mx = block_max(plain_x, b);
        CHECK(mx.index_() == 0 && mx.size() == m && mx.coeff(0) == hx.coeff(b - 1));
        CHECK(throws([&] { (void) block_sum(x, 7); }));
    }
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("block_sum_host: operands evaluated once, bad blocks refused, tape nodes transpose, %ld + %ld calls, no block left allocated\n",
           g_block_calls, g_repeat_calls);
    return 0;
}
#endif
