// block_psum (include/enoki/array.h) down to the C-ABI call and through the tape, on the host stand-in of the C ABI
// (host_abi_stub.h), without a GPU: a stand-alone program with its own main; tests/test_block_psum_host.py builds and runs it (also
// under -fsanitize=address,undefined).  The stand-in does not define ek_hip_psum_blocks; this file does, as plain host loops.
//
//   * an unevaluated operand (a unary map) is evaluated once, then the one call is made;
//   * a bad block size throws before the C ABI is reached (and before the operand is evaluated);
//   * block_psum of a tracked DiffArray records one node of the source's size; backward gives the direction-flipped scan of the
//     weights and forward the same scan of the seed, for all four flag combinations and from size-1 seeds;
//   * -DNO_ENTRY: without the entry in the C ABI the member throws and says which entry is missing;
//   * -DBARE_TYPE: a flat array type WITHOUT the member compiles and throws at run time;
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
// a second, tiny translation unit: the free function on an array type that has no block_psum_ member
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

int main() {
    Bare b;
    bool thrown = false;
    try { (void) enoki::block_psum(b, 2, true, false); }
    catch (const std::runtime_error &e) { thrown = std::string(e.what()) == "block_psum(): not available for this array type"; }
    CHECK(thrown);
    printf("block_psum_host: a type without the member compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

/// the definition in plain loops: sums run in scan order, an exclusive entry is the sum BEFORE its own term, the empty sum is +0
static std::vector<float> scanned(const std::vector<float> &x, size_t block, bool exclusive, bool reverse) {
    std::vector<float> r(x.size());
    for (size_t j = 0; j < x.size() / block; ++j) {
        float acc = 0.f;
        for (size_t k = 0; k < block; ++k) {
            const size_t i = j * block + (reverse ? block - 1 - k : k);
            const float incl = k == 0 ? x[i] : acc + x[i];
            r[i] = exclusive ? acc : incl;
            acc = incl;
        }
    }
    return r;
}

#ifndef NO_ENTRY
static long g_scan_calls = 0;

extern "C" int ek_hip_psum_blocks(int type, void *out, const void *in, size_t n, size_t block, int flags) {
    ++g_scan_calls;
    if (type != EK_F32) STUB_UNSUPPORTED("psum_blocks", type, flags);
    if (block == 0 || n % block || (flags & ~3)) { fprintf(stderr, "stand-in: a bad block size or flag reached the C ABI\n"); abort(); }
    const std::vector<float> x((const float *) in, (const float *) in + n);
    const std::vector<float> r = scanned(x, block, flags & EK_SCAN_EXCLUSIVE, flags & EK_SCAN_REVERSE);
    memcpy(out, r.data(), n * sizeof(float));
    return EK_OK;
}
extern "C" int ek_hip_psum_blocks_plan(int, size_t, size_t, int, int *regime, int *splits, size_t *workgroups) {
    *regime = 1; *splits = 1; *workgroups = 1;
    return EK_OK;
}
#endif

using namespace enoki;
using F = HIPArray<float>;
using D = DiffArray<F>;

static constexpr size_t B = 5, M = 1 << 14, N = B * M;      // (N: what a unary map needs to stay unevaluated)

template <typename A> static std::vector<float> host(const A &a) {
    std::vector<float> v(a.size());
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
    bool named = false;
    try { (void) block_psum(x, 3); }
    catch (const std::runtime_error &e) { named = std::string(e.what()).find("this C ABI has no entry ek_hip_psum_blocks") != std::string::npos; }
    CHECK(named);
    // ... but a bad block is refused first
    bool bad = false;
    try { (void) block_psum(x, 5); }
    catch (const std::runtime_error &e) { bad = std::string(e.what()).find("no whole number of blocks") != std::string::npos; }
    CHECK(bad);
    x = F();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("block_psum_host: without the entry the member throws and names it\n");
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
        const long u0 = g_unary_calls, c0 = g_scan_calls;
        F r = block_psum(s, B);
        CHECK(g_unary_calls == u0 + 1 && g_scan_calls == c0 + 1 && !s.mapped_() && r.size() == N);
        F r2 = block_psum(s, B, true, true);
        CHECK(g_unary_calls == u0 + 1 && g_scan_calls == c0 + 2);
        CHECK(host(r) == scanned(host(s), B, false, false) && host(r2) == scanned(host(s), B, true, true));
        CHECK(host(block_psum(s, B, true)) == scanned(host(s), B, true, false));
        CHECK(host(block_psum(s, B, false, true)) == scanned(host(s), B, false, true));
    }
    // (2) a bad block size throws before the C ABI is reached and before the operand is evaluated
    {
        F s = sin(x);
        const long u0 = g_unary_calls, c0 = g_scan_calls;
        CHECK(throws([&] { (void) block_psum(s, 0); }) && throws([&] { (void) block_psum(s, 7, true); }) &&
              throws([&] { (void) block_psum(s, N + 1, false, true); }));
        CHECK(g_unary_calls == u0 && g_scan_calls == c0 && s.mapped_());
    }
    // (3) a host scalar is an array of one entry; an empty array stays empty without a call
    {
        const long c0 = g_scan_calls;
        F one = block_psum(F(2.5f), 1);
        CHECK(one.size() == 1 && one.coeff(0) == 2.5f && throws([&] { (void) block_psum(F(2.5f), 2); }));
        F zero = block_psum(F(2.5f), 1, true);
        CHECK(zero.size() == 1 && zero.coeff(0) == 0.f);
        F none;
        CHECK(block_psum(none, 3).size() == 0);
        CHECK(g_scan_calls == c0 + 2);
    }
    hip_set_defer(false);
}

static void on_the_tape() {
    const size_t m = 64, b = 3, n = m * b;
    F hx = linspace<F>(-1.f, 1.f, n), hw = linspace<F>(1.f, 2.f, n), hv = linspace<F>(2.f, 3.f, n);
    const std::vector<float> ones(n, 1.f);
    for (int flags = 0; flags < 4; ++flags) {
        const bool excl = flags & 1, rev = flags & 2;
        // one node of the source's size; backward gives the scan of the weights from the other end
        {
            D x = D(hx);
            set_requires_gradient(x);
            const size_t nodes = Tape<F>::get()->node_count();
            D s = block_psum(x, b, excl, rev);
            CHECK(Tape<F>::get()->node_count() == nodes + 1 && s.index_() != 0 && s.size() == n);
            CHECK(host(detach(s)) == scanned(host(hx), b, excl, rev));
            D y = hsum(s * D(hw));
            backward(y);
            CHECK(host(gradient(x)) == scanned(host(hw), b, excl, !rev));
        }
        // ... and from the size-1 seed of backward(hsum(block_psum(x))): the scan of ones from the other end
        {
            D x = D(hx);
            set_requires_gradient(x);
            D y = hsum(block_psum(x, b, excl, rev));
            backward(y);
            CHECK(host(gradient(x)) == scanned(ones, b, excl, !rev));
        }
        // forward: the size-1 seed of forward(x) stands for n ones; an array seed gives its own scan
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = block_psum(x, b, excl, rev);
            forward(x);
            CHECK(host(gradient(s)) == scanned(ones, b, excl, rev));
        }
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = block_psum(x, b, excl, rev);
            set_gradient(x, hv, false);
            forward<D>();
            CHECK(host(gradient(s)) == scanned(host(hv), b, excl, rev));
        }
    }
    // an untracked array records nothing; a bad block on a tracked one throws
    {
        D plain_x = D(hx);
        const size_t nodes = Tape<F>::get()->node_count();
        D s = block_psum(plain_x, b);
        CHECK(s.index_() == 0 && Tape<F>::get()->node_count() == nodes);
        D x = D(hx);
        set_requires_gradient(x);
        CHECK(throws([&] { (void) block_psum(x, 7); }));
    }
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("block_psum_host: operands evaluated once, bad blocks refused, tape nodes scan from the other end, %ld calls, no block left allocated\n",
           g_scan_calls);
    return 0;
}
#endif
#endif
