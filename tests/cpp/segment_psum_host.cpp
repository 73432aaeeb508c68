// segment_psum (include/enoki/array.h) down to the C-ABI call and through the tape, on the host stand-in of the C ABI
// (host_abi_stub.h), without a GPU: a stand-alone program with its own main; tests/test_segment_psum_host.py builds and runs it
// (also under -fsanitize=address,undefined).  The stand-in does not define ek_hip_psum_segments; this file does, as a plain host
// loop over the clamp rule of ek_block.h.
//
//   * an unevaluated operand (a unary map) is evaluated once, then the one call is made;
//   * no entries: no call; no starts: one call that zero-fills; starts that are no UInt32 array are refused before the C ABI is
//     reached (and before the operand is evaluated);
//   * segment_psum of a tracked DiffArray records one node of n entries; for all four flag combinations backward gives the scan
//     from the other end with `exclusive` kept, forward the node's own scan, both also from a size-1 seed; the two sweeps are each
//     other's transpose; entries in front of every segment get gradient +0; `starts` gets none;
//   * the node keeps `starts` and releases it when it goes;
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
// a second, tiny translation unit: the free function on an array type that has no segment_psum_ member
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

int main() {
    Bare b, starts;
    bool thrown = false;
    try { (void) enoki::segment_psum(b, starts, true, false); }
    catch (const std::runtime_error &e) { thrown = std::string(e.what()) == "segment_psum(): not available for this array type"; }
    CHECK(thrown);
    printf("segment_psum_host: a type without the member compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/csrc/ek_block.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_psum_calls = 0;

/// the definition: per clamped segment a running sum from its first (reverse: last) entry, +0 outside the segments
static void psum_loop(float *out, const float *x, size_t n, const uint32_t *starts, size_t m, bool excl, bool rev) {
    std::vector<float> r(n, 0.f);                                    // (out may be x)
    for (size_t j = 0; j < m; ++j) {
        uint32_t lo, hi;
        ek::segment_clamp(starts[j], j + 1 < m ? starts[j + 1] : (uint32_t) n, (uint32_t) n, lo, hi);
        float acc = -0.f;
        for (uint32_t t = 0; t < hi - lo; ++t) {
            const uint32_t k = rev ? hi - 1 - t : lo + t;
            if (excl) r[k] = t ? acc : 0.f;
            acc += x[k];
            if (!excl) r[k] = acc;
        }
    }
    if (n) memcpy(out, r.data(), n * sizeof(float));
}

extern "C" int ek_hip_psum_segments(int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m, int flags) {
    ++g_psum_calls;
    if (type != EK_F32 || (flags & ~3)) STUB_UNSUPPORTED("psum_segments", type, flags);
    psum_loop((float *) out, (const float *) in, n, starts, m, flags & EK_SCAN_EXCLUSIVE, flags & EK_SCAN_REVERSE);
    return EK_OK;
}
extern "C" int ek_hip_psum_segments_plan(int, size_t, size_t, int, size_t *tile, size_t *tiles_per_workgroup, size_t *workgroups, int *launches) {
    *tile = 4096; *tiles_per_workgroup = 1; *workgroups = 1; *launches = 1;
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

static std::vector<float> psums(const std::vector<float> &x, const std::vector<uint32_t> &starts, bool excl, bool rev) {
    std::vector<float> r(x.size());
    psum_loop(r.data(), x.data(), x.size(), starts.data(), starts.size(), excl, rev);
    return r;
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
    F x = linspace<F>(-4.f, 4.f, N);
    (void) x.data();
    const std::vector<uint32_t> hs = ragged_starts();
    U starts = U::copy(hs.data(), hs.size());
    hip_set_defer(true);
    // (1) an unevaluated operand: one unary launch, one call -- and nothing again for the second call
    {
        F s = sin(x);
        CHECK(s.mapped_());
        const long u0 = g_unary_calls, c0 = g_psum_calls;
        F r = segment_psum(s, starts);
        CHECK(g_unary_calls == u0 + 1 && g_psum_calls == c0 + 1 && !s.mapped_() && r.size() == N);
        F r2 = segment_psum(s, starts, true, true);
        CHECK(g_unary_calls == u0 + 1 && g_psum_calls == c0 + 2);
        CHECK(host(r) == psums(host(s), hs, false, false) && host(r2) == psums(host(s), hs, true, true));
        CHECK(r.coeff(0) == 0.f && r.coeff(2) == 0.f && r.coeff(3) == s.coeff(3) && r.coeff(5) == s.coeff(4) + s.coeff(5));
        CHECK(host(segment_psum(s, starts, true)) == psums(host(s), hs, true, false));
        CHECK(host(segment_psum(s, starts, false, true)) == psums(host(s), hs, false, true));
    }
    // (2) starts that are no UInt32 array are refused before the C ABI is reached and before the operand is evaluated
    // (HIPArray converts between element types, so for a type WITH the member array.h refuses other starts when it compiles:
    //  static_assert(is_same<Starts, uint32_array_t<T>>).  A type that cannot take UInt32 starts at all throws at run time.)
    {
        static_assert(std::is_same_v<uint32_array_t<F>, U> && std::is_same_v<uint32_array_t<D>, DU>, "the starts are UInt32");
        static_assert(enoki::detail::has_segment_psum<F, U>::value && enoki::detail::has_segment_psum<D, DU>::value &&
                      !enoki::detail::has_segment_psum<F, std::string>::value, "the member takes a UInt32 array");
        F s = sin(x);
        const std::string not_starts = "0, 3, 7";
        const long u0 = g_unary_calls, c0 = g_psum_calls;
        CHECK(throws([&] { (void) segment_psum(s, not_starts); }) && throws([&] { (void) segment_psum(s, not_starts, true, true); }));
        CHECK(g_unary_calls == u0 && g_psum_calls == c0 && s.mapped_());
    }
    // (3) no entries: no call; no starts: no segment, one call that fills with zeros
    {
        const long c0 = g_psum_calls;
        U none;
        F nothing;
        CHECK(segment_psum(nothing, starts).size() == 0 && segment_psum(nothing, none, true).size() == 0 && g_psum_calls == c0);
        F zeros = segment_psum(x, none, false, true);
        CHECK(g_psum_calls == c0 + 1 && host(zeros) == std::vector<float>(N, 0.f));
    }
    hip_set_defer(false);
}

static void on_the_tape() {
    const size_t n = 200;
    const std::vector<uint32_t> hs = { 2, 2, 5, 6, 40, 40, 41, 150, 200, 230 };
    const size_t m = hs.size();
    F hx = linspace<F>(-1.f, 1.f, n), hw = linspace<F>(1.f, 2.f, n), hv = linspace<F>(2.f, 3.f, n);
    const std::vector<float> ones(n, 1.f);
    const size_t live = g_live.size();
    {
        DU starts = DU(U::copy(hs.data(), m));
        for (int mode = 0; mode < 4; ++mode) {
            const bool e = mode & 1, r = mode & 2;
            // one node of n entries; backward gives the scan of the weights from the other end, `exclusive` kept
            {
                D x = D(hx);
                set_requires_gradient(x);
                const size_t nodes = Tape<F>::get()->node_count();
                D p = segment_psum(x, starts, e, r);
                CHECK(Tape<F>::get()->node_count() == nodes + 1 && p.index_() != 0 && p.size() == n);
                CHECK(host(detach(p)) == psums(host(hx), hs, e, r));
                D y = hsum(p * D(hw));
                backward(y);
                const std::vector<float> g = host(gradient(x));
                CHECK(g == psums(host(hw), hs, e, !r));
                CHECK(g[0] == 0.f && g[1] == 0.f && !std::signbit(g[0]) && !std::signbit(g[1]));     // in front of every segment
                CHECK(starts.index_() == 0 && throws([&] { (void) gradient(starts); }));               // the starts stay untracked
            }
            // ... and from the size-1 seed of backward(hsum(segment_psum(x)))
            {
                D x = D(hx);
                set_requires_gradient(x);
                D y = hsum(segment_psum(x, starts, e, r));
                backward(y);
                CHECK(host(gradient(x)) == psums(ones, hs, e, !r));
            }
            // forward: the node's own scan of the seed, a size-1 seed and an array seed
            {
                D x = D(hx);
                set_requires_gradient(x);
                D p = segment_psum(x, starts, e, r);
                forward(x);
                CHECK(host(gradient(p)) == psums(ones, hs, e, r));
            }
            {
                D x = D(hx);
                set_requires_gradient(x);
                D p = segment_psum(x, starts, e, r);
                set_gradient(x, hv, false);
                forward<D>();
                CHECK(host(gradient(p)) == psums(host(hv), hs, e, r));
            }
            // the two sweeps transpose each other: <w, psum(x)> == <psum from the other end(w), x> on small integers
            {
                std::vector<float> xi(n), wi(n);
                for (size_t i = 0; i < n; ++i) { xi[i] = (float) ((int) (i * 7 % 13) - 6); wi[i] = (float) ((int) (i * 5 % 7) - 3); }
                const std::vector<float> s = psums(xi, hs, e, r), t = psums(wi, hs, e, !r);
                double lhs = 0, rhs = 0;
                for (size_t i = 0; i < n; ++i) { lhs += (double) wi[i] * s[i]; rhs += (double) t[i] * xi[i]; }
                CHECK(lhs == rhs);
                F fx = F::copy(xi.data(), n), fw = F::copy(wi.data(), n);
                CHECK(hsum(fw * segment_psum(fx, starts.value_(), e, r)).coeff(0) == (float) lhs);
                CHECK(hsum(segment_psum(fw, starts.value_(), e, !r) * fx).coeff(0) == (float) lhs);
            }
        }
        // an untracked source records nothing
        {
            D plain_x = D(hx);
            const size_t nodes = Tape<F>::get()->node_count();
            D p = segment_psum(plain_x, starts, true);
            CHECK(p.index_() == 0 && Tape<F>::get()->node_count() == nodes && p.size() == n);
        }
    }
    // the node keeps the starts while it lives and releases them with its edge
    {
        D x = D(hx);
        set_requires_gradient(x);
        const size_t before = g_live.size();
        D p;
        {
            DU starts = DU(U::copy(hs.data(), m));
            p = segment_psum(x, starts, true, false);
        }
        CHECK(g_live.size() == before + 2);                       // the prefix sums and the starts, which only the node holds now
        D y = hsum(p * D(hw));
        backward(y);
        CHECK(host(gradient(x)) == psums(host(hw), hs, true, true));
        p = D();
        y = D();
    }
    CHECK(g_live.size() == live);
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("segment_psum_host: operands evaluated once, bad shapes and a wrong starts type refused, tape sweeps transpose for all four "
           "flag pairs, starts released, %ld calls, no block left allocated\n", g_psum_calls);
    return 0;
}
#endif
