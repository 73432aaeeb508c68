// segment_sum / segment_prod / segment_min / segment_max / segment_repeat (include/enoki/array.h) down to the C-ABI calls and
// through the tape, on the host stand-in of the C ABI (host_abi_stub.h), without a GPU: a stand-alone program with its own main;
// tests/test_segment_sum_host.py builds and runs it (also under -fsanitize=address,undefined).  The stand-in does not define
// ek_hip_reduce_segments and ek_hip_repeat_segments; this file does, as plain host loops over the clamp rule of ek_block.h.
//
//   * the clamp rule (segment_clamp) on starts above n and on decreasing starts: lo <= hi <= n always;
//   * an unevaluated operand (a unary map) is evaluated once, then the one call is made;
//   * values that do not match the starts throw before the C ABI is reached (and before the operand is evaluated);
//   * segment_sum of a tracked DiffArray records one node of m entries; backward gives segment_repeat(w), forward
//     segment_sum(seed), both also from a size-1 seed; segment_repeat is the mirror image;
//   * segment_max of a tracked array throws, of an untracked one computes;
//   * the node keeps `starts` and releases it when it goes;
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
// a second, tiny translation unit: the free functions on an array type that has no segment_sum_ / segment_repeat_ members
struct Bare : enoki::ArrayTag { static constexpr size_t Depth = 1; };

template <typename F> static bool throws_unavailable(F &&f, const char *name) {
    try { f(); } catch (const std::runtime_error &e) { return std::string(e.what()) == std::string(name) + "(): not available for this array type"; }
    return false;
}

int main() {
    Bare b, starts;
    CHECK(throws_unavailable([&] { (void) enoki::segment_sum(b, starts); }, "segment_sum"));
    CHECK(throws_unavailable([&] { (void) enoki::segment_prod(b, starts); }, "segment_prod"));
    CHECK(throws_unavailable([&] { (void) enoki::segment_min(b, starts); }, "segment_min"));
    CHECK(throws_unavailable([&] { (void) enoki::segment_max(b, starts); }, "segment_max"));
    CHECK(throws_unavailable([&] { (void) enoki::segment_repeat(b, starts, 4); }, "segment_repeat"));
    printf("segment_sum_host: a type without the members compiles and throws\n");
    return 0;
}
#else

#include "host_abi_stub.h"
#include "../../enoki_amd/csrc/ek_block.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_segment_calls = 0, g_repeat_calls = 0;

extern "C" int ek_hip_reduce_segments(int op, int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m) {
    ++g_segment_calls;
    if (type != EK_F32) STUB_UNSUPPORTED("reduce_segments", type, op);
    const float *x = (const float *) in;
    for (size_t j = 0; j < m; ++j) {
        uint32_t lo, hi;
        ek::segment_clamp(starts[j], j + 1 < m ? starts[j + 1] : (uint32_t) n, (uint32_t) n, lo, hi);
        float acc = op == EK_HSUM ? 0.f : op == EK_HPROD ? 1.f : NAN;
        for (uint32_t k = lo; k < hi; ++k)
            acc = op == EK_HSUM ? acc + x[k] : op == EK_HPROD ? acc * x[k] : op == EK_HMIN ? fminf(acc, x[k]) : fmaxf(acc, x[k]);
        ((float *) out)[j] = acc;
    }
    return EK_OK;
}
extern "C" int ek_hip_repeat_segments(int type, void *out, const void *in, const uint32_t *starts, size_t m, size_t n) {
    ++g_repeat_calls;
    if (type != EK_F32) STUB_UNSUPPORTED("repeat_segments", type, 0);
    for (size_t i = 0; i < n; ++i) {
        size_t j = 0;
        while (j < m && starts[j] <= i) ++j;
        ((float *) out)[i] = j ? ((const float *) in)[j - 1] : 0.f;
    }
    return EK_OK;
}
extern "C" int ek_hip_reduce_segments_plan(int, size_t, size_t, int, int *route, int *group_lanes, int *splits, size_t *workgroups) {
    *route = 1; *group_lanes = 1; *splits = 1; *workgroups = 1;
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

static std::vector<float> sums(const std::vector<float> &x, const std::vector<uint32_t> &starts) {
    std::vector<float> r(starts.size());
    const uint32_t n = (uint32_t) x.size();
    for (size_t j = 0; j < r.size(); ++j) {
        uint32_t lo, hi;
        ek::segment_clamp(starts[j], j + 1 < r.size() ? starts[j + 1] : n, n, lo, hi);
        float acc = 0.f;
        for (uint32_t k = lo; k < hi; ++k) acc += x[k];
        r[j] = acc;
    }
    return r;
}

static std::vector<float> repeated(const std::vector<float> &v, const std::vector<uint32_t> &starts, size_t size) {
    std::vector<float> r(size, 0.f);
    for (size_t i = 0; i < size; ++i)
        for (size_t j = 0; j < starts.size() && starts[j] <= i; ++j) r[i] = v[j];
    return r;
}

template <typename Fn> static bool throws(Fn &&f) {
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

static void clamp_rule() {
    struct Case { uint32_t start, next, n, lo, hi; };
    const Case cases[] = {
        { 0, 3, 10, 0, 3 }, { 3, 3, 10, 3, 3 }, { 7, 10, 10, 7, 10 },
        { 7, 12, 10, 7, 10 }, { 12, 15, 10, 10, 10 }, { 0xFFFFFFFFu, 0xFFFFFFFFu, 10, 10, 10 },      // starts above n
        { 8, 2, 10, 8, 8 }, { 12, 2, 10, 10, 10 }, { 5, 0, 10, 5, 5 },                                 // decreasing starts
        { 0, 0, 0, 0, 0 }, { 4, 9, 0, 0, 0 },                                                          // an empty array
        { 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu },
    };
    for (const Case &c : cases) {
        uint32_t lo = 77, hi = 77;
        ek::segment_clamp(c.start, c.next, c.n, lo, hi);
        CHECK(lo == c.lo && hi == c.hi && lo <= hi && hi <= c.n);
    }
    // every pair of a small grid: inside the array whatever the values, and exact for ordered pairs
    for (uint32_t n = 0; n < 6; ++n)
        for (uint32_t s = 0; s < 9; ++s)
            for (uint32_t e = 0; e < 9; ++e) {
                uint32_t lo, hi;
                ek::segment_clamp(s, e, n, lo, hi);
                CHECK(lo <= hi && hi <= n);
                if (s <= e) CHECK(lo == std::min(s, n) && hi == std::min(e, n));
            }
}

// 5 * 16384 + 3 entries (what a unary map needs to stay unevaluated); segments of 0, 1, 2, .. entries, the first behind 3 entries
// that belong to none, the last ones empty at n
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
        const long u0 = g_unary_calls, c0 = g_segment_calls;
        F r = segment_sum(s, starts);
        CHECK(g_unary_calls == u0 + 1 && g_segment_calls == c0 + 1 && !s.mapped_() && r.size() == hs.size());
        F r2 = segment_max(s, starts);
        CHECK(g_unary_calls == u0 + 1 && g_segment_calls == c0 + 2);
        CHECK(host(r) == sums(host(s), hs));
        CHECK(std::isnan(r2.coeff(0)) && std::isnan(r2.coeff(hs.size() - 1)) && r2.coeff(1) == s.coeff(3));
        F w = cos(linspace<F>(0.f, 1.f, hs.size()));
        const long r0 = g_repeat_calls;
        F rep = segment_repeat(w, starts, N);
        CHECK(g_repeat_calls == r0 + 1 && rep.size() == N && host(rep) == repeated(host(w), hs, N));
        CHECK(rep.coeff(0) == 0.f && rep.coeff(2) == 0.f && rep.coeff(3) == w.coeff(1));
        // fewer and more entries than the last start
        CHECK(host(segment_repeat(w, starts, 100)) == repeated(host(w), hs, 100));
        CHECK(host(segment_repeat(w, starts, N + 9)) == repeated(host(w), hs, N + 9));
    }
    // (2) values that do not match the starts throw before the C ABI is reached and before the operand is evaluated
    {
        F s = sin(x);
        const long u0 = g_unary_calls, r0 = g_repeat_calls;
        CHECK(throws([&] { (void) segment_repeat(s, starts, N); }));
        CHECK(g_unary_calls == u0 && g_repeat_calls == r0 && s.mapped_());
    }
    // (3) no starts: no segment, no call; no entries: every segment is empty; no values: zeros
    {
        const long c0 = g_segment_calls, r0 = g_repeat_calls;
        U none;
        F nothing;
        CHECK(segment_sum(x, none).size() == 0 && g_segment_calls == c0);
        F empty = segment_sum(nothing, starts);
        CHECK(empty.size() == hs.size() && g_segment_calls == c0 + 1 && host(empty) == std::vector<float>(hs.size(), 0.f));
        F zeros = segment_repeat(nothing, none, 7);
        CHECK(g_repeat_calls == r0 + 1 && host(zeros) == std::vector<float>(7, 0.f));
        CHECK(segment_repeat(nothing, none, 0).size() == 0 && g_repeat_calls == r0 + 1);
    }
    hip_set_defer(false);
}

static void on_the_tape() {
    const size_t n = 200;
    const std::vector<uint32_t> hs = { 2, 2, 5, 6, 40, 40, 41, 150, 200, 230 };
    const size_t m = hs.size();
    F hx = linspace<F>(-1.f, 1.f, n), hw = linspace<F>(1.f, 2.f, m), hv = linspace<F>(2.f, 3.f, n);
    const size_t live = g_live.size();
    {
        DU starts = DU(U::copy(hs.data(), m));
        // segment_sum: one node of m entries; backward gives segment_repeat(w)
        {
            D x = D(hx);
            set_requires_gradient(x);
            const size_t nodes = Tape<F>::get()->node_count();
            D s = segment_sum(x, starts);
            CHECK(Tape<F>::get()->node_count() == nodes + 1 && s.index_() != 0 && s.size() == m);
            CHECK(host(detach(s)) == sums(host(hx), hs));
            D y = hsum(s * D(hw));
            backward(y);
            CHECK(host(gradient(x)) == repeated(host(hw), hs, n));
        }
        // ... and from the size-1 seed of backward(hsum(segment_sum(x))): one inside the segments, zero in front of the first
        {
            D x = D(hx);
            set_requires_gradient(x);
            D y = hsum(segment_sum(x, starts));
            backward(y);
            CHECK(host(gradient(x)) == repeated(std::vector<float>(m, 1.f), hs, n));
        }
        // forward through segment_sum: the size-1 seed of forward(x) gives every segment's length, an array seed its segment sums
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = segment_sum(x, starts);
            forward(x);
            CHECK(host(gradient(s)) == sums(std::vector<float>(n, 1.f), hs));
        }
        {
            D x = D(hx);
            set_requires_gradient(x);
            D s = segment_sum(x, starts);
            set_gradient(x, hv, false);
            forward<D>();
            CHECK(host(gradient(s)) == sums(host(hv), hs));
        }
        // segment_repeat is the mirror image: one node of n entries, backward gives segment_sum(v), forward segment_repeat(seed)
        {
            D a = D(hw);
            set_requires_gradient(a);
            const size_t nodes = Tape<F>::get()->node_count();
            D r = segment_repeat(a, starts, n);
            CHECK(Tape<F>::get()->node_count() == nodes + 1 && r.index_() != 0 && r.size() == n);
            CHECK(host(detach(r)) == repeated(host(hw), hs, n));
            D y = hsum(r * D(hv));
            backward(y);
            CHECK(host(gradient(a)) == sums(host(hv), hs));
        }
        {
            D a = D(hw);
            set_requires_gradient(a);
            D y = hsum(segment_repeat(a, starts, n));
            backward(y);
            CHECK(host(gradient(a)) == sums(std::vector<float>(n, 1.f), hs));
        }
        {
            D a = D(hw);
            set_requires_gradient(a);
            D r = segment_repeat(a, starts, n);
            forward(a);
            CHECK(host(gradient(r)) == repeated(std::vector<float>(m, 1.f), hs, n));
        }
        // the two nodes transpose each other: <w, segment_sum(x)> == <segment_repeat(w), x> on small integers
        {
            std::vector<float> xi(n), wi(m);
            for (size_t i = 0; i < n; ++i) xi[i] = (float) ((int) (i * 7 % 13) - 6);
            for (size_t j = 0; j < m; ++j) wi[j] = (float) ((int) (j * 5 % 7) - 3);
            const std::vector<float> s = sums(xi, hs), r = repeated(wi, hs, n);
            double lhs = 0, rhs = 0;
            for (size_t j = 0; j < m; ++j) lhs += (double) wi[j] * s[j];
            for (size_t i = 0; i < n; ++i) rhs += (double) r[i] * xi[i];
            CHECK(lhs == rhs);
            F fx = F::copy(xi.data(), n), fw = F::copy(wi.data(), m);
            CHECK(hsum(fw * segment_sum(fx, starts.value_())).coeff(0) == (float) lhs);
            CHECK(hsum(segment_repeat(fw, starts.value_(), n) * fx).coeff(0) == (float) lhs);
        }
        // no gradient for the other three: a tracked array throws, an untracked one computes
        {
            D x = D(hx);
            set_requires_gradient(x);
            CHECK(throws([&] { (void) segment_max(x, starts); }) && throws([&] { (void) segment_min(x, starts); }) &&
                  throws([&] { (void) segment_prod(x, starts); }));
            D plain_x = D(hx);
            D mx = segment_max(plain_x, starts);
            CHECK(mx.index_() == 0 && mx.size() == m && mx.coeff(2) == hx.coeff(5) && mx.coeff(3) == hx.coeff(39) && std::isnan(mx.coeff(0)));
            CHECK(throws([&] { (void) segment_repeat(x, starts, n); }));
        }
    }
    // the node keeps the starts while it lives and releases them with its edge
    {
        D x = D(hx);
        set_requires_gradient(x);
        const size_t before = g_live.size();
        D s;
        {
            DU starts = DU(U::copy(hs.data(), m));
            s = segment_sum(x, starts);
        }
        CHECK(g_live.size() == before + 2);                       // the sums and the starts, which only the node holds now
        D y = hsum(s * D(hw));
        backward(y);
        CHECK(host(gradient(x)) == repeated(host(hw), hs, n));
        s = D();
        y = D();
    }
    CHECK(g_live.size() == live);
}

int main() {
    clamp_rule();
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("segment_sum_host: clamp rule holds, operands evaluated once, bad shapes refused, tape nodes transpose, starts released, "
           "%ld + %ld calls, no block left allocated\n", g_segment_calls, g_repeat_calls);
    return 0;
}
#endif
