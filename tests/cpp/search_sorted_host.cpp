// search_sorted (include/enoki/array.h) down to the one C-ABI call, on the host stand-in of the C ABI (host_abi_stub.h), without a
// GPU: a stand-alone program with its own main; tests/test_search_sorted_host.py builds and runs it (also under
// -fsanitize=address,undefined).  The stand-in does not define ek_hip_search_sorted; this file does, as a plain host loop.
//
//   * unevaluated operands (a gather as the table, a unary map as the needles) are evaluated once, then the one call is made;
//   * a host-scalar needle gives an output of one entry;
//   * on DiffArray the search runs on the detached values: no node is recorded, the result has no gradient index;
//   * -DEXPECT_FAIL: a table and needles of different element types must stop the compilation (static_assert);
//   * no block stays allocated.
#include <enoki/hip.h>
#include <enoki/autodiff.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_search_calls = 0;
static size_t g_search_last_n = 0;

template <typename T> static void search_loop(uint32_t *out, const T *table, size_t K, const T *needles, size_t n, int right) {
    for (size_t i = 0; i < n; ++i) {
        size_t lo = 0, hi = K;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (right ? (table[mid] <= needles[i]) : (table[mid] < needles[i])) lo = mid + 1; else hi = mid;
        }
        out[i] = (uint32_t) lo;
    }
}
extern "C" int ek_hip_search_sorted(int type, uint32_t *out, const void *table, size_t K, const void *needles, size_t n, int right) {
    ++g_search_calls;
    g_search_last_n = n;
    if (type == EK_F32) search_loop(out, (const float *) table, K, (const float *) needles, n, right);
    else if (type == EK_U32) search_loop(out, (const uint32_t *) table, K, (const uint32_t *) needles, n, right);
    else STUB_UNSUPPORTED("search_sorted", type, 0);
    return EK_OK;
}
extern "C" int ek_hip_search_sorted_plan(int, size_t K, int *resident, int *stride, int *global_steps) {
    *resident = (int) K; *stride = 1; *global_steps = 0;
    return EK_OK;
}

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using D = DiffArray<F>;
using UD = DiffArray<U>;

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

#ifdef EXPECT_FAIL
U mismatched(const F &table, const U &needles) { return search_sorted(table, needles); }
#endif

static constexpr size_t K = 4096, N = 1 << 16;          // (what a gather / a unary map needs to stay unevaluated)

template <typename A> static std::vector<scalar_t<A>> host(const A &a) {
    std::vector<scalar_t<A>> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}

static std::vector<uint32_t> expected(const std::vector<float> &table, const std::vector<float> &needles, bool right) {
    std::vector<uint32_t> r(needles.size());
    for (size_t i = 0; i < r.size(); ++i)
        r[i] = (uint32_t) (std::isnan(needles[i]) ? 0 : right ? std::upper_bound(table.begin(), table.end(), needles[i]) - table.begin()
                                                              : std::lower_bound(table.begin(), table.end(), needles[i]) - table.begin());
    return r;
}

static void plain() {
    F sorted = floor(linspace<F>(-1.f, 1.f, K) * F(64.f)) * F(1.f / 64.f);       // runs of equal entries
    (void) sorted.data();
    F x = linspace<F>(-4.f, 4.f, N);
    (void) x.data();
    const std::vector<float> ht = host(sorted);

    hip_set_defer(true);
    // (1) both operands unevaluated: one gather, one unary launch, one search -- and nothing again for the second call
    {
        F table = gather<F>(sorted, arange<U>(K));
        F needles = sin(x);
        CHECK(table.deferred_() && needles.mapped_());
        const long g0 = g_gather_calls, u0 = g_unary_calls, s0 = g_search_calls;
        U left = search_sorted(table, needles);
        CHECK(g_gather_calls == g0 + 1 && g_unary_calls == u0 + 1 && g_search_calls == s0 + 1 && g_search_last_n == N);
        CHECK(!table.deferred_() && !needles.mapped_());
        U right = search_sorted(table, needles, true);
        CHECK(g_gather_calls == g0 + 1 && g_unary_calls == u0 + 1 && g_search_calls == s0 + 2);
        const std::vector<float> hn = host(needles);
        CHECK(host(left) == expected(ht, hn, false) && host(right) == expected(ht, hn, true));
        CHECK(host(left) != host(right));
    }
    // (2) a host scalar as the needle, as an array type and as a plain scalar: one entry out; a NaN needle: 0 on both sides
    {
        const long s0 = g_search_calls;
        U one = search_sorted(sorted, F(0.25f));
        CHECK(one.size() == 1 && g_search_calls == s0 + 1 && g_search_last_n == 1);
        CHECK(one.coeff(0) == expected(ht, { 0.25f }, false)[0]);
        U two = search_sorted(sorted, 0.25f, true);
        CHECK(two.size() == 1 && two.coeff(0) == expected(ht, { 0.25f }, true)[0] && two.coeff(0) > one.coeff(0));
        CHECK(search_sorted(sorted, F(NAN)).coeff(0) == 0 && search_sorted(sorted, F(NAN), true).coeff(0) == 0);
    }
    // (3) an empty table: zeros; no needles: an empty array and no call
    {
        F none;
        U r = search_sorted(none, x, true);
        CHECK(r.size() == N && r.coeff(0) == 0 && r.coeff(N - 1) == 0);
        const long s0 = g_search_calls;
        CHECK(search_sorted(sorted, none).size() == 0 && g_search_calls == s0);
    }
    // (4) unsigned entries compare unsigned
    {
        U table = arange<U>(K) * U(1u << 20);
        U r = search_sorted(table, U(0x80000000u), true);
        CHECK(r.coeff(0) == 2049);
    }
}

static void on_the_tape() {
    D table = D(linspace<F>(0.f, 1.f, K)), needles = D(linspace<F>(-.25f, 1.25f, N));
    set_requires_gradient(table);
    set_requires_gradient(needles);
    D scaled = needles * D(2.f) - D(0.5f);                     // a recorded node as the needle operand
    const size_t nodes = Tape<F>::get()->node_count();
    const long s0 = g_search_calls;
    UD pos = search_sorted(table, scaled);
    static_assert(std::is_same_v<decltype(search_sorted(table, scaled)), UD>, "the result is the module's UInt32 array");
    CHECK(Tape<F>::get()->node_count() == nodes && g_search_calls == s0 + 1);
    CHECK(pos.index_() == 0 && pos.size() == N);
    CHECK(host(detach(pos)) == expected(host(detach(table)), host(detach(scaled)), false));
    // the positions feed a gather whose gradient still reaches the table
    D y = hsum(gather<D>(table, pos & UD(U((uint32_t) K - 1))));
    backward(y);
    CHECK(gradient(table).size() == K);
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("search_sorted_host: operands evaluated once, %ld calls, no tape node, no block left allocated\n", g_search_calls);
    return 0;
}
