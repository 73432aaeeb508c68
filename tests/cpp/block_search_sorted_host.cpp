// block_search_sorted (include/enoki/array.h) down to the one C-ABI call, on the host stand-in of the C ABI (host_abi_stub.h),
// without a GPU: a stand-alone program with its own main; tests/test_block_search_sorted_host.py builds and runs it (also under
// -fsanitize=address,undefined).  The stand-in does not define ek_hip_search_sorted_blocks; this file does, as a plain host loop.
//
//   * unevaluated operands (a gather as the table, a unary map as the needles) are evaluated once, then the one call is made;
//   * blocked and indexed needles reach the entry with the rows, the row length and the row pointer they were called with;
//   * the length checks of the binding layer: a table that is no whole number of rows, needles that are no whole number per row,
//     a host-scalar needle with more than one row, rows of another length than the needles -- all refused before any call;
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
#include <stdexcept>
#include <vector>

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_block_search_calls = 0;
static size_t g_last_rows = 0, g_last_block = 0, g_last_n = 0;
static bool g_last_indexed = false;

template <typename T>
static void search_loop(uint32_t *out, const T *table, size_t R, size_t B, const T *needles, size_t n, const uint32_t *rows, int right) {
    for (size_t i = 0; i < n; ++i) {
        const size_t r = rows ? std::min<size_t>(rows[i], R - 1) : i / (n / R);
        const T *row = table + r * B;
        size_t lo = 0, hi = B;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (right ? (row[mid] <= needles[i]) : (row[mid] < needles[i])) lo = mid + 1; else hi = mid;
        }
        out[i] = (uint32_t) lo;
    }
}
extern "C" int ek_hip_search_sorted_blocks(int type, uint32_t *out, const void *table, size_t rows, size_t block, const void *needles,
                                           size_t n, const uint32_t *row_index, int right) {
    ++g_block_search_calls;
    g_last_rows = rows; g_last_block = block; g_last_n = n; g_last_indexed = row_index != nullptr;
    if (block == 0 || (!row_index && rows && n % rows != 0) || (rows == 0 && n != 0)) return EK_ERR_INVALID;
    if (type == EK_F32) search_loop(out, (const float *) table, rows, block, (const float *) needles, n, row_index, right);
    else if (type == EK_U32) search_loop(out, (const uint32_t *) table, rows, block, (const uint32_t *) needles, n, row_index, right);
    else STUB_UNSUPPORTED("search_sorted_blocks", type, 0);
    return EK_OK;
}

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using D = DiffArray<F>;
using UD = DiffArray<U>;

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)
#define CHECK_THROWS(expr) do { bool thrown = false; try { (void) (expr); } catch (const std::exception &) { thrown = true; }        \
                                if (!thrown) { fprintf(stderr, "FAILED %s:%d: no exception from %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

#ifdef EXPECT_FAIL
U mismatched(const F &table, const U &needles) { return block_search_sorted(table, needles, 4); }
#endif

static constexpr size_t R = 64, B = 64, M = 1024, N = R * M;       // (N: what a gather / a unary map needs to stay unevaluated)

template <typename A> static std::vector<scalar_t<A>> host(const A &a) {
    std::vector<scalar_t<A>> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}

static std::vector<uint32_t> expected(const std::vector<float> &table, const std::vector<float> &needles, size_t block, bool right,
                                      const std::vector<uint32_t> *rows = nullptr) {
    const size_t rows_in_table = table.size() / block;
    std::vector<uint32_t> r(needles.size());
    for (size_t i = 0; i < r.size(); ++i) {
        const size_t row = rows ? std::min<size_t>((*rows)[i], rows_in_table - 1) : i / (needles.size() / rows_in_table);
        const auto first = table.begin() + row * block, last = first + block;
        r[i] = (uint32_t) (std::isnan(needles[i]) ? 0 : right ? std::upper_bound(first, last, needles[i]) - first
                                                              : std::lower_bound(first, last, needles[i]) - first);
    }
    return r;
}

/// rows of B ascending entries with runs of equal ones; the rows descend: row r + 1 lies below row r
static F rows_of_entries() {
    std::vector<float> t(R * B);
    for (size_t r = 0; r < R; ++r)
        for (size_t k = 0; k < B; ++k) t[r * B + k] = 0.5f * (float) (k / 4) - 3.f * (float) r;
    return F::copy(t.data(), t.size());
}

static void plain() {
    F sorted = rows_of_entries();
    F x = linspace<F>(-4.f, 4.f, N);
    (void) x.data();
    const std::vector<float> ht = host(sorted);
    U rows = (arange<U>(N) * U(2654435761u)) & U(127u);              // half of them beyond the last row
    (void) rows.data();
    const std::vector<uint32_t> hr = host(rows);

    hip_set_defer(true);
    // (1) both operands unevaluated: one gather, one unary launch, one search -- and nothing again for the second call
    {
        F table = gather<F>(sorted, arange<U>(R * B));
        F needles = sin(x);
        CHECK(table.deferred_() && needles.mapped_());
        const long g0 = g_gather_calls, u0 = g_unary_calls, s0 = g_block_search_calls;
        U left = block_search_sorted(table, needles, B);
        CHECK(g_gather_calls == g0 + 1 && g_unary_calls == u0 + 1 && g_block_search_calls == s0 + 1);
        CHECK(g_last_rows == R && g_last_block == B && g_last_n == N && !g_last_indexed);
        CHECK(!table.deferred_() && !needles.mapped_());
        U right = block_search_sorted(table, needles, B, true);
        CHECK(g_gather_calls == g0 + 1 && g_unary_calls == u0 + 1 && g_block_search_calls == s0 + 2);
        const std::vector<float> hn = host(needles);
        CHECK(host(left) == expected(ht, hn, B, false) && host(right) == expected(ht, hn, B, true));
        // ... and with one row per needle
        U indexed = block_search_sorted(table, needles, rows, B, true);
        CHECK(g_block_search_calls == s0 + 3 && g_last_indexed && g_last_n == N && g_gather_calls == g0 + 1);
        CHECK(host(indexed) == expected(ht, hn, B, true, &hr));
        CHECK(host(indexed) != host(right));
    }
    // (2) a host-scalar needle: one entry with one row, or with a row given; refused for blocked needles over several rows
    {
        const long s0 = g_block_search_calls;
        U one = block_search_sorted(sorted, F(-0.25f), R * B);
        CHECK(one.size() == 1 && g_block_search_calls == s0 + 1 && g_last_rows == 1 && g_last_n == 1);
        U two = block_search_sorted(sorted, -185.f, U(63u), B, true);
        const std::vector<uint32_t> last_row = { 63u };
        CHECK(two.size() == 1 && g_last_indexed && two.coeff(0) == expected(ht, { -185.f }, B, true, &last_row)[0]);
        CHECK(two.coeff(0) > 0 && two.coeff(0) < B);
        const long s1 = g_block_search_calls;
        CHECK_THROWS(block_search_sorted(sorted, F(0.25f), B));
        CHECK_THROWS(block_search_sorted(sorted, 0.25f, B));
        CHECK(g_block_search_calls == s1);
    }
    // (3) the length checks, all before the call; no needles: an empty array and no call
    {
        const long s0 = g_block_search_calls;
        F none;
        CHECK_THROWS(block_search_sorted(sorted, x, 0));                           // rows of no entries
        CHECK_THROWS(block_search_sorted(sorted, x, B + 1));                       // no whole number of rows
        CHECK_THROWS(block_search_sorted(sorted, linspace<F>(0.f, 1.f, N - 1), B));   // no whole number of needles per row
        CHECK_THROWS(block_search_sorted(sorted, x, arange<U>(N - 1), B));         // rows of another length
        CHECK_THROWS(block_search_sorted(none, x, B));                             // needles and no row
        CHECK_THROWS(block_search_sorted(none, x, rows, B));
        CHECK(block_search_sorted(sorted, none, B).size() == 0 && block_search_sorted(none, none, B).size() == 0);
        CHECK(block_search_sorted(sorted, none, U(), B).size() == 0);
        CHECK(g_block_search_calls == s0);
    }
    // (4) unsigned entries compare unsigned
    {
        U table = (arange<U>(R * B) & U((uint32_t) (B - 1))) * U(1u << 26);        // every row: 0, 2^26, .., 63 * 2^26
        U r = block_search_sorted(table, full<U>(0x80000000u, R), B, true);
        CHECK(r.size() == R && r.coeff(0) == 33 && r.coeff(R - 1) == 33);
    }
}

static void on_the_tape() {
    D table = D(rows_of_entries()), needles = D(linspace<F>(-200.f, 20.f, N));
    set_requires_gradient(table);
    set_requires_gradient(needles);
    D scaled = needles * D(2.f) - D(0.5f);                     // a recorded node as the needle operand
    UD rows = UD((arange<U>(N) * U(2654435761u)) & U(127u));
    const size_t nodes = Tape<F>::get()->node_count();
    const long s0 = g_block_search_calls;
    UD pos = block_search_sorted(table, scaled, B);
    static_assert(std::is_same_v<decltype(block_search_sorted(table, scaled, B)), UD>, "the result is the module's UInt32 array");
    static_assert(std::is_same_v<decltype(block_search_sorted(table, scaled, rows, B)), UD>, "the result is the module's UInt32 array");
    UD indexed = block_search_sorted(table, scaled, rows, B, true);
    CHECK(Tape<F>::get()->node_count() == nodes && g_block_search_calls == s0 + 2);
    CHECK(pos.index_() == 0 && pos.size() == N && indexed.index_() == 0 && indexed.size() == N);
    const std::vector<uint32_t> hr = host(detach(rows));
    CHECK(host(detach(pos)) == expected(host(detach(table)), host(detach(scaled)), B, false));
    CHECK(host(detach(indexed)) == expected(host(detach(table)), host(detach(scaled)), B, true, &hr));
    // the positions feed a gather whose gradient still reaches the table
    D y = hsum(gather<D>(table, pos & UD(U((uint32_t) B - 1))));
    backward(y);
    CHECK(gradient(table).size() == R * B);
}

int main() {
    plain();
    on_the_tape();
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("block_search_sorted_host: operands evaluated once, %ld calls, length checks hold, no tape node, no block left allocated\n",
           g_block_search_calls);
    return 0;
}
