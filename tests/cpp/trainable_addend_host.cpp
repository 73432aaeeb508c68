// The kind-2 node with a host-scalar addend that REQUIRES A GRADIENT (include/enoki/hip.h, include/enoki/autodiff.h) under
// AddressSanitizer + LeakSanitizer + UBSan, without a GPU, against the host stand-in of the C ABI (host_abi_stub.h).  A stand-alone
// program with its own main; tests/test_trainable_addend_host.py builds and runs it twice:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tests/cpp/trainable_addend_host.cpp -o ...
//         The stand-in defines neither ek_hip_bucketed_pair_create_scalar nor ek_hip_bucketed_addend_adjoint: hip.h's weak
//         references stay null, DiffArray's guard arms as before and every program runs in element order with the eager bits.
//     ... -DTRAINABLE_ENTRIES_PRESENT
//         Both entries exist (defined below on top of the stand-in): the node forms although c requires a gradient, the adjoint of
//         the gather stays on the object and the gradient of c is ONE call of the new entry.
//
// Either way `y = hsum(sin(u)); backward(y)` gives the bits of eager evaluation for y, gradient(A) and gradient(c) in all eight
// spellings; a handle that reads u while the node is pending evaluates it (the gradient of c then comes from the element-order
// kernels), a write into A leaves the node its old contents.  The same with c a size-1 DEVICE array (ek_hip_bucketed_pair_create_scalar_device,
// defined below under the same macro): the node holds a reference on c's buffer and is among its readers, so a write to c evaluates
// a pending node first -- in both builds.  No block and no bucketed object stays allocated.
#include <enoki/hip.h>
#include <enoki/autodiff.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "host_abi_stub.h"
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_addend_adjoints = 0;
#ifdef TRAINABLE_ENTRIES_PRESENT
// the stand-in's object reads its addend from a table: one filled with c, kept until the program ends
static std::vector<float *> g_scalar_tables;
extern "C" int ek_hip_bucketed_pair_create_scalar(int type, int index_type, int op, const void *a, uint64_t addend_bits, size_t table_size,
                                                  const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                                  ek_hip_bucketed **out) {
    if (mask) { *out = nullptr; return EK_ERR_UNSUPPORTED; }       // (a dropped lane's u is +-c, not the stand-in's 0: not modelled here)
    float c;
    uint32_t bits = (uint32_t) addend_bits;
    memcpy(&c, &bits, 4);
    float *table = (float *) malloc(table_size * sizeof(float));
    for (size_t k = 0; k < table_size; ++k) table[k] = c;
    int rc = ek_hip_bucketed_pair_create_masked(type, index_type, op, a, table, table_size, x, index, nullptr, n, hints, out);
    if (rc != EK_OK) { free(table); return rc; }
    g_scalar_tables.push_back(table);
    return EK_OK;
}
// the scalar on the device: the stand-in reads the element when the object is made (hip.h evaluates a pending node before c changes)
static long g_device_creates = 0;
extern "C" int ek_hip_bucketed_pair_create_scalar_device(int type, int index_type, int op, const void *a, const void *addend, size_t table_size,
                                                         const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                                         ek_hip_bucketed **out) {
    uint32_t bits;
    memcpy(&bits, addend, 4);
    ++g_device_creates;
    return ek_hip_bucketed_pair_create_scalar(type, index_type, op, a, bits, table_size, x, index, mask, n, hints, out);
}
// scale * sum over all lanes of map_op(u), lanes added in element order (the order of the stand-in's hsum_safe_mul)
extern "C" int ek_hip_bucketed_addend_adjoint(ek_hip_bucketed *b, int map_op, uint64_t scale_bits, void *out) {
    ++g_addend_adjoints;
    float scale, acc = 0.f;
    uint32_t bits = (uint32_t) scale_bits;
    memcpy(&scale, &bits, 4);
    for (size_t i = 0; i < b->n; ++i) {
        const float v = unary_f(map_op, b->u ? b->u[i] : bucketed_u(b, i));
        acc += v == 0.f ? 0.f : v;
    }
    *(float *) out = acc * scale;
    return EK_OK;
}
static void release_scalar_tables() {
    for (float *t : g_scalar_tables) free(t);
    g_scalar_tables.clear();
}
static constexpr bool kEntries = true;
#else
static void release_scalar_tables() { }
static constexpr bool kEntries = false;
#endif

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using D = DiffArray<F>;
using UD = DiffArray<U>;

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

static std::vector<float> host(const F &a) {
    std::vector<float> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}
static bool same(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static constexpr size_t N = 1 << 16, K = 4096;

static F input(size_t n, float scale) {
    F x = linspace<F>(-3.f, 3.f, n) * F(scale);
    (void) x.data();
    return x;
}
static U indices() {
    U gi = (arange<U>(N) * U(2654435761u)) & U((uint32_t) K - 1u);
    (void) gi.data();
    return gi;
}

template <typename T> static T spell(int which, const T &g, const T &x, const T &c) {
    switch (which) {
        case 0: return fmadd(g, x, c);
        case 1: return fmsub(g, x, c);
        case 2: return fnmadd(g, x, c);
        case 3: return fnmsub(g, x, c);
        case 4: return g * x + c;
        case 5: return c + g * x;
        case 6: return g * x - c;
        default: return c - g * x;
    }
}

enum Disturb { kNone, kReadU, kWriteA, kDeviceC, kDeviceCWrite };
struct TapeResult { std::vector<float> y, gA, gc, seen; bool node; long scatters, adjoints; };

static TapeResult tape_step(int which, bool defer, Disturb disturb) {
    hip_set_defer(defer);
    TapeResult r;
    {
        F A0 = input(K, 1.f);
        // (kDeviceC: c as a size-1 DEVICE array, the state of a trained bias after an optimiser step)
        const float half = 0.5f;
        F c0 = disturb >= kDeviceC ? F::copy(&half, 1) : F(0.5f);
        D A = D(A0), x = D(input(N, 1.f)), c = D(c0);
        UD idx = UD(indices());
        set_requires_gradient(A);
        set_requires_gradient(c);
        const long s0 = g_bucketed_scatters, a0 = g_addend_adjoints;
        D u = spell<D>(which, gather<D>(A, idx), x, c);
        r.node = detach(u).paired_();
        D y = hsum(sin(u));
        if (disturb == kReadU) r.seen = host(detach(u));                       // a user handle reads u: element order from here on
        if (disturb == kWriteA) {
            // a write into the table while the node is pending: the node keeps the OLD contents (evaluated first, or the writer copies)
            scatter(A0, F(100.f), arange<U>(K));
            CHECK(A0.coeff(7) == 100.f);
            r.seen = host(detach(u));
        }
        if (disturb == kDeviceCWrite) {
            // a write to c while the node is pending: the node is evaluated FIRST (it is among the readers of c's buffer) and holds
            // the old value; the writer then sees its own
            const bool pending = detach(u).paired_();
            scatter(c0, F(7.f), arange<U>(1));
            CHECK(c0.coeff(0) == 7.f && !detach(u).paired_());
            (void) pending;
            r.seen = host(detach(u));
        }
        backward(y);
        r.y = host(detach(y));
        r.gA = host(gradient(A));
        r.gc = host(gradient(c));
        r.scatters = g_bucketed_scatters - s0;
        r.adjoints = g_addend_adjoints - a0;
    }
    hip_set_defer(true);
    return r;
}

int main() {
    hip_set_defer(true);
    size_t programs = 0;
    for (int which = 0; which < 8; ++which) {
        const TapeResult eager = tape_step(which, false, kNone), deferred = tape_step(which, true, kNone);
        CHECK(!eager.node && eager.adjoints == 0);
        // with both entries the node forms although c requires a gradient; the gather's adjoint and the gradient of c stay on the object
        CHECK(deferred.node == kEntries);
        CHECK(deferred.scatters == (kEntries ? 1 : 0) && deferred.adjoints == (kEntries ? 1 : 0));
        CHECK(eager.gc.size() == 1 && same(eager.y, deferred.y) && same(eager.gA, deferred.gA) && same(eager.gc, deferred.gc));
        CHECK(g_bucketed_live == 0);
        for (Disturb how : { kReadU, kWriteA }) {
            const TapeResult e = tape_step(which, false, how), d = tape_step(which, true, how);
            CHECK(d.node == kEntries && d.adjoints == 0 && d.scatters == 0);   // u was evaluated before backward(): no partition to sum on
            CHECK(same(e.seen, d.seen) && same(e.y, d.y) && same(e.gA, d.gA) && same(e.gc, d.gc));
            CHECK(same(d.y, eager.y) && same(d.gc, eager.gc));
            CHECK(g_bucketed_live == 0);
            programs += 2;
        }
        programs += 2;
    }
    // a size-1 device array as the addend, differentiable: the node forms with both entries, holds a reference on c's buffer, gives
    // the eager bits; a write to c evaluates the pending node first, in both builds
    for (int which = 0; which < 8; ++which) {
        const TapeResult e = tape_step(which, false, kDeviceC), d = tape_step(which, true, kDeviceC);
        CHECK(!e.node && d.node == kEntries);
        CHECK(d.scatters == (kEntries ? 1 : 0) && d.adjoints == (kEntries ? 1 : 0));
        CHECK(same(e.y, d.y) && same(e.gA, d.gA) && same(e.gc, d.gc));
        const TapeResult ew = tape_step(which, false, kDeviceCWrite), dw = tape_step(which, true, kDeviceCWrite);
        CHECK(dw.node == kEntries && dw.adjoints == 0 && dw.scatters == 0);
        CHECK(same(ew.seen, dw.seen) && same(ew.y, dw.y) && same(ew.gA, dw.gA) && same(ew.gc, dw.gc) && same(dw.y, e.y) && same(dw.gc, e.gc));
        CHECK(g_bucketed_live == 0);
        programs += 4;
    }
    {
        // the plain array: formed, explained, released with its handle; a view of a larger array is not accepted
        F A = input(K, 1.f), x = input(N, 1.f);
        U gi = indices();
        const float half = 0.5f;
        F c = F::copy(&half, 1);
        { F u = fmadd(gather<F>(A, gi), x, c); CHECK(u.paired_() == kEntries);
          CHECK((u.explain_().find("device addend") != std::string::npos) == kEntries); }
        CHECK(g_bucketed_live == 0);
    }
#ifdef TRAINABLE_ENTRIES_PRESENT
    CHECK(g_device_creates > 0);
#endif
    // explain() says where the gradient of the scalar will come from
    {
        F A = input(K, 1.f), x = input(N, 1.f);
        U gi = indices();
        F u = fmadd(gather<F>(A, gi), x, F(0.5f));
        CHECK((u.explain_().find("summed on the partition") != std::string::npos) == kEntries);
    }
    release_scalar_tables();
    CHECK(g_bucketed_live == 0);
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("trainable_addend_host: %zu programs agree with eager evaluation (%s), no block left allocated\n", programs,
           kEntries ? "entries present: the gradient of the scalar is summed on the object" : "entries absent: element-order fallback");
    return 0;
}
