// One buffer in SEVERAL source slots of one unevaluated node of HIPArray (include/enoki/hip.h) under AddressSanitizer +
// LeakSanitizer + UBSan, without a GPU, against the host stand-in of the C ABI (host_abi_stub.h).  A stand-alone program with its
// own main; tests/test_aliased_sources_host.py builds it once and runs it twice:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tests/cpp/aliased_sources_host.cpp -o ...
//     aliased_sources_host           64 Ki elements, the binding's own thresholds of deferral
//     aliased_sources_host --tiny    16 elements, every threshold lowered to 1 (ENOKI_HIP_DEFER_MIN, read once per process)
//
// A (n elements, n a power of two) is the table of the gathers AND x AND the addend table of a kind-2 node, or every operand of
// a kind-4 node.  A node takes its references and its place among the readers of its sources in ONE function
// (detail::HIPBuffer::make_pending) and gives them back in one (drop_deferred), both over Deferred::each_source(): while the node
// is pending it stands ONCE among A's readers and holds one reference on A per slot; a write into A (scatter, non-const data())
// evaluates it first, with the bits of the eager evaluation; a node that dies unevaluated gives every reference back.  The same
// with an unevaluated map on top of the node.  No block and no bucketed object stays allocated.
#include <enoki/hip.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "host_abi_stub.h"

// A size-1 DEVICE addend makes a kind-2 node only against a C ABI that has this entry (EK_OPTIONAL in enoki_hip.h).  Here it
// exists and declines every shape ("not covered": element order, same bits) -- what aliased_sources() is about is who holds
// and reads what while the node is pending.
extern "C" int ek_hip_bucketed_pair_create_scalar_device(int, int, int, const void *, const void *, size_t, const void *, const void *,
                                                         const uint8_t *, size_t, unsigned, ek_hip_bucketed **out) {
    *out = nullptr;
    return EK_ERR_UNSUPPORTED;
}

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

static std::vector<float> host(const F &a) {
    std::vector<float> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}
static bool same(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}
static F input(size_t n, float scale) {
    F x = linspace<F>(-3.f, 3.f, n) * F(scale);
    (void) x.data();
    return x;
}

struct AliasedShape {
    F (*make)(const F &A, const U &gi, const F &c);      // c: a size-1 device array
    uint32_t slots;                                      // source slots of the node that hold A
    bool arith;                                          // kind 4 (else kind 2)
    bool reads_c;
};
static const AliasedShape aliased_shapes[] = {
    { [](const F &A, const U &gi, const F &) { return fmadd(gather<F>(A, gi), A, gather<F>(A, gi)); }, 3, false, false },
    { [](const F &A, const U &gi, const F &) { return gather<F>(A, gi) * A; }, 2, false, false },
    { [](const F &A, const U &gi, const F &) { return gather<F>(A, gi) * A + F(0.5f); }, 2, false, false },
    { [](const F &A, const U &gi, const F &c) { return gather<F>(A, gi) * A + c; }, 2, false, true },
    { [](const F &A, const U &gi, const F &c) { return fmadd(gather<F>(A, gi), A, c); }, 2, false, true },
    { [](const F &A, const U &, const F &) { return fmadd(A, A, A); }, 3, true, false },
    { [](const F &A, const U &, const F &) { return A * A + A; }, 3, true, false },
};
static size_t times_among(const std::vector<enoki::detail::HIPBuffer *> &readers, const enoki::detail::HIPBuffer *node) {
    size_t count = 0;
    for (const enoki::detail::HIPBuffer *r : readers) count += r == node;
    return count;
}

static void aliased_sources(size_t n) {
    const U gi = (arange<U>(n) * U(2654435761u)) & U((uint32_t) n - 1u), all = arange<U>(n);
    F c = F(0.5f);
    (void) c.data();                                   // an evaluated, owned size-1 array
    const uint32_t c0 = c.buffer_()->ref_count;
    for (const AliasedShape &shape : aliased_shapes) {
        hip_set_defer(false);
        std::vector<float> want, want_map;
        {
            F Ae = input(n, 1.f), ue = shape.make(Ae, gi, c);
            CHECK(!ue.paired_() && !ue.arith_());
            want = host(ue);
            want_map = host(sin(ue));
        }
        hip_set_defer(true);
        for (int with_map = 0; with_map < 2; ++with_map) {
            for (int ending = 0; ending < 3; ++ending) {         // 0: scatter into A, 1: non-const data() of A, 2: the node dies unevaluated
                F A = input(n, 1.f);
                const uint32_t a0 = A.buffer_()->ref_count;
                CHECK(A.buffer_()->readers.empty());
                {
                    F u = shape.make(A, gi, c), m;
                    const auto *node = u.buffer_();
                    CHECK(shape.arith ? u.arith_() : u.paired_());
                    if (with_map) {
                        m = sin(u);
                        CHECK(m.mapped_() && (shape.arith ? u.arith_() : u.paired_()));
                        CHECK(node->ref_count == 2 && node->readers.size() == 1 && node->readers[0] == m.buffer_());
                    }
                    // (1) once among A's readers, (2) one reference per slot -- the gathers of the expression are gone by now
                    CHECK(A.buffer_()->readers.size() == 1 && times_among(A.buffer_()->readers, node) == 1);
                    CHECK(A.buffer_()->ref_count == a0 + shape.slots);
                    CHECK(c.buffer_()->ref_count == c0 + (shape.reads_c ? 1 : 0) && times_among(c.buffer_()->readers, node) == (shape.reads_c ? 1 : 0));
                    if (ending != 2) {
                        // (3) a write into A evaluates the node first; (4) with the bits of the eager evaluation
                        if (ending == 0) scatter(A, F(0.f), all);
                        else CHECK(A.data() != nullptr);
                        CHECK(!u.paired_() && !u.arith_() && u.buffer_() == node);
                        CHECK(A.buffer_()->ref_count == a0 && A.buffer_()->readers.empty());
                        CHECK(c.buffer_()->ref_count == c0 && c.buffer_()->readers.empty());
                        if (ending == 0) CHECK(A.coeff(n - 1) == 0.f);
                        CHECK(same(host(u), want));
                        if (with_map) CHECK(same(host(m), want_map));
                    }
                }
                // (5) every reference is back, whichever way the node went
                CHECK(A.buffer_()->ref_count == a0 && A.buffer_()->readers.empty());
                CHECK(c.buffer_()->ref_count == c0 && c.buffer_()->readers.empty());
            }
        }
    }
}

int main(int argc, char **argv) {
    const bool tiny = argc > 1 && strcmp(argv[1], "--tiny") == 0;
    if (tiny) setenv("ENOKI_HIP_DEFER_MIN", "1", 1);
    const size_t n = tiny ? 16 : (size_t) 1 << 16;       // (1 << 16: the smallest size the binding defers unary maps for)
    aliased_sources(n);
    CHECK(g_live.empty() && g_bucketed_live == 0 && enoki::detail::HIPBuffer::pending_head() == nullptr);
    printf("aliased_sources_host: %zu elements, %zu node shapes agree with eager evaluation, no block left allocated\n",
           n, sizeof(aliased_shapes) / sizeof(aliased_shapes[0]));
    return 0;
}
