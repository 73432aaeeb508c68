// The partition cache of include/enoki/hip.h (HIPBuffer::PartitionEntry: the bucket partition of a kind-2 node stays on its index
// array while index, x and mask cannot change, and the next node over the same three stands on it) under AddressSanitizer +
// LeakSanitizer + UBSan, without a GPU, against the host stand-in of the C ABI (host_abi_stub.h).  A stand-alone program with its
// own main; tests/test_partition_cache_host.py builds and runs it twice:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tests/cpp/partition_cache_host.cpp -o ...
//         The stand-in defines none of ek_hip_bucketed_partition_retain / ek_hip_bucket_partition_release /
//         ek_hip_bucketed_pair_create_on: hip.h's weak references stay null and every node partitions for itself.
//     ... -DPARTITION_ENTRIES_PRESENT
//         The entries exist (defined below on top of the stand-in).  A partition here is a COPY of (index, x, mask) as they were when
//         it was built, and an object made on it evaluates from that copy: a hit on a stale entry gives the OLD contents' result and
//         fails the comparison with eager evaluation.
//
// Every creation that runs a partition is counted (g_partitions_built); each scenario states how many it expects.  Directed
// scenarios, then a seeded walk over interleavings of: steps of four expression kinds, writes to index / x / mask, exports, mutable
// pointers, replaced handles, other tables, the mask coming and going, the cache switched off and on, handles of u kept alive.
// Every value equals eager evaluation (deferral switched off) bit for bit, and nothing stays allocated.
#include <enoki/hip.h>
#include <enoki/autodiff.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

// every creation entry of the stand-in ends in its create_masked / create: renamed, so that the ones below count what they forward
#define ek_hip_bucketed_pair_create_masked stub_bucketed_pair_create_masked
#include "host_abi_stub.h"
#undef ek_hip_bucketed_pair_create_masked
#include "../../enoki_amd/src/autodiff_impl.h"
namespace enoki { template struct Tape<HIPArray<float>>; }

static long g_partitions_built = 0;
static std::vector<float *> g_scalar_tables;       // tables filled with a scalar addend: kept until the program ends (the stand-in's objects do not own tables)
static float *scalar_table(size_t table_size, float c) {
    float *table = (float *) malloc(table_size * sizeof(float));
    for (size_t k = 0; k < table_size; ++k) table[k] = c;
    g_scalar_tables.push_back(table);
    return table;
}
extern "C" int ek_hip_bucketed_pair_create_masked(int type, int index_type, int op, const void *a, const void *c, size_t table_size,
                                                  const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                                  ek_hip_bucketed **out) {
    int rc = stub_bucketed_pair_create_masked(type, index_type, op, a, c, table_size, x, index, mask, n, hints, out);
    if (rc == EK_OK) ++g_partitions_built;
    return rc;
}
extern "C" int ek_hip_bucketed_pair_create_scalar(int type, int index_type, int op, const void *a, uint64_t addend_bits, size_t table_size,
                                                  const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                                  ek_hip_bucketed **out) {
    if (mask) { *out = nullptr; return EK_ERR_UNSUPPORTED; }       // (a dropped lane's u is +-c, not the stand-in's 0: not modelled here)
    float c;
    uint32_t bits = (uint32_t) addend_bits;
    memcpy(&c, &bits, 4);
    return ek_hip_bucketed_pair_create_masked(type, index_type, op, a, scalar_table(table_size, c), table_size, x, index, nullptr, n, hints, out);
}

static bool g_cache_on = true;                     // the stand-in's "partition_cache" tuning
static long g_partitions_live = 0, g_on_creates = 0;
#ifdef PARTITION_ENTRIES_PRESENT
struct ek_hip_bucket_partition {
    long refs;
    size_t n, table_size;
    float *x;
    uint32_t *idx;
    uint8_t *mask;
};
template <typename T> static T *clone(const T *p, size_t n) {
    if (!p) return nullptr;
    T *q = (T *) malloc(n * sizeof(T));
    memcpy(q, p, n * sizeof(T));
    return q;
}
extern "C" int ek_hip_bucketed_partition_retain(ek_hip_bucketed *b, ek_hip_bucket_partition **out) {
    *out = nullptr;
    if (!g_cache_on) return EK_ERR_UNSUPPORTED;
    *out = new ek_hip_bucket_partition{ 1, b->n, b->table_size, clone(b->x, b->n), clone(b->idx, b->n), clone(b->mask, b->n) };
    ++g_partitions_live;
    return EK_OK;
}
extern "C" int ek_hip_bucket_partition_release(ek_hip_bucket_partition *p) {
    if (p && --p->refs == 0) { free(p->x); free(p->idx); free(p->mask); delete p; --g_partitions_live; }
    return EK_OK;
}
extern "C" int ek_hip_bucketed_pair_create_on(ek_hip_bucket_partition *p, int type, int index_type, int op, const void *a, const void *c,
                                              const uint64_t *addend_bits, const void *addend_device, size_t table_size, size_t n,
                                              unsigned, int has_mask, ek_hip_bucketed **out) {
    *out = nullptr;
    if (!g_cache_on || !ek_hip_bucketed_applicable(type, index_type, table_size, n) || table_size != p->table_size || n != p->n ||
        (has_mask != 0) != (p->mask != nullptr) || ((addend_bits || addend_device) && has_mask))
        return EK_ERR_UNSUPPORTED;
    if (addend_bits) { float v; uint32_t bits = (uint32_t) *addend_bits; memcpy(&v, &bits, 4); c = scalar_table(table_size, v); }
    if (addend_device) c = scalar_table(table_size, *(const float *) addend_device);
    // no partition runs: the object reads the lists the partition kept
    ek_hip_bucketed *b = new ek_hip_bucketed{ op, (const float *) a, (const float *) c, table_size, n, clone(p->x, n), clone(p->idx, n), nullptr };
    b->mask = clone(p->mask, n);
    ++g_bucketed_live;
    ++g_on_creates;
    *out = b;
    return EK_OK;
}
static constexpr bool kEntries = true;
#else
static constexpr bool kEntries = false;
#endif

using namespace enoki;
using F = HIPArray<float>;
using U = HIPArray<uint32_t>;
using M = HIPArray<bool>;
using D = DiffArray<F>;
using UD = DiffArray<U>;

#define CHECK(expr) do { if (!(expr)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); exit(1); } } while (0)

static std::vector<float> host(const F &a) {
    std::vector<float> v(a.size());
    for (size_t i = 0; i < v.size(); ++i) v[i] = a.coeff(i);
    return v;
}
static bool same(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}
static uint32_t bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

static constexpr size_t N = 2048, K = 256;

// fresh, EVALUATED arrays whose mutable pointer nobody has seen (the const data() evaluates without handing one out)
static F values(size_t n, float scale, unsigned salt) {
    std::vector<float> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = scale * (float) ((double) ((i * 2654435761ull + salt * 40503ull) & 0xFFFF) / 32768.0 - 1.0);
    return F::copy(h.data(), n);
}
static U indices(size_t k, unsigned salt) {
    std::vector<uint32_t> h(N);
    for (size_t i = 0; i < N; ++i) h[i] = (uint32_t) (((i + salt) * 2654435761ull >> 7) % k);
    return U::copy(h.data(), N);
}
static M lanes(unsigned salt) {
    std::vector<uint8_t> h(N);
    for (size_t i = 0; i < N; ++i) h[i] = ((i + salt) & 3) != 0;
    return M::copy(h.data(), N);
}

// the four expression kinds of a step; all reduce in bucket order when the node forms
//   0  hsum(sin(fmadd(gather(A), x, gather(B))))          1  hsum(gather(A) * x)
//   2  hsum(fmadd(gather(A), x, 0.5f))  (unmasked only)   3  sincos of the two-table u, hsum of the sine with the cosine held (the hinted form)
struct Step { float y; std::vector<float> kept; };
static Step step(int kind, const F &A, const F &B, const F &x, const U &gi, const M *mask, F *keep_u = nullptr) {
    auto g = [&](const F &t) { return mask ? gather<F>(t, gi, *mask) : gather<F>(t, gi); };
    Step r{};
    if (kind == 0) {
        F u = fmadd(g(A), x, g(B));
        if (keep_u) *keep_u = u;
        r.y = hsum(sin(u)).coeff(0);
    } else if (kind == 1) {
        r.y = hsum(g(A) * x).coeff(0);
    } else if (kind == 2) {
        r.y = hsum(fmadd(g(A), x, F(0.5f))).coeff(0);
    } else {
        F u = fmadd(g(A), x, g(B));
        auto [s, c] = sincos(u);
        r.y = hsum(s).coeff(0);
        r.kept = host(c);
    }
    return r;
}
/// one step in the deferred mode, the same step eagerly: equal bits, and `expect` partitions built by the deferred one
static void checked_step_(int line, int kind, const F &A, const F &B, const F &x, const U &gi, const M *mask, long expect, F *keep_u = nullptr) {
    const long b0 = g_partitions_built;
    const Step d = step(kind, A, B, x, gi, mask, keep_u);
    const long built = g_partitions_built - b0;
    hip_set_defer(false);
    const Step e = step(kind, A, B, x, gi, mask);
    hip_set_defer(true);
    CHECK(bits(d.y) == bits(e.y) && same(d.kept, e.kept));
    if (built != expect) { fprintf(stderr, "FAILED %s:%d: kind %d built %ld partition(s), expected %ld\n", __FILE__, line, kind, built, expect); exit(1); }
}
#define checked_step(...) checked_step_(__LINE__, __VA_ARGS__)
static long hit(long otherwise) { return kEntries ? 0 : otherwise; }       // what a step over unchanged arrays builds

static void directed() {
    F A = values(K, 1.f, 1), B = values(K, 1.f, 2), x = values(N, 3.f, 3);
    U gi = indices(K, 0);
    M mask = lanes(0);
    // build, hit, hit with other tables, every kind of the same hint set on one partition
    checked_step(0, A, B, x, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, hit(1));
    F A2 = values(K, 1.f, 11), B2 = values(K, 1.f, 12);
    checked_step(0, A2, B2, x, gi, nullptr, hit(1));
    checked_step(1, A2, B2, x, gi, nullptr, hit(1));
    checked_step(2, A, B2, x, gi, nullptr, hit(1));
    CHECK(g_bucketed_live == 0 && g_partitions_live == (kEntries ? 1 : 0));
    // another hint set, the mask, another table size, another x: a miss each, then hits again
    checked_step(3, A, B, x, gi, nullptr, 1);
    checked_step(3, A2, B, x, gi, nullptr, hit(1));
    checked_step(0, A, B, x, gi, &mask, 1);
    checked_step(1, A, B, x, gi, &mask, hit(1));
    checked_step(0, A, B, x, gi, nullptr, 1);
    F Ah = values(K / 2, 1.f, 21), Bh = values(K / 2, 1.f, 22);
    U gih = indices(K / 2, 0);
    checked_step(0, Ah, Bh, x, gih, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, hit(1));             // (the entry of gi is untouched by gih's)
    F x2 = values(N, 2.f, 4);
    checked_step(0, A, B, x2, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, 1);                  // (one entry per index array: x2's replaced x's)
    CHECK(g_partitions_live == (kEntries ? 2 : 0));
    // writes: into x, into the index array, into the mask -- the NEW contents, and from then on (a pointer went out) a partition per step
    scatter(x, F(0.25f), arange<U>(64));
    checked_step(0, A, B, x, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, 1);
    x = values(N, 3.f, 5);
    checked_step(0, A, B, x, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, hit(1));
    scatter(gi, U(7u), arange<U>(32));
    checked_step(0, A, B, x, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, 1);
    gi = indices(K, 3);
    checked_step(0, A, B, x, gi, &mask, 1);
    checked_step(0, A, B, x, gi, &mask, hit(1));
    mask.data()[5] = !mask.coeff(5);
    checked_step(0, A, B, x, gi, &mask, 1);
    checked_step(0, A, B, x, gi, &mask, 1);
    checked_step(0, A, B, x, gi, nullptr, 1);                  // (without the array that was handed out: kept again)
    checked_step(0, A, B, x, gi, nullptr, hit(1));
    // a mutable pointer kept by the caller and written LATER, without a word
    float *raw = x.data();
    checked_step(0, A, B, x, gi, nullptr, 1);
    raw[17] = -2.5f;
    checked_step(0, A, B, x, gi, nullptr, 1);
    // an export: no node at all (an external writer), and none afterwards
    x = values(N, 3.f, 6);
    checked_step(0, A, B, x, gi, nullptr, 1);
    x.mark_exported_();
    checked_step(0, A, B, x, gi, nullptr, 0);
    x = values(N, 3.f, 7);
    // the cache switched off: one partition per step, the kept one is let go; on again: kept again
    checked_step(0, A, B, x, gi, nullptr, 1);
    g_cache_on = false;
    checked_step(0, A, B, x, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, 1);
    CHECK(g_partitions_live == 0);                             // (gih's went with the x it was built over)
    g_cache_on = true;
    checked_step(0, A, B, x, gi, nullptr, 1);
    checked_step(0, A, B, x, gi, nullptr, hit(1));
    // two live users: step N's u stays in a handle (its object alive) while step N + 1 stands on the same partition
    {
        F u1, u2;
        hip_set_defer(false);
        const std::vector<float> eu = host(fmadd(gather<F>(A, gi), x, gather<F>(B, gi))), eu2 = host(fmadd(gather<F>(A2, gi), x, gather<F>(B2, gi)));
        hip_set_defer(true);
        checked_step(0, A, B, x, gi, nullptr, hit(1), &u1);
        checked_step(0, A2, B2, x, gi, nullptr, hit(1), &u2);
        CHECK(g_bucketed_live == (u1.paired_() ? 1 : 0) + (u2.paired_() ? 1 : 0));
        CHECK(same(host(u2), eu2) && same(host(u1), eu));
    }
    CHECK(g_bucketed_live == 0);
}

// the handles of index, x, mask and a live u dropped in every order: the entry goes with whichever of the three goes first, the
// partition with its last object, and nothing is left
static void lifetimes() {
    int order[4] = { 0, 1, 2, 3 };
    size_t perms = 0;
    do {
        auto A = std::make_unique<F>(values(K, 1.f, 1)), B = std::make_unique<F>(values(K, 1.f, 2)), x = std::make_unique<F>(values(N, 3.f, 3));
        auto gi = std::make_unique<U>(indices(K, 1));
        auto mask = std::make_unique<M>(lanes(1));
        auto u = std::make_unique<F>();
        checked_step(0, *A, *B, *x, *gi, mask.get(), 1);
        checked_step(0, *A, *B, *x, *gi, mask.get(), hit(1), u.get());
        CHECK(g_partitions_live == (kEntries ? 1 : 0));
        for (int k = 0; k < 4; ++k) {
            switch (order[k]) {
                case 0: gi.reset(); break;
                case 1: x.reset(); break;
                case 2: mask.reset(); break;
                default: u.reset(); break;
            }
        }
        CHECK(g_bucketed_live == 0 && g_partitions_live == 0);
        ++perms;
    } while (std::next_permutation(order, order + 4));
    CHECK(perms == 24);
}

// ---- on the tape: the benchmark's step, index and x kept by the caller, fresh leaves every step ----------------------------------
struct TapeResult { std::vector<float> y, gA, gB; long built; };
static TapeResult tape_steps(bool defer, int steps, bool masked, int drop_order) {
    hip_set_defer(defer);
    TapeResult r{};
    {
        auto x = std::make_unique<D>(D(values(N, 3.f, 3)));
        auto idx = std::make_unique<UD>(UD(indices(K, 2)));
        M mask = lanes(2);
        const long b0 = g_partitions_built;
        std::unique_ptr<D> last_y;
        for (int s = 0; s < steps; ++s) {
            D A = D(values(K, 1.f, 30 + s)), B = D(values(K, 1.f, 60 + s));
            set_requires_gradient(A); set_requires_gradient(B);
            D u = masked ? fmadd(gather<D>(A, *idx, mask), *x, gather<D>(B, *idx, mask)) : fmadd(gather<D>(A, *idx), *x, gather<D>(B, *idx));
            auto y = std::make_unique<D>(hsum(sin(u)));
            backward(*y);
            r.y = host(detach(*y));
            r.gA = host(gradient(A));
            r.gB = host(gradient(B));
            last_y = std::move(y);
        }
        r.built = g_partitions_built - b0;
        // the caller's handles and what the tape still holds, let go in different orders
        if (drop_order == 0) { idx.reset(); x.reset(); last_y.reset(); }
        else if (drop_order == 1) { last_y.reset(); x.reset(); idx.reset(); }
        else { x.reset(); last_y.reset(); idx.reset(); }
    }
    hip_set_defer(true);
    return r;
}
static void tape_programs() {
    for (int masked = 0; masked < 2; ++masked)
        for (int order = 0; order < 3; ++order) {
            const TapeResult e = tape_steps(false, 3, masked != 0, order), d = tape_steps(true, 3, masked != 0, order);
            CHECK(same(e.y, d.y) && same(e.gA, d.gA) && same(e.gB, d.gB));
            CHECK(e.built == 0 && d.built == (kEntries ? 1 : 3));
            CHECK(g_bucketed_live == 0 && g_partitions_live == 0);
        }
}

// ---- seeded walk -------------------------------------------------------------------------------------------------
struct Slot { int id; bool sticky, exported; };
struct Model {
    bool valid = false;
    int gi = 0, x = 0, mask = 0;       // mask: -1 none
    size_t k = 0;
    unsigned hints = 0;
};
static void walk(unsigned seed, int length) {
    std::mt19937 rng(seed);
    int next_id = 1;
    auto fresh = [&]() { return Slot{ next_id++, false, false }; };
    size_t k = K;
    F A = values(k, 1.f, 1), B = values(k, 1.f, 2), x = values(N, 3.f, seed);
    U gi = indices(k, seed);
    M mask = lanes(seed);
    Slot sx = fresh(), sgi = fresh(), sm = fresh();
    bool masked = false;
    Model entry;
    struct Held { F u; std::vector<float> expect; };
    std::vector<Held> held;
    auto forget = [&](int id) { if (entry.valid && (entry.gi == id || entry.x == id || entry.mask == id)) entry.valid = false; };
    unsigned salt = 100;
    for (int t = 0; t < length; ++t) {
        const unsigned op = rng() % 20;
        if (op < 8) {
            int kind = (int) (op & 3);
            if (kind == 2 && masked) kind = 0;
            const unsigned hints = kind == 3 ? 3u : 0u;
            const bool forms = !sx.exported && !sgi.exported && !(masked && sm.exported);
            const bool cacheable = kEntries && !sx.sticky && !sgi.sticky && !(masked && sm.sticky);
            const bool found = cacheable && entry.valid && entry.gi == sgi.id && entry.x == sx.id && entry.mask == (masked ? sm.id : -1) &&
                               entry.k == k && entry.hints == hints;
            long expect = 0;
            if (forms) {
                expect = found && g_cache_on ? 0 : 1;
                if (found && !g_cache_on) entry.valid = false;
                if (expect && cacheable && g_cache_on) entry = Model{ true, sgi.id, sx.id, masked ? sm.id : -1, k, hints };
            }
            const bool keep = kind == 0 && held.size() < 2 && rng() % 3 == 0;
            F u;
            checked_step(kind, A, B, x, gi, masked ? &mask : nullptr, expect, keep ? &u : nullptr);
            if (keep) {
                hip_set_defer(false);
                std::vector<float> eu = host(masked ? fmadd(gather<F>(A, gi, mask), x, gather<F>(B, gi, mask)) : fmadd(gather<F>(A, gi), x, gather<F>(B, gi)));
                hip_set_defer(true);
                held.push_back(Held{ u, std::move(eu) });
            }
        } else if (op == 8) {              // a write into x (in place or into a copy: either way the handle's buffer is a scatter target now)
            scatter(x, F(0.125f * (float) (rng() % 16)), arange<U>(16) + U(rng() % 64));
            forget(sx.id);
            sx = Slot{ next_id++, true, sx.exported };       // (a sole handle writes in place: an export stays an export)
        } else if (op == 9) {
            scatter(gi, U((uint32_t) (rng() % k)), arange<U>(16) + U(rng() % 64));
            forget(sgi.id);
            sgi = Slot{ next_id++, true, sgi.exported };
        } else if (op == 10) {             // a mutable pointer, written through at once
            const unsigned which = rng() % 3;
            if (which == 0) { x.data()[rng() % N] = 0.5f; forget(sx.id); sx.sticky = true; }
            else if (which == 1) { gi.data()[rng() % N] = (uint32_t) (rng() % k); forget(sgi.id); sgi.sticky = true; }
            else { bool *m = mask.data(); m[rng() % N] = !m[rng() % N]; forget(sm.id); sm.sticky = true; }
        } else if (op == 11) {             // an export
            const unsigned which = rng() % 3;
            if (which == 0) { x.mark_exported_(); forget(sx.id); sx.sticky = sx.exported = true; }
            else if (which == 1) { gi.mark_exported_(); forget(sgi.id); sgi.sticky = sgi.exported = true; }
            else { mask.mark_exported_(); forget(sm.id); sm.sticky = sm.exported = true; }
        } else if (op < 15) {              // a handle replaced by a fresh array
            const unsigned which = rng() % 3;
            if (which == 0) { x = values(N, 3.f, ++salt); forget(sx.id); sx = fresh(); }
            else if (which == 1) { gi = indices(k, ++salt); forget(sgi.id); sgi = fresh(); }
            else { mask = lanes(++salt); forget(sm.id); sm = fresh(); }
        } else if (op == 15) {
            masked = !masked;
        } else if (op == 16) {             // the optimiser's update: other tables of the same size
            A = values(k, 1.f, ++salt); B = values(k, 1.f, ++salt);
        } else if (op == 17) {             // another table size (the index array stays in range of the smaller one)
            k = k == K ? K / 2 : K;
            A = values(k, 1.f, ++salt); B = values(k, 1.f, ++salt);
            if (k == K / 2) { gi = indices(k, ++salt); forget(sgi.id); sgi = fresh(); }
        } else if (op == 18) {
            g_cache_on = !g_cache_on;
        } else if (!held.empty()) {        // a u of an earlier step, still what it was then
            const size_t j = rng() % held.size();
            CHECK(same(host(held[j].u), held[j].expect));
            held.erase(held.begin() + (long) j);
        }
    }
    for (Held &h : held) CHECK(same(host(h.u), h.expect));
    g_cache_on = true;
}

int main() {
    setenv("ENOKI_HIP_DEFER_MIN", "1", 1);         // small arrays go through the deferred paths
    hip_set_defer(true);
    directed();
    CHECK(g_bucketed_live == 0 && g_partitions_live == 0);
    lifetimes();
    tape_programs();
    const int walks = 40;
    for (unsigned seed = 1; seed <= (unsigned) walks; ++seed) {
        walk(seed, 120);
        CHECK(g_bucketed_live == 0 && g_partitions_live == 0);
    }
    for (float *t : g_scalar_tables) free(t);
    CHECK(kEntries ? g_on_creates > 0 : g_on_creates == 0);
    if (!g_live.empty()) { fprintf(stderr, "FAILED: %zu block(s) left allocated\n", g_live.size()); return 1; }
    printf("partition_cache_host: directed scenarios, 24 drop orders and %d seeded walks agree with eager evaluation (%s), %ld partitions "
           "built, %ld objects made on a kept one, no block left allocated\n", walks,
           kEntries ? "entries present: partitions kept" : "entries absent: one partition per step", g_partitions_built, g_on_creates);
    return 0;
}
