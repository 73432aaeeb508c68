// Bucket-ordered evaluation of  u = fma(gather(A, idx), x, gather(C, idx))  and of what consumes it.
//
// What this replaces.  The reference's JIT emits a gather into the kernel of its consumer and fuses the whole chain
// up to the next horizontal operation into ONE kernel (src/cuda/jit.cu:984 cuda_jit_assemble, :1066-1217 the gather's
// ld.global inside the consumer, :1418-1471 cuda_eval); the adjoint scatter_add goes through atom.global.add
// (cuda.h:892-905).  An eager kernel that does the same lookups in ELEMENT order is bound by the L2 miss rate of the
// parameter tables, not by HBM: for K = 1 Mi entries the interleaved {A, C} table is 8 MiB, twice the 4 MiB L2 of an
// XCD, 54 % of the lookups miss and the kernel stops at 0.25 of the HBM roofline (profiles/rocprof_l2_r02.txt).
//
// What it does instead.  When the consumer of u does not care about the element order -- a horizontal reduction
// (hsum(sin(u))), and the adjoint scatter_add of the two gathers through the SAME index array -- the elements are
// processed BUCKET BY BUCKET:
//
//   1. count / scan / partition  (ek_binned.h, the scatter_add pipeline's own kernels) sorts (idx, x) by bucket of
//      16 Ki table entries (8 Ki for 8-byte types): idx is read twice (count, partition), x once; written: a 16-bit
//      bucket-local index and x in bucket order                                                4 + 8 + 6 B/elt
//   2. forward   one 1024-thread workgroup per piece of a bucket stages the bucket's {A, C} slice in LDS (128 KiB),
//                streams (l16, x_b), computes u = fma(A[l], x, C[l]) from LDS, reduces map(u) and -- when somebody
//                else still holds u -- keeps u in bucket order                                     6 (+ 4) B/elt
//   3. adjoint   Tape::backward() finds the partition on the node: one workgroup per piece streams (l16, u_b, x_b),
//                evaluates the value streams (cos(u_b), safe_mul(x_b, cos(u_b))) and adds them into LDS tables under
//                the exchange lock of the scatter_add pipeline; partial tables are folded            10 B/elt
//
// No lookup leaves the CU, no second count / scan / partition in the backward.  Every access that needs ELEMENT order
// (data(), an elementwise consumer, another index array) takes the element-order kernels (gathered.hip) -- same bits
// for u; reductions and gradients differ from the element-order path only by the order of their fp additions (parity
// class D, like every reduction / scatter_add of this library).  Deterministic mode never comes here.
#include "ek_bucketed.h"

namespace ek {

// ---- 2. forward ------------------------------------------------------------------------------------
// The streaming part, specialised for the unary op that is applied to u before the reduction (Map, compile time: the
// kernel switches ONCE, outside the loops -- a runtime switch per element would inline nine transcendental bodies into an
// eight-fold unrolled loop and blow the instruction cache).
// KeepPartner (Map = sin or cos only): what is kept in bucket order is not u but the OTHER half of sincos(u) -- one sincos
// evaluation yields the reduced half and the kept half (the cos(u) that the adjoint of sin needs), like the stand-alone
// sincos kernel fills both halves of a linked pair.
// FromKept: u is not formed from the table slice but read back from what an earlier pass kept (the lists have holes in the
// paged layout, so such a reduction walks the pages too).
template <typename T, int ROp, int V, int Map, bool KeepPartner, bool FromKept>
struct ForwardBody {
    using R = BucketReducer<ROp, T>;
    struct Step { Pack<uint16_t, 4> pi[V]; T px[V][4]; size_t pos[V]; };
    const PairRec<T> *rec;
    T *u_out;
    const uint16_t *pair_idx;
    const T *x_b, *kept;
    uint32_t lmask;
    int two;                 // != 0: u = a * x + c with a rounding each (EK_MULADD family) instead of one fma
    T acc[4];

    __device__ __forceinline__ T elem(uint32_t l, T x, int slot) {
        T u;
        if constexpr (FromKept) {
            u = x;
        } else {
            const PairRec<T> r = rec[l & lmask];
            u = pair_value(r.a, x, r.c, two);
        }
        if constexpr (KeepPartner) {
            static_assert(Map == EK_SIN || Map == EK_COS);
            T sn, cs;
            SinCosOp::apply(u, sn, cs);
            acc[slot] = R::combine(acc[slot], Map == EK_SIN ? sn : cs);
            return Map == EK_SIN ? cs : sn;
        } else {
            if constexpr (ROp != EK_REDUCE_NONE) acc[slot] = R::combine(acc[slot], UnaryOp<Map, T>::apply(u));
            return u;
        }
    }
    __device__ __forceinline__ void fetch(Step &s, int h, size_t pos) {
        s.pos[h] = pos;
        if constexpr (FromKept) {
            load4<T, true>(kept + pos, s.px[h]);
        } else {
            s.pi[h] = pack_load<uint16_t, 4, true>(pair_idx + pos);
            load4<T, true>(x_b + pos, s.px[h]);
        }
    }
    __device__ __forceinline__ void apply(const Step &s) {
#pragma unroll
        for (int h = 0; h < V; ++h) {
            T u[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = elem(FromKept ? 0u : (uint32_t) s.pi[h].v[j], s.px[h][j], j);
            if (u_out) {
                if constexpr (sizeof(T) == 4) {
                    Pack<T, 4> po;
#pragma unroll
                    for (int j = 0; j < 4; ++j) po.v[j] = u[j];
                    pack_store<T, 4, true>(u_out + s.pos[h], po);
                } else {
                    Pack<T, 2> p0, p1;
                    p0.v[0] = u[0]; p0.v[1] = u[1]; p1.v[0] = u[2]; p1.v[1] = u[3];
                    pack_store<T, 2, true>(u_out + s.pos[h], p0);
                    pack_store<T, 2, true>(u_out + s.pos[h] + 2, p1);
                }
            }
        }
    }
    __device__ __forceinline__ void one(size_t pos, bool on, int slot) {
        if (on) {
            const T u = FromKept ? elem(0u, kept[pos], slot) : elem(pair_idx[pos], x_b[pos], slot);
            if (u_out) u_out[pos] = u;
        }
    }
};

// flip_a / flip_c: the fma family differs by the signs of its first and third operand (fmsub: -c, fnmadd: -a, fnmsub:
// both); the signs are applied ONCE to the staged table entries -- exact -- and the inner loop is always one fma.
template <typename T, int ROp, int V, int PS, bool FromKept = false>
__global__ __launch_bounds__(kBucketThreads) void k_bucket_pair_forward(T *__restrict__ partials, T *__restrict__ u_out,
                                                                        const T *__restrict__ table_a, const T *__restrict__ table_c,
                                                                        T addend, size_t table_size, int flip_a, int flip_c, int two,
                                                                        const uint16_t *__restrict__ pair_idx,
                                                                        const T *__restrict__ x_b, const T *__restrict__ kept,
                                                                        BucketLists bl, int map_op, int keep_partner, int shift,
                                                                        BucketFinish<T> fin) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    PairRec<T> *rec = reinterpret_cast<PairRec<T> *>(lds_raw);
    __shared__ T wave_part[kBucketWaves];
    using R = BucketReducer<ROp, T>;
    const int Bins = 1 << shift;
    const uint32_t lmask = (uint32_t) Bins - 1u;
    int bucket;
    PieceRange range;
    const bool live = bucket_piece<PS>(bl, bucket, range);        // (workgroup-uniform; a launch has a few more workgroups than pieces)
    if (!live) {
        if constexpr (ROp != EK_REDUCE_NONE) bucket_finish<T, ROp>(R::identity(), partials, fin.ticket, fin.out, fin.active, fin.n, fin.zero_op, wave_part, fin.counters, fin.zero_u);
        return;
    }
    if constexpr (!FromKept) {
        stage_pair_slice<T, false>(rec, nullptr, table_a, table_c, addend, (size_t) bucket * Bins, table_size, Bins, flip_a, flip_c);
        __syncthreads();
    }

    T result = R::identity();
    auto run = [&](auto body) {
        body.rec = rec; body.u_out = u_out; body.pair_idx = pair_idx; body.x_b = x_b; body.kept = kept; body.lmask = lmask; body.two = two;
#pragma unroll
        for (int k = 0; k < 4; ++k) body.acc[k] = R::identity();
        walk_piece<PS, V>(bl, range, body);
        result = R::combine(R::combine(body.acc[0], body.acc[1]), R::combine(body.acc[2], body.acc[3]));
    };
#define EK_FWD_CASE(OP) case OP: run(ForwardBody<T, ROp, V, OP, false, FromKept>{}); break;
    if constexpr (ROp == EK_REDUCE_NONE) {
        run(ForwardBody<T, ROp, V, EK_COPY, false, FromKept>{});
    } else if (!FromKept && keep_partner && map_op == EK_SIN) {
        run(ForwardBody<T, ROp, V, EK_SIN, true, false>{});
    } else if (!FromKept && keep_partner && map_op == EK_COS) {
        run(ForwardBody<T, ROp, V, EK_COS, true, false>{});
    } else {
        switch (map_op) {
            EK_FWD_CASE(EK_NEG) EK_FWD_CASE(EK_ABS) EK_FWD_CASE(EK_SQRT) EK_FWD_CASE(EK_RCP) EK_FWD_CASE(EK_RSQRT)
            EK_FWD_CASE(EK_SIN) EK_FWD_CASE(EK_COS) EK_FWD_CASE(EK_EXP) EK_FWD_CASE(EK_LOG)
            EK_FWD_CASE(EK_RCP_SQR) EK_FWD_CASE(EK_RSQRT_SQR) EK_FWD_CASE(EK_RSQRT_CUBE)
            default: run(ForwardBody<T, ROp, V, EK_COPY, false, FromKept>{}); break;
        }
    }
#undef EK_FWD_CASE
    if constexpr (ROp != EK_REDUCE_NONE) {
        T v = result;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = R::combine(v, bucket_shfl_down(v, d));
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) wave_part[wave] = v;
        __syncthreads();
        if (threadIdx.x < 64) {
            v = threadIdx.x < kBucketWaves ? wave_part[threadIdx.x] : R::identity();
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) v = R::combine(v, bucket_shfl_down(v, d));
        }
        bucket_finish<T, ROp>(v, partials, fin.ticket, fin.out, fin.active, fin.n, fin.zero_op, wave_part, fin.counters, fin.zero_u);
    }
}


// ---- 3. adjoint ------------------------------------------------------------------------------------
// Value stream c of the scatter_add:  v_c = from_u(c) ? map_c(u) : imm_c,  times x with safe_mul semantics when weighted(c)
// (the tape's pending edge product w * g, autodiff.cpp:1191-1199) -- added to table c at the element's index.
template <typename T, int C> struct BucketStreams {
    int map_op[C];
    T imm[C];
    T scale[C];           // host scalar factor on the stream's value (before the weight)
    unsigned from_u, weighted;
    unsigned plain_x = 0;  // C == 1: the stream is x itself (scatter_add_paged)
};
// The streaming part.  Map >= 0: every stream that is a function of u applies THIS op (compile time; evaluated once per
// element however many streams share it -- the usual pair cos(u), x * cos(u)); Map < 0: per-stream ops chosen at run time.
// Spec = 1: the adjoint of a gathered pair as the tape issues it -- two streams, both the (kept / mapped) function of u, the
// SECOND one weighted by x: known at compile time, no per-element selects on the stream description.
// Spec = 2: ONE stream that is the partitioned value x itself -- a plain scatter_add(value, index) whose (index, value) pairs went
// through the page partition (scatter_add_paged below).
template <typename T, int C, int V, int Map, int Spec>
struct AccumulateBody {
    static constexpr bool Paired = C == 2 && sizeof(T) == 4;
    static_assert(Spec == 0 || (Spec == 1 && C == 2 && Map >= 0) || (Spec == 2 && C == 1));
    struct Step { Pack<uint16_t, 4> pi[V]; T pu[V][4], px[V][4]; };
    T *acc;
    BucketStreams<T, C> st;
    const uint16_t *pair_idx;
    const T *u_b, *x_b;
    int Bins;
    bool need_u, need_x;

    __device__ __forceinline__ void values(T u, T x, T (&v)[C]) const {
        T m = T(0);
        if constexpr (Map >= 0) m = UnaryOp<Map, T>::apply(u);
        if constexpr (Spec == 2) {
            v[0] = x;
        } else if constexpr (Spec == 1) {
            v[0] = m * st.scale[0];
            v[C - 1] = dev::safe_mul(x, m * st.scale[C - 1]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if constexpr (Map >= 0) v[c] = ((st.from_u >> c) & 1u) ? m : st.imm[c];
                else v[c] = ((st.from_u >> c) & 1u) ? unary_fused<T>(st.map_op[c], u) : st.imm[c];
                v[c] = v[c] * st.scale[c];
                if ((st.weighted >> c) & 1u) v[c] = dev::safe_mul(x, v[c]);
            }
        }
    }
    // every lane of a wave passes through the lock (its retry loop is wave-uniform): inactive lanes add nothing
    __device__ __forceinline__ void one(size_t pos, bool on, int) {
        const uint32_t l = on ? (uint32_t) pair_idx[pos] : 0u;
        const T u = (on && need_u) ? u_b[pos] : T(0), x = (on && need_x) ? x_b[pos] : T(0);
        T v[C];
        values(u, x, v);
        if constexpr (Paired) {
            lds_add_pair(reinterpret_cast<unsigned long long *>(acc) + (l & (Bins - 1)), v[0], v[C - 1], on);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) lds_add<true>(&acc[c * Bins + (l & (Bins - 1))], v[c], on);
        }
    }
    __device__ __forceinline__ void fetch(Step &s, int h, size_t pos) {
        s.pi[h] = pack_load<uint16_t, 4, true>(pair_idx + pos);
        if (need_u) load4<T, true>(u_b + pos, s.pu[h]);
        if (need_x) load4<T, true>(x_b + pos, s.px[h]);
    }
    __device__ __forceinline__ void apply(const Step &s) {
        // the values of all 4 V elements; two f32 tables: each element's pair is added right away, otherwise one batch of LDS
        // updates per table afterwards
        constexpr int NB = 4 * V;
        uint32_t l[NB];
        T v[C][NB];
#pragma unroll
        for (int h = 0; h < V; ++h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = h * 4 + j;
                const T u = need_u ? s.pu[h][j] : T(0), x = need_x ? s.px[h][j] : T(0);
                l[k] = (uint32_t) s.pi[h].v[j] & (Bins - 1);
                T vk[C];
                values(u, x, vk);
#pragma unroll
                for (int c = 0; c < C; ++c) v[c][k] = vk[c];
                if constexpr (Paired) {
                    // one claim right behind its element (claim, add, release, batched retry).  Claiming all 4 V bins of
                    // a step first -- one LDS round trip instead of 4 V dependent ones -- was measured again once the
                    // kernels took the bucket size at run time and lost: 0.185 vs 0.152 ms for {cos(u), x cos(u)}, 0.138
                    // vs 0.108 ms for {1, x}, equal for the rest (same box, 64 Mi elements): a lock held across a batch
                    // is met by the other 15 waves more often than its round trip costs.
                    lds_add_pair_one(reinterpret_cast<unsigned long long *>(acc), l[k], vk[0], vk[C - 1]);
                }
            }
        }
        if constexpr (!Paired) {
#pragma unroll
            for (int c = 0; c < C; ++c) lds_add_batch<T, NB>(acc + c * Bins, l, v[c]);
        }
    }
};

template <typename T, int C, int V, int PS>
__global__ __launch_bounds__(kBucketThreads) void k_bucket_accumulate(T *__restrict__ partials,
                                                                      const uint16_t *__restrict__ pair_idx,
                                                                      const T *__restrict__ u_b, const T *__restrict__ x_b,
                                                                      BucketLists bl, BucketStreams<T, C> st, int shift) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T *acc = reinterpret_cast<T *>(lds_raw);                 // C tables of Bins entries; two f32 tables: Bins {t0, t1} pairs
    const int Bins = 1 << shift;
    constexpr bool Paired = C == 2 && sizeof(T) == 4;
    int bucket;
    PieceRange range;
    if (!bucket_piece<PS>(bl, bucket, range)) return;
    for (int j = threadIdx.x; j < C * Bins; j += kBucketThreads) acc[j] = T(0);
    __syncthreads();

    // one op for all streams that read u?  (streams that do not read u do not care)
    int op = EK_COPY;
    bool uniform = true, first = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (!((st.from_u >> c) & 1u)) continue;
        if (first) { op = st.map_op[c]; first = false; }
        else uniform = uniform && st.map_op[c] == op;
    }
    auto run = [&](auto body, bool spec) {
        body.acc = acc; body.st = st; body.pair_idx = pair_idx; body.u_b = u_b; body.x_b = x_b; body.Bins = Bins;
        body.need_u = spec || st.from_u != 0;
        body.need_x = spec || st.weighted != 0;
        walk_piece<PS, V>(bl, range, body);
    };
#define EK_ACC_CASE(OP) case OP: run(AccumulateBody<T, C, V, OP, 0>{}, false); break;
#define EK_ACC_SPEC(OP) case OP: run(AccumulateBody<T, C, V, OP, 1>{}, true); break;
    bool done = false;
    if constexpr (C == 1) {
        if (st.plain_x) {
            auto body = AccumulateBody<T, C, V, EK_COPY, 2>{};
            body.acc = acc; body.st = st; body.pair_idx = pair_idx; body.u_b = u_b; body.x_b = x_b; body.Bins = Bins;
            body.need_u = false; body.need_x = true;
            walk_piece<PS, V>(bl, range, body);
            done = true;
        }
    }
    if constexpr (C == 2) {
        if (uniform && st.from_u == 3u && st.weighted == 2u) {         // (host side: the weighted stream is put second)
            done = true;
            switch (op) {
                EK_ACC_SPEC(EK_NEG) EK_ACC_SPEC(EK_ABS) EK_ACC_SPEC(EK_SQRT) EK_ACC_SPEC(EK_RCP) EK_ACC_SPEC(EK_RSQRT)
                EK_ACC_SPEC(EK_SIN) EK_ACC_SPEC(EK_COS) EK_ACC_SPEC(EK_EXP) EK_ACC_SPEC(EK_LOG)
                EK_ACC_SPEC(EK_RCP_SQR) EK_ACC_SPEC(EK_RSQRT_SQR) EK_ACC_SPEC(EK_RSQRT_CUBE)
                case EK_COPY: run(AccumulateBody<T, C, V, EK_COPY, 1>{}, true); break;
                default: done = false; break;       // an op without a compile-time body: the per-stream run-time form below
            }
        }
    }
#undef EK_ACC_SPEC
    if (done) {
    } else if (uniform) {
        // (an op that unary_fusable() accepts but that has no case here must never fall into the EK_COPY body -- it would scatter u
        // instead of op(u): it takes the run-time form, which evaluates unary_fused(op, u) per stream)
        switch (op) {
            EK_ACC_CASE(EK_NEG) EK_ACC_CASE(EK_ABS) EK_ACC_CASE(EK_SQRT) EK_ACC_CASE(EK_RCP) EK_ACC_CASE(EK_RSQRT)
            EK_ACC_CASE(EK_SIN) EK_ACC_CASE(EK_COS) EK_ACC_CASE(EK_EXP) EK_ACC_CASE(EK_LOG)
            EK_ACC_CASE(EK_RCP_SQR) EK_ACC_CASE(EK_RSQRT_SQR) EK_ACC_CASE(EK_RSQRT_CUBE)
            case EK_COPY: run(AccumulateBody<T, C, V, EK_COPY, 0>{}, false); break;
            default: run(AccumulateBody<T, C, V, -1, 0>{}, false); break;
        }
    } else {
        run(AccumulateBody<T, C, V, -1, 0>{}, false);
    }
#undef EK_ACC_CASE
    __syncthreads();
    // one bucket-sized partial per piece and table: table c at partials + c * gridDim.x * Bins (k_bin_fold_pieces)
#pragma unroll
    for (int c = 0; c < C; ++c) {
        T *out = partials + ((size_t) c * gridDim.x + blockIdx.x) * Bins;
        for (int j = threadIdx.x; j < Bins; j += kBucketThreads) out[j] = Paired ? acc[2 * j + c] : acc[c * Bins + j];
    }
}

// ---- host side -------------------------------------------------------------------------------------
// Counter blocks of the paged objects, kept by the context and handed from object to object: the first reducing launch of an object
// leaves its block's counters zeroed (bucket_finish: the last workgroup clears what the directory launch has consumed), so the next
// object that takes the block needs no fill -- the 768-word memset in front of every partition was 4.5 us of a 100 us shard step.
// Four blocks cover a tape that keeps a few objects alive; whoever finds none free (the slices of a large table, a captured step,
// whose blocks must come from the graph's own pool) allocates and fills as before.
struct MetaRing {
    static constexpr int kBlocks = 4;
    static constexpr size_t kPartials = 2048;                   // reduce partials a block has room for (max_pieces)
    void *block[kBlocks] = {};
    bool busy[kBlocks] = {}, clean[kBlocks] = {};
    // (16 bytes per piece: a float partial, or -- the fixed-point forward + adjoint kernel -- a 64-bit integer partial and a float one)
    static size_t bytes() { return (kPgCounterWords + 3 * (kMaxBuckets + 1) + 1) * sizeof(uint32_t) + kPartials * 16 + 16; }
};
static MetaRing &meta_ring() { static MetaRing *r = new MetaRing(); return *r; }

// The class weights of the page partition (ek_paged.h: kPgClasses) and the workgroups' loop stamps: one small device block per
// context, weights initialised to 1.  ENOKI_HIP_XCD_BALANCE=0 (tuning "xcd_balance") deals equal chunks as before.
struct ClassState {
    void *block = nullptr;             // uint32: weights[kPgClasses] | "the weights are being dealt" | - | stamps[1024] from word kPgClassStamps
    uint32_t *weights() { return (uint32_t *) block; }
    uint32_t *stamps() { return (uint32_t *) block + kPgClassStamps; }
};
static ClassState &class_state() { static ClassState *s = new ClassState(); return *s; }
static uint32_t *class_weights_or_null() {
    ClassState &s = class_state();
    if (!s.block) {
        if (refuse_while_capturing_quiet() != EK_OK) return nullptr;            // (a copy from the host is not part of a step graph)
        if (ek_hip_malloc((kPgClassStamps + 1024) * sizeof(uint32_t), &s.block) != EK_OK) { s.block = nullptr; return nullptr; }
        static const uint32_t ones[kPgClasses] = { kPgWeightOne, kPgWeightOne, kPgWeightOne, kPgWeightOne,
                                                   kPgWeightOne, kPgWeightOne, kPgWeightOne, kPgWeightOne };
        if (hipMemsetAsync(s.block, 0, (kPgClassStamps + 1024) * sizeof(uint32_t), ctx().stream) != hipSuccess ||
            hipMemcpyAsync(s.block, ones, sizeof(ones), hipMemcpyHostToDevice, ctx().stream) != hipSuccess) {
            ek_hip_free(s.block);
            s.block = nullptr;
            return nullptr;
        }
    }
    return s.weights();
}

} // namespace ek

/* diagnostics: the weights of the page partition's workgroup classes and the mean loop duration per class of the last stamped
   launch (100 MHz ticks); synchronises.  weights8 / ticks8: 8 entries each, zeros when no launch has used the weights yet. */
extern "C" EK_API int ek_hip_partition_class_state(uint32_t *weights8, uint32_t *ticks8, uint32_t *dealt) {
    using namespace ek;
    if (int rc = ensure_init()) return rc;
    if (!weights8 || !ticks8) return fail(EK_ERR_INVALID, "ek_hip_partition_class_state(): null pointer");
    for (int k = 0; k < kPgClasses; ++k) weights8[k] = ticks8[k] = 0;
    if (dealt) *dealt = 0;
    ClassState &s = class_state();
    if (!s.block) return EK_OK;
    if (int busy = refuse_while_capturing("ek_hip_partition_class_state()")) return busy;
    std::vector<uint32_t> host(kPgClassStamps + 1024);
    EK_HIP_CHECK(hipMemcpyAsync(host.data(), s.block, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx().stream));
    EK_HIP_CHECK(hipStreamSynchronize(ctx().stream));
    const unsigned W = (unsigned) ctx().num_cu < 1024u ? (unsigned) ctx().num_cu : 1024u;
    for (int k = 0; k < kPgClasses; ++k) {
        weights8[k] = host[k];
        uint64_t sum = 0, cnt = 0;
        for (unsigned w = k; w < W; w += kPgClasses) { sum += host[kPgClassStamps + w]; ++cnt; }
        ticks8[k] = cnt ? (uint32_t) (sum / cnt) : 0u;
    }
    if (dealt) *dealt = host[kPgClasses];
    return EK_OK;
}

namespace ek {

// Every partition that has left its first object (BucketPartition, ek_bucketed.h): the allocator's out-of-memory path asks here
// for the storage of those that only a caller's handle keeps.
static std::vector<BucketPartition *> &live_partitions() { static auto *v = new std::vector<BucketPartition *>(); return *v; }

} // namespace ek
void ek_hip_bucket_partition::free_storage() {
    using namespace ek;
    if (meta_slot >= 0) {
        MetaRing &r = meta_ring();
        r.busy[meta_slot] = false;
        r.clean[meta_slot] = meta_clean;
        meta_slot = -1;
        meta = nullptr;
    }
    for (void **p : { &meta, &pair_idx, &x_b, &page_lists, &refined }) {
        if (*p) ek_hip_free(*p);
        *p = nullptr;
    }
    refined_x = nullptr; refined_hdr = nullptr; refined_tiles = nullptr;
    refined_cap_tiles = 0; refined_bytes = 0;
    refine_state = -1;             // (what the stream was made from is gone)
}
namespace ek {

void partition_release(BucketPartition *p, bool object) {
    if (!p) return;
    if (object) p->objects--;
    if (--p->refs) return;
    auto &all = live_partitions();
    for (size_t i = 0; i < all.size(); ++i)
        if (all[i] == p) { all[i] = all.back(); all.pop_back(); break; }
    delete p;
}

size_t evict_idle_partitions() {
    size_t bytes = 0;
    for (BucketPartition *p : live_partitions()) {
        if (p->objects || p->evicted) continue;
        bytes += p->positions * (sizeof(uint16_t) + sizeof(float)) + p->refined_bytes;
        p->free_storage();
        p->evicted = true;
    }
    return bytes;
}

void release_meta_ring() {
    evict_idle_partitions();           // (a cache's partitions keep ring blocks busy)
    ClassState &cs = class_state();
    if (cs.block) { ek_hip_free(cs.block); cs.block = nullptr; }
    MetaRing &r = meta_ring();
    for (int k = 0; k < MetaRing::kBlocks; ++k) {
        if (r.block[k] && !r.busy[k]) { ek_hip_free(r.block[k]); r.block[k] = nullptr; r.clean[k] = false; }
    }
}

Bucketed::~Bucketed() {
    if (part) {
        // the lists and the counter block are the partition's: it hears whether a reducing launch of this object left the counters zeroed
        if (meta_clean) part->meta_clean = true;
        meta = pair_idx = x_b = page_lists = nullptr;
        meta_slot = -1;
        partition_release(part, true);
        part = nullptr;
    }
    if (meta_slot >= 0) {
        MetaRing &r = meta_ring();
        r.busy[meta_slot] = false;
        r.clean[meta_slot] = meta_clean;
        meta = nullptr;
    }
    if (meta_borrowed) meta = nullptr;
    for (void *p : { meta, early, page_lists, direct[0], direct[1] })     // (direct tables that nobody took; the mode words live in direct[0]'s block)
        if (p) ek_hip_free(p);
    if (!owner)
        for (void *p : { pair_idx, x_b, u_b, m_b })
            if (p) ek_hip_free(p);
}

static size_t bucket_target_pieces(size_t n, int n_buckets) {
    Context &c = ctx();
    static const int per_cu = [] { const char *e = getenv("ENOKI_HIP_BUCKET_PIECES_PER_CU"); return e ? atoi(e) : 1; }();
    static const size_t piece_elems = [] { const char *e = getenv("ENOKI_HIP_PIECE_ELEMS"); return e ? (size_t) atol(e) : (size_t) 32768; }();
    return std::max<size_t>(std::min<size_t>((size_t) std::max(per_cu, 1) * (size_t) c.num_cu, n / piece_elems), (size_t) n_buckets);
}


template <typename T, typename I, int Shift>
static int bucketed_create(Bucketed *b, const T *x, const I *index) {
    RoctxRange range("enoki-hip: bucket partition");
    Context &c = ctx();
    constexpr int Bins = 1 << Shift;
    b->shift = Shift;
    const size_t n = b->n;
    const int n_buckets = b->n_buckets = (int) ((b->table_size + Bins - 1) / Bins);
    b->positions = n;

    unsigned blocks = (unsigned) std::min<size_t>((size_t) c.num_cu * 4, (n + kTile - 1) / kTile);
    if (blocks == 0) blocks = 1;
    size_t chunk = (n + blocks - 1) / blocks;
    chunk = (chunk + kTile - 1) / kTile * kTile;
    blocks = (unsigned) ((n + chunk - 1) / chunk);

    const Arg<uint8_t> mask{ nullptr, 1, 0u };
    const Arg<T> xv{ x, T(0), 1u };
    const int vec_ok = aligned16(index) && aligned16(x);
    int rep_shift = 0;
    while ((n_buckets << (rep_shift + 1)) <= kMaxBuckets && rep_shift < 4) ++rep_shift;

    const uint32_t target_pieces = (uint32_t) bucket_target_pieces(n, n_buckets);
    b->max_pieces = target_pieces + (unsigned) n_buckets;
    const size_t count_entries = (size_t) n_buckets * blocks;
    const size_t meta_words = count_entries + 3 * kMaxBuckets + 2;
    if (int rc = ek_hip_malloc(meta_words * sizeof(uint32_t) + (size_t) b->max_pieces * sizeof(T) + 16, &b->meta)) return rc;
    if (int rc = ek_hip_malloc(n * sizeof(uint16_t), &b->pair_idx)) return rc;
    if (int rc = ek_hip_malloc(n * sizeof(T), &b->x_b)) return rc;
    uint32_t *counts = (uint32_t *) b->meta, *row_total = counts + count_entries;
    b->bucket_base = row_total + kMaxBuckets;
    b->piece_prefix = b->bucket_base + kMaxBuckets + 1;
    b->reduce_partials = (void *) (((uintptr_t) (counts + meta_words) + 15) & ~(uintptr_t) 15);

    hipLaunchKernelGGL((k_bin_count<I, Shift>), dim3(blocks), dim3(kThreads), 0, c.stream, counts, index, mask, n, chunk,
                       n_buckets, rep_shift, vec_ok);
    EK_LAUNCH_CHECK("bucket_count", n, n * sizeof(I));
    // (both scans in ONE single-workgroup launch were measured: 28 us against 4.8 + 5.3 us for these two -- 64 rows of 1024
    // counters are too much latency for one CU)
    hipLaunchKernelGGL(k_bin_scan_rows, dim3(n_buckets), dim3(1024), 0, c.stream, counts, row_total, blocks);
    hipLaunchKernelGGL(k_bin_scan_buckets, dim3(1), dim3(256), 0, c.stream, b->bucket_base, b->piece_prefix,
                       (const uint32_t *) row_total, n_buckets, target_pieces);
    EK_LAUNCH_CHECK("bucket_scan", count_entries, 2 * count_entries * sizeof(uint32_t));
    BinStreams<T, 1> st;
    st.value[0] = xv;
    st.weight[0] = Arg<T>{ nullptr, T(1), 0u };
    st.pair_val[0] = (T *) b->x_b;
    st.weighted = 0u;
    st.value_op[0] = EK_COPY;
    // (histogram replicas for the tile ranking, as in the count kernel: measured, no difference -- 0.2006 / 0.2014 / 0.2021 ms
    // for 1 / 2 / 4 replicas on one box; the ranking is not what bounds this kernel)
    hipLaunchKernelGGL((k_bin_partition<T, I, Shift, uint16_t, 1>), dim3(blocks), dim3(kThreads), 0, c.stream,
                       (uint16_t *) b->pair_idx, st, (const uint32_t *) counts, (const uint32_t *) b->bucket_base, index, mask, n,
                       chunk, n_buckets, 0, vec_ok);
    EK_LAUNCH_CHECK("bucket_partition", n, n * (sizeof(I) + sizeof(T)) + n * (sizeof(uint16_t) + sizeof(T)));
    return EK_OK;
}

/// A table of three or more slices: (index, x) are first split by SLICE into contiguous runs -- the count / scan / partition
/// kernels of ek_binned.h with 32-bit slice-local indices -- so that every slice's page partition reads only its own elements
/// (20 B/elt once instead of 8 B/elt per slice).  The slice populations stay on the device: slice s owns elements
/// [range[2 s], range[2 s] + range[2 s + 1]) of the split's output (runs start at multiples of 4 elements, so that the slices'
/// partitions load 16-byte vectors), and everything that follows reads its size from there -- no read-back, the split can be part
/// of a captured step graph.
struct CoarseSplit {
    void *idx = nullptr, *x = nullptr, *meta = nullptr;      // slice-local indices and x in slice order; counts / bases / ranges
    uint32_t *range = nullptr;                               // device: [S][2] first element, element count
    uint32_t *share = nullptr;                               // device: [S] the slice's share of a piece budget (coarse_split(.., budget))
    size_t elements = 0;                                     // what idx / x hold, the alignment gaps included
    ~CoarseSplit() {
        for (void *p : { idx, x, meta })
            if (p) ek_hip_free(p);
    }
};

// the runs of the split: slice s from a multiple of 4 elements on (bucket_base: where k_bin_partition places them)
// share (optional): `budget` pieces dealt to the slices by population, rounded up -- their sum stays within budget + S
static __global__ __launch_bounds__(64) void k_slice_ranges(uint32_t *__restrict__ range, uint32_t *__restrict__ bucket_base,
                                                             const uint32_t *__restrict__ row_total, int S,
                                                             uint32_t *__restrict__ share, uint32_t budget) {
    if (threadIdx.x != 0) return;
    uint32_t first = 0;
    uint64_t kept = 0;
    for (int s = 0; s < S; ++s) {
        const uint32_t cnt = row_total[s];
        bucket_base[s] = first;
        range[2 * s] = first;
        range[2 * s + 1] = cnt;
        first += (cnt + 3u) & ~3u;
        kept += cnt;
    }
    bucket_base[S] = first;
    if (share)
        for (int s = 0; s < S; ++s) {
            const uint64_t part = kept ? ((uint64_t) row_total[s] * budget + kept - 1) / kept : 0u;
            share[s] = part ? (uint32_t) part : 1u;
        }
}

constexpr int kMaxSlices = 64;

/// `budget` != 0 (scatter_add_sliced): cs.share[s] = the slice's share of that many pieces, and the launches carry scatter_add's names
template <int Shift>
static int coarse_split(CoarseSplit &cs, const float *x, const uint32_t *index, const Arg<uint8_t> &mask, size_t n, int S,
                        uint32_t budget = 0) {
    RoctxRange range("enoki-hip: slice partition");
    Context &c = ctx();
    unsigned blocks = (unsigned) std::min<size_t>((size_t) c.num_cu * 4, (n + kTile - 1) / kTile);
    if (blocks == 0) blocks = 1;
    size_t chunk = (n + blocks - 1) / blocks;
    chunk = (chunk + kTile - 1) / kTile * kTile;
    blocks = (unsigned) ((n + chunk - 1) / chunk);
    const int vec_ok = aligned16(index) && aligned16(x) && arg_aligned(mask);
    int rep_shift = 0;
    while ((S << (rep_shift + 1)) <= kMaxBuckets && rep_shift < 4) ++rep_shift;
    const size_t count_entries = (size_t) S * blocks;
    cs.elements = n + 4 * (size_t) S;
    if (int rc = ek_hip_malloc((count_entries + 4 * kMaxBuckets + 2) * sizeof(uint32_t), &cs.meta)) return rc;
    if (int rc = ek_hip_malloc(cs.elements * sizeof(uint32_t), &cs.idx)) return rc;
    if (int rc = ek_hip_malloc(cs.elements * sizeof(float), &cs.x)) return rc;
    uint32_t *counts = (uint32_t *) cs.meta, *row_total = counts + count_entries, *bucket_base = row_total + kMaxBuckets;
    cs.range = bucket_base + kMaxBuckets + 2;                // [2 kMaxSlices], then share[kMaxSlices]
    cs.share = budget ? cs.range + 2 * kMaxSlices : nullptr;
    hipLaunchKernelGGL((k_bin_count<uint32_t, Shift>), dim3(blocks), dim3(kThreads), 0, c.stream, counts, index, mask, n, chunk, S,
                       rep_shift, vec_ok);
    EK_LAUNCH_CHECK(budget ? "scatter_add_slice_count" : "bucket_slice_count", n, n * sizeof(uint32_t) + arg_bytes(mask, n));
    hipLaunchKernelGGL(k_bin_scan_rows, dim3(S), dim3(1024), 0, c.stream, counts, row_total, blocks);
    hipLaunchKernelGGL(k_slice_ranges, dim3(1), dim3(64), 0, c.stream, cs.range, bucket_base, (const uint32_t *) row_total, S, cs.share,
                       budget);
    EK_LAUNCH_CHECK(budget ? "scatter_add_slice_scan" : "bucket_slice_scan", count_entries, 2 * count_entries * sizeof(uint32_t));
    BinStreams<float, 1> st;
    st.value[0] = Arg<float>{ x, 0.f, 1u };
    st.weight[0] = Arg<float>{ nullptr, 1.f, 0u };
    st.pair_val[0] = (float *) cs.x;
    st.weighted = 0u;
    st.value_op[0] = EK_COPY;
    hipLaunchKernelGGL((k_bin_partition<float, uint32_t, Shift, uint32_t, 1>), dim3(blocks), dim3(kThreads), 0, c.stream,
                       (uint32_t *) cs.idx, st, (const uint32_t *) counts, (const uint32_t *) bucket_base, index, mask, n, chunk, S, 0,
                       vec_ok);
    EK_LAUNCH_CHECK(budget ? "scatter_add_slice_partition" : "bucket_slice_partition", n, n * 16 + arg_bytes(mask, n));
    return EK_OK;
}

/// One slice of a split table (CoarseSplit): its range and its pages are known on the device only.  The slices share ONE page pool
/// (the owner's pair_idx / x_b and full-page lists, paged_slice_pool_pages()) and the partition's working lists; `plan` is the
/// geometry of all of them (256 buckets, the whole input's element count as the bound).
struct PagedSlice {
    const uint32_t *range;         // device: [first element, element count] of the slice in the split's output
    uint32_t page0;                // s * paged_slice_gap()
    const PagedPlan *plan;
    Bucketed *owner;
    uint32_t *glist_full;          // the pool's full-page lists
    uint32_t *work;                // wdir | wlist (pool pages each) | cnt_full | loff | part ([kMaxBuckets][W] each)
    size_t pool_pages;
    // scatter_add_sliced: the slices' counter blocks and glist_part lists are parts of ONE allocation each, a fixed stride apart and
    // zeroed by one fill, so that ONE launch finds every slice's lists (SliceLists); the piece budget is shared out on the device
    void *meta = nullptr;                   // the slice's counter block (counters zeroed by the caller)
    uint32_t *glist_part = nullptr;
    const uint32_t *piece_share = nullptr;  // device: [0] pieces this slice may have (nullptr: the host's target for every slice)
};

/// The same object from the single-pass paged partition (ek_paged.h): 4-byte element types, n <= 2^30.  One streaming pass
/// over (index, x) + the page directory: no count pass, no scans.  pages32: above 128 buckets the caller wants 8-byte records and
/// 32-element pages instead of two planes and 64-element pages (a slice's plan says so itself).
template <typename I>
static int bucketed_create_paged(Bucketed *b, const float *x, const I *index, const Arg<uint8_t> &mask, int shift,
                                 const PagedSlice *slice = nullptr, bool pages32 = false) {
    RoctxRange range("enoki-hip: bucket partition (pages)");
    Context &c = ctx();
    b->shift = shift;
    const size_t n = b->n;             // (a slice: the bound, the whole input)
    const int n_buckets = b->n_buckets = (int) ((b->table_size + ((size_t) 1 << shift) - 1) >> shift);
    const PagedPlan p = slice ? *slice->plan : paged_plan(n, n_buckets, c.num_cu, c.tuning.xcd_balance != 0, false, pages32);
    if (p.W > 1024) return fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_pair_create(): %u workgroups", p.W);
    b->page_shift = p.page_shift;
    b->positions = slice ? slice->pool_pages << p.page_shift : p.page_slots << p.page_shift;
    const uint32_t target_pieces = (uint32_t) bucket_target_pieces(n, n_buckets);
    b->max_pieces = target_pieces + (unsigned) n_buckets;
    // meta: page totals [kPgReplicas][2][256] + meta row [256] (kPgCounterWords) | base_full[257] | base_part[257] | piece_prefix[257] | reduce partials
    const size_t meta_words = kPgCounterWords + 3 * (kMaxBuckets + 1) + 1;
    // the counter block: one of the context's ring when one is free (then usually without a fill, see MetaRing), else an allocation
    bool filled = false;
    static const bool use_ring = [] { const char *e = getenv("ENOKI_HIP_META_RING"); return !e || atoi(e) != 0; }();
    if (slice && slice->meta) {
        b->meta = slice->meta;
        b->meta_borrowed = true;
        filled = true;
    } else if (use_ring && b->max_pieces <= MetaRing::kPartials && refuse_while_capturing_quiet() == EK_OK) {
        MetaRing &r = meta_ring();
        for (int k = 0; k < MetaRing::kBlocks && b->meta_slot < 0; ++k) {
            if (r.busy[k]) continue;
            if (!r.block[k]) {
                if (ek_hip_malloc(MetaRing::bytes(), &r.block[k]) != EK_OK) break;
                r.clean[k] = false;
            }
            r.busy[k] = true;
            b->meta_slot = k;
            b->meta = r.block[k];
            filled = r.clean[k];
        }
    }
    if (b->meta_slot < 0 && !b->meta_borrowed)
        if (int rc = ek_hip_malloc(meta_words * sizeof(uint32_t) + (size_t) b->max_pieces * 16 + 16, &b->meta)) return rc;
    const size_t part_entries = (size_t) p.W * n_buckets;
    if (slice) {
        b->owner = slice->owner;
        b->pair_idx = slice->owner->pair_idx;
        b->x_b = slice->owner->x_b;
        if (!slice->glist_part)
            if (int rc = ek_hip_malloc((part_entries + 1) * sizeof(uint32_t), &b->page_lists)) return rc;
        b->glist_full = slice->glist_full;
        b->glist_part = slice->glist_part ? slice->glist_part : (uint32_t *) b->page_lists;
    } else {
        if (int rc = ek_hip_malloc(b->positions * sizeof(uint16_t), &b->pair_idx)) return rc;
        if (int rc = ek_hip_malloc(b->positions * sizeof(float), &b->x_b)) return rc;
        if (int rc = ek_hip_malloc((p.page_slots + part_entries + 1) * sizeof(uint32_t), &b->page_lists)) return rc;
        b->glist_full = (uint32_t *) b->page_lists;
        b->glist_part = b->glist_full + p.page_slots;
    }
    uint32_t *gtotal = (uint32_t *) b->meta;
    b->bucket_base = gtotal + kPgCounterWords;
    b->active = gtotal + kPgMetaBase + kPgMetaResult;        // (written by the directory launch from the partition's accumulators)
    b->ticket = gtotal + kPgMetaBase + kPgMetaFinishTicket;  // (zero between launches: reset by whoever draws the last ticket)
    b->has_mask = mask.vec != 0;
    b->base_part = b->bucket_base + kMaxBuckets + 1;
    b->piece_prefix = b->base_part + kMaxBuckets + 1;
    b->reduce_partials = (void *) (((uintptr_t) (gtotal + meta_words) + 15) & ~(uintptr_t) 15);
    // what only the two kernels below need: the workgroups' own page lists and counts
    Scratch work;
    if (!slice)
        if (int rc = work.alloc((2 * p.page_slots + 3 * part_entries) * sizeof(uint32_t))) return rc;
    PagedOut<float> out;
    out.lp = (uint16_t *) b->pair_idx;
    out.xp = (float *) b->x_b;
    const size_t list_slots = slice ? slice->pool_pages : p.page_slots;
    out.wdir = slice ? slice->work : (uint32_t *) work.ptr;
    out.wlist = out.wdir + list_slots;
    out.cnt_full = out.wlist + list_slots;
    out.loff = out.cnt_full + part_entries;
    out.part = out.loff + part_entries;
    out.gtotal = gtotal;
    out.active = gtotal + kPgMetaBase + kPgMetaAccum;
    out.lo = b->win_lo; out.span = b->win_span ? b->win_span : (uint32_t) std::min<size_t>(b->table_size, 0xFFFFFFFFu);
    out.range = slice ? slice->range : nullptr;
    out.range_page0 = slice ? slice->page0 : 0u;
    // tiles dealt to the classes w % 8 by the weights the previous launches fed back (ek_paged.h); a launch of at least 32 tiles per
    // workgroup stamps its loops and lets the directory launch update the weights
    // (ENOKI_HIP_XCD_BALANCE=2: the slots are provisioned and the loops stamped, but the chunks stay equal -- what
    // ek_hip_partition_class_state() then reports is the imbalance itself)
    uint32_t *class_block = p.balanced && !slice ? class_weights_or_null() : nullptr;
    out.class_w = c.tuning.xcd_balance == 1 ? class_block : nullptr;
    const bool stamped = class_block && n >= (size_t) 32 * kPgTile * p.W && p.W <= 1024;
    const bool feedback = stamped && out.class_w;
    out.class_stamp = stamped ? class_state().stamps() : nullptr;
    static const uint32_t band = [] { const char *e = getenv("ENOKI_HIP_XCD_BAND"); return e ? (uint32_t) atoi(e) : kPgWeightBand; }();
    out.class_band = band;
    if (!filled) {
        EK_HIP_CHECK(hipMemsetAsync(gtotal, 0, kPgCounterWords * sizeof(uint32_t), c.stream));
        note_launch("bucket_meta_clear", kPgCounterWords, kPgCounterWords * sizeof(uint32_t));   // (its own mark: a profiled run must not bill the fill to the partition)
    }
    const int vec_ok = aligned16(index) && aligned16(x) && arg_aligned(mask);
    auto launch = [&](auto kernel) -> int {
        // the workgroup's own page directory in the LDS behind the records when it fits next to them and the kernel's static
        // arrays (160 KiB per workgroup on gfx950: up to 128 buckets inputs up to ~64 Mi elements; the two planes of more than 128
        // buckets leave ~8 KiB at 256 buckets, inputs up to ~28 Mi elements); ENOKI_HIP_WDIR_LDS=0: through global memory
        static const bool want = [] { const char *e = getenv("ENOKI_HIP_WDIR_LDS"); return !e || atoi(e) != 0; }();
        size_t lds = p.lds;
        out.wdir_lds = 0;
        const size_t fixed_lds = want ? static_lds_of(kernel) : SIZE_MAX;
        if (fixed_lds != SIZE_MAX && fixed_lds + p.lds + (size_t) p.slots * sizeof(uint32_t) <= (size_t) 160 * 1024) {
            lds += (size_t) p.slots * sizeof(uint32_t);
            out.wdir_lds = slice ? p.slots : 1u;
        } else if (slice && fixed_lds != SIZE_MAX && fixed_lds + p.lds + 1024 * sizeof(uint32_t) <= (size_t) 160 * 1024) {
            // (a slice's slots are known on the device only: what the LDS has room for, each workgroup decides by its own count)
            const size_t room = ((size_t) 160 * 1024 - fixed_lds - p.lds) / sizeof(uint32_t);
            lds += room * sizeof(uint32_t);
            out.wdir_lds = (uint32_t) room;
        }
        if (int rc = allow_big_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3(p.W), dim3(kPgThreads), lds, c.stream, out, index, mask, x, n, p.chunk, n_buckets, shift,
                           p.cap, p.slots, vec_ok);
        return EK_OK;
    };
    int rc;
    if (slice) {
        // (the pool's geometry: 32-element pages for every slice; the slices' input has no mask -- the split dropped those lanes)
        if (p.page_shift != 5 || mask.vec) return fail(EK_ERR_INVALID, "bucketed_create_paged(): slice of an unexpected shape");
        rc = launch(k_page_partition<float, I, 5, false, false, true>);
    }
    // (more than 128 buckets: records in two planes, 64-element pages from rings of 96 -- ek_paged.h)
    else if (p.planes) rc = mask.vec ? launch(k_page_partition<float, I, 6, true, false, false, true>) : launch(k_page_partition<float, I, 6, false, false, false, true>);
    else if (p.page_shift == 6) rc = mask.vec ? launch(k_page_partition<float, I, 6, true>) : launch(k_page_partition<float, I, 6, false>);
    else rc = mask.vec ? launch(k_page_partition<float, I, 5, true>) : launch(k_page_partition<float, I, 5, false>);
    if (rc) return rc;
    EK_LAUNCH_CHECK("bucket_partition", n, n * (sizeof(I) + sizeof(float)) + arg_bytes(mask, n) + n * (sizeof(uint16_t) + sizeof(float)));
    if (slice)
        hipLaunchKernelGGL(k_page_directory<true>, dim3(n_buckets, kPgDirSlices), dim3(256), 0, c.stream, b->glist_full, b->glist_part, b->bucket_base,
                           b->base_part, b->piece_prefix, gtotal, (const uint32_t *) out.cnt_full,
                           (const uint32_t *) out.loff, (const uint32_t *) out.part, (const uint32_t *) out.wlist, p.W, p.slots, n_buckets,
                           target_pieces, (uint32_t *) nullptr, slice->piece_share, band, slice->range, slice->page0, p.page_shift);
    else
    hipLaunchKernelGGL(k_page_directory<false>, dim3(n_buckets, kPgDirSlices), dim3(256), 0, c.stream, b->glist_full, b->glist_part, b->bucket_base,
                       b->base_part, b->piece_prefix, gtotal, (const uint32_t *) out.cnt_full,
                       (const uint32_t *) out.loff, (const uint32_t *) out.part, (const uint32_t *) out.wlist, p.W, p.slots, n_buckets,
                       target_pieces, feedback ? class_state().weights() : (uint32_t *) nullptr, (const uint32_t *) out.class_stamp, band,
                       (const uint32_t *) nullptr, 0u, 0);
    EK_LAUNCH_CHECK("bucket_directory", p.page_slots, 2 * p.page_slots * sizeof(uint32_t));
    return EK_OK;
}


template <typename T, int ROp>
static int bucketed_forward_launch(Bucketed *b, void *out, int map_op, bool keep, int keep_op = EK_COPY) {
    Context &c = ctx();
    const size_t Bins = b->bins();
    const size_t lds = Bins * sizeof(PairRec<T>);
    // vectors per lane and step.  float: two (one: 6 % slower, four: 13 % slower, same box); double: one -- with two the
    // kernel needs more than the 128 registers a 1024-thread workgroup leaves a lane (12 spilled; the adjoint: 250)
    constexpr int VV = sizeof(T) == 8 ? 1 : 2;
    // keep the OTHER half of a sincos pair instead of u: only when it is exactly that (sin reduced, cos kept or vice versa)
    const bool partner = keep && ROp != EK_REDUCE_NONE &&
                         ((map_op == EK_SIN && keep_op == EK_COS) || (map_op == EK_COS && keep_op == EK_SIN));
    void **kept = partner ? &b->m_b : &b->u_b;
    if (keep && !*kept) {
        // (a slice keeps its values in the owner's pool, at the positions of its own pages)
        void **pool = b->owner ? (partner ? &b->owner->m_b : &b->owner->u_b) : kept;
        if (!*pool)
            if (int rc = ek_hip_malloc(b->positions * sizeof(T), pool)) return rc;
        *kept = *pool;
    }
    const int flip_a = b->flip_a(), flip_c = b->flip_c(), two = b->two_roundings();
    EK_BY_LAYOUT(b, {
        if (int rc = allow_big_lds(k_bucket_pair_forward<T, ROp, VV, PS>, lds)) return rc;
        hipLaunchKernelGGL((k_bucket_pair_forward<T, ROp, VV, PS>), dim3(b->max_pieces), dim3(kBucketThreads), lds, c.stream,
                           (T *) b->reduce_partials, keep ? (T *) *kept : (T *) nullptr, (const T *) b->table_a,
                           (const T *) b->table_c, b->template addend<T>(), b->table_size, flip_a, flip_c, two, (const uint16_t *) b->pair_idx,
                           (const T *) b->x_b, (const T *) nullptr, b->lists(), map_op, partner ? 1 : 0, b->shift,
                           b->template finish<T>(out, map_op, ROp != EK_REDUCE_NONE));
    });
    EK_LAUNCH_CHECK(ROp == EK_REDUCE_NONE ? "bucket_pair_fma" : "bucket_pair_fma_reduce", b->n,
                    b->n * (sizeof(uint16_t) + sizeof(T) + (keep ? sizeof(T) : 0)) + (b->table_c ? 2 : 1) * b->table_size * sizeof(T));
    b->launched_reducing();
    if (keep && partner) { b->has_m = true; b->m_op = keep_op; }
    else if (keep) b->has_u = true;
    if constexpr (ROp != EK_REDUCE_NONE) {
        if (!b->ticket) {
            hipLaunchKernelGGL((k_bucket_reduce_final<T, ROp>), dim3(1), dim3(256), 0, c.stream, (T *) out,
                               (const T *) b->reduce_partials, b->max_pieces, b->masked_ptr(), b->n, map_op, b->template dropped_u<T>());
            EK_LAUNCH_CHECK("reduce_stage2", (size_t) b->max_pieces, (size_t) b->max_pieces * sizeof(T) + sizeof(T));
        }
    }
    return EK_OK;
}

/// reduce_op over map_op(values) of what an earlier pass kept in list order (u, or the kept half of a sincos pair)
template <typename T, int ROp>
static int bucketed_reduce_kept_launch(Bucketed *b, void *out, int map_op, const void *values, int zero_op) {
    Context &c = ctx();
    constexpr int VV = sizeof(T) == 8 ? 1 : 2;
    EK_BY_LAYOUT(b, {
        hipLaunchKernelGGL((k_bucket_pair_forward<T, ROp, VV, PS, true>), dim3(b->max_pieces), dim3(kBucketThreads), 0, c.stream,
                           (T *) b->reduce_partials, (T *) nullptr, (const T *) nullptr, (const T *) nullptr, T(0), b->table_size, 0, 0, 0,
                           (const uint16_t *) b->pair_idx, (const T *) b->x_b, (const T *) values, b->lists(), map_op, 0, b->shift,
                           b->template finish<T>(out, zero_op));
    });
    EK_LAUNCH_CHECK("bucket_reduce_kept", b->n, b->n * sizeof(T));
    b->launched_reducing();
    if (!b->ticket) {
        hipLaunchKernelGGL((k_bucket_reduce_final<T, ROp>), dim3(1), dim3(256), 0, c.stream, (T *) out, (const T *) b->reduce_partials,
                           b->max_pieces, b->masked_ptr(), b->n, zero_op, b->template dropped_u<T>());
        EK_LAUNCH_CHECK("reduce_stage2", (size_t) b->max_pieces, (size_t) b->max_pieces * sizeof(T) + sizeof(T));
    }
    return EK_OK;
}

template <typename T>
static int bucketed_reduce_kept(Bucketed *b, int reduce_op, int map_op, void *out, const void *values, int zero_op) {
    // zero_op: what the masked-out lanes (u = 0) contribute, as a function of 0
    if (b->page_shift == 0) {          // contiguous lists have no holes: an ordinary reduction
        if (map_op == EK_COPY) return ek_hip_reduce(reduce_op, b->type, out, values, b->n);
        return ek_hip_reduce_map(reduce_op, map_op, b->type, out, values, b->n);
    }
    switch (reduce_op) {
        case EK_HSUM: return bucketed_reduce_kept_launch<T, EK_HSUM>(b, out, map_op, values, zero_op);
        case EK_HPROD: return bucketed_reduce_kept_launch<T, EK_HPROD>(b, out, map_op, values, zero_op);
        case EK_HMIN: return bucketed_reduce_kept_launch<T, EK_HMIN>(b, out, map_op, values, zero_op);
        case EK_HMAX: return bucketed_reduce_kept_launch<T, EK_HMAX>(b, out, map_op, values, zero_op);
        default: return fail(EK_ERR_INVALID, "ek_hip_bucketed_reduce(): unknown op %d", reduce_op);
    }
}

/// hsum of map_op(u) with the adjoint of the gathers -- the sums of keep_op(u) and x * keep_op(u) per entry -- formed in the
/// same pass (k_bucket_pair_forward_adjoint)

template <typename T>
static int bucketed_reduce(Bucketed *b, int reduce_op, int map_op, void *out, bool keep, int keep_op) {
    RoctxRange range("enoki-hip: bucket-ordered gather + fma + reduction");
    // a plan with half-size buckets was made for this: the sum of one half of sincos(u) whose other half is to be kept
    if (b->shift < bin_shift_of<T> && reduce_op == EK_HSUM && keep && !b->has_u && !b->has_m && !b->has_early &&
        early_pair_supported(map_op, keep_op))
        return bucketed_forward_adjoint_launch<T>(b, out, map_op, keep_op);
    if (b->has_m && map_op == b->m_op) return bucketed_reduce_kept<T>(b, reduce_op, EK_COPY, out, b->m_b, b->m_op);   // the kept half itself
    if (b->has_u) return bucketed_reduce_kept<T>(b, reduce_op, map_op, out, b->u_b, map_op);      // u already exists in list order
    switch (reduce_op) {
        case EK_HSUM: return bucketed_forward_launch<T, EK_HSUM>(b, out, map_op, keep, keep_op);
        case EK_HPROD: return bucketed_forward_launch<T, EK_HPROD>(b, out, map_op, keep, keep_op);
        case EK_HMIN: return bucketed_forward_launch<T, EK_HMIN>(b, out, map_op, keep, keep_op);
        case EK_HMAX: return bucketed_forward_launch<T, EK_HMAX>(b, out, map_op, keep, keep_op);
        default: return fail(EK_ERR_INVALID, "ek_hip_bucketed_reduce(): unknown op %d", reduce_op);
    }
}

template <typename T, int C>
static int bucketed_accumulate(Bucketed *b, T *const *bases, const BucketStreams<T, C> &st, const void *u_src, unsigned fresh) {
    Context &c = ctx();
    const size_t Bins = b->bins();
    const size_t lds = (size_t) C * Bins * sizeof(T);
    constexpr int VV = sizeof(T) == 8 ? 1 : 2;          // as in the forward kernel
    Scratch partials;
    if (int rc = partials.alloc((size_t) C * b->max_pieces * Bins * sizeof(T))) return rc;
    EK_BY_LAYOUT(b, {
        if (int rc = allow_big_lds(k_bucket_accumulate<T, C, VV, PS>, lds)) return rc;
        hipLaunchKernelGGL((k_bucket_accumulate<T, C, VV, PS>), dim3(b->max_pieces), dim3(kBucketThreads), lds, c.stream,
                           (T *) partials.ptr, (const uint16_t *) b->pair_idx, (const T *) u_src, (const T *) b->x_b, b->lists(), st,
                           b->shift);
    });
    EK_LAUNCH_CHECK("bucket_accumulate", (size_t) C * b->n,
                    b->n * (sizeof(uint16_t) + (st.from_u ? sizeof(T) : 0) + (st.weighted ? sizeof(T) : 0)) +
                    (size_t) C * b->max_pieces * Bins * sizeof(T));
    FoldTargets<T, C> targets;
    for (int s = 0; s < C; ++s) { targets.table[s] = bases[s]; targets.scale[s] = T(1); }
    hipLaunchKernelGGL((k_bin_fold_pieces<T, C>), dim3(fold_grid(b->table_size), C), dim3(256), 0, c.stream, targets,
                       (const T *) partials.ptr, (const uint32_t *) b->piece_prefix, b->table_size, (size_t) b->max_pieces * Bins, fresh,
                       b->shift);
    EK_LAUNCH_CHECK("scatter_add_fold", (size_t) C * b->table_size,
                    (size_t) C * ((size_t) b->max_pieces * Bins * sizeof(T) + 2 * b->table_size * sizeof(T)));
    return EK_OK;
}


// The per-piece tables of the fixed-point forward + adjoint kernel (bucketed_early.hip) into the gradient tables: 64-bit sums of
// all pieces of a bucket are added as INTEGERS (order-free: the result does not depend on which piece an element went to, nor on
// anything else that varies from run to run), converted once, scaled back by the power of two they were scaled up with, times the
// caller's factor.  A piece that ran under locks (piece_mode 1: max |x| not finite, or a NaN term) left floats, which are added on top.
template <int C>
__global__ __launch_bounds__(256) void k_fold_fixed_pieces(FoldTargets<float, C> targets, const long long *__restrict__ partials,
                                                           const uint32_t *__restrict__ piece_mode, const uint32_t *__restrict__ piece_prefix,
                                                           size_t table_size, size_t partial_stride, unsigned fresh, int shift,
                                                           const uint32_t *__restrict__ xmax_bits, int S0, int first_table,
                                                           const float *__restrict__ direct0, const float *__restrict__ direct1) {
    const size_t k0 = ((size_t) blockIdx.x * 256 + threadIdx.x) * kFoldPerLane;
    if (k0 >= table_size) return;
    const int c = first_table + (int) blockIdx.y;                 // 0: the plain sums, 1: the x-weighted sums
    float *__restrict__ target = targets.table[blockIdx.y];
    const bool direct = direct0 || direct1;                       // (one of the two may have left: ek_hip_bucketed_take_tables)
    if (!direct) partials += (size_t) c * partial_stride;
    const uint32_t b = (uint32_t) (k0 >> shift), local = (uint32_t) (k0 & (((size_t) 1 << shift) - 1));
    const bool is_fresh = (fresh >> blockIdx.y) & 1u;
    const uint32_t p0 = piece_prefix[b], p1 = piece_prefix[b + 1];
    // (128 bits: a piece's sums stay below 2^62 by the choice of the scale, a skewed bucket of many pieces may not)
    unsigned long long ilo[kFoldPerLane];
    long long ihi[kFoldPerLane];
    float fsum[kFoldPerLane], old[kFoldPerLane];
#pragma unroll
    for (int j = 0; j < kFoldPerLane; ++j) { ilo[j] = 0; ihi[j] = 0; fsum[j] = 0.f; old[j] = 0.f; }
    const int lim = (int) (table_size - k0 < (size_t) kFoldPerLane ? table_size - k0 : (size_t) kFoldPerLane);
    if (!is_fresh) {
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) old[j] = target[k0 + j];
    }
    const uint32_t xm = xmax_bits[0];
    if (direct) {
        // DIRECT tables (every bucket one piece; `partials` is null): plane c is a table of its own, the slot of bucket b its floats at
        // plane + b * Bins -- entry k0 at plane + k0.  (The kernel finished them as for a fresh table at scale 1: 0 + (0 * back + sum),
        // which the statements below leave as they are before the factor and the old value are applied.)
        const float *slotf = (c ? direct1 : direct0) + ((size_t) b << shift);
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) fsum[j] = __builtin_nontemporal_load(slotf + local + j);
    } else if (p1 - p0 == 1u) {
        // a bucket that is one piece wrote floats whatever it ran under (bucketed_early.hip): no mode to wait for, a quarter of the bytes
        const float *slotf = reinterpret_cast<const float *>(partials + ((size_t) p0 << shift));
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) fsum[j] = __builtin_nontemporal_load(slotf + local + j);
    } else
    for (uint32_t p = p0; p < p1; ++p) {
        // (mode and sums requested together: the 64-bit words of a slot can be read whatever the piece wrote into it)
        const long long *slot = partials + ((size_t) p << shift);
        const uint32_t mode = piece_mode[p];
        long long v[kFoldPerLane];
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) v[j] = j < lim ? __builtin_nontemporal_load(slot + local + j) : 0ll;
        if (mode == 0u) {
#pragma unroll
            for (int j = 0; j < kFoldPerLane; ++j) {
                const unsigned long long before = ilo[j];
                ilo[j] += (unsigned long long) v[j];
                ihi[j] += (v[j] >> 63) + (ilo[j] < before ? 1 : 0);
            }
        } else {
            const float *slotf = reinterpret_cast<const float *>(slot);
#pragma unroll
            for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) fsum[j] += slotf[local + j];
        }
    }
    const float back = fixed_scale(S0, xm, c == 1).back, f = targets.scale[blockIdx.y];
#pragma unroll
    for (int j = 0; j < kFoldPerLane; ++j) {
        if (j >= lim) continue;
        // (one conversion of the exact integer: the same integer gives the same float whatever the pieces were)
        const bool narrow = ihi[j] == ((long long) ilo[j] >> 63);
        float v = narrow ? (float) (long long) ilo[j] : (float) ((double) ihi[j] * 18446744073709551616.0 + (double) ilo[j]);
        v = v * back + fsum[j];
        if (f != 1.f) v = v * f;
        target[k0 + j] = old[j] + v;
    }
}

// ---- the adjoint of a SCALAR addend from the early sums ---------------------------------------------------------------------------
// Plane 0 of the per-piece tables of the forward + adjoint kernel holds, per table entry, the sum of keep_op(u) over the entry's
// lanes: its sum over all entries (plus what the dropped lanes contribute) is d/dc of hsum(map_op(u)) for u = a x +- c -- one small
// fold over data that is already in memory.  Every lane forms the values of four consecutive entries exactly as the scatter_add
// fold would write them into a fresh table (fixed-point pieces added as integers and converted once, float pieces on top), adds
// them in entry order, the workgroup adds its lanes by wave shuffles, and the LAST workgroup to arrive (finish ticket) adds the
// workgroups' partials in index order: the order of all additions is a function of the entry index alone -- no fp atomics.
/// Entries [k0, k0 + lim) of ONE plane of the fixed-point per-piece tables (`partials`: the plane's first slot; pieces [p0, p1) of the
/// entries' bucket): v[j] = (the integer sum, converted once) * back + the float pieces' sum -- the arithmetic of k_fold_fixed_pieces,
/// statement for statement (that kernel keeps its own copy: its code is the headline step's and does not move).
__device__ __forceinline__ void fixed_piece_sums_at(const long long *__restrict__ partials, const uint32_t *__restrict__ piece_mode,
                                                    const uint32_t p0, const uint32_t p1, const uint32_t local, const int lim,
                                                    const int shift, const float back, float (&v)[kFoldPerLane]) {
    // (128 bits: a piece's sums stay below 2^62 by the choice of the scale, a skewed bucket of many pieces may not)
    unsigned long long ilo[kFoldPerLane];
    long long ihi[kFoldPerLane];
    float fsum[kFoldPerLane];
#pragma unroll
    for (int j = 0; j < kFoldPerLane; ++j) { ilo[j] = 0; ihi[j] = 0; fsum[j] = 0.f; }
    if (p1 - p0 == 1u) {
        // a bucket that is one piece wrote floats whatever it ran under (bucketed_early.hip): no mode to wait for, a quarter of the bytes
        const float *slotf = reinterpret_cast<const float *>(partials + ((size_t) p0 << shift));
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) fsum[j] = __builtin_nontemporal_load(slotf + local + j);
    } else
    for (uint32_t p = p0; p < p1; ++p) {
        // (mode and sums requested together: the 64-bit words of a slot can be read whatever the piece wrote into it)
        const long long *slot = partials + ((size_t) p << shift);
        const uint32_t mode = piece_mode[p];
        long long w[kFoldPerLane];
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) w[j] = j < lim ? __builtin_nontemporal_load(slot + local + j) : 0ll;
        if (mode == 0u) {
#pragma unroll
            for (int j = 0; j < kFoldPerLane; ++j) {
                const unsigned long long before = ilo[j];
                ilo[j] += (unsigned long long) w[j];
                ihi[j] += (w[j] >> 63) + (ilo[j] < before ? 1 : 0);
            }
        } else {
            const float *slotf = reinterpret_cast<const float *>(slot);
#pragma unroll
            for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) fsum[j] += slotf[local + j];
        }
    }
#pragma unroll
    for (int j = 0; j < kFoldPerLane; ++j) {
        // (one conversion of the exact integer: the same integer gives the same float whatever the pieces were)
        const bool narrow = ihi[j] == ((long long) ilo[j] >> 63);
        const float s = narrow ? (float) (long long) ilo[j] : (float) ((double) ihi[j] * 18446744073709551616.0 + (double) ilo[j]);
        v[j] = s * back + fsum[j];
    }
}


template <typename T>
__device__ __forceinline__ T addend_adjoint_block_sum(T v, T *wave_part /* [4] shared */) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += bucket_shfl_down(v, d);
    __syncthreads();                                  // (wave_part may still be read by an earlier round)
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

/// the workgroups' partials in index order, the dropped lanes' map_op(+-c) each (NaN: one of them carried a non-finite x), the factor
template <typename T>
__device__ __forceinline__ void addend_adjoint_finish(T *__restrict__ out, const T *__restrict__ block_partials, unsigned count,
                                                      const uint32_t *__restrict__ active, size_t n, int map_op, T zero_u, T scale,
                                                      T *wave_part) {
    using Bits = std::conditional_t<sizeof(T) == 4, uint32_t, unsigned long long>;
    T v = T(0);
    for (unsigned i = threadIdx.x; i < count; i += 256) {
        const Bits b = __hip_atomic_load(reinterpret_cast<const Bits *>(block_partials) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        T p;
        __builtin_memcpy(&p, &b, sizeof(T));
        v += p;
    }
    const T r = addend_adjoint_block_sum(v, wave_part);
    if (threadIdx.x == 0) {
        const T all = bucket_dropped_lanes<T, EK_HSUM>(r, active ? n - (size_t) active[0] : 0, active && active[1], map_op, zero_u);
        out[0] = scale != T(1) ? all * scale : all;
    }
}

template <typename T, bool Fixed>
__global__ __launch_bounds__(256) void k_addend_adjoint_fold(T *__restrict__ out, T *__restrict__ block_partials, uint32_t *__restrict__ ticket,
                                                             const void *__restrict__ plane0, const uint32_t *__restrict__ piece_mode,
                                                             const uint32_t *__restrict__ piece_prefix, size_t table_size, int shift,
                                                             const uint32_t *__restrict__ xmax_bits, int S0,
                                                             const uint32_t *__restrict__ active, size_t n, int map_op, T zero_u, T scale) {
    using Bits = std::conditional_t<sizeof(T) == 4, uint32_t, unsigned long long>;
    __shared__ T wave_part[4];
    __shared__ uint32_t s_last;
    const size_t k0 = ((size_t) blockIdx.x * 256 + threadIdx.x) * kFoldPerLane;
    T v = T(0);
    if (k0 < table_size) {
        const uint32_t b = (uint32_t) (k0 >> shift), local = (uint32_t) (k0 & (((size_t) 1 << shift) - 1));
        const uint32_t p0 = piece_prefix[b], p1 = piece_prefix[b + 1];
        const int lim = (int) (table_size - k0 < (size_t) kFoldPerLane ? table_size - k0 : (size_t) kFoldPerLane);
        T e[kFoldPerLane];
        if constexpr (Fixed) {
            fixed_piece_sums_at((const long long *) plane0, piece_mode, p0, p1, local, lim, shift, fixed_scale(S0, xmax_bits[0], false).back, e);
        } else {
            const T *partials = (const T *) plane0;
#pragma unroll
            for (int j = 0; j < kFoldPerLane; ++j) e[j] = T(0);
            for (uint32_t p = p0; p < p1; ++p) {
                const T *slot = partials + ((size_t) p << shift) + local;
#pragma unroll
                for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) e[j] += __builtin_nontemporal_load(slot + j);
            }
        }
#pragma unroll
        for (int j = 0; j < kFoldPerLane; ++j) if (j < lim) v += T(0) + e[j];      // (0 + e: the entry of a fresh table, as the fold writes it)
    }
    const T r = addend_adjoint_block_sum(v, wave_part);
    if (threadIdx.x == 0) {
        Bits bits;
        __builtin_memcpy(&bits, &r, sizeof(T));
        __hip_atomic_store(reinterpret_cast<Bits *>(block_partials) + blockIdx.x, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket && finish_ticket(ticket);
    }
    __syncthreads();
    if (!s_last) return;
    addend_adjoint_finish<T>(out, block_partials, gridDim.x, active, n, map_op, zero_u, scale, wave_part);
    if (threadIdx.x == 0) finish_ticket_reset(ticket);
}

/// objects without a finish ticket (8-byte element types): the last step as a launch of its own
template <typename T>
__global__ __launch_bounds__(256) void k_addend_adjoint_final(T *__restrict__ out, const T *__restrict__ block_partials, unsigned count,
                                                              const uint32_t *__restrict__ active, size_t n, int map_op, T zero_u, T scale) {
    __shared__ T wave_part[4];
    addend_adjoint_finish<T>(out, block_partials, count, active, n, map_op, zero_u, scale, wave_part);
}

template <typename T> __global__ void k_scale_one(T *__restrict__ out, T scale) { out[0] = out[0] * scale; }

/// out[0] = scale * (the sum of plane 0 over the entries + the dropped lanes' terms when `count_dropped`): the object holds early
/// sums of map_op
template <typename T>
static int bucketed_addend_adjoint_fold(Bucketed *b, int map_op, T scale, void *out, bool count_dropped) {
    Context &c = ctx();
    const unsigned grid = fold_grid(b->table_size);
    Scratch partials;
    if (int rc = partials.alloc((size_t) grid * sizeof(T))) return rc;
    const uint32_t *active = count_dropped ? b->masked_ptr() : nullptr;
    const uint32_t *xmax = b->early_fixed ? b->active + (kPgMetaResultXmax - kPgMetaResult) : nullptr;
    const size_t slot = b->early_fixed ? sizeof(long long) : sizeof(T);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, c.stream, (T *) out, (T *) partials.ptr, b->ticket, (const void *) b->early,
                           (const uint32_t *) b->early_modes, (const uint32_t *) b->piece_prefix, b->table_size, b->shift, xmax, b->early_S0,
                           active, b->n, map_op, b->template dropped_u<T>(), scale);
    };
    if constexpr (std::is_same_v<T, float>) {
        if (b->early_fixed) go(k_addend_adjoint_fold<float, true>); else go(k_addend_adjoint_fold<float, false>);
    } else {
        go(k_addend_adjoint_fold<T, false>);
    }
    EK_LAUNCH_CHECK("addend_adjoint_fold", b->table_size, (size_t) b->max_pieces * b->bins() * slot + (size_t) grid * sizeof(T));
    if (!b->ticket) {
        hipLaunchKernelGGL((k_addend_adjoint_final<T>), dim3(1), dim3(256), 0, c.stream, (T *) out, (const T *) partials.ptr, grid, active,
                           b->n, map_op, b->template dropped_u<T>(), scale);
        EK_LAUNCH_CHECK("reduce_stage2", (size_t) grid, (size_t) grid * sizeof(T) + sizeof(T));
    }
    return EK_OK;
}

template <typename T>
static int bucketed_scatter_add(Bucketed *b, int count, void *const *bases, const int *from_u, const int *map_ops,
                                const uint64_t *imm_bits, const int *weighted, const int *fresh, const uint64_t *scale_bits) {
    RoctxRange range("enoki-hip: bucket-ordered scatter_add");
    T scale[4] = { T(1), T(1), T(1), T(1) };
    if (scale_bits)
        for (int s = 0; s < count; ++s) memcpy(&scale[s], &scale_bits[s], sizeof(T));
    if (b->has_early && count >= 1 && count <= 2) {
        // exactly the streams that the forward pass summed already -- early_op(u), and x * early_op(u)?  Fold them.
        bool match = true;
        for (int s = 0; s < count; ++s)
            match = match && from_u[s] && (map_ops ? map_ops[s] : (int) EK_COPY) == b->early_op;
        if (count == 2) match = match && (weighted[0] != 0) != (weighted[1] != 0);
        // (direct tables: a plane that a gradient array took over -- ek_hip_bucketed_take_tables -- is no longer here to be folded)
        if (b->early_direct)
            for (int s = 0; s < count; ++s) match = match && b->direct[weighted[s] ? 1 : 0] != nullptr;
        if (match) {
            Context &c = ctx();
            const size_t stride = (size_t) b->max_pieces * b->bins();
            const unsigned grid = fold_grid(b->table_size);
            if constexpr (std::is_same_v<T, float>) {
                if (b->early_fixed) {
                    const uint32_t *xmax = b->active + (kPgMetaResultXmax - kPgMetaResult);
                    // (direct tables -- a factor other than 1, a target that holds data, one fresh target of two: the same fold reads them)
                    const long long *slots = b->early_direct ? nullptr : (const long long *) b->early;
                    const float *direct0 = b->early_direct ? (const float *) b->direct[0] : nullptr;
                    const float *direct1 = b->early_direct ? (const float *) b->direct[1] : nullptr;
                    if (count == 2) {
                        const int s_plain = weighted[0] ? 1 : 0, s_weighted = 1 - s_plain;
                        FoldTargets<float, 2> targets;
                        targets.table[0] = (float *) bases[s_plain];
                        targets.table[1] = (float *) bases[s_weighted];
                        targets.scale[0] = scale[s_plain];
                        targets.scale[1] = scale[s_weighted];
                        const unsigned fr = fresh ? ((fresh[s_plain] ? 1u : 0u) | (fresh[s_weighted] ? 2u : 0u)) : 0u;
                        hipLaunchKernelGGL((k_fold_fixed_pieces<2>), dim3(grid, 2), dim3(256), 0, c.stream, targets, slots,
                                           (const uint32_t *) b->early_modes, (const uint32_t *) b->piece_prefix, b->table_size, stride, fr, b->shift,
                                           xmax, b->early_S0, 0, direct0, direct1);
                    } else {
                        FoldTargets<float, 1> targets;
                        targets.table[0] = (float *) bases[0];
                        targets.scale[0] = scale[0];
                        hipLaunchKernelGGL((k_fold_fixed_pieces<1>), dim3(grid, 1), dim3(256), 0, c.stream, targets, slots,
                                           (const uint32_t *) b->early_modes, (const uint32_t *) b->piece_prefix, b->table_size, stride,
                                           (fresh && fresh[0]) ? 1u : 0u, b->shift, xmax, b->early_S0, weighted[0] ? 1 : 0, direct0, direct1);
                    }
                    EK_LAUNCH_CHECK("scatter_add_fold", (size_t) count * b->table_size,
                                    (size_t) count * ((b->early_direct ? b->table_size * sizeof(T) : stride * sizeof(long long)) + 2 * b->table_size * sizeof(T)));
                    return EK_OK;
                }
            }
            if (count == 2) {
                // partial table 0: unweighted, 1: weighted
                const int s_plain = weighted[0] ? 1 : 0, s_weighted = 1 - s_plain;
                FoldTargets<T, 2> targets;
                targets.table[0] = (T *) bases[s_plain];
                targets.table[1] = (T *) bases[s_weighted];
                targets.scale[0] = scale[s_plain];
                targets.scale[1] = scale[s_weighted];
                const unsigned fr = fresh ? ((fresh[s_plain] ? 1u : 0u) | (fresh[s_weighted] ? 2u : 0u)) : 0u;
                hipLaunchKernelGGL((k_bin_fold_pieces<T, 2>), dim3(grid, 2), dim3(256), 0, c.stream, targets, (const T *) b->early,
                                   (const uint32_t *) b->piece_prefix, b->table_size, stride, fr, b->shift);
            } else {
                FoldTargets<T, 1> targets;
                targets.table[0] = (T *) bases[0];
                targets.scale[0] = scale[0];
                hipLaunchKernelGGL((k_bin_fold_pieces<T, 1>), dim3(grid, 1), dim3(256), 0, c.stream, targets,
                                   (const T *) b->early + (weighted[0] ? stride : 0), (const uint32_t *) b->piece_prefix,
                                   b->table_size, stride, (fresh && fresh[0]) ? 1u : 0u, b->shift);
            }
            EK_LAUNCH_CHECK("scatter_add_fold", (size_t) count * b->table_size,
                            (size_t) count * (stride * sizeof(T) + 2 * b->table_size * sizeof(T)));
            return EK_OK;
        }
    }
    bool need_u = false, all_kept = b->has_m;
    for (int s = 0; s < count; ++s) {
        need_u = need_u || from_u[s];
        if (from_u[s]) all_kept = all_kept && (map_ops ? map_ops[s] : (int) EK_COPY) == b->m_op;
    }
    // every stream that reads u wants exactly the half of sincos(u) that the forward kept: stream it as is
    const bool use_kept = need_u && all_kept;
    if (need_u && !use_kept && !b->has_u)
        if (int rc = bucketed_forward_launch<T, EK_REDUCE_NONE>(b, nullptr, EK_COPY, true)) return rc;
    const void *u_src = use_kept ? b->m_b : b->u_b;
    // two tables per launch: their LDS tables fill the 128 KiB a workgroup may use
    for (int s0 = 0; s0 < count; s0 += 2) {
        const int C = std::min(2, count - s0);
        T *tb[2] = { (T *) bases[s0], C == 2 ? (T *) bases[s0 + 1] : nullptr };
        if (C == 2) {
            BucketStreams<T, 2> st{};
            // the weighted stream second (the tape queues the adjoints of the addend and of the factor in either order): the
            // kernel has a compile-time form for { f(u), x * f(u) }
            const bool swap = weighted[s0] && !weighted[s0 + 1];
            if (swap) std::swap(tb[0], tb[1]);
            for (int s = 0; s < 2; ++s) {
                const int src = s0 + (swap ? 1 - s : s);
                st.map_op[s] = (map_ops && !use_kept) ? map_ops[src] : (int) EK_COPY;
                memcpy(&st.imm[s], &imm_bits[src], sizeof(T));
                st.scale[s] = scale[src];
                st.from_u |= (from_u[src] ? 1u : 0u) << s;
                st.weighted |= (weighted[src] ? 1u : 0u) << s;
            }
            const int f0 = swap ? s0 + 1 : s0, f1 = swap ? s0 : s0 + 1;
            const unsigned fr = fresh ? ((fresh[f0] ? 1u : 0u) | (fresh[f1] ? 2u : 0u)) : 0u;
            if (int rc = bucketed_accumulate<T, 2>(b, tb, st, u_src, fr)) return rc;
        } else {
            BucketStreams<T, 1> st{};
            st.map_op[0] = (map_ops && !use_kept) ? map_ops[s0] : (int) EK_COPY;
            memcpy(&st.imm[0], &imm_bits[s0], sizeof(T));
            st.scale[0] = scale[s0];
            st.from_u = from_u[s0] ? 1u : 0u;
            st.weighted = weighted[s0] ? 1u : 0u;
            if (int rc = bucketed_accumulate<T, 1>(b, tb, st, u_src, (fresh && fresh[s0]) ? 1u : 0u)) return rc;
        }
    }
    return EK_OK;
}

// ---- plain scatter_add(value, index, mask) through the page partition ------------------------------------------------------
// The LDS-binned scatter_add of scatter_binned.hip reads the indices twice and needs two scans before it can place a pair
// (count 5 + partition 15 + accumulate 6 B per pair, five launches).  The single-pass page partition of the bucket-ordered path
// does the same job for ONE f32 value stream in 14 + 6 B and three launches + the fold: the (index, value) pairs are partitioned
// into pages by bucket of 16 Ki table entries, every piece of a bucket adds its values into an LDS table under the exchange
// lock, the per-piece tables are folded into the target.  Same sums up to the order of the additions (class D, like the binned
// path); out-of-range indices and masked-out pairs are dropped.
int scatter_add_paged(float *base, size_t table_size, const float *value, const uint32_t *index, const Arg<uint8_t> &mask, size_t n) {
    RoctxRange range("enoki-hip: scatter_add (paged)");
    ek::Bucketed obj;
    obj.type = EK_F32; obj.index_type = EK_U32; obj.op = EK_FMADD;
    obj.n = n; obj.table_size = table_size;
    // 32-element pages above 128 buckets (2 - 4 Mi bins), by choice: the accumulation under the exchange locks does not gain from
    // 64-element pages what the partition does and loses on skewed indices (64 Mi adds into 4 Mi bins, same call: uniform 319 -> 302 us,
    // zipf(1.3) 1.96 -> 2.37 ms with bucket_accumulate 1.50 -> 1.99 ms; profiles/probe_paged_planes_r07.txt)
    if (int rc = bucketed_create_paged<uint32_t>(&obj, value, index, mask, bin_shift_of<float>, nullptr, /* pages32 */ true)) return rc;
    BucketStreams<float, 1> st{};
    st.map_op[0] = EK_COPY; st.imm[0] = 0.f; st.scale[0] = 1.f;
    st.from_u = 0u; st.weighted = 1u; st.plain_x = 1u;
    float *bases[1] = { base };
    return bucketed_accumulate<float, 1>(&obj, bases, st, nullptr, 0u);
}

bool scatter_add_paged_applicable(size_t table_size, size_t n) {
    // (from 32 buckets on: with a handful of buckets every element of a tile meets the same few LDS counters -- 64 Mi adds into
    // 64 Ki bins: 0.51 ms paged against 0.36 ms binned, 256 Ki bins: equal, 1 Mi: 0.28 against 0.33, 4 Mi: 0.31 against 0.39;
    // profiles/probe_scatter_paged_r05.txt)
    return ctx().tuning.bucket_ordered && !ctx().tuning.deterministic && n >= ((size_t) 1 << 18) && n < ((size_t) 1 << 30) &&
           table_size >= (size_t) 32 * bins_of<float> && table_size <= (size_t) kMaxBuckets * bins_of<float>;
}

// ---- scatter_add(value, index, mask) into a table beyond 256 buckets, sized on the device ----------------------------------------
// The adjoint of every gather from a large table that is not in the bucket-ordered menu, and a plain scatter_add from user code.
// (index, value) are split by slice of 256 buckets (coarse_split: masked-out pairs and indices beyond the last slice are dropped
// there), every slice partitions its own run into ONE page pool (k_page_partition<.., DevRange> + k_page_directory<true>, its size
// read from range[s] on entry), then ONE launch adds the pairs of all slices' pieces in the LDS and ONE launch folds the per-piece
// tables into base + s * span.  Nothing is read back and the host decides nothing from the index values: the call can be part of a
// captured step graph, and every replay follows the slice populations it finds.  An empty slice has no pieces, its fold adds nothing.
//
// The two launches over all slices number the pieces FLAT: slice s owns pieces [P_s, P_s + q_s), q_s = the last entry of its piece
// prefix, P_s the sum of those of the slices before it -- S <= 64 words that one wave of every workgroup reads and scans.  A piece's
// workgroup then finds its bucket and its pages in slice s's lists, which lie a fixed stride apart (SliceLists: 48 bytes of kernel
// arguments whatever S is; no descriptor table to copy to the device).  The piece budget of one unsliced call is dealt to the slices
// by population on the device (k_slice_ranges), so the partial tables of all slices together are `budget + S + one per bucket`.
struct SliceLists {
    const uint32_t *meta;          // S counter blocks, meta_stride words apart: counters | base_full[257] | base_part[257] | piece_prefix[257]
    const uint32_t *glist_full;    // the pool's full-page list (the slices' bases are pool positions)
    const uint32_t *glist_part;    // S lists, part_stride entries apart
    uint32_t meta_stride, part_stride;
    size_t table_size;
    int S, shift;
};
constexpr uint32_t kSliceBaseFull = kPgCounterWords, kSliceBasePart = kSliceBaseFull + kMaxBuckets + 1,
                   kSlicePiecePrefix = kSliceBasePart + kMaxBuckets + 1;

__device__ __forceinline__ int slice_buckets(const SliceLists &sl, int s) {
    const size_t span = (size_t) kMaxBuckets << sl.shift, left = sl.table_size - (size_t) s * span;
    return (int) (((left < span ? left : span) + ((size_t) 1 << sl.shift) - 1) >> sl.shift);
}
/// lane s < S of the calling wave: pieces of slice s in `count`, and of slices 0 .. s in the result
__device__ __forceinline__ uint32_t slice_piece_scan(const SliceLists &sl, int s, uint32_t &count) {
    count = s < sl.S ? sl.meta[(size_t) s * sl.meta_stride + kSlicePiecePrefix + slice_buckets(sl, s)] : 0u;
    uint32_t incl = count;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (s >= d) incl += up;
    }
    return incl;
}
__device__ __forceinline__ BucketLists slice_lists(const SliceLists &sl, int s) {
    const uint32_t *m = sl.meta + (size_t) s * sl.meta_stride;
    return BucketLists{ m + kSliceBaseFull, m + kSlicePiecePrefix, m + kSliceBasePart, sl.glist_full,
                        sl.glist_part + (size_t) s * sl.part_stride, slice_buckets(sl, s) };
}

/// grid: the bound on the pieces of all slices together; a workgroup beyond the pieces that exist leaves at once
template <int V>
__global__ __launch_bounds__(kBucketThreads) void k_bucket_accumulate_slices(float *__restrict__ partials,
                                                                             const uint16_t *__restrict__ pair_idx,
                                                                             const float *__restrict__ x_b, SliceLists sl) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float *acc = reinterpret_cast<float *>(lds_raw);
    __shared__ uint32_t s_slice[3];                 // the slice of piece blockIdx.x, its first piece, pieces of all slices
    const int Bins = 1 << sl.shift;
    if (threadIdx.x < 64) {
        uint32_t count;
        const uint32_t incl = slice_piece_scan(sl, (int) threadIdx.x, count);
        if (incl - count <= blockIdx.x && blockIdx.x < incl) { s_slice[0] = threadIdx.x; s_slice[1] = incl - count; }
        if (threadIdx.x == 63) s_slice[2] = incl;
    }
    __syncthreads();
    if (blockIdx.x >= s_slice[2]) return;
    const BucketLists bl = slice_lists(sl, (int) s_slice[0]);
    int bucket;
    PieceRange range;
    if (!bucket_piece_at<5>(bl, blockIdx.x - s_slice[1], bucket, range)) return;
    for (int j = threadIdx.x; j < Bins; j += kBucketThreads) acc[j] = 0.f;
    __syncthreads();
    AccumulateBody<float, 1, V, EK_COPY, 2> body{};
    body.acc = acc; body.pair_idx = pair_idx; body.u_b = nullptr; body.x_b = x_b; body.Bins = Bins;
    body.need_u = false; body.need_x = true;
    walk_piece<5, V>(bl, range, body);
    __syncthreads();
    float *out = partials + (size_t) blockIdx.x * Bins;
    for (int j = threadIdx.x; j < Bins; j += kBucketThreads) out[j] = acc[j];
}

/// target[k] += the partial tables of the pieces of k's bucket; a workgroup covers 1024 consecutive entries: one bucket of one slice
__global__ __launch_bounds__(256) void k_bin_fold_slices(float *__restrict__ target, const float *__restrict__ partials, SliceLists sl) {
    __shared__ uint32_t s_first;                    // first piece of this workgroup's slice
    const size_t kb = (size_t) blockIdx.x * 256 * kFoldPerLane;
    const int s = (int) (kb >> (sl.shift + 8));
    if (threadIdx.x < 64) {
        uint32_t count;
        const uint32_t incl = slice_piece_scan(sl, (int) threadIdx.x, count);
        if ((int) threadIdx.x == s) s_first = incl - count;
    }
    __syncthreads();
    const size_t k0 = kb + (size_t) threadIdx.x * kFoldPerLane;
    if (k0 >= sl.table_size) return;
    const uint32_t b = (uint32_t) (k0 >> sl.shift) & (kMaxBuckets - 1), local = (uint32_t) (k0 & (((size_t) 1 << sl.shift) - 1));
    const uint32_t *piece_prefix = sl.meta + (size_t) s * sl.meta_stride + kSlicePiecePrefix;
    const uint32_t p0 = s_first + piece_prefix[b], p1 = s_first + piece_prefix[b + 1];
    fold_pieces_at<float, 8>(target, partials, p0, p1, k0, local, sl.table_size, sl.shift, false, 1.f);
}

static bool scatter_paged_enabled() {
    static const bool paged = [] { const char *e = getenv("ENOKI_HIP_SCATTER_PAGED"); return !e || atoi(e) != 0; }();
    return paged;
}

bool scatter_add_sliced_applicable(size_t table_size, size_t n) {
    constexpr size_t span = (size_t) kMaxBuckets * bins_of<float>;
    return scatter_paged_enabled() && ctx().tuning.bucket_ordered && !ctx().tuning.deterministic && n >= ((size_t) 1 << 18) &&
           n < ((size_t) 1 << 30) && table_size > span && table_size <= (size_t) kMaxSlices * span;
}

int scatter_add_sliced(float *base, size_t table_size, const float *value, const uint32_t *index, const Arg<uint8_t> &mask, size_t n) {
    RoctxRange range("enoki-hip: scatter_add (slices, paged)");
    Context &c = ctx();
    constexpr int Shift = bin_shift_of<float>;
    constexpr size_t Bins = bins_of<float>, span = (size_t) kMaxBuckets * Bins;
    const int S = (int) ((table_size + span - 1) / span);
    if (S < 2 || S > kMaxSlices) return fail(EK_ERR_UNSUPPORTED, "scatter_add_sliced(): %zu bins", table_size);
    // the piece budget: what one unsliced call takes (one piece per CU) per slice up to FOUR slices -- never fewer pieces than the
    // host-sized path gave a table of up to 16 Mi bins -- and no more beyond; dealt to the slices by population on the device (every
    // populated bucket has a piece of its own on top).  With ONE call's budget over all slices a zipf-distributed index array, whose
    // hot bin holds a quarter of the pairs, left that bin to 64 pieces: accumulate 2.17 ms against 1.78 ms (64 Mi adds, K = 16 Mi).
    const uint32_t budget = (uint32_t) bucket_target_pieces(n, kMaxBuckets) * (uint32_t) std::min(S, 4);
    const size_t total_buckets = (table_size + Bins - 1) / Bins, max_pieces = (size_t) budget + (size_t) S + total_buckets;
    CoarseSplit cs;
    if (int rc = coarse_split<Shift + 8>(cs, value, index, mask, n, S, budget)) return rc;
    // every slice with the geometry of a full one (256 buckets; the pool is built on 32-element pages) and the whole input as its bound
    const PagedPlan plan = paged_plan(n, kMaxBuckets, c.num_cu, false, false, /* pages32 */ true);
    if (plan.page_shift != 5 || plan.W > 1024) return fail(EK_ERR_UNSUPPORTED, "scatter_add_sliced(): %u workgroups", plan.W);
    const size_t pool_pages = paged_slice_pool_pages(cs.elements, S, plan.W, plan.page_shift);
    const uint32_t meta_stride = (kSlicePiecePrefix + kMaxBuckets + 1 + 3u) & ~3u, part_stride = plan.W * (uint32_t) kMaxBuckets + 1u;
    Bucketed pool;                              // owns the page pool, the full-page list, all slices' glist_part and counter blocks
    pool.type = EK_F32; pool.index_type = EK_U32; pool.op = EK_FMADD;
    pool.n = n; pool.table_size = table_size;
    pool.positions = pool_pages << plan.page_shift;
    if (int rc = ek_hip_malloc(pool.positions * sizeof(uint16_t), &pool.pair_idx)) return rc;
    if (int rc = ek_hip_malloc(pool.positions * sizeof(float), &pool.x_b)) return rc;
    if (int rc = ek_hip_malloc((pool_pages + (size_t) S * part_stride) * sizeof(uint32_t), &pool.page_lists)) return rc;
    if (int rc = ek_hip_malloc((size_t) S * meta_stride * sizeof(uint32_t), &pool.meta)) return rc;
    Scratch work, partials;
    if (int rc = work.alloc((2 * pool_pages + 3 * (size_t) plan.W * kMaxBuckets) * sizeof(uint32_t))) return rc;
    if (int rc = partials.alloc(max_pieces * Bins * sizeof(float))) return rc;
    uint32_t *glist_full = (uint32_t *) pool.page_lists, *glist_part = glist_full + pool_pages;
    EK_HIP_CHECK(hipMemsetAsync(pool.meta, 0, (size_t) S * meta_stride * sizeof(uint32_t), c.stream));
    note_launch("bucket_meta_clear", (size_t) S * meta_stride, (size_t) S * meta_stride * sizeof(uint32_t));
    const Arg<uint8_t> all{ nullptr, 1, 0u };
    for (int s = 0; s < S; ++s) {
        Bucketed sub;
        sub.type = EK_F32; sub.index_type = EK_U32; sub.op = EK_FMADD;
        sub.n = n;                              // (the bound: the slice's own size is range[2 s + 1], on the device)
        sub.table_size = std::min(span, table_size - (size_t) s * span);
        sub.win_lo = 0;
        sub.win_span = (uint32_t) sub.table_size;
        PagedSlice ps{ cs.range + 2 * s, (uint32_t) s * paged_slice_gap(plan.W, plan.page_shift), &plan, &pool, glist_full,
                       (uint32_t *) work.ptr, pool_pages };
        ps.meta = (uint32_t *) pool.meta + (size_t) s * meta_stride;
        ps.glist_part = glist_part + (size_t) s * part_stride;
        ps.piece_share = cs.share + s;
        if (int rc = bucketed_create_paged<uint32_t>(&sub, (const float *) cs.x, (const uint32_t *) cs.idx, all, Shift, &ps)) return rc;
    }
    const SliceLists sl{ (const uint32_t *) pool.meta, glist_full, glist_part, meta_stride, part_stride, table_size, S, Shift };
    constexpr int VV = 2;                       // as bucketed_accumulate<float, 1>
    const size_t lds = Bins * sizeof(float);
    if (int rc = allow_big_lds(k_bucket_accumulate_slices<VV>, lds)) return rc;
    hipLaunchKernelGGL((k_bucket_accumulate_slices<VV>), dim3((unsigned) max_pieces), dim3(kBucketThreads), lds, c.stream,
                       (float *) partials.ptr, (const uint16_t *) pool.pair_idx, (const float *) pool.x_b, sl);
    EK_LAUNCH_CHECK("bucket_accumulate", n, n * (sizeof(uint16_t) + sizeof(float)) + max_pieces * Bins * sizeof(float));
    hipLaunchKernelGGL(k_bin_fold_slices, dim3(fold_grid(table_size)), dim3(256), 0, c.stream, base, (const float *) partials.ptr, sl);
    EK_LAUNCH_CHECK("scatter_add_fold", table_size, max_pieces * Bins * sizeof(float) + 2 * table_size * sizeof(float));
    return EK_OK;
}

// ---- partition of an index array alone (ek_hip_index_partition_*) ------------------------------------------------------
struct IndexPartition {
    ek_hip_index_partition_info info{};
    void *meta = nullptr, *local = nullptr, *lists = nullptr;
    ~IndexPartition() {
        for (void *p : { meta, local, lists })
            if (p) ek_hip_free(p);
    }
};

// The index array alone through the single-pass page partition (k_page_partition<.., IndexOnly>): idx 4 (+ mask 1) read, 4 written per
// entry, two launches -- instead of count + two scans + partition (idx read twice: 14 B per entry, four launches; 124 us of cfg4's 245 us
// step at 32 Mi rays).  4-byte records give every one of up to 256 buckets two 64-element pages of LDS.
static int index_partition_run_paged(IndexPartition *ip, const uint32_t *index, const Arg<uint8_t> &mask, size_t n, int n_buckets, int shift) {
    RoctxRange range("enoki-hip: index partition (pages)");
    Context &c = ctx();
    const PagedPlan p = paged_plan(n, n_buckets, c.num_cu, false, true);
    if (p.W > 1024) return fail(EK_ERR_UNSUPPORTED, "ek_hip_index_partition_create(): %u workgroups", p.W);
    const size_t meta_words = kPgCounterWords + 3 * (kMaxBuckets + 1) + 1;
    if (int rc = ek_hip_malloc(meta_words * sizeof(uint32_t), &ip->meta)) return rc;
    if (int rc = ek_hip_malloc((p.page_slots << p.page_shift) * sizeof(uint32_t), &ip->local)) return rc;
    const size_t part_entries = (size_t) p.W * n_buckets;
    if (int rc = ek_hip_malloc((p.page_slots + part_entries + 1) * sizeof(uint32_t), &ip->lists)) return rc;
    uint32_t *gtotal = (uint32_t *) ip->meta, *base_full = gtotal + kPgCounterWords, *base_part = base_full + kMaxBuckets + 1,
             *piece_prefix = base_part + kMaxBuckets + 1;
    uint32_t *glist_full = (uint32_t *) ip->lists, *glist_part = glist_full + p.page_slots;
    Scratch work;
    if (int rc = work.alloc((2 * p.page_slots + 3 * part_entries) * sizeof(uint32_t))) return rc;
    PagedOut<float> out{};
    out.lp = nullptr;
    out.xp = (float *) ip->local;
    out.wdir = (uint32_t *) work.ptr;
    out.wlist = out.wdir + p.page_slots;
    out.cnt_full = out.wlist + p.page_slots;
    out.loff = out.cnt_full + part_entries;
    out.part = out.loff + part_entries;
    out.gtotal = gtotal;
    out.active = gtotal + kPgMetaBase + kPgMetaAccum;
    out.lo = 0; out.span = (uint32_t) std::min<size_t>(ip->info.range, 0xFFFFFFFFu);
    out.class_w = nullptr; out.class_stamp = nullptr; out.class_band = kPgWeightBand;
    // (a kernel of our own: the runtime's memset is a launch with its own barrier packets around it -- the step's widest gap)
    if (int rc = ek_hip_fill(EK_U32, gtotal, 0, kPgCounterWords)) return rc;
    const int vec_ok = aligned16(index) && arg_aligned(mask);
    auto launch = [&](auto kernel) -> int {
        size_t lds = p.lds;
        out.wdir_lds = 0;
        const size_t fixed_lds = static_lds_of(kernel);
        if (fixed_lds != SIZE_MAX && fixed_lds + p.lds + (size_t) p.slots * sizeof(uint32_t) <= (size_t) 160 * 1024) {
            lds += (size_t) p.slots * sizeof(uint32_t);
            out.wdir_lds = 1;
        }
        if (int rc = allow_big_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3(p.W), dim3(kPgThreads), lds, c.stream, out, index, mask, (const float *) nullptr, n, p.chunk, n_buckets,
                           shift, p.cap, p.slots, vec_ok);
        return EK_OK;
    };
    int rc;
    if (p.page_shift == 6) rc = mask.vec ? launch(k_page_partition<float, uint32_t, 6, true, true>) : launch(k_page_partition<float, uint32_t, 6, false, true>);
    else rc = mask.vec ? launch(k_page_partition<float, uint32_t, 5, true, true>) : launch(k_page_partition<float, uint32_t, 5, false, true>);
    if (rc) return rc;
    EK_LAUNCH_CHECK("index_partition", n, n * 2 * sizeof(uint32_t) + arg_bytes(mask, n));
    hipLaunchKernelGGL(k_page_directory<false>, dim3(n_buckets, kPgDirSlices), dim3(256), 0, c.stream, glist_full, glist_part, base_full,
                       base_part, piece_prefix, gtotal, (const uint32_t *) out.cnt_full, (const uint32_t *) out.loff,
                       (const uint32_t *) out.part, (const uint32_t *) out.wlist, p.W, p.slots, n_buckets, 0u,
                       (uint32_t *) nullptr, (const uint32_t *) nullptr, kPgWeightBand, (const uint32_t *) nullptr, 0u, 0);
    EK_LAUNCH_CHECK("index_partition_directory", p.page_slots, 2 * p.page_slots * sizeof(uint32_t));
    ip->info.bucket_base = base_full;
    ip->info.local = (const uint32_t *) ip->local;
    ip->info.page_shift = p.page_shift;
    ip->info.pages_full = glist_full;
    ip->info.pages_part = glist_part;
    ip->info.part_base = base_part;
    return EK_OK;
}

template <typename I, int Shift>
static int index_partition_run(IndexPartition *ip, const I *index, const Arg<uint8_t> &mask, size_t n, int n_buckets) {
    RoctxRange range("enoki-hip: index partition");
    Context &c = ctx();
    unsigned blocks = (unsigned) std::min<size_t>((size_t) c.num_cu * 4, (n + kTile - 1) / kTile);
    if (blocks == 0) blocks = 1;
    size_t chunk = (n + blocks - 1) / blocks;
    chunk = (chunk + kTile - 1) / kTile * kTile;
    blocks = (unsigned) ((n + chunk - 1) / chunk);
    const int vec_ok = aligned16(index) && arg_aligned(mask);
    int rep_shift = 0;
    while ((n_buckets << (rep_shift + 1)) <= kMaxBuckets && rep_shift < 4) ++rep_shift;
    const size_t count_entries = (size_t) n_buckets * blocks;
    if (int rc = ek_hip_malloc((count_entries + 2 * kMaxBuckets + 2) * sizeof(uint32_t), &ip->meta)) return rc;
    if (int rc = ek_hip_malloc((n ? n : 1) * sizeof(uint32_t), &ip->local)) return rc;
    uint32_t *counts = (uint32_t *) ip->meta, *row_total = counts + count_entries, *bucket_base = row_total + kMaxBuckets;
    hipLaunchKernelGGL((k_bin_count<I, Shift>), dim3(blocks), dim3(kThreads), 0, c.stream, counts, index, mask, n, chunk, n_buckets,
                       rep_shift, vec_ok);
    EK_LAUNCH_CHECK("index_partition_count", n, n * sizeof(I) + arg_bytes(mask, n));
    hipLaunchKernelGGL(k_bin_scan_rows, dim3(n_buckets), dim3(1024), 0, c.stream, counts, row_total, blocks);
    hipLaunchKernelGGL(k_bin_scan_buckets, dim3(1), dim3(256), 0, c.stream, bucket_base, (uint32_t *) nullptr,
                       (const uint32_t *) row_total, n_buckets, 0u);
    EK_LAUNCH_CHECK("index_partition_scan", count_entries, 2 * count_entries * sizeof(uint32_t));
    BinStreams<uint32_t, 1> st{};
    st.value[0] = Arg<uint32_t>{ nullptr, 0u, 0u };
    st.weight[0] = Arg<uint32_t>{ nullptr, 1u, 0u };
    st.pair_val[0] = nullptr;
    st.value_op[0] = EK_COPY;
    hipLaunchKernelGGL((k_bin_partition<uint32_t, I, Shift, uint32_t, 1, false, true>), dim3(blocks), dim3(kThreads), 0, c.stream,
                       (uint32_t *) ip->local, st, (const uint32_t *) counts, (const uint32_t *) bucket_base, index, mask, n, chunk,
                       n_buckets, 0, vec_ok);
    EK_LAUNCH_CHECK("index_partition", n, n * (sizeof(I) + sizeof(uint32_t)) + arg_bytes(mask, n));
    ip->info.bucket_base = bucket_base;
    ip->info.local = (const uint32_t *) ip->local;
    return EK_OK;
}

} // namespace ek

using namespace ek;

// A table beyond 256 buckets is cut into SLICES of 256 buckets: one object per slice, each made by a pass over (index, x) that
// keeps the indices of its slice (PagedOut::lo / span) -- S passes of 8 B/elt instead of one, still without a lookup that
// leaves the CU.  Reductions combine the slices' results (and add the masked-out lanes' terms once), the scatter_add of slice s
// goes to entries [s span, (s + 1) span) of its tables.
struct ek_hip_bucketed : ek::Bucketed {
    std::vector<ek_hip_bucketed *> slices;
    void *addend_table = nullptr;    // owned: the addend table of an object made from a DEVICE scalar (ek_hip_bucketed_pair_create_scalar_device)
    const void *partitioned[3] = { nullptr, nullptr, nullptr };   // index, x, mask as the creation saw them (ek_hip_bucketed_partition_retain asks where they live)
    size_t slice_span = 0;
    bool slices_split = false;       // the slices hold disjoint parts of the input (CoarseSplit) instead of filtered views of all of it
    ~ek_hip_bucketed() { for (ek_hip_bucketed *s : slices) delete s; if (addend_table) ek_hip_free(addend_table); }
};
struct SliceCounts { const uint32_t *active[kMaxSlices]; const uint32_t *flag; };

template <typename T, int ROp>
__global__ __launch_bounds__(64) void k_slices_combine(T *__restrict__ out, const T *__restrict__ partial, int slices, SliceCounts counts,
                                                       size_t n, int map_op, T zero_u) {
    using R = ek::BucketReducer<ROp, T>;
    if (threadIdx.x != 0) return;
    T r = R::identity();
    size_t kept = 0;
    bool nonfinite = counts.flag && counts.flag[0];
    for (int s = 0; s < slices; ++s) { r = R::combine(r, partial[s]); kept += counts.active[s][0]; nonfinite = nonfinite || counts.active[s][1]; }
    out[0] = ek::bucket_dropped_lanes<T, ROp>(r, n - kept, nonfinite, map_op, zero_u);
}

/// ek_hip_bucketed_addend_adjoint over the slices of a large table: the slices' sums in slice order, the lanes NO slice kept counted
/// once, the caller's factor -- one rounding behind the sum, as the last workgroup of k_addend_adjoint_fold applies it
__global__ __launch_bounds__(64) void k_addend_adjoint_combine(float *__restrict__ out, const float *__restrict__ partial, int slices,
                                                               SliceCounts counts, size_t n, int map_op, float zero_u, float scale) {
    if (threadIdx.x != 0) return;
    float r = 0.f;
    size_t kept = 0;
    bool nonfinite = counts.flag && counts.flag[0];
    for (int s = 0; s < slices; ++s) { r += partial[s]; kept += counts.active[s][0]; nonfinite = nonfinite || counts.active[s][1]; }
    const float all = ek::bucket_dropped_lanes<float, EK_HSUM>(r, n - kept, nonfinite, map_op, zero_u);
    out[0] = scale != 1.f ? all * scale : all;
}

// (tables of three or more slices under a mask: the split by slice drops the masked-out lanes before any page partition sees
// them, so their x is looked at here -- 5 B/elt of a shape that already pays 20 B/elt for the split)
__global__ __launch_bounds__(256) void k_masked_nonfinite(uint32_t *__restrict__ flag, const uint32_t *__restrict__ xbits,
                                                          const uint8_t *__restrict__ mask, size_t n) {
    bool bad = false;
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t) gridDim.x * 256)
        bad = bad || (!mask[i] && (xbits[i] & 0x7F800000u) == 0x7F800000u);
    if (bad) atomicOr(flag, 1u);
}
struct ek_hip_index_partition : ek::IndexPartition { };


extern "C" {

int ek_hip_bucketed_applicable(int type, int index_type, size_t table_size, size_t n) {
    if (type != EK_F32 && type != EK_F64) return 0;
    if (index_type != EK_U32 && index_type != EK_I32) return 0;
    if (ctx().tuning.deterministic || !ctx().tuning.bucket_ordered) return 0;
    const size_t bins = type == EK_F64 ? (size_t) bins_of<double> : (size_t) bins_of<float>;
    // (4-byte types go through pages whose numbers are packed with an element count: 2^30 elements at most; their tables may
    // have up to kMaxSlices slices of 256 half-size buckets)
    return n >= ((size_t) 1 << 18) && n < ((size_t) 1 << (type == EK_F64 ? 32 : 30)) && table_size > bins &&
           table_size <= (size_t) kMaxBuckets * bins * (type == EK_F64 ? 1 : kMaxSlices / 2);
}

int ek_hip_bucketed_pair_create(int type, int index_type, int op, const void *table_a, const void *table_c, size_t table_size,
                                const void *x, const void *index, size_t n, ek_hip_bucketed **out) {
    return ek_hip_bucketed_pair_create_hinted(type, index_type, op, table_a, table_c, table_size, x, index, n, 0u, out);
}

int ek_hip_bucketed_pair_create_hinted(int type, int index_type, int op, const void *table_a, const void *table_c, size_t table_size,
                                       const void *x, const void *index, size_t n, unsigned hints, ek_hip_bucketed **out) {
    return ek_hip_bucketed_pair_create_masked(type, index_type, op, table_a, table_c, table_size, x, index, nullptr, n, hints, out);
}

/// The bucket shift of a float table that ONE paged object covers, as the hints and the tuning select it; -1: the table is cut
/// into slices.  (What an object asks of a partition it wants to stand on: the same shift, ek_hip_bucketed_pair_create_on.)
static int paged_single_shift(size_t table_size, unsigned hints) {
    const size_t bins = (size_t) bins_of<float>;
    const bool adjoint = (hints & EK_BUCKETED_HINT_ADJOINT) && ctx().tuning.early_adjoint;
    const bool want_half = adjoint && table_size <= (size_t) 2 * kMaxBuckets * (bins / 2);
    if (table_size > (size_t) kMaxBuckets * (want_half ? bins / 2 : bins)) return -1;
    const bool half = adjoint && table_size <= (size_t) kMaxBuckets * (bins / 2);
    const bool quarter = half && (hints & EK_BUCKETED_HINT_BOUNDED) && early_fixed_enabled() &&
                         table_size <= (size_t) kMaxBuckets * (bins / 4);
    return bin_shift_of<float> - (half ? (quarter ? 2 : 1) : 0);
}

/// the object of op(A[index], x, C[index]) (addend == nullptr), or of op(A[index], x, *addend) with a host scalar (table_c == nullptr)
/// bad_op: what an op outside the seven returns (the table entry points have always said "unsupported", the scalar one says "invalid")
static int bucketed_pair_create(int type, int index_type, int op, const void *table_a, const void *table_c, const uint64_t *addend,
                                size_t table_size, const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                ek_hip_bucketed **out, int bad_op) {
    *out = nullptr;
    if (op != EK_FMADD && op != EK_FMSUB && op != EK_FNMADD && op != EK_FNMSUB && op != EK_MULADD && op != EK_MULSUB && op != EK_NMULADD)
        return fail(bad_op, "ek_hip_bucketed_pair_create(): op %d is neither of the fma family nor a product-then-sum", op);
    if (!ek_hip_bucketed_applicable(type, index_type, table_size, n))
        return fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_pair_create(): shape not covered (type %d, %zu lookups into %zu entries%s)",
                    type, n, table_size, ctx().tuning.deterministic ? ", deterministic mode" : "");
    ek_hip_bucketed *b = new ek_hip_bucketed();
    b->type = type; b->index_type = index_type; b->op = op;
    b->n = n; b->table_size = table_size;
    b->table_a = table_a; b->table_c = table_c;
    if (addend) { b->scalar_addend = true; b->addend_bits = *addend; }
    b->partitioned[0] = index; b->partitioned[1] = x; b->partitioned[2] = mask;
    int rc;
    // valid int32 indices are non-negative: same bits as uint32
    // EK_BUCKETED_HINT_ADJOINT: buckets of half the size, so that a bucket's table slice AND its two gradient tables fit the LDS
    // together (k_bucket_pair_forward_adjoint) -- when the table still fits kMaxBuckets of those
    const size_t bins = type == EK_F64 ? (size_t) bins_of<double> : (size_t) bins_of<float>;
    const bool half = (hints & EK_BUCKETED_HINT_ADJOINT) && ctx().tuning.early_adjoint && table_size <= (size_t) kMaxBuckets * (bins / 2);
    if (type == EK_F32) {
        const Arg<uint8_t> m{ mask, 1, mask ? 1u : 0u };
        // half-size buckets (early adjoint) while the table needs at most two slices of them; beyond that the per-slice costs
        // (a partition launch, table slices staged and folded per piece) weigh more than the second pass over the lists: full-size
        // buckets halve the number of slices (K = 16 Mi, 64 Mi lookups, same box: 8 slices 53.8, 4 slices 57.0 Gelem/s)
        const bool want_half = (hints & EK_BUCKETED_HINT_ADJOINT) && ctx().tuning.early_adjoint &&
                               table_size <= (size_t) 2 * kMaxBuckets * (bins / 2);
        const size_t sel_bins = want_half ? bins / 2 : bins, span = (size_t) kMaxBuckets * sel_bins;
        if (table_size > span) {
            const int S = (int) ((table_size + span - 1) / span);
            b->slice_span = span;
            rc = EK_OK;
            // two slices: each reads all of (index, x) and keeps its own; three or more: split by slice first, then every slice
            // partitions its own run into ONE page pool -- sized from n and S alone, the runs' lengths stay on the device
            CoarseSplit cs;
            const bool split = S >= 3;
            const int slice_shift = bin_shift_of<float> - (want_half ? 1 : 0);
            PagedPlan pool_plan;
            size_t pool_pages = 0;
            Scratch pool_work;
            if (split) {
                rc = want_half ? coarse_split<bin_shift_of<float> - 1 + 8>(cs, (const float *) x, (const uint32_t *) index, m, n, S)
                               : coarse_split<bin_shift_of<float> + 8>(cs, (const float *) x, (const uint32_t *) index, m, n, S);
                // every slice with the geometry of a full one (256 buckets; the pool is built on 32-element pages) and the whole input as its bound
                pool_plan = paged_plan(n, kMaxBuckets, ctx().num_cu, false, false, /* pages32 */ true);
                pool_pages = paged_slice_pool_pages(cs.elements, S, pool_plan.W, pool_plan.page_shift);
                b->positions = pool_pages << pool_plan.page_shift;
                if (rc == EK_OK) rc = ek_hip_malloc(b->positions * sizeof(uint16_t), &b->pair_idx);
                if (rc == EK_OK) rc = ek_hip_malloc(b->positions * sizeof(float), &b->x_b);
                if (rc == EK_OK) rc = ek_hip_malloc(pool_pages * sizeof(uint32_t), &b->page_lists);
                if (rc == EK_OK) rc = pool_work.alloc((2 * pool_pages + 3 * (size_t) pool_plan.W * kMaxBuckets) * sizeof(uint32_t));
            }
            if (split && rc == EK_OK && mask) {
                // the split drops the masked-out lanes: whether one of them carried a non-finite x is found out here
                rc = ek_hip_malloc(16, &b->meta);
                if (rc == EK_OK) {
                    EK_HIP_CHECK(hipMemsetAsync(b->meta, 0, 16, ctx().stream));
                    const unsigned grid = (unsigned) std::min<size_t>((n + 255) / 256, (size_t) ctx().num_cu * 8);
                    hipLaunchKernelGGL(k_masked_nonfinite, dim3(grid), dim3(256), 0, ctx().stream, (uint32_t *) b->meta, (const uint32_t *) x, mask, n);
                    EK_LAUNCH_CHECK("bucket_masked_nonfinite", n, n * 5);
                }
            }
            const Arg<uint8_t> all{ nullptr, 1, 0u };
            for (int sl = 0; sl < S && rc == EK_OK; ++sl) {
                ek_hip_bucketed *sub = new ek_hip_bucketed();
                b->slices.push_back(sub);
                sub->type = type; sub->index_type = index_type; sub->op = op;
                sub->table_size = std::min(span, table_size - (size_t) sl * span);
                sub->table_a = (const float *) table_a + (size_t) sl * span;
                sub->table_c = table_c ? (const float *) table_c + (size_t) sl * span : nullptr;
                sub->scalar_addend = b->scalar_addend; sub->addend_bits = b->addend_bits;      // (every slice stages the scalar)
                sub->correct_masked = false;
                if (split) {
                    // the slice's own elements (indices already local to the slice), as many as the device says -- n at most
                    sub->n = n;
                    sub->win_lo = 0;
                    sub->win_span = (uint32_t) sub->table_size;
                    const PagedSlice ps{ cs.range + 2 * sl, (uint32_t) sl * paged_slice_gap(pool_plan.W, pool_plan.page_shift), &pool_plan,
                                         b, (uint32_t *) b->page_lists, (uint32_t *) pool_work.ptr, pool_pages };
                    rc = bucketed_create_paged<uint32_t>(sub, (const float *) cs.x, (const uint32_t *) cs.idx, all, slice_shift, &ps);
                } else {
                    sub->n = n;
                    sub->win_lo = (uint32_t) ((size_t) sl * span);
                    sub->win_span = (uint32_t) sub->table_size;
                    rc = bucketed_create_paged<uint32_t>(sub, (const float *) x, (const uint32_t *) index, m, bin_shift_of<float> - (want_half ? 1 : 0));
                }
            }
            b->slices_split = split;
        } else {
            // EK_BUCKETED_HINT_BOUNDED on top of the adjoint hint: buckets of a QUARTER of the size (4 Ki entries), whose records and two planes
            // of 64-bit fixed-point sums fit the LDS (bucketed_early.hip) -- while the table is within kMaxBuckets of those
            rc = bucketed_create_paged<uint32_t>(b, (const float *) x, (const uint32_t *) index, m, paged_single_shift(table_size, hints));
        }
    } else if (mask) {
        rc = fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_pair_create_masked(): masks with 4-byte element types only");
    } else {
        if (half) rc = bucketed_create<double, uint32_t, bin_shift_of<double> - 1>(b, (const double *) x, (const uint32_t *) index);
        else rc = bucketed_create<double, uint32_t, bin_shift_of<double>>(b, (const double *) x, (const uint32_t *) index);
    }
    if (rc != EK_OK) { delete b; return rc; }
    *out = b;
    return EK_OK;
}

int ek_hip_bucketed_pair_create_masked(int type, int index_type, int op, const void *table_a, const void *table_c, size_t table_size,
                                       const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                       ek_hip_bucketed **out) {
    if (int rc = ensure_init()) return rc;
    if (!out || !table_a || !x || !index) return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create(): null pointer");
    if (!table_c && op != EK_MULADD)
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create(): a NULL addend table (the product gather(A, idx) * x alone) goes with EK_MULADD");
    return bucketed_pair_create(type, index_type, op, table_a, table_c, nullptr, table_size, x, index, mask, n, hints, out, EK_ERR_UNSUPPORTED);
}

int ek_hip_bucketed_pair_create_scalar(int type, int index_type, int op, const void *table_a, uint64_t addend_bits, size_t table_size,
                                       const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                       ek_hip_bucketed **out) {
    if (int rc = ensure_init()) return rc;
    if (!out || !table_a || !x || !index) return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_scalar(): null pointer");
    return bucketed_pair_create(type, index_type, op, table_a, nullptr, &addend_bits, table_size, x, index, mask, n, hints, out, EK_ERR_INVALID);
}

int ek_hip_bucketed_pair_create_scalar_device(int type, int index_type, int op, const void *table_a, const void *addend, size_t table_size,
                                              const void *x, const void *index, const uint8_t *mask, size_t n, unsigned hints,
                                              ek_hip_bucketed **out) {
    if (int rc = ensure_init()) return rc;
    if (!out || !table_a || !addend || !x || !index) return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_scalar_device(): null pointer");
    *out = nullptr;
    if (op != EK_FMADD && op != EK_FMSUB && op != EK_FNMADD && op != EK_FNMSUB && op != EK_MULADD && op != EK_MULSUB && op != EK_NMULADD)
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_scalar_device(): op %d is neither of the fma family nor a product-then-sum", op);
    if (mask) return fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_pair_create_scalar_device(): a device scalar under a mask is not covered");
    if (!ek_hip_bucketed_applicable(type, index_type, table_size, n))
        return fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_pair_create_scalar_device(): shape not covered (type %d, %zu lookups into %zu entries)",
                    type, n, table_size);
    // the scalar, broadcast on the stream into a table the object owns: from here on the object is the two-table one
    void *table = nullptr;
    const size_t elem = type == EK_F64 ? sizeof(double) : sizeof(float);
    if (int rc = ek_hip_malloc(table_size * elem, &table)) return rc;
    const ek_operand c{ addend, 0, 1 };
    int rc = ek_hip_unary(EK_COPY, type, table, &c, table_size);
    if (rc == EK_OK) rc = bucketed_pair_create(type, index_type, op, table_a, table, nullptr, table_size, x, index, nullptr, n, hints, out, EK_ERR_INVALID);
    if (rc != EK_OK) { ek_hip_free(table); return rc; }
    (*out)->addend_table = table;
    (*out)->addend_broadcast = true;
    return EK_OK;
}

int ek_hip_bucketed_partition_retain(ek_hip_bucketed *b, ek_hip_bucket_partition **out) {
    if (!b || !out) return fail(EK_ERR_INVALID, "ek_hip_bucketed_partition_retain(): null pointer");
    *out = nullptr;
    // the single-object paged form, made outside a capture (a captured step's partition lives in the graph's pool and is refilled by
    // every replay); quiet: "not available" is an answer, not an error
    if (!ctx().tuning.partition_cache || b->type != EK_F32 || !b->slices.empty() || b->owner || b->meta_borrowed || !b->page_shift ||
        b->win_span || !b->correct_masked || refuse_while_capturing_quiet() != EK_OK)
        return EK_ERR_UNSUPPORTED;
    // (an array that lives in a step graph's pool is rewritten by every replay of the graph, and nobody hears of it)
    for (const void *src : b->partitioned)
        if (src && graph_pool_owns(src)) return EK_ERR_UNSUPPORTED;
    if (!b->part) {
        // the storage changes hands: from here on the object stands on the partition like every later one
        BucketPartition *p = new BucketPartition();
        p->type = b->type; p->index_type = b->index_type; p->shift = b->shift;
        p->n = b->n; p->table_size = b->table_size; p->has_mask = b->has_mask;
        p->meta = b->meta; p->pair_idx = b->pair_idx; p->x_b = b->x_b; p->page_lists = b->page_lists;
        p->meta_slot = b->meta_slot; p->meta_clean = false;
        p->n_buckets = b->n_buckets; p->page_shift = b->page_shift; p->max_pieces = b->max_pieces; p->positions = b->positions;
        p->bucket_base = b->bucket_base; p->piece_prefix = b->piece_prefix; p->base_part = b->base_part;
        p->glist_full = b->glist_full; p->glist_part = b->glist_part;
        p->active = b->active; p->ticket = b->ticket; p->reduce_partials = b->reduce_partials;
        p->refs = p->objects = 1;
        b->part = p;
        live_partitions().push_back(p);
        set_evict_hook(evict_idle_partitions);
    }
    b->part->refs++;
    *out = b->part;
    return EK_OK;
}

int ek_hip_bucket_partition_release(ek_hip_bucket_partition *p) {
    partition_release(p, false);
    return EK_OK;
}

int ek_hip_bucketed_pair_create_on(ek_hip_bucket_partition *p, int type, int index_type, int op, const void *table_a, const void *table_c,
                                   const uint64_t *addend_bits, const void *addend_device, size_t table_size, size_t n, unsigned hints,
                                   int has_mask, ek_hip_bucketed **out) {
    if (int rc = ensure_init()) return rc;
    if (!p || !out || !table_a) return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_on(): null pointer");
    *out = nullptr;
    if ((table_c != nullptr) + (addend_bits != nullptr) + (addend_device != nullptr) > 1)
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_on(): more than one addend");
    if (op != EK_FMADD && op != EK_FMSUB && op != EK_FNMADD && op != EK_FNMSUB && op != EK_MULADD && op != EK_MULSUB && op != EK_NMULADD)
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_on(): op %d is neither of the fma family nor a product-then-sum", op);
    if (!table_c && !addend_bits && !addend_device && op != EK_MULADD)
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_pair_create_on(): the product gather(A, idx) * x alone goes with EK_MULADD");
    // quiet from here on: the caller partitions for itself
    if (!ctx().tuning.partition_cache || p->evicted || refuse_while_capturing_quiet() != EK_OK) return EK_ERR_UNSUPPORTED;
    if (type != p->type || index_type != p->index_type || table_size != p->table_size || n != p->n || (has_mask != 0) != p->has_mask ||
        (addend_device && has_mask) || !ek_hip_bucketed_applicable(type, index_type, table_size, n) ||
        paged_single_shift(table_size, hints) != p->shift)
        return EK_ERR_UNSUPPORTED;
    // (the object counts from here on: an allocation below that runs out of memory must not take this partition's storage back)
    p->refs++; p->objects++;
    void *table = nullptr;
    if (addend_device) {
        // (as ek_hip_bucketed_pair_create_scalar_device: the scalar, broadcast on the stream into a table the object owns)
        int rc = ek_hip_malloc(table_size * sizeof(float), &table);
        const ek_operand c{ addend_device, 0, 1 };
        if (rc == EK_OK) rc = ek_hip_unary(EK_COPY, type, table, &c, table_size);
        if (rc != EK_OK) {
            if (table) ek_hip_free(table);
            partition_release(p, true);
            return rc;
        }
    }
    ek_hip_bucketed *b = new ek_hip_bucketed();
    b->type = type; b->index_type = index_type; b->op = op;
    b->n = n; b->table_size = table_size;
    b->table_a = table_a; b->table_c = table ? table : table_c;
    b->addend_table = table;
    b->addend_broadcast = table != nullptr;
    if (addend_bits) { b->scalar_addend = true; b->addend_bits = *addend_bits; }
    b->shift = p->shift; b->has_mask = p->has_mask;
    b->n_buckets = p->n_buckets; b->page_shift = p->page_shift; b->max_pieces = p->max_pieces; b->positions = p->positions;
    b->meta = p->meta; b->pair_idx = p->pair_idx; b->x_b = p->x_b; b->page_lists = p->page_lists;
    b->meta_slot = p->meta_slot;
    b->bucket_base = p->bucket_base; b->piece_prefix = p->piece_prefix; b->base_part = p->base_part;
    b->glist_full = p->glist_full; b->glist_part = p->glist_part;
    b->active = p->active; b->ticket = p->ticket; b->reduce_partials = p->reduce_partials;
    b->part = p;
    b->stands_on_kept = true;
    *out = b;
    return EK_OK;
}

int ek_hip_bucketed_reduce(ek_hip_bucketed *b, int reduce_op, int map_op, void *out, int keep_values, int keep_op) {
    if (int rc = ensure_init()) return rc;
    if (!b || !out) return fail(EK_ERR_INVALID, "ek_hip_bucketed_reduce(): null pointer");
    if (map_op != EK_COPY && !unary_fusable(map_op))
        return fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_reduce(): op %d cannot be applied on load", map_op);
    if (!b->slices.empty()) {
        Scratch partial;
        if (int rc = partial.alloc(b->slices.size() * sizeof(float))) return rc;
        SliceCounts counts{};
        int S = 0;
        for (ek_hip_bucketed *sub : b->slices) {
            if (int rc = bucketed_reduce<float>(sub, reduce_op, map_op, (float *) partial.ptr + S, keep_values != 0, keep_op)) return rc;
            counts.active[S++] = sub->active;
        }
        counts.flag = (const uint32_t *) b->meta;          // (tables of three or more slices under a mask; null otherwise)
        Context &c = ctx();
#define EK_COMBINE(OP) hipLaunchKernelGGL((k_slices_combine<float, OP>), dim3(1), dim3(64), 0, c.stream, (float *) out, (const float *) partial.ptr, S, counts, b->n, map_op, b->dropped_u<float>())
        switch (reduce_op) {
            case EK_HSUM: EK_COMBINE(EK_HSUM); break;
            case EK_HPROD: EK_COMBINE(EK_HPROD); break;
            case EK_HMIN: EK_COMBINE(EK_HMIN); break;
            case EK_HMAX: EK_COMBINE(EK_HMAX); break;
            default: return fail(EK_ERR_INVALID, "ek_hip_bucketed_reduce(): unknown op %d", reduce_op);
        }
#undef EK_COMBINE
        EK_LAUNCH_CHECK("reduce_stage2", (size_t) S, (size_t) S * sizeof(float));
        return EK_OK;
    }
    if (b->type == EK_F32) return bucketed_reduce<float>(b, reduce_op, map_op, out, keep_values != 0, keep_op);
    return bucketed_reduce<double>(b, reduce_op, map_op, out, keep_values != 0, keep_op);
}

int ek_hip_bucketed_scatter_add(ek_hip_bucketed *b, int count, void *const *bases, const int *from_u, const int *map_ops,
                                const uint64_t *imm_bits, const int *weighted, const int *fresh) {
    return ek_hip_bucketed_scatter_add_scaled(b, count, bases, from_u, map_ops, imm_bits, weighted, fresh, nullptr);
}

int ek_hip_bucketed_early_pair(int map_op, int keep_op) { return early_pair_supported(map_op, keep_op) ? 1 : 0; }

int ek_hip_bucketed_take_tables(ek_hip_bucketed *b, int count, const int *from_u, const int *map_ops, const int *weighted,
                                const uint64_t *scale_bits, void **tables) {
    if (!b || !from_u || !weighted || !tables || count < 1) return fail(EK_ERR_INVALID, "ek_hip_bucketed_take_tables(): bad arguments");
    // the object holds direct tables, and the streams are exactly the early ones (the match of bucketed_scatter_add), unscaled
    if (count > 2 || !b->slices.empty() || b->type != EK_F32 || !b->has_early || !b->early_direct) return EK_ERR_UNSUPPORTED;
    for (int s = 0; s < count; ++s) {
        if (!from_u[s] || (map_ops ? map_ops[s] : (int) EK_COPY) != b->early_op) return EK_ERR_UNSUPPORTED;
        if (scale_bits && (uint32_t) scale_bits[s] != 0x3F800000u) return EK_ERR_UNSUPPORTED;
        if (!b->direct[weighted[s] ? 1 : 0]) return EK_ERR_UNSUPPORTED;
    }
    if (count == 2 && (weighted[0] != 0) == (weighted[1] != 0)) return EK_ERR_UNSUPPORTED;
    for (int s = 0; s < count; ++s) {
        void *&plane = b->direct[weighted[s] ? 1 : 0];
        tables[s] = plane;             // the caller's from here on (ek_hip_free)
        plane = nullptr;
    }
    if (!b->direct[0]) b->direct_modes = nullptr;          // (they went with plane 0's block)
    // the sums have left: a second request for them is an unmatched one (the streams are evaluated on the lists), the next forward +
    // adjoint launch of this object allocates new tables.  A plane that was not asked for (count 1) stays: a later request for IT is
    // still answered from it, by a take or by the fold -- the bits of the path without direct tables.
    if (!b->direct[0] && !b->direct[1]) {
        b->has_early = false;
        b->early_direct = false;
    }
    return EK_OK;
}

int ek_hip_bucketed_scatter_add_scaled(ek_hip_bucketed *b, int count, void *const *bases, const int *from_u, const int *map_ops,
                                       const uint64_t *imm_bits, const int *weighted, const int *fresh, const uint64_t *scale_bits) {
    if (int rc = ensure_init()) return rc;
    if (!b || !bases || !from_u || !imm_bits || !weighted || count < 1 || count > 4)
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_scatter_add(): bad arguments");
    for (int s = 0; s < count; ++s) {
        if (!bases[s]) return fail(EK_ERR_INVALID, "ek_hip_bucketed_scatter_add(): null table");
        if (from_u[s] && map_ops && map_ops[s] != EK_COPY && !unary_fusable(map_ops[s]))
            return fail(EK_ERR_UNSUPPORTED, "ek_hip_bucketed_scatter_add(): op %d cannot be applied on load", map_ops[s]);
    }
    if (!b->slices.empty()) {
        for (size_t sl = 0; sl < b->slices.size(); ++sl) {
            void *sb[4];
            for (int s = 0; s < count; ++s) sb[s] = (float *) bases[s] + sl * b->slice_span;
            // (a slice that received no element has no pieces: the fold still writes a fresh table's zeros there)
            if (int rc = bucketed_scatter_add<float>(b->slices[sl], count, sb, from_u, map_ops, imm_bits, weighted, fresh, scale_bits)) return rc;
        }
        return EK_OK;
    }
    if (b->type == EK_F32) return bucketed_scatter_add<float>(b, count, bases, from_u, map_ops, imm_bits, weighted, fresh, scale_bits);
    return bucketed_scatter_add<double>(b, count, bases, from_u, map_ops, imm_bits, weighted, fresh, scale_bits);
}

int ek_hip_bucketed_addend_adjoint(ek_hip_bucketed *b, int map_op, uint64_t scale_bits, void *out) {
    if (int rc = ensure_init()) return rc;
    if (!b || !out) return fail(EK_ERR_INVALID, "ek_hip_bucketed_addend_adjoint(): null pointer");
    if (!b->scalar_addend && !b->addend_table) return fail(EK_ERR_INVALID, "ek_hip_bucketed_addend_adjoint(): the object has no scalar addend");
    if (map_op != EK_COPY && !unary_chainable(map_op))
        return fail(EK_ERR_INVALID, "ek_hip_bucketed_addend_adjoint(): op %d cannot be applied on load", map_op);
    Context &c = ctx();
    const bool f64 = b->type == EK_F64;
    float scale_f = 1.f;
    double scale_d = 1.0;
    if (f64) memcpy(&scale_d, &scale_bits, sizeof(double)); else memcpy(&scale_f, &scale_bits, sizeof(float));
    // the forward pass left the sums of exactly this function per table entry (in every slice): one fold over plane 0
    bool early = b->slices.empty() ? b->has_early && b->early_op == map_op : true;
    for (const ek_hip_bucketed *sub : b->slices) early = early && sub->has_early && sub->early_op == map_op;
    if (early && !b->slices.empty()) {
        // a slice's sum leaves out the lanes the slice dropped (most of them are another slice's): they are counted ONCE, below
        Scratch partial;
        if (int rc = partial.alloc(b->slices.size() * sizeof(float))) return rc;
        SliceCounts counts{};
        int S = 0;
        for (ek_hip_bucketed *sub : b->slices) {
            if (int rc = bucketed_addend_adjoint_fold<float>(sub, map_op, 1.f, (float *) partial.ptr + S, false)) return rc;
            counts.active[S++] = sub->active;
        }
        counts.flag = (const uint32_t *) b->meta;
        hipLaunchKernelGGL(k_addend_adjoint_combine, dim3(1), dim3(64), 0, c.stream, (float *) out, (const float *) partial.ptr, S,
                           counts, b->n, map_op, b->dropped_u<float>(), scale_f);
        EK_LAUNCH_CHECK("reduce_stage2", (size_t) S, (size_t) S * sizeof(float));
        return EK_OK;
    } else if (early) {
        return f64 ? bucketed_addend_adjoint_fold<double>(b, map_op, scale_d, out, true)
                   : bucketed_addend_adjoint_fold<float>(b, map_op, scale_f, out, true);
    } else {
        // no such sums: the bucket-ordered reduction, one more pass over the pages (every lane counted, the dropped ones included)
        if (int rc = ek_hip_bucketed_reduce(b, EK_HSUM, map_op, out, 0, EK_COPY)) return rc;
    }
    // (the reduction wrote the plain sum: the factor is one more one-thread launch on this path only)
    if (f64 ? scale_d != 1.0 : scale_f != 1.f) {
        if (f64) hipLaunchKernelGGL((k_scale_one<double>), dim3(1), dim3(1), 0, c.stream, (double *) out, scale_d);
        else hipLaunchKernelGGL((k_scale_one<float>), dim3(1), dim3(1), 0, c.stream, (float *) out, scale_f);
        EK_LAUNCH_CHECK("addend_adjoint_scale", (size_t) 1, 2 * (f64 ? sizeof(double) : sizeof(float)));
    }
    return EK_OK;
}

int ek_hip_bucketed_piece_counts(ek_hip_bucketed *b, uint32_t *pieces, uint32_t *largest) {
    if (int rc = ensure_init()) return rc;
    if (!b || !pieces || !largest) return fail(EK_ERR_INVALID, "ek_hip_bucketed_piece_counts(): null pointer");
    if (int busy = refuse_while_capturing("ek_hip_bucketed_piece_counts()")) return busy;
    *pieces = *largest = 0;
    std::vector<const ek_hip_bucketed *> objs;
    if (b->slices.empty()) objs.push_back(b);
    for (const ek_hip_bucketed *sub : b->slices) objs.push_back(sub);
    std::vector<uint32_t> prefix;
    for (const ek_hip_bucketed *o : objs) {
        if (!o->piece_prefix || o->n_buckets <= 0) continue;
        prefix.assign((size_t) o->n_buckets + 1, 0u);
        EK_HIP_CHECK(hipMemcpyAsync(prefix.data(), o->piece_prefix, prefix.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx().stream));
        EK_HIP_CHECK(hipStreamSynchronize(ctx().stream));
        *pieces += prefix[(size_t) o->n_buckets] - prefix[0];
        for (int k = 0; k < o->n_buckets; ++k) *largest = std::max(*largest, prefix[(size_t) k + 1] - prefix[(size_t) k]);
    }
    return EK_OK;
}

int ek_hip_bucketed_destroy(ek_hip_bucketed *b) {
    delete b;
    return EK_OK;
}

int ek_hip_index_partition_create(int index_type, const void *index, const ek_operand *mask, size_t n, size_t range,
                                  ek_hip_index_partition **out) {
    if (int rc = ensure_init()) return rc;
    if (!out || !index || !mask) return fail(EK_ERR_INVALID, "ek_hip_index_partition_create(): null pointer");
    *out = nullptr;
    if (index_type != EK_U32 && index_type != EK_I32)
        return fail(EK_ERR_UNSUPPORTED, "ek_hip_index_partition_create(): 32-bit index arrays only");
    if (n == 0 || n >= ((size_t) 1 << 32) || range == 0 || range > ((size_t) kMaxBuckets << 19))
        return fail(EK_ERR_UNSUPPORTED, "ek_hip_index_partition_create(): %zu indices into %zu entries is out of range", n, range);
    Arg<uint8_t> m;
    if (int rc = make_arg<uint8_t>(mask, n, m, "ek_hip_index_partition_create")) return rc;
    // the smallest bucket size of {4 Ki, 16 Ki, 128 Ki, 512 Ki} entries that covers the range with <= 256 buckets
    static const int shifts[] = { 12, 14, 17, 19 };
    int shift = 19;
    for (int sft : shifts)
        if (((range + ((size_t) 1 << sft) - 1) >> sft) <= (size_t) kMaxBuckets) { shift = sft; break; }
    ek_hip_index_partition *ip = new ek_hip_index_partition();
    ip->info.shift = shift;
    ip->info.n_buckets = (int) ((range + ((size_t) 1 << shift) - 1) >> shift);
    ip->info.n = n;
    ip->info.range = range;
    int rc;
    const uint32_t *idx = (const uint32_t *) index;          // valid int32 indices are non-negative: same bits as uint32
    // large inputs over many buckets: the single-pass page partition (ENOKI_HIP_INDEX_PAGED=0: count / scan / partition as before)
    static const bool paged = [] { const char *e = getenv("ENOKI_HIP_INDEX_PAGED"); return !e || atoi(e) != 0; }();
    if (paged && ctx().tuning.bucket_ordered && n >= ((size_t) 1 << 20) && n < ((size_t) 1 << 30) && ip->info.n_buckets >= 32) {
        rc = index_partition_run_paged(ip, idx, m, n, ip->info.n_buckets, shift);
        if (rc == EK_OK) { *out = ip; return EK_OK; }
        if (rc != EK_ERR_UNSUPPORTED && rc != EK_ERR_OOM) { delete ip; return rc; }
        (void) hipGetLastError();
        for (void **q : { &ip->meta, &ip->local, &ip->lists }) { if (*q) ek_hip_free(*q); *q = nullptr; }
        ip->info.page_shift = 0;
    }
    switch (shift) {
        case 12: rc = index_partition_run<uint32_t, 12>(ip, idx, m, n, ip->info.n_buckets); break;
        case 14: rc = index_partition_run<uint32_t, 14>(ip, idx, m, n, ip->info.n_buckets); break;
        case 17: rc = index_partition_run<uint32_t, 17>(ip, idx, m, n, ip->info.n_buckets); break;
        default: rc = index_partition_run<uint32_t, 19>(ip, idx, m, n, ip->info.n_buckets); break;
    }
    if (rc != EK_OK) { delete ip; return rc; }
    *out = ip;
    return EK_OK;
}

int ek_hip_index_partition_get(const ek_hip_index_partition *p, ek_hip_index_partition_info *info) {
    if (!p || !info) return fail(EK_ERR_INVALID, "ek_hip_index_partition_get(): null pointer");
    *info = p->info;
    return EK_OK;
}

int ek_hip_index_partition_destroy(ek_hip_index_partition *p) {
    delete p;
    return EK_OK;
}

} // extern "C"
