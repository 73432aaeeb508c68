/*
 * include/enoki_hip.h -- C ABI of libenoki-hip.so, the MI355X (gfx950) array runtime.
 *
 * This is the drop-in boundary for the reference's `libenoki-cuda.so` (exports declared in
 * /root/reference/include/enoki/cuda.h:27-200).  The reference's exports are C++-mangled and
 * operate on *trace indices* of a PTX JIT; this library is eager: every entry point takes raw
 * device pointers + element counts and launches one pre-compiled HIP kernel on the library's
 * stream.  `include/enoki/hip.h` (HIPArray<T>) is the C++ binding that sits on top of it and
 * plays the role of `CUDAArray<T>` (cuda.h:205-954); INTEGRATION.md shows the reference-side
 * stub a maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ / torch types.
 *  - every function returns 0 on success or a negative EK_ERR_* code; ek_hip_last_error()
 *    returns a thread-local human readable message.  HIP API failures are reported the same
 *    way (the reference exits the process, src/cuda/common.cu:268-286; a library should not).
 *  - all work is enqueued on ONE stream (ek_hip_stream()/ek_hip_set_stream()); nothing
 *    synchronizes unless documented (ek_hip_sync, *_to_host copies, all/any/count).
 *  - masks are arrays of uint8_t (0/1), as in the reference (src/cuda/jit.cu:1137-1144).
 *  - operands of vertical ops are `ek_operand`: a device array of `size` n or 1 (size-1
 *    operands broadcast, cuda.h semantics via jit.cu:776-782), or an immediate scalar.
 */
#ifndef ENOKI_HIP_C_API_H
#define ENOKI_HIP_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#  define EK_API
#else
#  define EK_API __attribute__((visibility("default")))
#endif
/* An entry point that a caller can do without: declared WEAK for everybody but the library itself, so that code compiled
 * against this header still links and loads against a C ABI that predates the entry (or a host stand-in of the ABI) -- the
 * function's address is then null, and the caller asks before it calls. */
#if defined(_WIN32) || defined(EK_HIP_LIBRARY)
#  define EK_OPTIONAL
#else
#  define EK_OPTIONAL __attribute__((weak))
#endif

/* Element types -- the subset of EnokiType (src/cuda/common.cuh:25-40) on the hot path. */
typedef enum {
    EK_BOOL = 0, EK_I32 = 1, EK_U32 = 2, EK_I64 = 3, EK_U64 = 4, EK_F32 = 5, EK_F64 = 6,
    EK_TYPE_COUNT = 7
} ek_type;

typedef enum {
    EK_OK = 0,
    EK_ERR_INVALID = -1,      /* bad argument (null pointer, unknown op/type, size mismatch) */
    EK_ERR_UNSUPPORTED = -2,  /* op not defined for this element type */
    EK_ERR_HIP = -3,          /* a HIP runtime call failed; see ek_hip_last_error() */
    EK_ERR_OOM = -4           /* allocation failed even after trimming the cache */
} ek_status;

/* Unary ops.  cuda.h:418-543 (abs_ .. tzcnt_) and array_math.h (sin/cos/exp/log, CPU algorithm).
 * EK_TAN .. EK_CBRT (f32 only): the "second wave" the reference composes generically from traced
 * primitives (array_math.h:466-474, 555, 666, 900, 997-1348); here one fused kernel each. */
typedef enum {
    EK_NEG = 0, EK_ABS, EK_NOT, EK_SQRT, EK_RCP, EK_RSQRT, EK_FLOOR, EK_CEIL, EK_ROUND, EK_TRUNC,
    EK_SIN, EK_COS, EK_EXP, EK_LOG, EK_POPCNT, EK_LZCNT, EK_TZCNT, EK_SIGN, EK_COPY,
    EK_TAN, EK_COT, EK_ASIN, EK_ACOS, EK_ATAN, EK_SINH, EK_COSH, EK_TANH, EK_ASINH, EK_ACOSH, EK_ATANH,
    EK_CBRT,
    EK_ERF, EK_ERFC, EK_ERFINV, EK_I0E, EK_DAWSON, EK_ERFI, EK_LGAMMA, EK_TGAMMA,   /* special.h:56-312, f32 and f64 */
    /* what the derivatives of rcp and rsqrt are made of, as ONE function of the argument each (autodiff.h:381-403: -sqr(result),
     * -.5 result^3 with result = rcp(x) / rsqrt(x)): r r with r = 1 / x;  r r and r (r r) with r = 1 / sqrt(x) -- the roundings of
     * the eager products, so that a consumer which applies an op while it loads can form them from x */
    EK_RCP_SQR, EK_RSQRT_SQR, EK_RSQRT_CUBE,
    /* round 6: the derivative weights of tan, tanh and atan as ONE function of the argument each, with the roundings of the compositions
     * the reference records (autodiff.h:532-541 sqr(sec(x)), :685-696 sqr(sech(x)), :606-616 rcp(1 + sqr(x)); sec = rcp(cos),
     * sech = rcp(cosh), array_math.h:463-464, 1181-1183): r r with r = 1 / cos(x);  r r with r = 1 / cosh(x);  1 / (1 + x x) */
    EK_SEC_SQR, EK_SECH_SQR, EK_RCP_1P_SQR,
    EK_UNARY_COUNT
} ek_unary_op;

/* Binary ops.  cuda.h:341-385, 408-416, 499-580; safe_mul = autodiff.cpp:1191-1205;
 * atan2(y, x) / pow / fmod / ldexp = array_math.h:603-664, 956-958, 1381-1383, 677-680 (atan2, pow, ldexp: f32). */
typedef enum {
    EK_ADD = 0, EK_SUB, EK_MUL, EK_DIV, EK_MOD, EK_MIN, EK_MAX, EK_MULHI, EK_AND, EK_OR, EK_XOR,
    EK_SL, EK_SR, EK_SAFE_MUL, EK_ATAN2, EK_POW, EK_FMOD, EK_LDEXP,
    EK_BINARY_COUNT
} ek_binary_op;

/* Ternary ops.  cuda.h:387-406; safe_fmadd = autodiff.cpp:1207-1221.
 * EK_MULADD / EK_MULSUB / EK_NMULADD (floating point): a * b + c, a * b - c, c - a * b written with OPERATORS -- a multiplication
 * and an addition with a rounding each, what `a*x+b` means in the reference (separate packet operations are never contracted,
 * SURVEY 8c) -- as ONE pass over the operands.  A caller-visible op only so that a product left unevaluated by HIPArray can be
 * finished by the addition that consumes it; bit-identical to ek_hip_binary(EK_MUL) followed by EK_ADD / EK_SUB. */
typedef enum {
    EK_FMADD = 0, EK_FMSUB, EK_FNMADD, EK_FNMSUB, EK_SAFE_FMADD, EK_MULADD, EK_MULSUB, EK_NMULADD,
    EK_TERNARY_COUNT
} ek_ternary_op;

/* Comparisons -> u8 mask.  cuda.h:582-630. */
typedef enum { EK_EQ = 0, EK_NEQ, EK_LT, EK_LE, EK_GT, EK_GE, EK_COMPARE_COUNT } ek_compare_op;

/* Horizontal reductions.  cuda.h:693-759 / src/cuda/horiz.cu:162-268. */
typedef enum { EK_HSUM = 0, EK_HPROD, EK_HMIN, EK_HMAX, EK_REDUCE_COUNT } ek_reduce_op;

/* Mask reductions.  cuda.h:761-794 / horiz.cu:284-354. */
typedef enum { EK_ALL = 0, EK_ANY, EK_COUNT, EK_MASK_REDUCE_COUNT } ek_mask_reduce_op;

/* An operand of a vertical op: device array (`ptr` != NULL, `size` == n or 1) or an immediate
   (`ptr` == NULL; the scalar's bit pattern in the low bytes of `imm`). */
typedef struct {
    const void *ptr;
    uint64_t imm;
    size_t size;
} ek_operand;

/* ---------------------------------------------------------------------------------------------
 *  Runtime: device, stream, memory, diagnostics
 *  replaces cuda_malloc, cuda_free, cuda_malloc_trim, cuda_sync, cuda_memcpy_to_device/from_device,
 *  cuda_mem_get_info, cuda_whos, cuda_set_log_level
 *  (cuda.h:109-200; src/cuda/jit.cu:1683-1896, common.cu:104-122)
 * ------------------------------------------------------------------------------------------- */
EK_API int ek_hip_init(int device);                 /* select device, create stream (idempotent) */
EK_API int ek_hip_device(void);                     /* device ordinal in use, -1 before init */
EK_API int ek_hip_device_count(void);
EK_API void *ek_hip_stream(void);                   /* hipStream_t */
EK_API int ek_hip_set_stream(void *hip_stream);     /* adopt a caller-owned stream (e.g. torch's) */
EK_API int ek_hip_sync(void);                       /* hipStreamSynchronize on the library stream */
EK_API const char *ek_hip_last_error(void);

EK_API int ek_hip_malloc(size_t bytes, void **out);         /* caching allocator, 256-B aligned */
EK_API int ek_hip_free(void *ptr);                          /* returns the block to the cache */
EK_API int ek_hip_malloc_trim(void);                        /* release cached blocks to the driver */
EK_API int ek_hip_host_malloc(size_t bytes, void **out);    /* pinned host memory */
EK_API int ek_hip_host_free(void *ptr);
EK_API int ek_hip_mem_get_info(size_t *free_bytes, size_t *total_bytes);
EK_API int ek_hip_memcpy_to_device(void *dst, const void *src, size_t bytes);   /* blocking */
EK_API int ek_hip_memcpy_to_host(void *dst, const void *src, size_t bytes);     /* blocking */
EK_API int ek_hip_memcpy_device(void *dst, const void *src, size_t bytes);      /* async d2d */
EK_API int ek_hip_memset(void *dst, int byte, size_t bytes);                    /* async */
/* malloc'd, NUL-terminated allocator report; caller frees with free() (cuda_whos, cuda.cpp:40) */
EK_API char *ek_hip_whos(void);
EK_API void ek_hip_set_log_level(uint32_t level);   /* 0 silent .. 3 every launch (cuda.h:195-200) */
EK_API uint32_t ek_hip_log_level(void);
EK_API uint64_t ek_hip_launch_count(void);          /* kernels launched since init (diagnostics) */
/* Kernels that callers launch THEMSELVES on ek_hip_stream() (the fused kernels that enoki/vectorize.h instantiates from user
   code) report here so that they show up in ek_hip_launch_count(), the ENOKI_HIP_LOG=3 trace and ek_hip_profile_*;
   `bytes` = algorithmic bytes of the launch.  `name` must outlive the profile (a string literal). */
EK_API int ek_hip_note_launch(const char *name, size_t n, size_t bytes);
/* One process-wide pointer variable for the C++ binding (include/enoki/hip.h keeps the head of its list of unevaluated
   buffers here): header-only code that is compiled into several shared objects needs ONE home for such state, and this
   library is the one object they all link.  Returns the variable's address; never NULL; no initialisation needed. */
EK_API void **ek_hip_binding_slot(void);
/* Step graphs (hipGraph): between ek_hip_graph_begin() and ek_hip_graph_end() every launch of this library -- kernels,
   memsets, device-to-device copies -- is CAPTURED on the library stream instead of executed; ek_hip_graph_launch()
   replays the captured step without any host-side work (no tape walk, no allocator, no per-kernel launch call), which
   is what strong scaling needs once a shard's step is a dozen kernels of 10-50 us.  Memory that the captured code
   allocates comes from a pool private to the graph and stays reserved until ek_hip_graph_destroy(): the arrays that
   are alive when the capture ends (results, gradients) keep their addresses, and every replay refreshes their contents.
   Not capturable (fail with EK_ERR_INVALID / EK_ERR_HIP): anything that reads back to the host -- ek_hip_memcpy_to_host,
   ek_hip_mask_reduce (all / any / count), deterministic scatter_add under a mask array, ek_hip_profile_*, and a mode-0
   scatter_add into more than 4 Mi bins (2 Mi for 8-byte types) on its host-sized path: 8-byte and integer element types, a
   scalar value or index operand, tables beyond 256 Mi bins (see ek_hip_scatter_add).
   The reference has no counterpart: its cuda_eval() re-assembles and re-launches PTX per evaluation (jit.cu:1385-1471). */
typedef struct ek_hip_graph ek_hip_graph;
EK_API int ek_hip_graph_begin(void);
EK_API int ek_hip_graph_end(ek_hip_graph **out);
EK_API int ek_hip_graph_launch(ek_hip_graph *graph);
EK_API uint64_t ek_hip_graph_launch_count(const ek_hip_graph *graph);   /* kernel launches inside one replay */
EK_API int ek_hip_graph_destroy(ek_hip_graph *graph);
EK_API int ek_hip_set_tuning(const char *key, int value);   /* "reduce_blocks_per_cu", "scatter_add_binned", "deterministic", "gather_records", "bucket_ordered", "early_adjoint", "partition_cache", "partition_refine" (0 never, 1 automatic, 2 whenever the shape is covered), "direct_tables" (ek_hip_bucketed_take_tables: 0 never, 1 for tables of 256 Ki entries and more, 2 whenever the shape is covered), "sort_radix" (ek_hip_sort: 0 never the radix route, 1 automatic, 2 for every n >= 2) */
/* Per-kernel timing: between begin and end one HIP event is recorded on the library stream after every
   launch.  ek_hip_profile_end() synchronizes and returns a malloc'd JSON array (caller free()s) of
   {"kernel", "launches", "total_ms", "bytes", "elements"}; `bytes` are the ALGORITHMIC bytes of the
   launches (distinct operand bytes + output bytes; broadcast operands count 0). */
EK_API int ek_hip_profile_begin(void);
EK_API char *ek_hip_profile_end(void);

/* ---------------------------------------------------------------------------------------------
 *  Vertical (elementwise) ops: out[i] = op(a[i or 0], ...), i in [0, n)
 * ------------------------------------------------------------------------------------------- */
EK_API int ek_hip_unary(int op, int type, void *out, const ek_operand *a, size_t n);
EK_API int ek_hip_binary(int op, int type, void *out, const ek_operand *a, const ek_operand *b, size_t n);
EK_API int ek_hip_ternary(int op, int type, void *out, const ek_operand *a, const ek_operand *b,
                          const ek_operand *c, size_t n);
/* sincos_: both outputs from one pass over the input (array_math.h:261-367) */
EK_API int ek_hip_sincos(int type, void *out_sin, void *out_cos, const ek_operand *a, size_t n);
/* sincosh: sinh and cosh from one exp() (array_math.h:1067-1127), what DiffArray::sinh_/cosh_ call (autodiff.h:635-657) */
EK_API int ek_hip_sincosh(int type, void *out_sinh, void *out_cosh, const ek_operand *a, size_t n);
EK_API int ek_hip_compare(int op, int type, uint8_t *out_mask, const ek_operand *a, const ek_operand *b, size_t n);
/* select_: out = mask ? t : f (cuda.h:632-639); `mask` is an EK_BOOL operand */
EK_API int ek_hip_select(int type, void *out, const ek_operand *mask, const ek_operand *t,
                         const ek_operand *f, size_t n);
/* converting constructor (cuda.h:236-247): float->int truncates, int->float rounds to nearest */
EK_API int ek_hip_cast(int src_type, int dst_type, void *out, const ek_operand *a, size_t n);

/* ---------------------------------------------------------------------------------------------
 *  Initialization (cuda.h:641-691; horiz.cu:28-32; common.cu:56-102)
 * ------------------------------------------------------------------------------------------- */
EK_API int ek_hip_fill(int type, void *out, uint64_t imm_bits, size_t n);
/* out[i] = start + i*step, computed in the element type (integer types wrap) */
EK_API int ek_hip_arange(int type, void *out, int64_t start, int64_t step, size_t n);
/* out[i] = fmadd(i, step, min), step = (max-min)/(n-1)  (cuda.h:655-663) */
EK_API int ek_hip_linspace(int type, void *out, double min, double max, size_t n);
EK_API int ek_hip_reverse(int type, void *out, const void *in, size_t n);
/* out = srcs[0] | srcs[1] | ... (sizes in elements, count <= 8) in ONE launch: the staging step of the packed all-reduce
 * (scalar loss + K-element gradients -> one flat buffer), where three small copies would cost three launches */
EK_API int ek_hip_concat(int type, void *out, int count, const void *const *srcs, const size_t *sizes);
/* The staging step of a REDUCE-SCATTER over `rows` ranks: every source (sizes[k] a multiple of `rows`) is seen as [rows, c_k]
 * and the sources are concatenated along the columns -- out[r] = srcs[0][r] | srcs[1][r] | ..., i.e. row r holds the chunks of
 * all tables that rank r will own -- in ONE launch (count <= 8, 4- and 8-byte types).  A source of ONE entry is copied into
 * every row: a scalar partial sum (the loss) rides on the same reduce-scatter -- every rank then receives sum_r(loss_r) in
 * that column -- instead of on a collective of its own. */
EK_API int ek_hip_concat_rows(int type, void *out, size_t rows, int count, const void *const *srcs, const size_t *sizes);

/* ---------------------------------------------------------------------------------------------
 *  Indexed memory ops (cuda.h:845-905).  `index_type` in {EK_I32, EK_U32, EK_I64, EK_U64};
 *  element stride = sizeof(type); `mask` may be an immediate operand (all lanes on/off).
 * ------------------------------------------------------------------------------------------- */
EK_API int ek_hip_gather(int type, int index_type, void *out, const void *base,
                         const ek_operand *index, const ek_operand *mask, size_t n);
/* out[i] = mask[i] && address[i] ? *(type *) (address[i] + byte_offset) : 0: a data member read out of INSTANCE memory through an
 * array of 64-bit object addresses -- what ENOKI_CALL_SUPPORT_GETTER does on the device (array_call.h:269-283:
 * gather<Return, 1>(nullptr, self + offset, mask) from managed instance memory).  The addresses must be readable by the GPU
 * (ek_hip_host_malloc / ENOKI_PINNED_OPERATOR_NEW, like the reference's pinned instances, array_macro.h:361). */
EK_API int ek_hip_gather_address(int type, void *out, const ek_operand *address, int64_t byte_offset, const ek_operand *mask, size_t n);
/* Gather of a structure-of-arrays value: `count` (2..4) tables of the same element type share ONE index / mask array
 * (gather<Array<HIPArray<T>, N>>(...), array_struct.h:9-40 calls gather_ once per component).  outs[c][i] =
 * mask[i] ? bases[c][index[i]] : 0.  4- and 8-byte element types. */
EK_API int ek_hip_gather_multi(int type, int index_type, int count, void *const *outs, const void *const *bases,
                               const ek_operand *index, const ek_operand *mask, size_t n);
/* The same with the tables' common length known (`base_size` entries each; 0 = unknown, plain ek_hip_gather_multi).  When
 * the tables are too large for the L2 and there are enough lookups to pay for it, the components are first staged as
 * packed 8- or 16-byte records {x, y(, z, w)} and every lane issues ONE request per element instead of `count`: random
 * lookups are bound by the number of memory requests, not by bytes.  Same results bit for bit.
 * Replaces the per-component gather_ calls of array_struct.h:9-40 for Array<CUDAArray<T>, N> sources. */
enum { EK_GATHER_PER_TABLE = 0, EK_GATHER_ONE_LAUNCH = 1, EK_GATHER_RECORDS = 2 };
/* which of the three ek_hip_gather_multi_sized() would take for this shape (callers that can leave per-table gathers
 * unevaluated -- enoki/hip.h consumes them inside the next arithmetic kernel -- ask before committing to a launch) */
EK_API int ek_hip_gather_multi_plan(int type, int index_type, int count, size_t base_size, size_t n);
EK_API int ek_hip_gather_multi_sized(int type, int index_type, int count, void *const *outs, const void *const *bases,
                                     size_t base_size, const ek_operand *index, const ek_operand *mask, size_t n);
/* An operand that is read THROUGH an index array: value[i] = mask[i] ? table[index[i]] : 0 -- a gather (cuda.h:845-864)
 * whose result is consumed by the next vertical op instead of being written out.  The reference gets this for free:
 * its JIT emits the gather's `ld.global` into the consumer's kernel (jit.cu:1066-1217). */
typedef struct {
    const void *table;       /* `table_size` elements of the op's element type */
    size_t table_size;
    ek_operand index;        /* EK_U32 / EK_I32 ARRAY of the op's size */
    int index_type;
    ek_operand mask;         /* EK_BOOL array of the op's size, or an immediate */
} ek_gathered;
/* out[i] = op(x0[i], x1[i] (, x2[i])) where operand k is `*gathered[k]` when that pointer is non-NULL and `*operands[k]`
 * otherwise; `arity` 2 (`op` an ek_binary_op: ADD, SUB, MUL) or 3 (`op` an ek_ternary_op: FMADD .. FNMSUB), EK_F32 / EK_F64.
 * One gathered operand per launch -- or, for the fma family, a gathered first (or second) AND third operand that share
 * their index and mask arrays and table size: the two tables are interleaved into {a, c} records first and every element
 * issues ONE 8-byte lookup (random lookups are request-rate bound, not byte bound).  Bit-identical to ek_hip_gather followed by
 * ek_hip_binary / ek_hip_ternary; returns EK_ERR_UNSUPPORTED for every other combination (callers then do exactly that). */
EK_API int ek_hip_map_gathered(int arity, int op, int type, void *out, const ek_operand *const *operands,
                               const ek_gathered *const *gathered, size_t n);
/* Bucket-ordered evaluation of  u[i] = op(A[index[i]], x[i], C[index[i]])  (op of the fma family) for consumers that do not
 * care about the ELEMENT order of u: horizontal reductions, and the adjoint scatter_add of the two gathers through the same
 * index array.  The reference gets the forward half from its JIT -- the gathers' ld.global and the arithmetic are emitted
 * into one kernel per evaluation (src/cuda/jit.cu:984, 1066-1217, 1418-1471) -- and pays atom.global.add per element in the
 * adjoint (cuda.h:892-905).  Here (index, x) is partitioned ONCE by bucket of 16 Ki table entries (8 Ki for 8-byte types);
 * every bucket's {A, C} slice is then served from LDS (no lookup leaves the CU: element-order lookups into tables beyond
 * the 4 MiB L2 of an XCD run at 0.25 of the HBM roofline), and the adjoint reuses the partition instead of counting,
 * scanning and partitioning again.
 *   create        the partition -- 4-byte element types: ONE streaming pass into pages (csrc/ek_paged.h: full-line pages per bucket,
 *                 no count pass, no scans) + the page directory; 8-byte types: count / scan / partition into contiguous runs;
 *                 4-byte tables beyond 256 buckets are cut into slices of 256 buckets, one filtered pass per slice.
 *                 `table_a`, `table_c` (`table_size` entries each), are read by later calls:
 *                 the caller keeps them alive and unchanged for the lifetime of the object.  x and index: n-element arrays.
 *                 EK_ERR_UNSUPPORTED for shapes the path does not cover (ask ek_hip_bucketed_applicable first): tables of
 *                 one bucket, 8-byte tables of more than 256 buckets, 4-byte tables of more than 32 x 256, fewer than 256 Ki or
 *                 (4-byte types) 2^30 or more lookups, deterministic mode, non-fp types.  Indices outside the table are dropped.
 *   reduce        out[0] = reduce_op over map_op(u)  (map_op: EK_COPY or an op ek_hip_reduce_map accepts); keep_values != 0
 *                 also keeps u in bucket order for later calls (4 B/elt more) -- or, when {map_op, keep_op} = {EK_SIN, EK_COS},
 *                 the OTHER half of sincos(u): one sincos per element yields the reduced and the kept half, and a later
 *                 scatter_add of that half (the cos(u) of d/du sin(u)) streams it as is.  keep_op = EK_COPY: keep u.
 *   scatter_add   bases[c][index[i]] += (weighted[c] ? safe_mul(x[i], v_c[i]) : v_c[i]),  v_c = from_u[c] ? map_ops[c](u) :
 *                 the scalar imm_bits[c];  count 1..4 tables of table_size entries.  fresh (may be NULL): fresh[c] != 0 says
 *                 that table c holds no data yet -- a gradient buffer that would otherwise be zero-filled first: its sums are
 *                 WRITTEN (bases[c][k] = sum), saving the fill and the read of the old contents.  The tables must be
 *                 distinct buffers (Tape::flush_pending never queues two scatters into one node's gradient, and
 *                 HIPArray::scatter_add_multi_ un-shares copy-on-write handles before it calls this).
 *   create_hinted hints = EK_BUCKETED_HINT_ADJOINT: the caller expects `reduce(EK_HSUM, sin | cos, keep the other half)` followed
 *                 by the scatter_add of that half and of x times that half -- y = hsum(sin(u)) recorded on a tape whose gathers
 *                 need gradients (autodiff.cpp:899-918 gather, :1191-1199 the edge product).  Because that adjoint is linear in
 *                 its seed, the partition is then made with buckets of HALF the size, the reduce call forms both sums in the
 *                 same pass over (l16, x) -- table slice and gradient tables share the LDS; the kept half is neither written nor
 *                 read back -- and the scatter_add call only folds the per-piece tables.  Any other sequence of calls on a
 *                 hinted object works as on an unhinted one.  Ignored for tables beyond 256 half-size buckets and when
 *                 ek_hip_set_tuning("early_adjoint", 0).
 *                 hints |= EK_BUCKETED_HINT_BOUNDED (round 6): the pair of functions is bounded by 1 (sin / cos).  The partition is
 *                 then made with buckets of a QUARTER of the size and the two sums per table entry are formed in 64-bit FIXED
 *                 POINT by non-returning LDS atomics (scale from the bound 1, from max |x| -- which the partition records -- and
 *                 from n, so that no sum can leave 63 bits): no locks, and sums that do not depend on the order of the additions --
 *                 the gradients are BIT-IDENTICAL from run to run (the reference's scatter_add is fixed-order: dynamic.h:517-534).
 *                 A term of 24 significant bits is exact from 2^-13 of its bound upwards; below that its error is < 2^-37 of the
 *                 bound at 64 Mi elements.  Not finite max |x|, or a NaN term (non-finite table entries, an overflowing u): the
 *                 pieces concerned run under the exchange locks as without the hint.  Ignored beyond 256 quarter-size buckets
 *                 (K > 1 Mi entries) and under ENOKI_HIP_EARLY_SUMS=locks.
 * Values of u are bit-identical to the element-order kernels; reductions and sums differ by the ORDER of their fp
 * additions only (unspecified, like ek_hip_reduce / ek_hip_scatter_add mode 0). */
typedef struct ek_hip_bucketed ek_hip_bucketed;
enum { EK_BUCKETED_HINT_ADJOINT = 1, EK_BUCKETED_HINT_BOUNDED = 2 };
EK_API int ek_hip_bucketed_applicable(int type, int index_type, size_t table_size, size_t n);
EK_API int ek_hip_bucketed_pair_create(int type, int index_type, int op, const void *table_a, const void *table_c,
                                       size_t table_size, const void *x, const void *index, size_t n, ek_hip_bucketed **out);
EK_API int ek_hip_bucketed_pair_create_hinted(int type, int index_type, int op, const void *table_a, const void *table_c,
                                              size_t table_size, const void *x, const void *index, size_t n, unsigned hints,
                                              ek_hip_bucketed **out);
/* table_c == NULL with op == EK_MULADD: the product  u = gather(A, idx) * x  alone (no addend table; u = a x + (-0) = a x bit for
 * bit) -- reductions and the adjoint scatter_add of the ONE gather (the stream x * f'(u)) run in bucket order like the pair's.
 * Both gathers under ONE mask array (cuda.h:845-864: masked-out lanes gather 0): inactive entries are dropped by the partition,
 * and what they would have contributed is added by the final step of a reduction: u = fma(0, x, 0) is 0 for a finite x (the lane
 * enters as map_op(0)) and NaN for an infinite or NaN x -- hsum / hprod then are NaN, exactly as the reference's lane-by-lane
 * evaluation (dynamic.h:632-650) and this library's element-order kernels say.  Dropped lanes scatter nothing.
 * ONE rule for every dropped lane: an index outside [0, table_size) -- unspecified in the reference (cuda.h:845-905) -- is
 * treated like a cleared mask bit with a finite x (u = 0, contributes map_op(0), scatters nothing), for a single object and for
 * the slices of a large table alike.
 * mask: n bytes or NULL; 4-byte element types only. */
EK_API int ek_hip_bucketed_pair_create_masked(int type, int index_type, int op, const void *table_a, const void *table_c,
                                              size_t table_size, const void *x, const void *index, const uint8_t *mask, size_t n,
                                              unsigned hints, ek_hip_bucketed **out);
/* create_scalar: u = op(A[index], x, c) with ONE host scalar c in place of the addend table -- `fmadd(gather(A, idx), x, 0.5f)`,
 * `gather(A, idx) * x + 0.5f`.  addend_bits: c as bits of the element type.  All seven ops (the fma family, EK_MULADD / EK_MULSUB /
 * EK_NMULADD); any other op: EK_ERR_INVALID.  The kernels are the pair's: c is staged into every {a, c} record of a bucket's
 * table slice (with the sign of the op, like a table entry), so every call on the object behaves as with a table filled with c --
 * except for the lanes the partition drops (mask bit clear, index outside the table): only the gather is masked, their u is
 * fma(0, x, +-c) = +-c for a finite x (-c for EK_FMSUB / EK_FNMSUB / EK_MULSUB), and a reduction counts map_op(+-c) for each
 * (a zero c: map_op(+0)); a non-finite x there makes hsum / hprod NaN as above.  They scatter nothing.  A NaN or infinite c takes
 * the fixed-point adjoint sums (EK_BUCKETED_HINT_BOUNDED) down the lock path like a non-finite table entry.  mask, hints, shapes and
 * return codes as for create_masked.  EK_OPTIONAL: enoki/hip.h asks for the entry's address first and evaluates in element
 * order without it. */
EK_API EK_OPTIONAL int ek_hip_bucketed_pair_create_scalar(int type, int index_type, int op, const void *table_a, uint64_t addend_bits,
                                              size_t table_size, const void *x, const void *index, const uint8_t *mask, size_t n,
                                              unsigned hints, ek_hip_bucketed **out);
/* create_scalar_device: create_scalar with the scalar in DEVICE memory -- `addend` points to one element of the object's type, the
 * state of a trained bias after `c = c - lr * gradient(c)` (the tape's size-1 gradient, autodiff.cpp:851-853, makes c a size-1
 * array).  The element is read ON THE STREAM, never by the host: no synchronisation, no read-back, so the object can be created and
 * used inside ek_hip_graph_begin / _end and a replay sees the value *addend holds at replay time.  The call broadcasts the element
 * into a table of table_size entries that the object owns (one launch, 4 or 8 B per entry) and every later call on the object reads
 * the scalar from there with the kernels of the two-table object -- the kernels of the benchmark's step, unchanged; a NaN or
 * infinite value sends the fixed-point pieces down the lock path at run time like a non-finite table entry.  The caller keeps
 * `addend` alive and unchanged for the lifetime of the object, like the tables.  ek_hip_bucketed_addend_adjoint accepts the
 * object.  mask must be NULL (EK_ERR_UNSUPPORTED otherwise: a lane the partition drops would have to count map_op(+-c), which
 * only the host-scalar kernels carry; a lane whose index points outside the table counts map_op(0) here, as for two tables).
 * Ops, hints, shapes and the other return codes as for create_scalar.  EK_OPTIONAL like create_scalar. */
EK_API EK_OPTIONAL int ek_hip_bucketed_pair_create_scalar_device(int type, int index_type, int op, const void *table_a, const void *addend,
                                              size_t table_size, const void *x, const void *index, const uint8_t *mask, size_t n,
                                              unsigned hints, ek_hip_bucketed **out);
/* addend_adjoint: out[0] = scale * (sum over ALL n lanes of map_op(u_i)), one element of the object's type on the device -- the
 * gradient of the scalar addend c of  y = hsum(f(u)),  u = op(A[index], x, c),  with map_op = f': the tape's edge from u to a
 * size-1 source sums weight * gradient over u's entries (autodiff.cpp:851-853 broadcasts the size-1 gradient first, :1191-1199
 * forms the edge product).  The sign of du/dc (-1 for EK_FMSUB / EK_FNMSUB / EK_MULSUB) is the tape's edge weight and is NOT
 * applied here; scale_bits: a host factor, bits of the element type.
 * When the object holds early sums of exactly map_op (reduce(EK_HSUM, f, keep, map_op) of a hinted object ran), plane 0 of the
 * per-piece tables is folded by ONE launch: per table entry the value scatter_add would fold into a fresh table for the unweighted
 * stream (fixed-point pieces added as 128-bit integers, converted once and scaled back; float pieces on top), the entry values
 * added in an order fixed by the entry index alone (deterministic; with fixed-point sums bit-identical from run to run).  Without
 * such sums: ek_hip_bucketed_reduce(b, EK_HSUM, map_op, ..) -- one more pass over the lists, never element order.  The lanes the
 * partition dropped have u = +-c and count map_op(+-c) each, ONCE for a sliced table; NaN when one of them carried a non-finite x
 * (as the forward value).  scale is applied to the finished sum inside the fold's last step (a sliced table: inside the launch that
 * combines the slices); only the reduction path needs one more one-thread launch for a scale other than 1.
 * An object without a scalar addend, or a map_op ek_hip_reduce_map refuses: EK_ERR_INVALID.
 * EK_OPTIONAL: without the entry enoki/hip.h keeps a scalar addend that requires a gradient in element order. */
EK_API EK_OPTIONAL int ek_hip_bucketed_addend_adjoint(ek_hip_bucketed *b, int map_op, uint64_t scale_bits, void *out);
EK_API int ek_hip_bucketed_reduce(ek_hip_bucketed *b, int reduce_op, int map_op, void *out, int keep_values, int keep_op);
EK_API int ek_hip_bucketed_scatter_add(ek_hip_bucketed *b, int count, void *const *bases, const int *from_u, const int *map_ops,
                                       const uint64_t *imm_bits, const int *weighted, const int *fresh);
/* scatter_add with a host scalar factor per stream: v_c = scale_c * (from_u[c] ? map_ops[c](u) : imm_c) -- what the tape sends
 * down for backward(c * y), for the -sin(u) of d/du cos(u), ...: the product of an unevaluated function of u with a host scalar
 * (enoki/hip.h: HIPArray::scaled_map_).  scale_bits = NULL: all ones.  Sums that the reduce call of a hinted object formed
 * early are folded with the factor. */
EK_API int ek_hip_bucketed_scatter_add_scaled(ek_hip_bucketed *b, int count, void *const *bases, const int *from_u, const int *map_ops,
                                              const uint64_t *imm_bits, const int *weighted, const int *fresh, const uint64_t *scale_bits);
/* != 0: a hinted object sums keep_op(u) and x * keep_op(u) per table entry inside reduce(EK_HSUM, map_op, keep, keep_op):
 * {sin, cos}, {cos, sin}, {log, rcp} and {f, f} for f in neg abs sqrt rcp rsqrt sin cos exp log */
EK_API int ek_hip_bucketed_early_pair(int map_op, int keep_op);
/* The adjoint without a kernel.  On a kept partition whose buckets are ONE piece each (tuning "direct_tables", ENOKI_HIP_DIRECT_TABLES:
 * 1, the default, for tables of 256 Ki entries and more; 2 for every table; 0 never) the forward + adjoint kernel of a hinted object writes the sums of keep_op(u) and of x * keep_op(u) per
 * table entry in table layout, finished as ek_hip_bucketed_scatter_add would finish them in a FRESH table at scale 1 -- bit for bit.
 * When the scatter_add that backward() is about to issue is exactly those streams (count 1 or 2: the plain and / or the weighted one,
 * from_u / map_ops / weighted as for scatter_add), every scale_bits[s] is 1.0f (NULL: all ones) and every target is fresh, the caller
 * takes the tables over instead: tables[s] receives stream s's buffer of table_size floats, allocated by ek_hip_malloc -- the caller
 * owns it from then on and frees it with ek_hip_free.  The object forgets the sums: a second request is answered
 * EK_ERR_UNSUPPORTED and the scatter_add that follows evaluates the streams on the lists.  Tables nobody takes are freed with the object.
 * EK_ERR_UNSUPPORTED (no error message; nothing changed): not that situation -- call ek_hip_bucketed_scatter_add_scaled as before.
 * EK_OPTIONAL: without the entry enoki/hip.h folds every step. */
EK_API EK_OPTIONAL int ek_hip_bucketed_take_tables(ek_hip_bucketed *b, int count, const int *from_u, const int *map_ops, const int *weighted,
                                                   const uint64_t *scale_bits, void **tables);
/* diagnostics: how the partition cut the object's buckets -- *pieces: pieces that exist (all slices of a large table together),
 * *largest: the most pieces any ONE bucket was cut into (1: every populated bucket is one piece; the per-piece tables of the early
 * sums then hold floats, see ek_hip_bucketed_scatter_add).  Reads the piece prefix back: synchronises, refuses while a step graph
 * is being captured. */
EK_API int ek_hip_bucketed_piece_counts(ek_hip_bucketed *b, uint32_t *pieces, uint32_t *largest);
EK_API int ek_hip_bucketed_destroy(ek_hip_bucketed *b);
/* The PARTITION of an object -- the bucket-ordered lists of (index, x, mask), the page directory, the counts -- depends on (index, x,
 * mask, table size, the bucket size the hints select) only: not on the tables, the op or the addend.  A caller whose index, x and
 * mask arrays keep their contents from step to step (a fit over fixed connectivity: the tables change, the lookups do not) keeps it
 * and stands every later object on it; such an object costs no launch and only its per-expression state (kept u, early sums).
 * partition_retain: a counted handle on the partition of an object that has JUST been created.  partition_release gives it back; the
 *   storage lives until the last object on it and the last handle are gone.  Any number of objects may be alive on one partition.
 * pair_create_on: the object of op(A[index], x, addend) on an existing partition.  table_c / addend_bits / addend_device: the addend
 *   table, a host scalar (bits of the element type), one element in device memory (broadcast into a table the object owns: one launch,
 *   as ek_hip_bucketed_pair_create_scalar_device) -- at most one; none: the product alone (EK_MULADD).  The caller vouches that index,
 *   x and mask hold what they held when the partition was built.
 * Both answer EK_ERR_UNSUPPORTED -- without an error message: the caller partitions for itself -- for anything but the single-object
 * paged form (4-byte element types, tables of one slice), while a step graph is being captured (a captured step's partition is part
 * of the graph; so is an index, x or mask array that lives in a graph's pool: every replay rewrites it), and with the tuning "partition_cache" = 0 (ENOKI_HIP_PARTITION_CACHE=0).  pair_create_on also when type, index type,
 * table size, n, mask presence or the bucket size that `hints` select differ from the partition's, and when the partition was
 * EVICTED: an allocation that runs out of device memory takes back the storage of partitions that no object stands on.
 * EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and partitions every step without them. */
typedef struct ek_hip_bucket_partition ek_hip_bucket_partition;
EK_API EK_OPTIONAL int ek_hip_bucketed_partition_retain(ek_hip_bucketed *b, ek_hip_bucket_partition **out);
EK_API EK_OPTIONAL int ek_hip_bucket_partition_release(ek_hip_bucket_partition *p);
EK_API EK_OPTIONAL int ek_hip_bucketed_pair_create_on(ek_hip_bucket_partition *p, int type, int index_type, int op, const void *table_a,
                                              const void *table_c, const uint64_t *addend_bits, const void *addend_device,
                                              size_t table_size, size_t n, unsigned hints, int has_mask, ek_hip_bucketed **out);
/* ---- multi-GPU without python / torch (csrc/dist.cpp) -------------------------------------------------------------------------
 * One process per GPU.  Index-range sharding: rank r owns [r n / P, (r + 1) n / P) of EVERY size-n array (ek_hip_dist_shard_range),
 * so all vertical operations are local; size-1 arrays and gather tables are replicated.  The exchange steps -- a horizontal result,
 * the gradient of a replicated table -- are RCCL collectives on the library stream, ordered with the kernels (no host wait):
 *   rank 0: ek_hip_dist_unique_id(id);  ship the 128 bytes to the other ranks;  every rank: ek_hip_dist_init(rank, world, id)
 *   y = hsum over all shards:   ek_hip_reduce(EK_HSUM, ...local shard...) then ek_hip_dist_all_reduce(type, EK_HSUM, y, 1)
 *   table gradients:            ek_hip_dist_all_reduce(type, EK_HSUM, g, K), or ek_hip_dist_reduce_scatter (rank r receives bins
 *                               [r c, (r + 1) c) of the sum; send holds world * c entries) + ek_hip_dist_all_gather when needed
 * reduce_op: EK_HSUM | EK_HPROD | EK_HMIN | EK_HMAX.  world == 1 with a NULL id needs no RCCL at all (collectives are local).
 * librccl.so is loaded on first use (no link-time dependency) and ONE copy per process: ENOKI_HIP_RCCL_PATH when set, else the copy
 * that is already mapped (a python caller has torch's own librccl.so: the collectives of torch.distributed and these then share
 * one RCCL runtime), else the loader's search path; ek_hip_dist_rccl_path() says which file it was.  The collectives refuse to run
 * while a step graph is being captured (EK_ERR_UNSUPPORTED, the capture stays valid) and are no-ops for n == 0.  The reference
 * has no counterpart; python callers use enoki_amd.dist (torch.distributed) for the same exchange. */
EK_API int ek_hip_dist_unique_id(void *id128);
EK_API int ek_hip_dist_init(int rank, int world, const void *id128);
EK_API int ek_hip_dist_world(int *rank, int *world);
EK_API int ek_hip_dist_shard_range(size_t n, int rank, int world, size_t *begin, size_t *end);
EK_API int ek_hip_dist_all_reduce(int type, int reduce_op, void *buf, size_t n);
EK_API int ek_hip_dist_reduce_scatter(int type, int reduce_op, void *recv, const void *send, size_t recv_count);
EK_API int ek_hip_dist_all_gather(int type, void *recv, const void *send, size_t send_count);
EK_API int ek_hip_dist_finalize(void);
EK_API const char *ek_hip_dist_rccl_path(void);
/* Partition of an INDEX array by bucket of the range it points into: the active entries (mask) of `index` are grouped by
 * bucket = index >> shift and stored as bucket-local indices (index & ((1 << shift) - 1)), bucket b at local[bucket_base[b] ..
 * bucket_base[b + 1]).  shift is the smallest of {12, 14, 17, 19} with <= 256 buckets for `range` entries (range <= 128 Mi).
 * This is what a program needs whose gather and scatter go through the SAME index array and whose body depends on the
 * gathered values only (tests/sphere.cpp:58-83 behind a pixel permutation): it can then run per TARGET entry, bucket by
 * bucket, with coalesced reads of the source slice and coalesced writes of the target slice instead of two random accesses
 * per element (enoki/vectorize_indexed.h builds that kernel from a user functor).  count + scan + partition: 5 + 9 B per
 * entry with a mask array.  The pointers in the info struct are DEVICE pointers owned by the object. */
typedef struct ek_hip_index_partition ek_hip_index_partition;
typedef struct {
    int shift, n_buckets;
    size_t n, range;
    const uint32_t *bucket_base;      /* n_buckets + 1 entries; bucket_base[n_buckets] = number of active entries */
    const uint32_t *local;            /* bucket-local indices in bucket order */
    /* round 6 -- page_shift != 0: the PAGED layout (single-pass partition, csrc/ek_paged.h; large inputs).  `local` then holds
       pages of 2^page_shift bucket-local indices; bucket b owns the complete pages pages_full[bucket_base[b] .. bucket_base[b + 1])
       and the partially filled ones pages_part[part_base[b] .. part_base[b + 1]) (entry = page << 6 | count - 1).  The order of
       the elements inside a bucket is unspecified.  page_shift == 0: one contiguous run per bucket as before. */
    int page_shift;
    const uint32_t *pages_full, *pages_part, *part_base;
} ek_hip_index_partition_info;
EK_API int ek_hip_index_partition_create(int index_type, const void *index, const ek_operand *mask, size_t n, size_t range,
                                         ek_hip_index_partition **out);
EK_API int ek_hip_index_partition_get(const ek_hip_index_partition *p, ek_hip_index_partition_info *info);
EK_API int ek_hip_index_partition_destroy(ek_hip_index_partition *p);
EK_API int ek_hip_scatter(int type, int index_type, void *base, const ek_operand *value,
                          const ek_operand *index, const ek_operand *mask, size_t n);
/* mode 0: fastest -- LDS-binned accumulation for large inputs (needs `base_size`), hardware atomics otherwise;
           the order of fp additions is unspecified, like the reference's atom.global.add;
   mode 1: deterministic -- stable radix sort by index + sequential per-bin sums: bit-identical to the CPU
           reference's element-order accumulation (dynamic.h:517-534).  Needs `base_size` and an
           index array; under a mask ARRAY it synchronizes once (the number of active pairs is read back), otherwise not
           at all.  Integer types are exact in either mode.
   Tables beyond 4 Mi bins (2 Mi for 8-byte types), mode 0, 256 Ki+ elements: the pairs are split by slice of the table first.
   float32 value ARRAYS through a 32-bit index array into up to 256 Mi bins keep the slice populations on the device (one
   page pool for all slices, one accumulate and one fold launch over all of them): no synchronisation, and the call -- from
   here, per stream from ek_hip_scatter_add_multi, from Tape::backward() as the adjoint of a gather -- can be part of a captured
   step graph.  Every other such call (8-byte and integer types, scalar operands, "bucket_ordered" = 0) reads the slice
   populations back: it synchronises once, and under a capture it fails with EK_ERR_INVALID and leaves the capture valid.
   64-bit index arrays of 256 Ki+ elements into a table of known size <= 2^32 are narrowed once (the reference's tape
   records gather offsets as Int64, autodiff.cpp:355-366) and then take the same paths as 32-bit ones. */
EK_API int ek_hip_scatter_add(int type, int index_type, void *base, size_t base_size,
                              const ek_operand *value, const ek_operand *index,
                              const ek_operand *mask, size_t n, int mode);
/* `count` (1..4) scatter_adds through ONE index / mask array into `count` tables of `base_size` entries each:
 *     bases[c][index[i]] += weights && weights[c] ? safe_mul(*weights[c], *values[c])[i] : (*values[c])[i]
 * This is what Tape::backward() issues for gathers that share their index array (the adjoint of gather is
 * scatter_add, autodiff.cpp:362-381); a weight is the pending edge product w * g of the sweep (autodiff.cpp:871-876,
 * safe_mul 1191-1199), fused into the read instead of being materialised first.  The indices are read and binned
 * once for all tables.  Same modes and accumulation-order caveats as ek_hip_scatter_add; inputs the fused path does
 * not cover are executed as `count` separate scatter_adds (same results). */
EK_API int ek_hip_scatter_add_multi(int type, int index_type, int count, void *const *bases, size_t base_size,
                                    const ek_operand *const *values, const ek_operand *const *weights,
                                    const ek_operand *index, const ek_operand *mask, size_t n, int mode);

/* ek_hip_scatter_add_multi with a unary operation applied to value stream c while it is loaded:
 *     bases[c][index[i]] += w_c[i] * map_c(values[c][i]),   map_c = value_ops[c]  (EK_COPY: none; value_ops == NULL: none)
 * Ops as for ek_hip_reduce_map, floating point types.  This is the adjoint of `gather` when the incoming gradient is
 * itself an unevaluated unary result -- the cos(u) of d/du sin(u) in `hsum(sin(gather(A, i) * x + gather(B, i)))` --
 * so the derivative array is never written or re-read (HIPArray defers fusable unary ops until their first consumer).
 * Paths without an on-load map (deterministic mode, tables of <= 16 Ki bins, 64-bit indices) evaluate the op first. */
EK_API int ek_hip_scatter_add_multi_map(int type, int index_type, int count, void *const *bases, size_t base_size,
                                        const ek_operand *const *values, const int *value_ops,
                                        const ek_operand *const *weights, const ek_operand *index, const ek_operand *mask,
                                        size_t n, int mode);

/* ---------------------------------------------------------------------------------------------
 *  Horizontal ops.  Results of ek_hip_reduce* stay on the device (`out` = 1 element, async);
 *  mask reductions return to the host and therefore synchronize (cuda.h:761-794).
 * ------------------------------------------------------------------------------------------- */
/* Diagnostics of the bucket partition's load balancing.  The single-pass page partition runs one workgroup per compute unit and
 * deals the input to the eight workgroup CLASSES w % 8 (the XCD a workgroup is dispatched to) in proportion to weights that the
 * library feeds back on the device from the classes' loop durations (OPT-IN: tuning "xcd_balance" / ENOKI_HIP_XCD_BALANCE = 1; 2 records
 * the durations of equal chunks without dealing by them; 0, the default, does neither and this call reports zeros; Q16: 65536 =
 * an equal share).  weights8 / ticks8 receive the current weights and the mean loop duration per class of the last stamped launch
 * in 100 MHz ticks (zeros before the first), *dealt (may be NULL) whether the weights are currently applied -- they are once a class
 * is more than 4 % away from an equal share, until all are back within 2 %; the call synchronises. */
EK_API int ek_hip_partition_class_state(uint32_t *weights8, uint32_t *ticks8, uint32_t *dealt);
EK_API int ek_hip_reduce(int op, int type, void *out, const void *in, size_t n);
/* A CHAIN: base(src[0 .. arity)) under n_maps unary ops (map_ops[0] first), evaluated in ONE pass over the operands -- the fused
 * kernel that the reference's JIT assembles for the vertical ops between two evaluation points (src/cuda/jit.cu:1066-1217,
 * :1418-1508), here as a descriptor interpreted by a pre-compiled kernel (a wave-uniform switch per stage around the loop over a
 * lane's 16-byte vector; no kernel per combination).  arity 1: the source itself; arity 2: base_op = EK_ADD | EK_SUB | EK_MUL;
 * arity 3: the fma family and EK_MULADD / EK_MULSUB / EK_NMULADD.  map_ops: the ops ek_hip_reduce_map accepts.  Operands are
 * arrays of n elements, arrays of one element or immediates.  Values are bit-identical to the op-by-op evaluation
 * (ek_hip_ternary, then ek_hip_unary per map); ek_hip_reduce_chain reduces them (order unspecified, like ek_hip_reduce),
 * ek_hip_map_chain writes them.  hsum(sin(exp(fmadd(a, x, b)))) then moves 12 B/elt instead of 28. */
typedef struct {
    int arity, base_op;
    ek_operand src[3];
    int n_maps;
    int map_ops[3];
} ek_chain;
EK_API int ek_hip_reduce_chain(int reduce_op, int type, void *out, const ek_chain *chain, size_t n);
EK_API int ek_hip_map_chain(int type, void *out, const ek_chain *chain, size_t n);
/* ek_hip_map_chain with a tail -- a factor and a second output:
 *     out[i]  = chain(i) * scale           scale: an immediate (ptr == NULL), or NULL for none; one more rounding, like the eager product
 *     out2[i] = op2(w[i], out[i])          op2 = EK_MUL | EK_SAFE_MUL, w an array of n elements
 * Either of out / out2 may be NULL (not both; out2 == NULL: op2 and w are ignored).  This is what the sweep of Tape::backward()
 * asks for at u = fmadd(a, x, b) under y = hsum(sin(u)) (src/autodiff/autodiff.cpp:838-988: grad_b = 1 * grad_u,
 * grad_a = x * grad_u with grad_u = cos(u)): a, x, b are read once and both gradients written, 20 B/elt, where the op-by-op
 * evaluation writes cos(u), re-reads it and multiplies (24 B/elt after a stored u).  Bits as op by op. */
EK_API int ek_hip_map_chain_product(int type, void *out, void *out2, const ek_chain *chain, const ek_operand *scale, int op2,
                                    const ek_operand *w, size_t n);
/* op(map_op(in[0..n))) in ONE pass over `in`: the unary operation is applied while loading (hsum(sin(x)): 4 B/element
 * instead of 12).  map_op: EK_NEG, EK_ABS, EK_SQRT, EK_RCP, EK_RSQRT, EK_SIN, EK_COS, EK_EXP, EK_LOG; floating point
 * types; n >= 1.  Same element values and the same reduction tree as ek_hip_unary followed by ek_hip_reduce (bit-identical
 * results).  The reference reaches this through its trace: `hsum(sin(x))` is one PTX kernel + the CUB reduction
 * (jit.cu:560-760, horiz.cu:162-268); HIPArray defers fusable unary ops until their first consumer. */
EK_API int ek_hip_reduce_map(int op, int map_op, int type, void *out, const void *in, size_t n);
/* fused backward edge to a scalar source: out[0] = hsum(safe_mul(w, g))  (autodiff.cpp:867-871) */
EK_API int ek_hip_hsum_safe_mul(int type, void *out, const ek_operand *w, const ek_operand *g, size_t n);
EK_API int ek_hip_mask_reduce(int op, const uint8_t *mask, size_t n, uint64_t *host_result);
/* inclusive prefix sum (cuda.h:717-726 / horiz.cu:182-200) */
EK_API int ek_hip_psum(int type, void *out, const void *in, size_t n);
/* Lower / upper bound in a sorted table: out[i] = the number of entries t of table[0 .. K) with t < needles[i] (right != 0:
 * t <= needles[i]) -- inverting a CDF, finding a spline interval, sampling a discrete distribution.  What
 * binary_search(0, K, [&](i) { return gather(T, min(i, K - 1)) < v; }) (array_utils.h:130-171) returns, bit for bit, in ONE launch
 * instead of log2(K) + 1 rounds of four vertical ops.  I32 .. F64 (EK_BOOL: EK_ERR_UNSUPPORTED); the comparisons are the type's own:
 * unsigned for U32 / U64, -0.0 < 0.0 false, denormals not flushed, a NaN needle compares false everywhere and yields 0 on both
 * sides (numpy.searchsorted answers K).  The table is sorted ascending and holds no NaN; otherwise the result is unspecified, but
 * the call stays in bounds and terminates.  K = 0: zeros.  K >= 2^32: EK_ERR_UNSUPPORTED.  No host wait: capturable.
 * Tables of up to 64 KiB are searched in LDS; of a larger one every stride-th entry is, and the last log2(stride) steps of a
 * search read a window of `stride` consecutive entries in global memory.  ek_hip_search_sorted_plan (host only) reports that
 * split for a type and K: *resident entries or samples in LDS, *stride (1: resident whole), *global_steps per needle. */
EK_API int ek_hip_search_sorted(int type, uint32_t *out, const void *table, size_t K, const void *needles, size_t n, int right);
EK_API int ek_hip_search_sorted_plan(int type, size_t K, int *resident, int *stride, int *global_steps);
/* The same search with one sorted row per needle: `table` holds `rows` rows of `block` consecutive entries, each sorted ascending
 * and free of NaN (the rows need not be ordered against each other), and out[e] = the number of entries t of needle e's row with
 * t < needles[e] (right != 0: t <= needles[e]), a row-local value in 0 .. block -- the per-row CDFs that ek_hip_psum_blocks writes,
 * one spline per object.  row_index == NULL (blocked needles): n is a multiple of `rows` and needle e belongs to row
 * e / (n / rows), "M samples per ray".  Otherwise needle e belongs to row min(row_index[e], rows - 1): the clamp is part of the
 * contract, no row value reads outside the table.  What binary_search(0, block, [&](i) { return gather(T, row * block +
 * min(i, block - 1)) < v; }) returns, bit for bit and from run to run, in ONE launch, without the `row` array; types, comparisons and
 * NaN needles as for ek_hip_search_sorted.  block == 0, n % rows != 0 for blocked needles, rows == 0 with n > 0, a null pointer with
 * n > 0: EK_ERR_INVALID; other types and rows * block >= 2^32: EK_ERR_UNSUPPORTED; n == 0: nothing is launched.  The pointers need
 * only element alignment.  No scratch, no read-back, no host wait: capturable.
 * ek_hip_search_sorted_blocks_plan (host only, no device access; indexed != 0: with a row_index; compute_units == 0: 256) reports the
 * route -- *route 0 nothing to do; 1 tile of rows (blocked, a row fits 64 KiB of LDS: a workgroup stages *rows_per_tile consecutive
 * rows with 16-byte loads and searches their needles in LDS; with few rows of many needles *workgroups_per_row > 1 workgroups stage
 * the same row and take a piece of its needles each); 2 sampled row (blocked, larger rows: per row the two-level search of
 * ek_hip_search_sorted, *workgroups_per_row as before); 3 indexed, the whole table staged in LDS; 4 indexed, every step in global
 * memory (saves launches and index traffic, not bandwidth); 5 blocked with rows == 1: forwarded to ek_hip_search_sorted -- and the
 * search inside a row: *resident entries or samples in LDS (route 4: read in global memory instead), *stride (1: the row is resident
 * whole), *global_steps per needle after the resident ones.  A sampled row with few needles per workgroup stages fewer samples. */
EK_API int ek_hip_search_sorted_blocks(int type, uint32_t *out, const void *table, size_t rows, size_t block, const void *needles,
                                       size_t n, const uint32_t *row_index, int right);
EK_API int ek_hip_search_sorted_blocks_plan(int type, size_t rows, size_t block, size_t n, int indexed, int compute_units, int *route,
                                            int *rows_per_tile, int *workgroups_per_row, int *resident, int *stride, int *global_steps);
/* Block reductions: out[j] = reduce_op(in[j * block .. (j + 1) * block)) for j < n / block -- the samples of a pixel summed into
 * the image, the rows of a row-major matrix -- without the index array of scatter_add(zero(n / block), x, arange(n) / block).
 * op: EK_HSUM / EK_HPROD / EK_HMIN / EK_HMAX with the semantics of ek_hip_reduce (integer sums and products wrap; floating point
 * hmin / hmax are minNum / maxNum: a NaN is ignored unless the whole block is NaN, -0 < +0); I32 .. F64.  block == 0 or
 * n % block != 0: EK_ERR_INVALID; n == 0: nothing is launched; block == 1 is a device copy; block == n IS ek_hip_reduce (bit
 * for bit).  The pointers need only element alignment.  No atomics, no read-back, no host wait (capturable); the result is
 * bit-identical from run to run for a given (type, op, n, block, pointer alignment, device).
 * ek_hip_reduce_blocks_plan (host only, no device access; compute_units == 0: 256) reports the route ek_hip_reduce_blocks takes:
 * *regime 0 copy, 1 whole-array reduction, 2 packed (a workgroup stages a tile of whole blocks in LDS, a power-of-two group of
 * adjacent lanes per block), 3 one workgroup per block, 4 split (few large blocks: *splits >= 2 pieces per block and a packed
 * fold of the partials; *splits == 1 otherwise), and *workgroups, the grid of its first launch.
 * EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and throws without them. */
EK_API EK_OPTIONAL int ek_hip_reduce_blocks(int op, int type, void *out, const void *in, size_t n, size_t block);
EK_API EK_OPTIONAL int ek_hip_reduce_blocks_plan(int type, size_t n, size_t block, int compute_units, int *regime, int *splits, size_t *workgroups);
/* The transpose of the block sum (numpy.repeat): out[i] = in[i / block] for i < m * block, without the index array of
 * gather(v, arange(m * block) / block).  Keyed on the element size: I32 .. F64.  block == 0: EK_ERR_INVALID; m == 0: nothing is
 * launched; block == 1 is a device copy.  16-byte stores wherever `out` allows; one division per lane.  EK_OPTIONAL as above. */
EK_API EK_OPTIONAL int ek_hip_repeat(int type, void *out, const void *in, size_t m, size_t block);
/* Per-block prefix sums: for block j < n / block and position k < block, with x = in + j * block,
 *     out[j * block + k] = x[0] + .. + x[k]            flags == 0
 *                          x[0] + .. + x[k - 1]        EK_SCAN_EXCLUSIVE
 *                          x[k] + .. + x[block - 1]    EK_SCAN_REVERSE
 *                          x[k + 1] + .. + x[block-1]  EK_SCAN_EXCLUSIVE | EK_SCAN_REVERSE
 * the empty sum being +0 (+0.0) -- the optical depth in front of every sample of a ray, the per-row CDFs of a row-major table,
 * running counts inside a segment -- in one pass, where psum(x) - repeat(gather(psum(x), block starts), block) takes four and
 * subtracts two large sums to get a small one.  I32 .. F64 (EK_BOOL or an unknown type: EK_ERR_UNSUPPORTED); integer sums wrap.
 * block == 0, n % block != 0, a null pointer with n > 0 or a flag bit other than the two: EK_ERR_INVALID; n == 0: nothing is
 * launched.  The pointers need only element alignment; out and in are identical or do not overlap.  Guarantees:
 *   - every output is a sum of its own terms only: nothing is ever subtracted, an exclusive result is not "inclusive minus x";
 *   - an inclusive entry with one term is that input bit for bit, -0.0 included;
 *   - an exclusive entry k is bit for bit the inclusive entry k - 1 of the same array (k + 1 for EK_SCAN_REVERSE);
 *   - no value of one block ever reaches another block's output: a NaN or an infinity in block j leaves blocks j - 1 and j + 1 alone;
 *   - the shape of every sum is fixed by (type, n, block, flags, pointer alignment, number of compute units): the result is
 *     bit-identical from run to run;
 *   - no atomics on data, no read-back, no host wait: the call can be captured into a step graph; scratch comes from ek_hip_malloc
 *     and is freed stream-ordered;
 *   - no kernel waits for another workgroup -- no ticket, no descriptor, no look-back, no polling loop: what one workgroup needs
 *     from another is a separate launch on the stream, so no kernel of this entry can spin.
 * ek_hip_psum_blocks_plan (host only, no device access; compute_units == 0: 256) reports the route: *regime 0 copy or zero fill
 * (block == 1), 1 packed (block <= 1024: tiles of whole blocks scanned in LDS), 2 one workgroup per block, 3 split (fewer than
 * 2 x compute_units blocks of at least 16 Ki entries: *splits >= 2 pieces per block, their totals, an exclusive scan of the
 * totals, the pieces with their carry-in; *splits == 1 otherwise), and *workgroups, the grid of its first launch.
 * EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and throws without them. */
enum { EK_SCAN_EXCLUSIVE = 1, EK_SCAN_REVERSE = 2 };
EK_API EK_OPTIONAL int ek_hip_psum_blocks(int type, void *out, const void *in, size_t n, size_t block, int flags);
EK_API EK_OPTIONAL int ek_hip_psum_blocks_plan(int type, size_t n, size_t block, int compute_units, int *regime, int *splits, size_t *workgroups);
/* Stable sort inside every block: for row j < n / block, with x = in + j * block and p the permutation that puts x in order,
 *     out_index[j * block + k]  = p[k]  (the row-local position 0 .. block - 1 of the entry that lands at slot k;
 *                                        + j * block with EK_SORT_FLAT_INDEX: ready for a gather from another array)
 *     out_values[j * block + k] = x[p[k]], the entry's own bits
 * -- a ray's hits in depth order, a row of prefix sums made ascending for ek_hip_search_sorted_blocks, old and new samples merged.
 * Order: ascending by `<`; entries that compare equal keep their input order (stable); -0.0 and +0.0 compare equal and keep their
 * bits; every NaN, whatever its sign bit or payload, comes after all numbers, in input order.  EK_SORT_DESCENDING orders by `>`,
 * ties still in input order, NaN still last.  Per row this is numpy.argsort(row, kind="stable"), descending
 * numpy.argsort(-row, kind="stable") for floating point and numpy.argsort(~row, kind="stable") for integers, exactly.
 * Either output pointer may be NULL (not both): that output is neither computed into memory nor needs a buffer.  I32 .. F64
 * (EK_BOOL or an unknown type: EK_ERR_UNSUPPORTED); n > 2^32 - 1: EK_ERR_UNSUPPORTED.  block == 0, n % block != 0, both outputs
 * NULL, a null `in` with n > 0, an unknown flag bit, or `in` and the outputs (or the two outputs) overlapping: EK_ERR_INVALID;
 * n == 0: nothing is launched.  The pointers need only element alignment.  Guarantees:
 *   - the order is total on (key, input position), so the result is a function of the input alone: bit-identical from run to run;
 *   - no atomics, no read-back, no host wait: capturable into a step graph; scratch comes from ek_hip_malloc and is freed
 *     stream-ordered;
 *   - no kernel waits for another workgroup: what one workgroup needs from another is a later launch on the stream.
 * ek_hip_sort_blocks_plan (host only, no device access; want_index and compute_units change no route today) reports *route:
 * 0 trivial (block == 1: copy / zeros / 0, 1, 2, ..), 1 packed (block <= 2048: *tile_rows whole rows per workgroup, padded to a
 * power of two and sorted at once by a bitonic network in LDS), 2 one workgroup per row (block <= *chunk: 8192 entries for 4-byte
 * types, 4096 for 8-byte types), 3 chunks and merges (longer rows: chunks of *chunk entries sorted to scratch, then
 * *merge_passes = ceil(log2(ceil(block / chunk))) merge launches, the last of which writes the caller's outputs: 1 + *merge_passes
 * launches in all), and *workgroups, the grid of its first launch.  EK_OPTIONAL as above. */
#define EK_SORT_DESCENDING 1
#define EK_SORT_FLAT_INDEX 2
EK_API EK_OPTIONAL int ek_hip_sort_blocks(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, size_t block, int flags);
EK_API EK_OPTIONAL int ek_hip_sort_blocks_plan(int type, size_t n, size_t block, int want_index, int compute_units, int *route,
                                               size_t *tile_rows, size_t *chunk, int *merge_passes, size_t *workgroups);
/* Ragged segments: the counterpart of ek_hip_reduce_blocks for segments of different lengths -- the samples of a ray that are left
 * after compress(), the hits of a ray in a mesh.  `starts` is a device array of m non-decreasing positions; with starts[m] := n,
 * segment j is in[lo_j .. hi_j) with lo_j = min(starts[j], n) and hi_j = max(lo_j, min(starts[j + 1], n)).  Entries in front of
 * starts[0] belong to no segment.  The starts of given counts are their exclusive prefix sum: ek_hip_psum_blocks(EK_U32, starts,
 * counts, m, m, EK_SCAN_EXCLUSIVE).
 *     out[j] = reduce_op(in[lo_j .. hi_j))        for j < m
 * op: EK_HSUM / EK_HPROD / EK_HMIN / EK_HMAX with the semantics of ek_hip_reduce (integer sums and products wrap; floating point
 * hmin / hmax are minNum / maxNum, -0 < +0); an empty segment yields the identity: +0, 1, NaN for floating point hmin / hmax
 * (like a block of NaNs), the type's max / lowest for integer hmin / hmax.  I32 .. F64 (EK_BOOL or an unknown type:
 * EK_ERR_UNSUPPORTED); n or m above 2^32 - 1: EK_ERR_UNSUPPORTED; an unknown op, a null `out` or `starts`, a null `in` with
 * n > 0 or a pointer that is not element-aligned: EK_ERR_INVALID; m == 0: nothing is launched; n == 0: every entry is the identity.
 * The pointers need only element alignment.  Guarantees:
 *   - `starts` is never read back, so it cannot be validated; whatever it holds, no kernel reads outside in[0 .. n) and
 *     starts[0 .. m) or writes outside out[0 .. m), every out[j] is written exactly once and every kernel terminates.  With
 *     non-decreasing starts, some of which may exceed n, the result is as defined above; with starts that decrease somewhere the
 *     values are unspecified;
 *   - no value of one segment reaches another segment's output;
 *   - no atomics, no read-back, no host wait: capturable into a step graph; scratch comes from ek_hip_malloc and is freed
 *     stream-ordered;
 *   - no kernel waits for another workgroup -- no ticket, no look-back, no polling loop;
 *   - the route and every grid depend on (type, n, m, number of compute units, pointer alignment) only, never on the contents of
 *     `starts`; the shape of every sum is a function of those and of `starts`: the result is bit-identical from run to run.
 * ek_hip_reduce_segments_plan (host only, no device access; compute_units == 0: 256) reports the route, which is chosen from the
 * mean length ceil(n / m): *route 0 nothing (m == 0), 1 grouped (n <= 1024 m: a workgroup owns a fixed number of consecutive
 * segments, walks their entries in LDS tiles, *group_lanes = 2^ceil(log2(clamp(mean, 1, 64))) adjacent lanes per segment;
 * *group_lanes == 0 otherwise), 2 one workgroup per segment, 3 split (fewer than 2 x compute_units segments of mean >= 16 Ki:
 * *splits >= 2 pieces per segment, whose length follows the segment's own, and a packed fold of the partials; *splits == 1
 * otherwise), and *workgroups, the grid of its first launch.
 * ek_hip_repeat_segments is the transpose of the segment sum over n output entries:
 *     out[i] = in[j] for the last j < m with starts[j] <= i (among equal starts: the non-empty segment), 0 if there is none
 * -- gather(v, search_sorted(starts, arange(n), right) - 1) without the index array.  Keyed on the element size: I32 .. F64.
 * m == 0: zeros; n == 0: nothing is launched.  Every out[i] is written exactly once, and no read leaves in[0 .. m) and
 * starts[0 .. m), whatever `starts` holds; 16-byte stores wherever `out` allows.  The other guarantees hold as above.
 * EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and throws without them. */
EK_API EK_OPTIONAL int ek_hip_reduce_segments(int op, int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m);
EK_API EK_OPTIONAL int ek_hip_repeat_segments(int type, void *out, const void *in, const uint32_t *starts, size_t m, size_t n);
EK_API EK_OPTIONAL int ek_hip_reduce_segments_plan(int type, size_t n, size_t m, int compute_units, int *route, int *group_lanes, int *splits,
                                                   size_t *workgroups);
/* Prefix sums inside ragged segments: the counterpart of ek_hip_psum_blocks for the segments of ek_hip_reduce_segments.  With
 * starts[m] := n, segment j is [lo_j, hi_j) with lo_j = min(starts[j], n) and hi_j = max(lo_j, min(starts[j + 1], n)); for entry i
 * of segment j
 *     out[i] = in[lo_j] + .. + in[i]                    flags == 0
 *              in[lo_j] + .. + in[i - 1]                EK_SCAN_EXCLUSIVE (the segment's first entry: +0)
 *              in[i] + .. + in[hi_j - 1]                EK_SCAN_REVERSE
 *              in[i + 1] + .. + in[hi_j - 1]            EK_SCAN_EXCLUSIVE | EK_SCAN_REVERSE (the segment's last entry: +0)
 * -- the optical depth in front of every sample that compress() left of a ray, a CDF per segment -- where the whole-array
 * spelling psum(x) - repeat_segments(gather(psum(x), starts), starts, n) takes four passes and subtracts two large running sums
 * to get a small one.  The entries in front of min(starts[0], n) belong to no segment: their result is +0 in all four modes; with
 * m == 0 the whole result is +0; n == 0: nothing is launched.  Empty segments own no entry and change nothing.  I32 .. F64
 * (EK_BOOL or an unknown type: EK_ERR_UNSUPPORTED); integer sums wrap.  n or m above 2^32 - 1: EK_ERR_UNSUPPORTED; a flag bit
 * other than the two, a null or misaligned `out` or `in` with n > 0, a null or misaligned `starts` with n > 0 and m > 0:
 * EK_ERR_INVALID, before anything is launched.  out == in is allowed; any other overlap is the caller's error.
 *   - every output is a sum of its own segment's terms only; nothing is ever subtracted;
 *   - an inclusive entry with one term is its input bit for bit, -0.0 included;
 *   - an exclusive entry IS the neighbouring inclusive entry of a call without EK_SCAN_EXCLUSIVE, moved and never recomputed:
 *     entry i - 1 forward, entry i + 1 with EK_SCAN_REVERSE;
 *   - a NaN or an infinity stays inside its segment; one in front of starts[0] reaches nothing;
 *   - floating point prefix sums are sums in a fixed tree order: they are NOT guaranteed to ascend entry by entry;
 *   - the shape of every sum is a function of (type, flags, n, m, pointer alignment, number of compute units) and of the contents
 *     of `starts`: the result is bit-identical from run to run;
 *   - no global atomics, no ticket, descriptor, look-back or polling loop, no kernel waits for another workgroup, no read-back and
 *     no host wait; scratch comes from ek_hip_malloc and is freed stream-ordered: capturable into a step graph and replayable
 *     with other contents in `starts`;
 *   - `starts` is never validated (that would need a read-back): whatever it holds, every read lies inside in[0 .. n) and
 *     starts[0 .. m), every entry of out[0 .. n) is written exactly once and nothing outside it, and every loop's trip count is
 *     bounded by n, m or a constant.  Starts above n are clamped and give the result above; where `starts` decreases only the
 *     values are unspecified.
 * ONE output-driven route: a workgroup owns a run of consecutive tiles of *tile = 16 KiB / element size output entries, marks the
 * starts that fall into a tile as head flags in LDS and scans (value, flag) pairs there; what reaches a workgroup's first tile from
 * before it comes from two earlier launches (a total per workgroup, their scan by one workgroup).  ek_hip_psum_segments_plan
 * (host only, no device access; compute_units == 0: 256) reports *tile, *tiles_per_workgroup = ceil(tiles / min(tiles,
 * 4 x compute_units)) with tiles = ceil(n / *tile), *workgroups = ceil(tiles / *tiles_per_workgroup) and *launches (1 for one
 * workgroup, 3 otherwise); the last three are 0 for n == 0 or m == 0.  Nothing but its arguments enters.
 * EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and throws without them. */
EK_API EK_OPTIONAL int ek_hip_psum_segments(int type, void *out, const void *in, size_t n, const uint32_t *starts, size_t m, int flags);
EK_API EK_OPTIONAL int ek_hip_psum_segments_plan(int type, size_t n, size_t m, int compute_units, size_t *tile, size_t *tiles_per_workgroup,
                                                 size_t *workgroups, int *launches);
/* Every needle searched in ITS OWN ragged segment of a flat table: the counterpart of ek_hip_search_sorted_blocks for the segments
 * of ek_hip_reduce_segments, and the call that reads the per-segment CDF that ek_hip_psum_segments writes.  With
 * table_starts[m] := nt, segment j is [lo_j, hi_j) with lo_j = min(table_starts[j], nt) and hi_j = max(lo_j,
 * min(table_starts[j + 1], nt)); every segment is expected to be sorted ascending and free of NaN, the segments need not be ordered
 * against each other.  The segment of needle e is named in exactly one of two ways:
 *   needle_starts (m entries)   the last j with needle_starts[j] <= e, the rule of ek_hip_repeat_segments: segment j gets
 *                               needle_starts[j + 1] - needle_starts[j] consecutive needles, none is allowed; a needle in front of
 *                               needle_starts[0] has no segment.  m == 0: no needle has one, and needle_starts may be null;
 *   row_index (n entries)       segment min(row_index[e], m - 1); m == 0 with n != 0: EK_ERR_INVALID.
 *     out[e] = the number of entries t of the needle's segment with t < needles[e]      flags == 0
 *              ... with t <= needles[e]                                                  EK_SEARCH_RIGHT
 *              lo_j + that number, the position in `table` (it may equal hi_j)           EK_SEARCH_FLAT
 * A needle without a segment, an empty segment and a NaN needle yield 0 (the comparisons are the type's own); nt == 0 yields
 * zeros; n == 0: nothing is launched.  For every other needle, on sorted segments, out[e] is numpy.searchsorted(table[lo_j:hi_j],
 * needles[e], side) bit for bit.  I32 .. F64, table and needles of the same type (EK_BOOL or an unknown type:
 * EK_ERR_UNSUPPORTED); nt, m or n above 2^32 - 1: EK_ERR_UNSUPPORTED; a flag bit other than the two, both owners or (with m != 0)
 * neither, a null `out`, `needles`, `table` (nt > 0) or `table_starts` (m > 0) with n > 0, a pointer that is no multiple of its
 * element size: EK_ERR_INVALID, before anything is launched.
 *   - no atomics, no scratch memory, no read-back, no host wait, no kernel waits for another workgroup: capturable into a step
 *     graph and replayable with other contents in all three index arrays; bit-identical from run to run;
 *   - the index arrays are never validated (that would need a read-back): whatever they hold, every read lies inside
 *     table[0 .. nt), the starts' [0 .. m) and needles' and row_index' [0 .. n), every entry of out[0 .. n) is written exactly
 *     once and nothing outside it, every loop's trip count is bounded by a constant, log2(nt) or log2(m), and every result lies in
 *     0 .. hi_j - lo_j of the clamped segment the needle was assigned to (with EK_SEARCH_FLAT in 0 .. nt).  Where starts decrease or
 *     a segment is not sorted only the VALUES are unspecified.
 * Three routes, chosen from (type, nt, m, n, compute units) alone: 1 paired tiles (needle_starts: a workgroup owns consecutive
 * tiles of *tile_needles needles, stages a window of at most *window starts of both arrays and at most *lds_entries table entries
 * of the tile's segments in LDS; a needle whose clamped segment is not staged is searched in global memory), 2 indexed with the
 * table staged whole (row_index, nt <= *lds_entries), 3 indexed in global memory.  ek_hip_search_sorted_segments_plan (host only,
 * no device access; indexed != 0: with a row_index; compute_units == 0: 256) reports them with *tiles_per_workgroup =
 * ceil(tiles / min(tiles, 2 x compute_units)), tiles = ceil(n / *tile_needles), and *workgroups = ceil(tiles /
 * *tiles_per_workgroup); *window is 0 for routes 2 and 3; n == 0: route 0 and no workgroups.  Nothing but its arguments enters.
 * EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and throws without them. */
#define EK_SEARCH_RIGHT 1
#define EK_SEARCH_FLAT  2
EK_API EK_OPTIONAL int ek_hip_search_sorted_segments(int type, uint32_t *out, const void *table, size_t nt, const uint32_t *table_starts,
                                                     size_t m, const void *needles, size_t n, const uint32_t *needle_starts,
                                                     const uint32_t *row_index, int flags);
EK_API EK_OPTIONAL int ek_hip_search_sorted_segments_plan(int type, size_t nt, size_t m, size_t n, int indexed, int compute_units, int *route,
                                                          size_t *tile_needles, size_t *tiles_per_workgroup, size_t *workgroups,
                                                          size_t *lds_entries, size_t *window);
/* Stable sort inside every ragged segment: the counterpart of ek_hip_sort_blocks for the segments of ek_hip_reduce_segments (starts[m]
 * := n; segment j is [lo_j, hi_j) with lo_j = min(starts[j], n) and hi_j = max(lo_j, min(starts[j + 1], n))).  With x = in + lo_j
 * and p the permutation that puts x in order,
 *     out_index[lo_j + k]  = p[k]  (the segment-local position of the entry that lands at slot k; + lo_j with EK_SORT_FLAT_INDEX:
 *                                   ready for a gather from another array)
 *     out_values[lo_j + k] = x[p[k]], the entry's own bits, fetched through the sorted position
 * -- a ray's hits in depth order once rays keep different counts, and the call that makes the segments ascend that
 * ek_hip_search_sorted_segments expects (a float CDF from ek_hip_psum_segments need not).  Order, ties, -0.0, NaN and both flags are
 * those of ek_hip_sort_blocks: per segment numpy.argsort(segment, kind="stable"), descending argsort(-segment) for floating point
 * and argsort(~segment) for integers, exactly; ek_hip_sort_segments(x, arange(m) * B) is bit-equal to ek_hip_sort_blocks(x, B).
 * Entries in front of min(starts[0], n) belong to no segment and stay where they are: out_values copies them, out_index holds
 * their own position i in both modes (this prefix counts from 0); m == 0: the whole array is such a prefix, and starts may be null.
 * Empty segments own nothing.  Either output pointer may be NULL (not both): that output is neither computed into memory nor
 * needs a buffer.  I32 .. F64 (EK_BOOL or an unknown type: EK_ERR_UNSUPPORTED); n or m above 2^32 - 1: EK_ERR_UNSUPPORTED; both
 * outputs NULL, a null `in` or (m > 0) `starts` with n > 0, an unknown flag bit, a pointer that is no multiple of its element size,
 * or `in` and the outputs (or the two outputs) overlapping: EK_ERR_INVALID, before anything is launched; n == 0: nothing is
 * launched.  The pointers need only element alignment.  Guarantees:
 *   - the order is total on (key, input position): bit-identical from run to run;
 *   - no global atomics, no read-back, no host wait, no kernel waits for another workgroup; the launch sequence is fixed by
 *     (type, n, m, compute units), so the call is capturable into a step graph and replayable with other contents in `starts`;
 *     scratch comes from ek_hip_malloc and is freed stream-ordered;
 *   - `starts` is never validated (that would need a read-back): whatever it holds, every read lies inside in[0 .. n) and
 *     starts[0 .. m), every entry of each requested output is written, nothing outside them, a flat result lies in [0, n) and so
 *     does a local one, and every loop's trip count is bounded by a host-known number or the log2 of one.  Where `starts` does not
 *     ascend only the values are unspecified.
 * ONE output-driven route: a workgroup owns a run of consecutive tiles of *tile = 2048 entries, marks the starts that fall into a
 * tile as head flags in LDS and sorts the tile's composites by (run in tile, key, position) in one bitonic network; a segment
 * inside one tile is final there, the pieces of a segment that crosses a tile boundary go to scratch and are merged by *merges =
 * ceil(log2(*tiles)) launches, pass p over pairs of groups of 2^p tiles.  A one-workgroup launch in between counts, on the device,
 * how many passes the data need; the workgroups of every later pass return at once.  ek_hip_sort_segments_plan (host only, no device
 * access; compute_units == 0: 256; want_index changes nothing today) reports *tile, *tiles = ceil(n / *tile), *tiles_per_workgroup
 * = ceil(tiles / min(tiles, 8 x compute_units)), *workgroups = ceil(tiles / *tiles_per_workgroup), *merges, *merge_workgroups (the
 * grid of a merge launch), *launches (1 for one tile, 2 + *merges otherwise) and *scratch_bytes (0 for one tile; else one buffer of
 * n composites of 8 or 12 bytes, two from two merges on, and tiles + 1 words); all but *tile are 0 for n == 0 or m == 0 (m == 0 is
 * a copy and a count).  EK_OPTIONAL: enoki/hip.h asks for the entries' addresses first and throws without them. */
EK_API EK_OPTIONAL int ek_hip_sort_segments(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, const uint32_t *starts,
                                            size_t m, int flags);
EK_API EK_OPTIONAL int ek_hip_sort_segments_plan(int type, size_t n, size_t m, int want_index, int compute_units, size_t *tile, size_t *tiles,
                                                 size_t *tiles_per_workgroup, size_t *workgroups, int *merges, size_t *merge_workgroups,
                                                 int *launches, size_t *scratch_bytes);
/* Stable sort of a whole array: with p the permutation that puts the n entries of `in` in order,
 *     out_index[k]  = p[k]  (the position of the entry that lands at slot k: ready for a gather from another array)
 *     out_values[k] = in[p[k]], the entry's own bits, fetched through the sorted position
 * -- the call that makes the hits of a ray, the fragments of a pixel or the particles of a cell consecutive, as every *_blocks and
 * *_segments entry presumes: sort the ids, gather the payload through out_index, and ek_hip_search_sorted(sorted ids, 0 .. m - 1)
 * gives the `starts` of the segments.  Order, ties, -0.0, NaN and EK_SORT_DESCENDING are those of ek_hip_sort_blocks, and the result
 * is bit for bit that of ek_hip_sort_blocks(.., n, block = n, flags): numpy.argsort(x, kind="stable"), descending argsort(-x) for
 * floating point and argsort(~x) for integers.  EK_SORT_FLAT_INDEX is accepted and changes nothing.  Either output pointer may be
 * NULL (not both): that output is neither written nor allocated.  I32 .. F64 (EK_BOOL: EK_ERR_UNSUPPORTED); more than 2^32 - 1
 * entries: EK_ERR_UNSUPPORTED; an unknown flag bit, a null `in` with n > 0, a misaligned pointer, `in` overlapping an output or the
 * outputs overlapping each other: EK_ERR_INVALID, all before any launch; n == 0 launches nothing.
 * Guarantees: the order is total on (key, position), so the result is bit-identical from run to run; no global atomics; no kernel
 * waits for another workgroup (no look-back, no ticket); no read-back and no host wait; the launch sequence is fixed by (type, n,
 * compute units, tuning), so the call can be captured into a step graph and replayed with other contents; scratch comes from
 * ek_hip_malloc and is freed stream-ordered.
 * ek_hip_sort_plan (host only, no device access; compute_units == 0: 256; want_index changes nothing) reports *route: 0 trivial
 * (n <= 1), 1 forwarded to ek_hip_sort_blocks with block == n, 2 radix: *passes = 4 or 8 (the key bytes) least-significant-digit
 * passes of 8 bits over (key, position) pairs, each a per-workgroup digit count, two scans of the counts and a stable scatter that
 * ranks with wave ballots; *tile entries per tile (route 1: block_sort's chunk), *tiles_per_workgroup = ceil(tiles / min(tiles,
 * 2 x compute_units)) with tiles = ceil(n / *tile), *workgroups = ceil(tiles / *tiles_per_workgroup) (route 1: the grid of the first
 * launch), *launches (route 2: 4 x *passes; route 1: those of ek_hip_sort_blocks) and *scratch_bytes.  The tuning "sort_radix"
 * (ek_hip_set_tuning) picks between routes 1 and 2: 0 always forwards, 1 (default) takes the radix route from the measured crossover
 * on -- one threshold per element size, never below block_sort's chunk + 1 --, 2 takes it for every n >= 2; the plan reports the
 * route under the current setting.  EK_OPTIONAL: enoki/hip.h asks for the entry's address first and throws without it. */
EK_API EK_OPTIONAL int ek_hip_sort(int type, void *out_values, uint32_t *out_index, const void *in, size_t n, int flags);
EK_API EK_OPTIONAL int ek_hip_sort_plan(int type, size_t n, int want_index, int compute_units, int *route, int *passes, size_t *tile,
                                        size_t *tiles_per_workgroup, size_t *workgroups, int *launches, size_t *scratch_bytes);

/* Stable sort of (key, element number) pairs by the low `key_bits` bits of 32-bit keys:
 *     keys_out = keys sorted ascending, perm_out[j] = original position of keys_out[j]; equal keys keep their order.
 * The building block of partition() -- the reference sorts (pointer, lane) pairs with a 64-bit CUB radix sort and run-length
 * encodes them (cuda_partition, src/cuda/horiz.cu:35-122); callers here first map the pointers to dense 32-bit keys.
 * ceil(key_bits / 8) ballot-ranked LSD passes, 20 B per entry and pass. */
EK_API int ek_hip_sort_pairs(int key_bits, const uint32_t *keys, size_t n, uint32_t *keys_out, uint32_t *perm_out);

/* PCG32 draw (include/enoki/random.h:68-133): one fused kernel that advances `state` by `inc` where `mask`
 * is set (state_out[i] = mask[i] ? state[i] * 0x5851f42d4c957f2d + inc[i] : state[i]) and writes the output
 * function of the OLD state: u32[n], f32[n] in [0,1), f64[n] in [0,1), or u64[n] (two steps; the FIRST draw is the high
 * word, which is what the pinned g++ reference build produces for random.h:87-89). */
typedef enum { EK_PCG32_UINT32 = 0, EK_PCG32_FLOAT32, EK_PCG32_UINT64, EK_PCG32_FLOAT64 } ek_pcg32_kind;
EK_API int ek_hip_pcg32_next(int kind, void *out, uint64_t *state_out, const ek_operand *state,
                             const ek_operand *inc, const ek_operand *mask, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* ENOKI_HIP_C_API_H */
