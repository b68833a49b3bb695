/* mi355_spmv.h — C ABI of the MI355X-native CSR SpMV engine (libmi355spmv.so).
 *
 * Drop-in boundary.  The reference (peakcrosser7/spmv-samples) has no FFI of its
 * own: its operator boundary is the header-only C++ template
 *
 *   template <index_t, offset_t, mat_value_t, vec_x_value_t, vec_y_value_t>
 *   void SpMV(const std::string& kind_str, index_t n_rows, index_t n_cols,
 *             offset_t nnz, const offset_t* Ap, const index_t* Aj,
 *             const mat_value_t* Ax, const vec_x_value_t* x, vec_y_value_t* y);
 *                                          (reference include/spmv.h:29-48)
 *
 * and every kind behind it is `SpMV_<kind>(n_rows, n_cols, nnz, Ap, Aj, Ax, x, y)`
 * with that same 8-argument device-pointer signature, registered by one
 * `X("label", SpMV_<kind>)` row of the SPMV_KINDS X-macro (include/spmv.h:18-27,
 * README.md:28-45).  The entry points below are what such a kind binds: plain
 * pointers and sizes, no C++ or torch types.  spmv-samples_amd/host/spmv/mi355.hpp
 * holds the template kinds that call them; INTEGRATION.md shows the two lines a
 * maintainer of the reference adds.
 *
 * Conventions carried over from the reference:
 *   - Ap, Aj, Ax, x, y are DEVICE pointers owned by the caller (main.cu:48-74).
 *   - index_t is 32-bit (main.cu:15); offset_t is 32- or 64-bit; values are
 *     float or double, the same type for A, x and y (main.cu:17).
 *   - y is fully overwritten (beta = 0), empty rows give 0 (cpu_navie.hpp:10-15).
 *   - The reference aborts on a device error (common.cuh:13-23).  The C ABI never
 *     aborts: it returns a status; the C++ kinds turn non-zero into abort().
 *
 * Symbol suffix:  _<i32|i64>_<f32|f64>  =  offset_t width, value type.
 */
#ifndef MI355_SPMV_H
#define MI355_SPMV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_SPMV_VERSION 310 /* 0.3.1 */
/* Additions since 310 that a caller can test for at compile time (the entry points themselves: dlsym).  The number
 * above did NOT move with them: MI355_SPMV_VERSION / mi355_spmv_version() alone do not tell a library that has the
 * pattern entry points from one that has not — test this macro, or look the symbols up.                          */
#define MI355_SPMV_HAS_PATTERN 1 /* MI355_VAL_PATTERN, mi355_spmv_merge_pattern_*, mi355_spmv_plan_get_mat_type */
#define MI355_SPMV_HAS_MULTI 1   /* mi355_spmv_multi_*: Y = A X for k vectors in one pass over A */
#define MI355_SPMV_HAS_MULTI_SEMIRING 1 /* mi355_spmv_multi_create_typed / _set_semiring / _get_types / _genl_* / _pattern_* */
#define MI355_SPMV_HAS_MULTI_HALF 1 /* mi355_spmv_multi_create_half / _half_*: X and Y in binary16 / bfloat16, fp32 arithmetic */
#define MI355_SPMV_HAS_MULTI_TRANSPOSED 1 /* mi355_spmv_csr_transpose, mi355_spmv_multi_create_permuted / _create_transposed / _transposed_* */
#define MI355_SPMV_HAS_SDDMM 1 /* mi355_spmv_sddmm_*: dot(U[r], V[c]) at every stored entry (r, c) of A in one pass over A */
#define MI355_SPMV_HAS_SDDMM_HALF 1 /* mi355_spmv_sddmm_create_half / _get_types / _half_*: U and V in binary16 / bfloat16, fp32 Ax and out */
#define MI355_SPMV_HAS_ROW_SOFTMAX 1 /* mi355_spmv_row_softmax_*: softmax over the stored entries of every row (edge softmax), and its gradient */
#define MI355_SPMV_HAS_ATTENTION 1 /* mi355_spmv_attention_*: O = softmax(scale Q K^T + bias, on the stored entries of A) V in one pass over A */
#define MI355_SPMV_HAS_ATTENTION_HALF 1 /* mi355_spmv_attention_create_half / _get_types / _half_*: Q, K, V and O in binary16 / bfloat16, fp32 bias, lse and arithmetic */
#define MI355_SPMV_HAS_ATTENTION_BACKWARD 1 /* mi355_spmv_attention_bwd_*: dQ, dK, dV (and dbias) of fused sparse attention from O, dO and lse, nothing of nnz size kept */
#define MI355_SPMV_HAS_ATTENTION_HEADS 1 /* mi355_spmv_attention[_bwd]_reserve_heads / _get_heads_max / _execute_heads: the heads of sparse attention, forward and backward, in one call */
#define MI355_SPMV_HAS_ATTENTION_BACKWARD_HALF 1 /* mi355_spmv_attention_bwd_create_half / _get_types / _half_*: the eight matrices in binary16 / bfloat16, fp32 bias, lse, dbias and arithmetic */
#define MI355_SPMV_HAS_HALF_MATRIX 1 /* MI355_VAL_F16 / MI355_VAL_BF16 as a mat_type (VECTOR), mi355_spmv_narrow_values */

/* status codes */
enum {
    MI355_SPMV_OK = 0,
    MI355_SPMV_EINVAL = 1,  /* bad size / null pointer / unknown enum          */
    MI355_SPMV_ENOTSUP = 2, /* type combination or kind not built              */
    MI355_SPMV_EHIP = 3,    /* a HIP runtime call failed (see _last_error)     */
    MI355_SPMV_ENOMEM = 4,  /* scratch allocation failed                       */
    MI355_SPMV_ENODEV = 5   /* no gfx950 device visible                        */
};

/* kinds — the three hot variants of the reference, rebuilt for wave64:
 *   VECTOR  CSR-vector, per-row sub-wave reduction
 *           (replaces SpMV_cusp_warp_reduce, include/spmv/cusp/cusp_warp_reduce.cuh:138-147)
 *   MERGE   merge-path load-balanced SpMV: search -> tile -> fix-up
 *           (replaces SpMV_merge_based / SpMV_merge_based_generalized,
 *            include/spmv/merge_based/merge_based.cuh:22-56,
 *            include/spmv/merge_genl/merge_genl.cuh:41-79)
 *   LIGHT   dynamic row distribution from global atomic row counters
 *           (replaces SpMV_light_vector / SpMV_light_warp,
 *            include/spmv/LightSpMV.cuh:379-416)                              */
enum { MI355_KIND_VECTOR = 0, MI355_KIND_MERGE = 1, MI355_KIND_LIGHT = 2, MI355_KIND_COUNT = 3,
       /* plan_create / plan_acquire / the mi355_spmv_auto_* one-shots / dist_create_local only: the library picks.  The
        * reference leaves the choice of kind to the command line (main.cu:26-30); a caller that has no opinion gets
        * MERGE when the row lengths are skewed (the heaviest run of rows a workgroup would take holds more than twice
        * the mean: power-law matrices, where merge-path is ahead of the row kinds on every measured config) and for
        * integer values, VECTOR otherwise.  A heuristic on structure, not a measurement (bench.py measures);
        * plan_get_info().kind reports what was picked.                                                            */
       MI355_KIND_AUTO = 100 };
enum { MI355_OFF_I32 = 0, MI355_OFF_I64 = 1 };
enum { MI355_VAL_F32 = 0, MI355_VAL_F64 = 1,
       /* 32-bit integers: the MERGE kind only (every semiring; two's-complement wrap-around, exact whatever the
        * reduction order).  The reference's generalized merge kind is a template over the value types and its
        * functor (merge_genl.cuh:19-38, :134-150); this is the integer / boolean instance of it.  VECTOR / LIGHT
        * plans and alpha / beta return MI355_SPMV_ENOTSUP for it.                                              */
       MI355_VAL_I32 = 2,
       /* A PATTERN matrix: no stored values, every entry is one in the type of x and y (a Matrix Market `pattern`
        * file, an unweighted graph).  Valid ONLY as the mat_type of mi355_spmv_plan_create_typed, MERGE kind: as
        * x_type / y_type and as the val_type of every other entry point it is an error.                        */
       MI355_VAL_PATTERN = 3,
       /* Matrix values stored in 16 bits — IEEE binary16, or bfloat16 (the upper half of an fp32) — under fp32 x and
        * y: every value is widened exactly as it meets x, products and sums are fp32.  Valid ONLY as the mat_type of
        * mi355_spmv_plan_create_typed, VECTOR kind, x_type = y_type = F32: as x_type / y_type and as the val_type of
        * every other entry point they are MI355_SPMV_EINVAL.  mi355_spmv_narrow_values makes such values.        */
       MI355_VAL_F16 = 4, MI355_VAL_BF16 = 5 };

/* semirings of the generalized merge kind.  The reference's
 * SpMV_merge_based_generalized takes a functor_t with initialize / combine / reduce
 * (include/spmv/merge_genl/merge_genl.cuh:19-38; CPU twin include/spmv/cpu_navie.hpp:20-34)
 * and ships (+, *); a C ABI cannot take a C++ functor: the tuned kernels enumerate these (any OTHER functor, and any
 * mix of the five types, goes through mi355_spmv_functor_* below — its text compiled at run time):
 *   PLUS_TIMES  y[r] = sum_k  Ax[k] * x[Aj[k]]           (identity 0)      — every other entry point
 *   MIN_PLUS    y[r] = min_k (Ax[k] + x[Aj[k]])          (identity +inf; INT32_MAX for integers) — shortest-path relaxation
 *   MAX_TIMES   y[r] = max_k (Ax[k] * x[Aj[k]])          (identity -inf)   — widest / most reliable path
 *   MAX_PLUS    y[r] = max_k (Ax[k] + x[Aj[k]])          (identity -inf)   — longest path, Viterbi
 *   OR_AND      y[r] = OR_k (Ax[k] != 0 AND x[Aj[k]] != 0) as 1.0 / 0.0  (identity 0)
 *                                                                         — boolean SpMV: one BFS / reachability step */
enum { MI355_SEMIRING_PLUS_TIMES = 0, MI355_SEMIRING_MIN_PLUS = 1, MI355_SEMIRING_MAX_TIMES = 2,
       MI355_SEMIRING_MAX_PLUS = 3, MI355_SEMIRING_OR_AND = 4, MI355_SEMIRING_COUNT = 5 };

/* plan flags */
enum {
    MI355_PLAN_DEFAULT = 0,
    /* Keep results that depend only on Ap (merge-path tile coordinates) across
     * executes instead of recomputing them every call.  Valid while the caller
     * leaves Ap unchanged.  Off by default: every execute runs every kernel of
     * the kind.                                                                */
    MI355_PLAN_REUSE_STRUCTURE = 1,
    /* What a default plan holds: scratch memory, launch shapes, and — a VECTOR plan
     * of a banded matrix — a PACKED INDEX: one 16-bit number per nonzero, the
     * column's position inside the LDS window of x that its chunk of rows stages
     * (0xFFFF: outside it).  The banded kernel streams that instead of Aj, i.e. 2
     * instead of 4 bytes per nonzero of index on every execute (the S32-band
     * target reads 0.76 of the bytes).  Cost: 2 bytes per nonzero of device memory
     * for the life of the plan and one extra pass over Aj at create.  It is built
     * when the plan runs csr_vector_window_kernel with one window of at most
     * 65 535 elements placed from the band the structure probe saw, equal-row
     * chunks, and Aj is 16-byte aligned; if the memory cannot
     * be had the plan is created without it.  plan_info reports its size.  It IS
     * derived from the contents of Aj — which a plan's caller may not change
     * anyway (see create below).
     * With this flag the plan holds nothing derived from the contents of Aj.  The
     * one-shot entry points and plan_acquire always set it: their plans are found
     * again by pointer and stay right for arrays rewritten in place.
     * MI355_SPMV_PACK=0 in the environment has the same effect on every plan.   */
    MI355_PLAN_NO_INDEX_COPY = 2
};

/* ---- one-shot entry points -------------------------------------------------
 * Same 8 arguments as the reference's SpMV_<kind> (include/spmv.h:29-34) plus a
 * hipStream_t (NULL = the null stream, which is what the reference launches on).
 * Allocates its scratch, runs, synchronises the stream, frees the scratch — the
 * per-call life cycle of the reference kinds (LightSpMV.cuh:274-276, :314;
 * merge_based.cuh:34-56).  Returns a status code.                              */
#define MI355_SPMV_DECLARE(KIND, SUF, OFF, VAL)                                          \
    int mi355_spmv_##KIND##_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, \
                                  const int32_t* Aj, const VAL* Ax, const VAL* x, VAL* y, \
                                  void* stream);
#define MI355_SPMV_DECLARE_KIND(KIND)                 \
    MI355_SPMV_DECLARE(KIND, i32_f32, int32_t, float)  \
    MI355_SPMV_DECLARE(KIND, i32_f64, int32_t, double) \
    MI355_SPMV_DECLARE(KIND, i64_f32, int64_t, float)  \
    MI355_SPMV_DECLARE(KIND, i64_f64, int64_t, double)

MI355_SPMV_DECLARE_KIND(vector) /* replaces SpMV_cusp_warp_reduce  cusp_warp_reduce.cuh:138 */
MI355_SPMV_DECLARE_KIND(merge)  /* replaces SpMV_merge_based[_generalized] merge_based.cuh:22, merge_genl.cuh:41 */
MI355_SPMV_DECLARE_KIND(light)  /* replaces SpMV_light_vector/_warp  LightSpMV.cuh:379, :400 */
MI355_SPMV_DECLARE_KIND(auto)   /* MI355_KIND_AUTO: one of the three, picked from the structure */

/* generalized merge-path SpMV: the reference's SpMV_merge_based_generalized
 * (include/spmv/merge_genl/merge_genl.cuh:41-79) with the semiring as an argument.  */
#define MI355_SPMV_DECLARE_GENL(SUF, OFF, VAL)                                                  \
    int mi355_spmv_merge_genl_##SUF(int semiring, int32_t n_rows, int32_t n_cols, OFF nnz,      \
                                    const OFF* Ap, const int32_t* Aj, const VAL* Ax,            \
                                    const VAL* x, VAL* y, void* stream);
MI355_SPMV_DECLARE_GENL(i32_f32, int32_t, float)
MI355_SPMV_DECLARE_GENL(i32_f64, int32_t, double)
MI355_SPMV_DECLARE_GENL(i64_f32, int64_t, float)
MI355_SPMV_DECLARE_GENL(i64_f64, int64_t, double)
MI355_SPMV_DECLARE_GENL(i32_i32, int32_t, int32_t)   /* integer values: identities 0 / INT32_MAX / INT32_MIN, OR_AND as 1 / 0 */
MI355_SPMV_DECLARE_GENL(i64_i32, int64_t, int32_t)

/* ---- plan entry points -----------------------------------------------------
 * The reference re-creates scratch on every call (quirks 7-9 of SURVEY.md §2c);
 * a plan keeps scratch and launch shapes across the timing loop of main.cu:102-113.
 * create: sizes + structure pointers (Ap/Aj are retained, not copied, and must
 *         outlive the plan; their CONTENTS are read here — a structure probe,
 *         for VECTOR / LIGHT the chunk boundaries, and for a banded VECTOR plan
 *         one pass over all of Aj that builds its packed index (plan flags above;
 *         not with MI355_PLAN_NO_INDEX_COPY) — so they must already be valid
 *         and must not change while the plan lives: executes of a plan with a
 *         packed index read the columns from that copy).  Synchronises the device.
 * execute: asynchronous on `stream`, no host sync, no allocation, kernels only
 *         (hipGraph-capturable: tests/test_gpu_parity.py).  A plan serves ONE
 *         stream at a time (its scratch — merge coordinates and carries, the LIGHT
 *         counters — belongs to the execute in flight); concurrent executes need
 *         one plan each.
 * destroy: frees scratch and the packed index (hipFree: waits for the device). */
typedef struct mi355_spmv_plan mi355_spmv_plan;

int mi355_spmv_plan_create(mi355_spmv_plan** plan, int kind, int off_type, int val_type,
                           int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                           const int32_t* Aj, int flags);
/* The reference's operator has separate matrix / x / y value types (include/spmv.h:29-34; its generalized merge
 * kind computes in the y type, merge_genl.cuh:29-31).  Built here: all three equal (every kind), and an fp32
 * MATRIX under fp64 x and y for the MERGE kind — values are widened as they meet x, products and sums are fp64
 * (the mixed-precision case that halves the matrix stream).  Other combinations return MI355_SPMV_ENOTSUP.
 * execute then takes Ax as float*, x / y as double*.                                                         */
/* mat_type = MI355_VAL_PATTERN, x_type = y_type = F32 / F64 / I32, kind MERGE (AUTO becomes MERGE; VECTOR / LIGHT return
 * MI355_SPMV_ENOTSUP): the matrix has a structure and no values.  The plan is shaped exactly as the valued MERGE plan
 * of that vector type (same tiles and runs, same window of x); its executes always walk the tiles (merge_tile_kernel)
 * with every product combine(1, x[col]), and IGNORE Ax: it may be NULL, and no kernel reads or forms an address from
 * it.  4 bytes per nonzero cross HBM instead of 8 (fp32) or 12 (fp64), and Ax need not exist.  All five semirings;
 * alpha / beta under (+, *) for the float types.  The sums are those of the valued plan executed with Ax = ones, bit
 * for bit, whenever that plan walks its tiles too.                                                                   */
/* mat_type = MI355_VAL_F16 / MI355_VAL_BF16, x_type = y_type = F32, kind VECTOR (AUTO becomes VECTOR; MERGE / LIGHT and
 * any other x / y type return MI355_SPMV_ENOTSUP): execute takes Ax as 16-bit values (8-byte aligned for the fast
 * path), x / y as float*.  The plan is shaped exactly as the fp32 VECTOR plan of the same structure and flags
 * (plan_get_shape is byte-identical; plan_get_info().val_type stays F32, plan_get_mat_type says 4 / 5), so a banded
 * matrix streams 2 + 2 bytes per nonzero with the packed index and 4 + 2 with MI355_PLAN_NO_INDEX_COPY, where fp32
 * streams 2 + 4 and 4 + 4; a row's products are added in the fp32 plan's order, so y equals the fp32 plan's y on the
 * widened values bit for bit.  That fast path covers equal-row chunks with one window of x or none.  Weight-cut
 * chunks, several bands, the swept window, giant rows and small matrices run the plain one-pass kernel instead
 * (plan_get_info then says main_kernel = "csr_vector_kernel", window_elems = 0, n_kernels = 1), as does an execute
 * whose Ax is not 8-byte aligned or whose Aj / x are not 16-byte aligned.  alpha / beta work; set_semiring stays
 * ENOTSUP as for every VECTOR plan; no one-shot entry points, no row blocks, no dist_*.                              */
int mi355_spmv_plan_create_typed(mi355_spmv_plan** plan, int kind, int off_type, int mat_type, int x_type,
                                 int y_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                                 const int32_t* Aj, int flags);
/* The mat_type a plan was created with (= its val_type unless plan_create_typed said otherwise).                    */
int mi355_spmv_plan_get_mat_type(const mi355_spmv_plan* plan, int* mat_type);
/* dst[i] = src[i] rounded to dst_type (MI355_VAL_F16 / MI355_VAL_BF16; anything else: MI355_SPMV_EINVAL), i < n, device
 * pointers: round to nearest even, overflow to +-inf, NaN stays NaN, subnormals kept.  Asynchronous on `stream`.    */
int mi355_spmv_narrow_values(int dst_type, int64_t n, const float* src, void* dst, void* stream);
/* One-shot SpMV with a pattern matrix: the arguments of mi355_spmv_merge_genl_* without Ax.  A plan per call.       */
int mi355_spmv_merge_pattern_i32_f32(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap,
                                    const int32_t* Aj, const float* x, float* y, void* stream);
int mi355_spmv_merge_pattern_i32_f64(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap,
                                    const int32_t* Aj, const double* x, double* y, void* stream);
int mi355_spmv_merge_pattern_i32_i32(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap,
                                    const int32_t* Aj, const int32_t* x, int32_t* y, void* stream);
int mi355_spmv_merge_pattern_i64_f32(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap,
                                    const int32_t* Aj, const float* x, float* y, void* stream);
int mi355_spmv_merge_pattern_i64_f64(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap,
                                    const int32_t* Aj, const double* x, double* y, void* stream);
int mi355_spmv_merge_pattern_i64_i32(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap,
                                    const int32_t* Aj, const int32_t* x, int32_t* y, void* stream);
int mi355_spmv_merge_f32mat_f64vec_i32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap,
                                       const int32_t* Aj, const float* Ax, const double* x, double* y, void* stream);
int mi355_spmv_merge_f32mat_f64vec_i64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap,
                                       const int32_t* Aj, const float* Ax, const double* x, double* y, void* stream);
int mi355_spmv_plan_execute(mi355_spmv_plan* plan, const void* Ax, const void* x, void* y,
                            void* stream);
int mi355_spmv_plan_destroy(mi355_spmv_plan* plan);
/* y = alpha * A x + beta * y for the following executes (any kind, (+, *) semiring; default 1, 0:
 * y overwritten).  SURVEY §8(f)-4: the reference's cuSPARSE kind passes alpha = 1, beta = 0
 * (include/spmv/cusparse.cuh:42-43) and its vendored CUB carries the same two scalars, disabled
 * (merge_based/agent_spmv_orig.cuh:425-433, dispatch_spmv_orig.cuh:802).  y is read only when beta != 0. */
int mi355_spmv_plan_set_alpha_beta(mi355_spmv_plan* plan, double alpha, double beta);
/* MERGE plans only (ENOTSUP otherwise): choose the semiring of the following executes.  */
int mi355_spmv_plan_set_semiring(mi355_spmv_plan* plan, int semiring);
/* Block the host until `stream` has drained (hipStreamSynchronize), so that a
 * host-only C++ caller can bracket Timer::kernel_stop() the way the reference's
 * kinds do with cudaDeviceSynchronize() (cusp_warp_reduce.cuh:131) without
 * including HIP headers.                                                        */
int mi355_spmv_stream_synchronize(void* stream);

/* Launch shape chosen by the plan (for reports and tests).                     */
typedef struct mi355_spmv_plan_info {
    int32_t kind, off_type, val_type;
    int32_t lanes_per_row;    /* T: sub-wave width (VECTOR, LIGHT); 0 for MERGE    */
    int32_t elems_per_lane;   /* nonzeros one lane loads per step (4 = 16-B loads) */
    int32_t block_threads;
    int64_t grid_blocks;      /* blocks of the main kernel                         */
    int64_t tile_items;       /* MERGE: merge items per tile                       */
    int64_t n_tiles;          /* MERGE: tiles; LIGHT: row chunks                   */
    int64_t rows_per_chunk;   /* LIGHT: rows per dequeue                           */
    int64_t scratch_bytes;    /* device memory held by the plan: scratch + packed index */
    int32_t n_kernels;        /* kernels launched per execute                      */
    int32_t window_elems;     /* elements of x staged through LDS per workgroup (0 = none) */
    int32_t window_segments;  /* 1 = one window; 2..4 = that many column bands staged side by side */
    char main_kernel[64];     /* substring of the dominant kernel's symbol name    */
    int32_t balanced_chunks;  /* VECTOR, LIGHT: 1 = row chunks cut by weight (nonzeros + mean row length per
                                 row) because equal-row chunks were uneven, 0 = equal-row chunks           */
    int32_t rows_cap;         /* VECTOR, LIGHT: most rows a chunk can hold                                 */
    int64_t n_chunks;         /* VECTOR, LIGHT: row chunks                                                 */
    char knobs[160];          /* the MI355_* tuning variables that were set when the plan was created, "NAME=value ..." */
    int64_t packed_index_bytes;   /* VECTOR: bytes of the plan's packed index (2 per nonzero + padding); 0 = the plan reads Aj */
    int64_t packed_index_escapes; /* ... and how many nonzeros lie outside their chunk's window (their columns are read from Aj) */
} mi355_spmv_plan_info;
int mi355_spmv_plan_get_info(const mi355_spmv_plan* plan, mi355_spmv_plan_info* info);

/* ---- row-block plans --------------------------------------------------------
 * rows are independent, so a matrix is cut into contiguous row blocks (one or more per GPU)
 * and each block is an ordinary CSR SpMV.  For the concatenated y to equal the one-GPU y BIT FOR BIT with
 * the row-local kinds (VECTOR, LIGHT), a block must sum every row exactly as the whole matrix's plan does:
 * same lanes per row, same workgroup size, same chunks (hence the same per-chunk vector width and the same
 * window of x), same long-row and giant-row treatment, same 16-byte phase of every row start.  So:
 *   mi355_spmv_plan_get_shape   the launch-shape decisions of a plan, as plain data (can be sent to other
 *                               processes);
 *   mi355_spmv_plan_partition   nnz-balanced cut points that fall on the plan's chunk boundaries;
 *   mi355_spmv_plan_create_block  a plan for rows [row_begin, row_begin + n_rows) of that matrix which inherits
 *                               the shape.  Its arrays are a 16-byte-aligned VIEW of the whole CSR:
 *                               Aj / Ax start at element (Ap_whole[row_begin] & ~3) and Ap[i] =
 *                               Ap_whole[row_begin + i] - (Ap_whole[row_begin] & ~3), so Ap[0] is 0..3 (the
 *                               "phase") and nnz is the END offset Ap[n_rows].  No copy of Aj / Ax is needed on
 *                               the device that holds the whole matrix.  Unless the block ends where the whole
 *                               matrix ends, Aj / Ax must be READABLE up to the next multiple of 4 elements
 *                               past nnz (a view of the whole arrays is; a copy is padded): the tail of the
 *                               block's last row is then read in whole 16-byte groups, as the whole plan does.
 * MERGE blocks take the same arrays but are shaped on their own (tile boundaries move with the cut anyway;
 * results stay inside the parity bound); shape may then be NULL.                              */
typedef struct mi355_spmv_plan_shape {
    int32_t struct_bytes;             /* sizeof(mi355_spmv_plan_shape) of the library that filled it */
    int32_t kind, off_type, val_type;
    int32_t n_rows, n_cols;           /* the whole matrix */
    int64_t nnz;
    int32_t lanes_per_row, elems_per_lane, block_threads;
    int32_t balanced_chunks, rows_cap, giant_rows_enabled;
    int64_t rows_per_chunk, n_chunks, bal_k, bal_q, giant_len;
    int32_t window_elems, window_bytes, window_from_band, window_segments, probe_ok, long_steps;
    int64_t band_lo, band_hi, seg_lo[4], seg_hi[4];
    int32_t window_sweep;             /* 1 = the band is wider than any window: one group of rows per chunk, the window sweeps it */
    int32_t small_plain;              /* 1 = VECTOR / LIGHT on a small matrix: the plain one-pass kernel (lanes_per_row lanes, 4-byte loads) */
} mi355_spmv_plan_shape;
int mi355_spmv_plan_get_shape(const mi355_spmv_plan* plan, mi355_spmv_plan_shape* shape);
/* parts + 1 entries each: row_cuts[p] = first row of block p, chunk_cuts[p] = its first chunk in the plan's
 * numbering (0 for MERGE), nnz_cuts[p] = Ap[row_cuts[p]].  Cuts are multiples of 4 rows (or n_rows), chosen so
 * that nnz_cuts[p] ~ p * nnz / parts.  Reads Ap on the device (synchronises).                              */
int mi355_spmv_plan_partition(const mi355_spmv_plan* plan, int parts, int64_t* row_cuts, int64_t* chunk_cuts,
                              int64_t* nnz_cuts);
int mi355_spmv_plan_create_block(mi355_spmv_plan** plan, int kind, int off_type, int val_type,
                                 const mi355_spmv_plan_shape* whole, int64_t row_begin, int64_t chunk_begin,
                                 int64_t n_chunks, int64_t nnz_begin_whole,
                                 int32_t n_rows, int32_t n_cols, int64_t nnz_end, const void* Ap,
                                 const int32_t* Aj, int flags);

/* ---- multi-GPU: row blocks, x replicated, allgatherv(y) over RCCL/xGMI -------------------------------
 * The reference is single-device (main.cu:53, common.cuh:8); the north star adds one node of 8 GPUs:
 * contiguous nnz-balanced row blocks, x replicated, the y slices concatenated on every GPU.  RCCL has no
 * allgatherv: block p is broadcast from its owner into its displacement of every GPU's y (grouped
 * ncclBroadcast calls on a dedicated stream).  Each GPU's rows are cut into `sub_blocks` blocks so that the
 * slice of block s travels while block s + 1 is being computed.  RCCL (librccl.so.1) is loaded on first use,
 * and only when more than one GPU takes part: libmi355spmv.so itself links the HIP runtime only.
 *
 * LOCAL mode — one process drives all the GPUs (the reference's single-threaded harness, `--ngpu N`):
 *   create_local   Ap / Aj of the WHOLE matrix on the current device ("home"); blocks are dealt to
 *                  `devices` in order (parts = n_devices * sub_blocks); remote blocks get copies of
 *                  their slice of Ap / Aj, the home device's blocks are views.
 *   scatter_values / replicate_x   refresh the remote copies of Ax / x from home-device arrays
 *   execute(d, Ax, x, y, stream)   Ax / x / y on the home device; Ax or x may be NULL = "unchanged since the
 *                  last scatter / replicate"; non-NULL pointers are scattered / replicated first (the drop-in
 *                  semantics of SpMV(kind, ...), which hands over home-device arrays on every call).  y (n_rows)
 *                  receives the full result on the home device; every other GPU holds it too (device_y).
 * RANK mode — one process per GPU (torch.distributed / MPI style launch):
 *   unique_id      128 bytes made by ONE rank, distributed by the caller's own means
 *   create_rank    this rank's blocks (parts_per_rank consecutive blocks of the global cut list), its slice
 *                  of the structure; `whole` = the shape of the whole matrix's plan when bitwise identity
 *                  with a one-GPU run is wanted (NULL: every block is shaped on its own)
 *   execute(d, Ax, x, y, stream)   Ax = this rank's values (view described above), x = this GPU's copy of
 *                  x, y = this GPU's full-length y.
 * With one GPU (n_devices == 1 / world == 1) no communicator is made and execute is the blocks' plain
 * executes on the caller's stream.
 * STATUS: world > 1 is EXPERIMENTAL — it has run only against an emulation of RCCL (several "GPUs" on one device,
 * tests/cpp/fake_rccl.cpp): schedule, counts, displacements and stream order are tested, RCCL itself and xGMI are not. */
typedef struct mi355_spmv_dist mi355_spmv_dist;
int mi355_spmv_dist_create_local(mi355_spmv_dist** dist, int kind, int off_type, int val_type,
                                 int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                                 const int32_t* Aj, int n_devices, const int* devices, int sub_blocks,
                                 int flags);
int mi355_spmv_dist_unique_id(void* id128);
int mi355_spmv_dist_create_rank(mi355_spmv_dist** dist, int kind, int off_type, int val_type,
                                int rank, int world, const void* id128, int parts_per_rank,
                                const int64_t* row_cuts, const int64_t* chunk_cuts, const int64_t* nnz_cuts,
                                const mi355_spmv_plan_shape* whole, int32_t n_cols,
                                int32_t n_rows_local, int64_t nnz_end_local, const void* Ap_local,
                                const int32_t* Aj_local, int flags);
int mi355_spmv_dist_scatter_values(mi355_spmv_dist* dist, const void* Ax, void* stream);
int mi355_spmv_dist_replicate_x(mi355_spmv_dist* dist, const void* x, void* stream);
int mi355_spmv_dist_execute(mi355_spmv_dist* dist, const void* Ax, const void* x, void* y, void* stream);
/* The same with flags, so that a scaling report can tell compute from exchange (north star: "1/2/4/8-GPU GFLOP/s and
 * bandwidth-fraction scaling reported"; SURVEY §8(e): "report compute-only and end-to-end scaling"):
 *   MI355_DIST_EXEC_SKIP_EXCHANGE   the blocks' kernels with the whole stream choreography, no RCCL call: afterwards
 *                                   every GPU holds ITS rows of y only;
 *   MI355_DIST_EXEC_EXCHANGE_ONLY   no kernel: the allgatherv of whatever y holds.
 * Collective like execute: every rank / GPU passes the same flags.                                                   */
enum { MI355_DIST_EXEC_DEFAULT = 0, MI355_DIST_EXEC_SKIP_EXCHANGE = 1, MI355_DIST_EXEC_EXCHANGE_ONLY = 2 };
int mi355_spmv_dist_execute_ex(mi355_spmv_dist* dist, const void* Ax, const void* x, void* y, void* stream,
                               int exec_flags);
/* How the y slices travel.  RCCL has no allgatherv (SURVEY §5 last row names three ways to make one); all three are
 * built behind this one API, per sub-block s, on the communication stream:
 *   BCAST      one group of in-place ncclBroadcast, root = owner of block (root, s): a ring per root;
 *   SENDRECV   one group of ncclSend / ncclRecv, every GPU sends its block to every peer and receives theirs:
 *              point to point, all xGMI links at once;
 *   ALLGATHER  one ncclAllGather: in place in y when the blocks of sub-block s are equal and adjacent (one block per
 *              GPU on a uniform matrix), else through a staging buffer padded to the largest block (one pack and
 *              one unpack kernel around it).
 * AUTO (default, or MI355_DIST_EXCHANGE=auto): when more than one GPU takes part, create times MI355_DIST_TRIALS (5)
 * exchanges of each on scratch buffers, agrees on the maximum over ranks (ncclAllReduce) and keeps the fastest;
 * dist_get_info reports the choice and the trial times.  set_exchange changes it later (collective: every rank the
 * same value, no execute in flight).                                                                               */
enum { MI355_DIST_EXCHANGE_AUTO = 0, MI355_DIST_EXCHANGE_BCAST = 1, MI355_DIST_EXCHANGE_SENDRECV = 2,
       MI355_DIST_EXCHANGE_ALLGATHER = 3, MI355_DIST_EXCHANGE_COUNT = 4 };
int mi355_spmv_dist_set_exchange(mi355_spmv_dist* dist, int exchange);
typedef struct mi355_spmv_dist_info {
    int32_t world, rank, sub_blocks, local_mode;
    int32_t exchange;          /* MI355_DIST_EXCHANGE_* in use (never AUTO; BCAST when world == 1: unused)        */
    int32_t auto_picked;       /* 1 = chosen by the timed trial at create                                        */
    int32_t allgather_in_place;/* 1 = every sub-block's ALLGATHER goes straight into y (no staging)              */
    int32_t reserved0;
    float trial_us[MI355_DIST_EXCHANGE_COUNT];   /* per exchange of all sub-blocks, max over ranks; 0 = not timed */
    int64_t max_block_rows;    /* largest block (the padded count of ALLGATHER)                                  */
    int64_t staging_bytes;     /* per GPU, ALLGATHER through staging                                             */
    char exchange_name[16];
} mi355_spmv_dist_info;
int mi355_spmv_dist_get_info(const mi355_spmv_dist* dist, mi355_spmv_dist_info* info);
/* A dist handle holds COPIES of the structure (a rebased Ap per block; Aj on the other GPUs), so unlike the one-shot
 * plan cache it is wrong for a matrix rewritten in place.  For callers with the reference's semantics — SpMV(kind,
 * ...) reads its arrays on every call — this compares a fingerprint of the caller's Ap (every offset) and Aj (a
 * strided sample of 64 K entries) with the one taken at create: one small kernel and one 16-byte read-back
 * (synchronises `stream`).  LOCAL mode only.  *changed = 1: destroy the handle and create it again.             */
int mi355_spmv_dist_structure_changed(mi355_spmv_dist* dist, const void* Ap, const int32_t* Aj, void* stream,
                                      int* changed);
int mi355_spmv_dist_set_alpha_beta(mi355_spmv_dist* dist, double alpha, double beta);
/* number of blocks, and the global cut rows (parts + 1 entries)                */
int mi355_spmv_dist_parts(const mi355_spmv_dist* dist);
int mi355_spmv_dist_cuts(const mi355_spmv_dist* dist, int64_t* row_cuts);
/* launch shape of this process's block `part` (0 .. devices_of_this_process * sub_blocks - 1)             */
int mi355_spmv_dist_part_info(const mi355_spmv_dist* dist, int part, mi355_spmv_plan_info* info);
/* LOCAL mode: GPU `device_index`'s (position in `devices`) copies of y / x      */
void* mi355_spmv_dist_device_y(mi355_spmv_dist* dist, int device_index);
void* mi355_spmv_dist_device_x(mi355_spmv_dist* dist, int device_index);
int mi355_spmv_dist_destroy(mi355_spmv_dist* dist);

/* Re-read the MI355_* tuning variables from the environment (they are otherwise parsed once per process;
 * plans keep the values they were created under and report the non-default ones in plan_info.knobs). */
int mi355_spmv_knobs_reload(void);

/* The one-shot entry points keep their last few plans, found again by the pointers and sizes of Ap / Aj, the types, the
 * kind and the device (the reference's harness calls a kind 2 000 times in a row on one matrix, main.cu:102-113; plan
 * creation is a third of such a call on the target).  Safe if the arrays were rewritten in place: a kept plan holds
 * launch-shape decisions only (it is created with MI355_PLAN_NO_INDEX_COPY, so it has no packed index; plans with giant
 * rows, whose row list is structure, are never kept).
 * MI355_SPMV_PLAN_CACHE=0 disables it; this call destroys the kept plans and frees their scratch.                  */
int mi355_spmv_cache_release(void);
/* The same for a caller that wants its own timer between the steps (the C++ mirror of the reference boundary,
 * host/spmv/mi355.hpp): acquire = a kept plan for this matrix or a new one (MI355_PLAN_NO_INDEX_COPY); release = hand it back after the
 * stream it ran on has been synchronised (executed_ok = 0 after a failed execute: the plan is destroyed).  A plan whose
 * semiring was changed is handed back with it (the next acquirer sets its own); alpha / beta other than 1 / 0 are not kept. */
int mi355_spmv_plan_acquire(mi355_spmv_plan** plan, int kind, int off_type, int val_type, int32_t n_rows,
                            int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj);
int mi355_spmv_plan_release(mi355_spmv_plan* plan, int executed_ok);

/* MERGE only, for parity tests: copy the tile start coordinates the search
 * kernel produced by the last execute to HOST arrays of n_tiles+1 entries
 * (synchronises).  Integers: compared bit-exactly with the oracle's restatement
 * of thread_search.cuh:15-49.                                                  */
int mi355_spmv_plan_merge_coords(mi355_spmv_plan* plan, int64_t* tile_row, int64_t* tile_nnz);

/* ---- COO -> CSR on the device --------------------------------------------------
 * The result of the reference's ToCsr (include/load.hpp:420-474), bit for bit: Ap[r] = number of entries whose row
 * is below r; inside a row the entries keep their input order; duplicates are kept; columns are not sorted.  The
 * order is the input's, never that of atomics: two calls give identical outputs.
 *   rows, cols    nnz device int32 indices (any order: file order, an edge list, ...)
 *   vals          nnz device values of val_type (F32, F64 or I32: only the element size matters), or NULL
 *   Ap            n_rows + 1 device offsets of off_type;  Aj: nnz int32;  Ax: nnz values, NULL exactly when vals is
 *   perm          NULL, or nnz int64: perm[k] = the source index of CSR slot k (re-value later: Ax = vals[perm])
 *   workspace     NULL: *workspace_bytes = the bytes needed, return OK (touches no device, needs no GPU);
 *                 otherwise device memory of *workspace_bytes >= that many bytes; the call allocates nothing
 * Sizes follow plan_create: with MI355_OFF_I32 nnz <= INT32_MAX (else EINVAL).  nnz >= 2^32 returns
 * MI355_SPMV_ENOTSUP (the sort carries 32-bit source indices).  n_rows == 0 and nnz == 0 writes Ap = [0].
 * Every entry is checked first: a row outside [0, n_rows) or a column outside [0, n_cols) returns MI355_SPMV_EINVAL,
 * mi355_spmv_last_error() names the first such entry (index, row, col), and no output is written.
 * The work is enqueued on `stream`, which is then synchronised once (to read the check's result); nothing is kept
 * between calls.  Kernels and traffic: DESIGN.md §3.7.                                                               */
int mi355_spmv_coo_to_csr(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                          const int32_t* rows, const int32_t* cols, const void* vals,
                          void* Ap, int32_t* Aj, void* Ax, int64_t* perm,
                          void* workspace, size_t* workspace_bytes, void* stream);

/* The same for the STORED entries of a `symmetric` Matrix Market file (the lower or upper triangle, as the file lists
 * them): the outputs equal, bit for bit, ToCsr of the COO that the reference's LoadCoo makes of such a file
 * (include/load.hpp:362-403): for stored entry i in order, (r, c, v), then (c, r, v) right after it if r != c — the
 * diagonal once — then the stable sort by row.  So inside a CSR row the entries keep the order of that expanded
 * sequence, duplicates are kept, columns are not sorted, and a list that holds both (i, j) and (j, i) gives four
 * entries.  The expanded COO is never built and never crosses the bus: the caller uploads the stored entries only.
 *   mi355_spmv_coo_symmetric_nnz   *nnz_expanded = nnz_stored + the number of entries with rows[i] != cols[i]: a
 *                 device reduction on `stream`, which is synchronised once; it sizes Aj / Ax / perm.
 *   rows, cols    nnz_stored device int32 indices;  vals: nnz_stored device values or NULL
 *   nnz_expanded  what Aj / Ax / perm were allocated for.  The call checks it on the device against the true count
 *                 before anything is sized by it; a mismatch returns MI355_SPMV_EINVAL, mi355_spmv_last_error()
 *                 holds both numbers, and nothing is written to Ap / Aj / Ax / perm.
 *   Ap            n_rows + 1 offsets of off_type;  Aj: nnz_expanded int32;  Ax: nnz_expanded values, NULL exactly
 *                 when vals is
 *   perm          NULL, or nnz_expanded int64: perm[k] = the index of the STORED entry behind CSR slot k.  An entry
 *                 and its mirror share one index, so Ax = vals[perm] re-values the expanded matrix from the file's
 *                 value list (rows[perm[k]] is slot k's row, or its column when slot k is a mirror).
 *   workspace     as above: NULL is the size query (no device is touched); it depends on both counts.
 * Every stored entry is checked first: row and col must BOTH be inside [0, n_rows) and inside [0, n_cols), because
 * the mirror is stored too (the loader's rule for symmetric files).  The first bad entry is named in the error, no
 * output is written, and the stream is still synchronised exactly once.
 * Sizes: with MI355_OFF_I32 nnz_expanded <= INT32_MAX (else EINVAL); nnz_expanded outside
 * [nnz_stored, 2 nnz_stored] is EINVAL; nnz_expanded >= 2^32 returns MI355_SPMV_ENOTSUP, and so does
 * nnz_stored >= 2^31: the sort's 32-bit payload carries the stored index and a mirror bit.                          */
int mi355_spmv_coo_symmetric_nnz(int64_t nnz_stored, const int32_t* rows, const int32_t* cols, void* stream,
                                 int64_t* nnz_expanded);
int mi355_spmv_coo_to_csr_symmetric(int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                    int64_t nnz_stored, int64_t nnz_expanded,
                                    const int32_t* rows, const int32_t* cols, const void* vals,
                                    void* Ap, int32_t* Aj, void* Ax, int64_t* perm,
                                    void* workspace, size_t* workspace_bytes, void* stream);

/* ---- a generalized SpMV whose functor is the CALLER'S code --------------------
 * The reference's SpMV_merge_based_generalized is a template over a functor_t with three static members
 * (include/spmv/merge_genl/merge_genl.cuh:19-38; CPU twin include/spmv/cpu_navie.hpp:20-34)
 *     y_t initialize();   y_t combine(const mat_t& nonzero, const x_t& x);   y_t reduce(const y_t& lhs, const y_t& rhs);
 * and over five independent types (include/spmv.h:29-34).  A C ABI cannot take a C++ type, but it can take its TEXT:
 *   source        C++ source that defines the functor (and any type it needs); __host__ __device__ __forceinline__
 *                 are understood, so a functor written for the reference is passed as it is (hiprtc has no
 *                 <cmath>: INFINITY and NAN are defined in front of the text)
 *   functor_type  the type to use, as written in C++: "MyFunctor", "MergeFunctor<float, float, double>"
 *   off_type      MI355_OFF_I32 / MI355_OFF_I64;  index_t is int
 *   mat_type, x_type, y_type   the three value types as C++ type names: "float", "double", "int", "long long", or a
 *                 trivially copyable struct the source defines (an (value, index) pair for an arg-max, say)
 * compile: the text is compiled for gfx950 at run time (hiprtc, bound on first use; no device needed);
 *          MI355_SPMV_EINVAL = the text did not compile, mi355_spmv_functor_compile_log() holds the compiler's output
 *          (this thread's last compile), MI355_SPMV_ENOTSUP = no libhiprtc.so on this machine.
 * spmv:    y[r] = reduce over the row of combine(Ax[k], x[Aj[k]]) starting from initialize(), every row written
 *          (an empty row gets initialize()).  Asynchronous on `stream`, no scratch, no host synchronisation.  As in the
 *          reference's device code, reduce must be associative and commutative and initialize() its identity.
 * This is the GENERAL path (T lanes per row, plain gathers of x); the five enumerated semirings of the merge kind
 * above are the tuned one.                                                                                          */
typedef struct mi355_spmv_functor mi355_spmv_functor;
int mi355_spmv_functor_compile(mi355_spmv_functor** functor, const char* source, const char* functor_type, int off_type,
                               const char* mat_type, const char* x_type, const char* y_type);
const char* mi355_spmv_functor_compile_log(void);
int mi355_spmv_functor_spmv(mi355_spmv_functor* functor, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                            const int32_t* Aj, const void* Ax, const void* x, void* y, void* stream);
int mi355_spmv_functor_destroy(mi355_spmv_functor* functor);

/* ---- multi-vector SpMV: Y = alpha * A X + beta * Y for k vectors in one pass over A ------------------------------
 * For callers with several right-hand sides (block Krylov, several loads, GNN features, PageRank batches), who would
 * otherwise call plan_execute k times and stream the matrix — and waste most of every gathered line of x — k times.
 * The reference's operator has one x and one y (include/spmv.h:29-34): this has no counterpart there.
 *   X   n_cols x k, ROW-major: X[c * ldx + j] is element c of vector j, ldx >= k
 *   Y   n_rows x k, likewise:  Y[r * ldy + j], ldy >= k;  Y[:, j] = alpha * A X[:, j] + beta * Y[:, j] for j < k
 * Elements j >= k of a row of X are never read, of a row of Y never written; with beta = 0 (the default; alpha = 1)
 * Y is never read.  Rows of X / Y are accessed 16 bytes per lane when the pointer and ld * sizeof(value) are 16-byte
 * aligned, else element by element.
 * Types: mi355_spmv_multi_create makes {I32, I64} offsets x {F32, F64} values under the (+, *) semiring and returns
 * MI355_SPMV_ENOTSUP for MI355_VAL_I32 / MI355_VAL_PATTERN; semirings, int32 values and pattern matrices come from
 * mi355_spmv_multi_create_typed below, 16-bit X and Y from mi355_spmv_multi_create_half below that.  Column-major X and
 * the dist_* entry points are not built.
 * The work is cut by NONZEROS: a wave owns a slice of slice_len merge items (row ends + nonzeros), so empty rows and
 * hub rows cost what they hold; a row that crosses slices leaves carries in scratch (sized for k_max at create), and
 * a fix-up kernel adds them in slice order — no float atomics: two executes on the same inputs give the same bits.
 * Columns are served in tiles of 4 / 8 / 16 / 32 (fp32) or 2 / 4 / 8 / 16 (fp64); another k takes the next width with
 * the surplus masked; k above the widest takes ceil(k / widest) passes over A inside the one execute.
 * Life cycle as plan_*: create may allocate and synchronise, retains Ap / Aj (not copied; it does not read them);
 * execute is asynchronous on `stream`, allocates nothing, never synchronises, launches kernels only (graph-capturable);
 * one stream at a time per object; 1 <= k <= k_max.  Argument errors are refused before any device call.         */
typedef struct mi355_spmv_multi mi355_spmv_multi;
typedef struct mi355_spmv_multi_info {
    int32_t off_type, val_type, k_max;
    int32_t slice_len;       /* merge items (row ends + nonzeros) per slice = per wave                    */
    int32_t block_threads;
    int32_t widest_tile;     /* columns of the widest tile                                                */
    int32_t passes;          /* passes over A per execute with k = k_max                                  */
    int32_t n_kernels;       /* kernels per execute with k = k_max: the passes + the fix-up               */
    int64_t n_slices;
    int64_t grid_blocks;     /* workgroups of one pass                                                    */
    int64_t scratch_bytes;   /* device memory held: the slices' carry rows and carry values for k_max     */
    char main_kernel[64];
} mi355_spmv_multi_info;
int mi355_spmv_multi_create(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                            int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max);
int mi355_spmv_multi_set_alpha_beta(mi355_spmv_multi* multi, double alpha, double beta);
int mi355_spmv_multi_execute(mi355_spmv_multi* multi, const void* Ax, const void* X, int64_t ldx,
                             void* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_get_info(const mi355_spmv_multi* multi, mi355_spmv_multi_info* info);
int mi355_spmv_multi_destroy(mi355_spmv_multi* multi);
/* One-shots: create (k_max = k), execute, synchronise the stream, destroy.  No plan is kept between calls.       */
int mi355_spmv_multi_i32_f32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
                            const float* Ax, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_i32_f64(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
                            const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_i64_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
                            const float* Ax, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_i64_f64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
                            const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);

/* ---- multi-vector SpMV over a semiring, int32 values and pattern matrices (MI355_SPMV_HAS_MULTI_SEMIRING) ----------
 * For callers with k vectors and a graph: multi-source BFS / reachability ((or, and) on a pattern matrix), batched
 * SSSP and hop counts ((min, +)), batched Viterbi and widest path ((max, +), (max, *)), integer counting ((+, *) on
 * int32) — one pass over A instead of k executes of a MERGE plan.
 *   Y[r, j] = reduce over the nonzeros n of row r of combine(Ax[n], X[Aj[n], j])      for j < k
 * with (reduce, combine) of MI355_SEMIRING_*; under a PATTERN matrix Ax[n] is one (in the type of X and Y) and Ax is
 * never read.  An empty row gets the identity of reduce: 0 ((+, *), (or, and)), +inf ((min, +)), -inf ((max, *),
 * (max, +)); INT32_MAX / INT32_MIN for int32.  Every element j < k of every row is written; elements j >= k are never
 * touched.  Y is read only under (+, *) with beta != 0.  int32 arithmetic wraps.  No atomics: two executes on the same
 * inputs give the same bits.  (or, and) takes any non-zero as true and writes 0 / 1.
 *   create_typed   vec_type (the type of X, Y and of all arithmetic) in {F32, F64, I32}; mat_type = vec_type or
 *                  MI355_VAL_PATTERN.  PATTERN / F16 / BF16 as vec_type: MI355_SPMV_EINVAL; any other mix (an fp32
 *                  matrix under fp64 vectors, F16 / BF16 matrices): MI355_SPMV_ENOTSUP.  Everything else as
 *                  mi355_spmv_multi_create; mi355_spmv_multi_get_info reports vec_type as val_type.
 *   set_semiring   for the following executes (default MI355_SEMIRING_PLUS_TIMES); nothing is re-sized.  alpha / beta
 *                  exist for (+, *) on F32 / F64 only, as with plan_set_semiring / plan_set_alpha_beta: a semiring
 *                  other than PLUS_TIMES while alpha / beta != 1 / 0, or set_alpha_beta to anything but 1 / 0 under
 *                  such a semiring or on an I32 object, is MI355_SPMV_ENOTSUP; an unknown semiring is EINVAL.
 *   execute        of a PATTERN object ignores Ax (it may be NULL).
 * Out of scope: harness labels (the reference's operator has one x), dist_*, column-major X, and caller-text functors
 * (mi355_spmv_functor_*) on the multi path.                                                                        */
int mi355_spmv_multi_create_typed(mi355_spmv_multi** out, int off_type, int mat_type, int vec_type, int32_t n_rows,
                                  int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max);
int mi355_spmv_multi_set_semiring(mi355_spmv_multi* multi, int semiring);
/* Any of the three pointers may be NULL.                                                                         */
int mi355_spmv_multi_get_types(const mi355_spmv_multi* multi, int* mat_type, int* vec_type, int* semiring);
/* One-shots under a semiring: create_typed (k_max = k), set_semiring, execute, synchronise the stream, destroy;
 * mi355_spmv_multi_pattern_* take the same arguments without Ax.  Argument errors are refused before any device call. */
int mi355_spmv_multi_genl_i32_f32(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const float* Ax, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_genl_i32_f64(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_genl_i32_i32(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const int32_t* Ax, const int32_t* X, int64_t ldx, int32_t* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_genl_i64_f32(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const float* Ax, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_genl_i64_f64(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_genl_i64_i32(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const int32_t* Ax, const int32_t* X, int64_t ldx, int32_t* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_pattern_i32_f32(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_pattern_i32_f64(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_pattern_i32_i32(int semiring, int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const int32_t* X, int64_t ldx, int32_t* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_pattern_i64_f32(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_pattern_i64_f64(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_pattern_i64_i32(int semiring, int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const int32_t* X, int64_t ldx, int32_t* Y, int64_t ldy, int32_t k, void* stream);

/* ---- multi-vector SpMV with 16-bit vectors and fp32 arithmetic (MI355_SPMV_HAS_MULTI_HALF) -------------------------
 * For callers who hold X in 16 bits (GNN features, low-precision block Krylov, batched propagation) and would
 * otherwise widen X, run, and narrow Y: two passes over the vectors saved, and half the gather traffic.
 *   X, Y      row-major as above, both in vec_type: MI355_VAL_F16 (binary16) or MI355_VAL_BF16 (bfloat16)
 *   matrix    values in vec_type, or in MI355_VAL_F32
 * Every stored 16-bit value is widened exactly to fp32; products and sums are fp32.  For a row's fp32 sum S,
 * out = alpha * S, + beta * float(Yold) when beta != 0, and Y = out rounded to vec_type ONCE: nearest even, overflow
 * to +-inf, NaN stays NaN — also for a row that crosses slices (its carries and its last piece stay fp32 in scratch and
 * the fix-up is the row's only writer).  Only (+, *) is built.  Everything else is the contract above: columns j >= k
 * are never read or written, beta == 0 never reads Y, an empty row gets beta * Y (rounded once), any ldx, ldy >= k
 * (16-byte accesses when the pointer and ld * 2 are multiples of 16), no atomics, kernels only.
 * Tiles are 8 / 16 / 32 / 64 columns; scratch is n_slices * (4 + 2 * carry_ld * 4) bytes, carry_ld = k_max rounded up
 * to a multiple of 64.
 *   create_half   vec_type outside {F16, BF16} or an unknown type: MI355_SPMV_EINVAL; a known mat_type other than
 *                 vec_type or F32 (F16 under BF16, F64, I32, PATTERN): MI355_SPMV_ENOTSUP; the size and pointer checks
 *                 of mi355_spmv_multi_create, *out cleared on failure.
 *   The object is executed, scaled, reported and destroyed by mi355_spmv_multi_execute / _set_alpha_beta / _get_info
 *   (val_type = vec_type, widest_tile = 64) / _get_types (the stored matrix type) / _destroy; _set_semiring to anything
 *   but MI355_SEMIRING_PLUS_TIMES is MI355_SPMV_ENOTSUP.
 * Out of scope: semirings and PATTERN in 16 bits, fp32 Y from 16-bit X, dist_*, column-major X.                    */
int mi355_spmv_multi_create_half(mi355_spmv_multi** out, int off_type, int mat_type, int vec_type, int32_t n_rows,
                                 int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max);
/* One-shots with the matrix in the vectors' type (Ax, X, Y: binary16 / bfloat16 as stored): the arguments of
 * mi355_spmv_multi_<off>_<val>.  Argument errors are refused before any device call.                              */
int mi355_spmv_multi_half_i32_f16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_half_i32_bf16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_half_i64_f16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_half_i64_bf16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream);

/* ---- transposed multi-vector SpMV, Y = alpha * A^T X + beta * Y, in three layers (MI355_SPMV_HAS_MULTI_TRANSPOSED) ---
 * For callers who train or attend over a graph: the gradient of multi-vector SpMV with respect to X is A^T dY, and the
 * gradient of SDDMM with respect to V is (A o dOut)^T U — two products with the transpose of a matrix whose VALUES change
 * on every step while its structure does not.  So the structure of A^T is built once, and the values are never moved:
 * an execute reads the caller's Ax, in A's own CSR order, through a slot map.  DESIGN.md 3.14.
 *
 * 1. mi355_spmv_csr_transpose: the structure of A^T on the device, deterministic.
 *   Ap, Aj        the CSR structure of A (n_rows + 1 device offsets of off_type, nnz device int32 columns)
 *   Apt           n_cols + 1 device offsets of off_type;  Ajt: nnz int32, Ajt[t] = the row of A behind transposed slot t
 *   perm          nnz 32-bit indices: perm[t] = the CSR slot of A behind transposed slot t (Axt = Ax[perm])
 *   Inside a column the slots are in ASCENDING SOURCE SLOT order (a stable sort by column): rows ascend, duplicates keep
 *   their order, two calls give identical outputs — never the order of atomics.
 *   workspace     NULL: *workspace_bytes = the bytes needed, return OK (touches no device, needs no GPU); otherwise
 *                 device memory of at least that many bytes; the call allocates nothing.
 * Sizes as coo_to_csr: with MI355_OFF_I32 nnz <= INT32_MAX (else EINVAL); nnz >= 2^32 is MI355_SPMV_ENOTSUP.  Ap and Aj
 * are checked first: offsets that do not ascend from 0 to nnz, or a column outside [0, n_cols), return MI355_SPMV_EINVAL,
 * mi355_spmv_last_error() names the first offender, and no output is written.  The work is enqueued on `stream`, which
 * is then synchronised once.                                                                                       */
int mi355_spmv_csr_transpose(int off_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                             void* Apt, int32_t* Ajt, uint32_t* perm, void* workspace, size_t* workspace_bytes, void* stream);

/* 2. mi355_spmv_multi_create_permuted: a multi-vector object whose matrix values are read through a permutation,
 *   Y[r, j] = alpha * sum over the nonzeros n of row r of Ax[perm[n]] * X[Aj[n], j] + beta * Y[r, j]
 * with Ax, at execute, an array of n_values values.  perm may repeat indices (the mirrors of a symmetric file share one
 * value: the perm of mi355_spmv_coo_to_csr_symmetric) and may leave values unused.  The work is cut, carried and fixed
 * up exactly as a plain object's; the result is, bit for bit, that of a plain object executed on Ax[perm].
 *   perm_type     MI355_OFF_I32: 32-bit indices (what mi355_spmv_csr_transpose writes); MI355_OFF_I64: the int64 of
 *                 mi355_spmv_coo_to_csr
 *   perm          nnz device indices.  Create checks EVERY index against [0, n_values) on the device (on `stream`, which
 *                 it synchronises): a bad one is MI355_SPMV_EINVAL, mi355_spmv_last_error() names the first, and no
 *                 object is made.  The object keeps its own 4-byte copy (no execute can gather out of bounds, and the
 *                 stream carries 4 bytes per nonzero): the caller's perm is not retained.  n_values >= 2^32: ENOTSUP.
 * fp32 / fp64 values and the (+, *) semiring with alpha / beta only: MI355_VAL_I32, MI355_VAL_PATTERN, F16 and BF16 are
 * MI355_SPMV_ENOTSUP (a pattern matrix has no values to permute), and so is mi355_spmv_multi_set_semiring to anything
 * else.  Everything else — k_max, the argument checks before any device call, execute (asynchronous, allocation-free,
 * kernels only: graph-capturable), set_alpha_beta, get_info (main_kernel = "multi_perm_slice_kernel"), destroy — is
 * mi355_spmv_multi_create's.                                                                                       */
int mi355_spmv_multi_create_permuted(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                     int64_t nnz, const void* Ap, const int32_t* Aj, int perm_type, const void* perm,
                                     int64_t n_values, int32_t k_max, void* stream);
/* What a permuted or transposed object holds besides its carries (any pointer may be NULL): the values its executes'
 * Ax has (a plain object: nnz), the bytes of structure and permutation it owns (a plain object: 0), and whether its Ap
 * and Aj are its own (a transposed object) or the caller's.                                                         */
int mi355_spmv_multi_get_perm_info(const mi355_spmv_multi* multi, int64_t* n_values, int64_t* held_bytes, int* owns_structure);
/* The object's Ap, Aj and perm copied to the caller's device arrays (rows + 1 offsets, nnz int32, nnz 32-bit indices; any
 * of the three may be NULL), asynchronously on `stream`: of a transposed object, the CSR structure of A^T.            */
int mi355_spmv_multi_copy_structure(const mi355_spmv_multi* multi, void* Ap, int32_t* Aj, uint32_t* perm, void* stream);

/* 3. mi355_spmv_multi_create_transposed: layers 1 and 2 composed.  Ap and Aj describe A (n_rows x n_cols); the object
 * owns Apt, Ajt and perm — (n_cols + 1) offsets + 8 nnz bytes, reported by get_perm_info and freed by destroy — and does
 * not retain Ap / Aj.  Create allocates, runs the transpose on `stream` and synchronises it; a bad Ap or Aj is EINVAL as
 * in layer 1.  mi355_spmv_multi_execute(multi, Ax, X, ldx, Y, ldy, k, stream) then takes Ax in A's CSR order (nnz
 * values), X as n_rows x k and Y as n_cols x k; an empty column of A gives beta * Y.  Types as layer 2.
 * Out of scope: a transposed single-vector plan, semirings / int32 / 16-bit types, dist_*, harness labels.           */
int mi355_spmv_multi_create_transposed(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                       int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max, void* stream);
/* One-shots: create_transposed (k_max = k), execute, synchronise the stream, destroy.                              */
int mi355_spmv_multi_transposed_i32_f32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const float* Ax, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_transposed_i32_f64(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_transposed_i64_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const float* Ax, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t k, void* stream);
int mi355_spmv_multi_transposed_i64_f64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t k, void* stream);

/* ---- SDDMM: the dot of a row of U and a row of V at every stored entry of A (MI355_SPMV_HAS_SDDMM) ------------------
 * For callers who train or attend over a graph: the gradient of multi-vector SpMV with respect to Ax
 * (dAx = SDDMM of dY and X), the edge score of graph attention, the edge residual of a factorisation on a sparse sample.
 *   out[n] = alpha * s[n] * sum_{j < k} U[r(n) * ldu + j] * V[Aj[n] * ldv + j]  +  beta * out[n]    for n < nnz
 * r(n) is the row that owns entry n; s[n] = Ax[n], or 1 when Ax is NULL (a pattern matrix: no address is formed from Ax).
 *   U     n_rows x k, ROW-major, ldu >= k        V     n_cols x k, ROW-major, ldv >= k
 *   out   nnz values of the value type, in CSR order; it must not overlap Ax, U or V
 * Elements j >= k of a row of U or V are never read; with beta = 0 (the default; alpha = 1) out is never read.  Rows of
 * U / V are read 16 bytes per lane when the pointer and ld * sizeof(value) are 16-byte aligned, else element by element;
 * both add in the same order: an element of out depends on its row of U, its row of V, s, alpha, beta, its old value and
 * k only, never on where the entry lies in A nor on alignment, and two executes on the same inputs give the same bits.
 * Types: {I32, I64} offsets x {F32, F64} values.  MI355_VAL_I32: MI355_SPMV_ENOTSUP; PATTERN / F16 / BF16 / unknown as
 * val_type: MI355_SPMV_EINVAL (a pattern MATRIX is Ax = NULL at execute).  16-bit U / V under fp32 values are an object
 * of their own (mi355_spmv_sddmm_create_half, below).  Semirings, column-major operands and the dist_* entry points are
 * not built.
 * The work is cut as the multi-vector kind's: a wave owns a slice of slice_len merge items (row ends + nonzeros).  Each
 * element of out has one writer: no carries, no scratch, no atomics, ONE kernel per execute for any k >= 1.
 * Life cycle: create retains Ap / Aj (not copied; it does not read them), allocates nothing on the device and makes no
 * device call; execute is asynchronous on `stream`, allocates nothing, never synchronises, launches one kernel
 * (graph-capturable; none when nnz or n_rows is 0); one stream at a time per object.  Every argument error (a null
 * pointer with nonzero sizes, k < 1, ldu or ldv < k, a negative size, nnz beyond 32-bit offsets, an unknown off_type) is
 * MI355_SPMV_EINVAL before any device call, and the text of the last error names the argument.                    */
typedef struct mi355_spmv_sddmm mi355_spmv_sddmm;
typedef struct mi355_spmv_sddmm_info {
    int32_t off_type, val_type;
    int32_t slice_len;       /* merge items (row ends + nonzeros) per slice = per wave                    */
    int32_t block_threads;
    int64_t n_slices;
    int64_t grid_blocks;     /* workgroups of the one kernel                                              */
    char main_kernel[64];
} mi355_spmv_sddmm_info;
int mi355_spmv_sddmm_create(mi355_spmv_sddmm** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                            int64_t nnz, const void* Ap, const int32_t* Aj);
int mi355_spmv_sddmm_set_alpha_beta(mi355_spmv_sddmm* sddmm, double alpha, double beta);
int mi355_spmv_sddmm_execute(mi355_spmv_sddmm* sddmm, const void* Ax, const void* U, int64_t ldu,
                             const void* V, int64_t ldv, void* out, int32_t k, void* stream);
int mi355_spmv_sddmm_get_info(const mi355_spmv_sddmm* sddmm, mi355_spmv_sddmm_info* info);
int mi355_spmv_sddmm_destroy(mi355_spmv_sddmm* sddmm);
/* One-shots: create, execute, destroy.  They do not synchronise the stream.                                      */
int mi355_spmv_sddmm_i32_f32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, const float* Ax,
    const float* U, int64_t ldu, const float* V, int64_t ldv, float* out, int32_t k, void* stream);
int mi355_spmv_sddmm_i32_f64(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, const double* Ax,
    const double* U, int64_t ldu, const double* V, int64_t ldv, double* out, int32_t k, void* stream);
int mi355_spmv_sddmm_i64_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, const float* Ax,
    const float* U, int64_t ldu, const float* V, int64_t ldv, float* out, int32_t k, void* stream);
int mi355_spmv_sddmm_i64_f64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, const double* Ax,
    const double* U, int64_t ldu, const double* V, int64_t ldv, double* out, int32_t k, void* stream);

/* ---- SDDMM with 16-bit U and V and fp32 values and arithmetic (MI355_SPMV_HAS_SDDMM_HALF) ---------------------------
 * For callers who keep features in 16 bits (mi355_spmv_multi_create_half) and want dAx or edge scores without widening
 * dY and X first: no widening pass over the n x k operands, and half the bytes gathered per column.
 *   out[n] = alpha * s[n] * sum_{j < k} float(U[r(n) * ldu + j]) * float(V[Aj[n] * ldv + j])  +  beta * out[n]
 *   U, V      row-major as above, both in ONE vec_type: MI355_VAL_F16 (binary16) or MI355_VAL_BF16 (bfloat16)
 *   Ax, out   fp32 (Ax NULL: a pattern matrix, s = 1)
 * Every stored 16-bit value is widened exactly to fp32; products and sums are fp32; nothing is rounded to 16 bits.
 * Everything else is the contract above: columns j >= k are never read, beta == 0 never reads out, any ldu, ldv >= k
 * (16-byte loads when the pointer and ld * 2 are multiples of 16, else element by element; both add in the same order),
 * one writer per element, no carries, no scratch, no atomics, ONE kernel per execute for any k >= 1 (none when nnz or
 * n_rows is 0), graph-capturable.  A lane's 16 bytes are 8 columns: tiles of 8 / 16 / 32 / 64 columns, so the order of
 * addition differs from the fp32 object's (4 columns per lane) and the two agree within rounding, not bit for bit
 * (bit for bit where every partial sum is exact, as on small integers).
 *   create_half   vec_type outside {F16, BF16}: MI355_SPMV_EINVAL (the text names vec_type); every other check is
 *                 mi355_spmv_sddmm_create's; *out cleared on failure; no device call.
 *   The object is executed, scaled, reported and destroyed by mi355_spmv_sddmm_execute / _set_alpha_beta / _get_info
 *   (val_type = MI355_VAL_F32, main_kernel = "sddmm_half_slice_kernel") / _destroy.
 *   get_types     (F32, F16 | BF16) for this object, (val_type, val_type) for one of mi355_spmv_sddmm_create; either
 *                 pointer may be NULL.
 * Out of scope: 16-bit out / Ax, fp32 U with 16-bit V or the reverse, semirings, column-major operands, dist_*, harness
 * labels, an autograd.Function.                                                                                    */
int mi355_spmv_sddmm_create_half(mi355_spmv_sddmm** out, int off_type, int vec_type, int32_t n_rows, int32_t n_cols,
                                 int64_t nnz, const void* Ap, const int32_t* Aj);
int mi355_spmv_sddmm_get_types(const mi355_spmv_sddmm* sddmm, int* val_type, int* vec_type);
/* One-shots (U, V: binary16 / bfloat16 as stored): create_half, execute, destroy.  They do not synchronise the stream. */
int mi355_spmv_sddmm_half_i32_f16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, const float* Ax,
    const void* U, int64_t ldu, const void* V, int64_t ldv, float* out, int32_t k, void* stream);
int mi355_spmv_sddmm_half_i32_bf16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, const float* Ax,
    const void* U, int64_t ldu, const void* V, int64_t ldv, float* out, int32_t k, void* stream);
int mi355_spmv_sddmm_half_i64_f16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, const float* Ax,
    const void* U, int64_t ldu, const void* V, int64_t ldv, float* out, int32_t k, void* stream);
int mi355_spmv_sddmm_half_i64_bf16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, const float* Ax,
    const void* U, int64_t ldu, const void* V, int64_t ldv, float* out, int32_t k, void* stream);

/* ---- Row softmax over the stored entries of a CSR matrix, "edge softmax" (MI355_SPMV_HAS_ROW_SOFTMAX) ------------------
 * For callers who attend over a graph: the step between the edge scores (SDDMM) and the aggregation (multi-vector SpMV
 * with the result as Ax), and its gradient, without leaving the library for nnz-sized temporaries.
 *   forward    v[n] = scale * x[n];  m_r = max over row r of v;  out[n] = exp(v[n] - m_r) / sum over row r of exp(v - m_r)
 *   backward   t_r = sum over row r of p * dp;  dx[n] = scale * p[n] * (dp[n] - t_r)        (p = the forward's output)
 * x, out, p, dp, dx: nnz values of the value type in CSR order.  Aj is retained for symmetry with the other objects and
 * never read.  scale is 1 after create (the 1 / sqrt(d) of attention: set_scale).
 * Empty rows write nothing.  A row of one entry gives exactly 1.  An entry x[n] = -inf (a masked edge; scale > 0) gives
 * exactly +0, and a row whose entries are ALL -inf gives +0 everywhere, not NaN.
 * In place is allowed: out may be x; dx may be dp or p.  Every element is read by the lane that writes it, and none is
 * read after another wave has written it.  Any other overlap of operands is not allowed.
 * No atomics: two executes on the same inputs give the same bits.  Unlike SDDMM's, the bits of an element depend on
 * where the cuts fall in its row: a row's statistic ((max, sum) forward, the sum backward) is combined by group of 64
 * nonzeros of a slice in ascending order, then by slice in ascending order.
 * Types: {I32, I64} offsets x {F32, F64} values.  MI355_VAL_I32: MI355_SPMV_ENOTSUP; PATTERN / F16 / BF16 / unknown:
 * MI355_SPMV_EINVAL.  16-bit x, a fused SDDMM-softmax-SpMM, a column (transposed) softmax and dist_* entry points are
 * not built.
 * The work is cut as the multi-vector kind's (slice_len merge items per wave).  Three kernels per execute, always the
 * same three: the slices (every row inside a slice is finished from registers: x crosses memory once, out once), a
 * fix-up of the rows that cross slices (one thread per slice), and a finish pass over those rows' pieces.
 * Life cycle: create retains Ap / Aj (not copied, not read) and allocates scratch_bytes = O(n_slices) on the current
 * device (its only device call; none when nnz or n_rows is 0); execute / backward are asynchronous on `stream`,
 * allocate nothing, never synchronise and decide nothing from device data (graph-capturable; no launch when nnz or
 * n_rows is 0); one stream at a time per object.  Every argument error is MI355_SPMV_EINVAL before any device call,
 * and the text of the last error names the argument.                                                             */
typedef struct mi355_spmv_row_softmax mi355_spmv_row_softmax;
typedef struct mi355_spmv_row_softmax_info {
    int32_t off_type, val_type;
    int32_t slice_len;       /* merge items (row ends + nonzeros) per slice = per wave                    */
    int32_t block_threads;
    int64_t n_slices;
    int64_t grid_blocks;     /* workgroups of the slice kernel (and of the finish kernel)                 */
    int64_t scratch_bytes;   /* device memory the object owns                                             */
    char main_kernel[64];
} mi355_spmv_row_softmax_info;
int mi355_spmv_row_softmax_create(mi355_spmv_row_softmax** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                  int64_t nnz, const void* Ap, const int32_t* Aj);
int mi355_spmv_row_softmax_set_scale(mi355_spmv_row_softmax* m, double scale);
int mi355_spmv_row_softmax_execute(mi355_spmv_row_softmax* m, const void* x, void* out, void* stream);
int mi355_spmv_row_softmax_backward(mi355_spmv_row_softmax* m, const void* p, const void* dp, void* dx, void* stream);
int mi355_spmv_row_softmax_get_info(const mi355_spmv_row_softmax* m, mi355_spmv_row_softmax_info* info);
int mi355_spmv_row_softmax_destroy(mi355_spmv_row_softmax* m);
/* One-shots (forward): create, set_scale, execute, synchronise the stream, destroy — the scratch must outlive the
 * kernels, as the multi-vector one-shots' does.                                                                    */
int mi355_spmv_row_softmax_i32_f32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const float* x, float* out, double scale, void* stream);
int mi355_spmv_row_softmax_i32_f64(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj,
    const double* x, double* out, double scale, void* stream);
int mi355_spmv_row_softmax_i64_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const float* x, float* out, double scale, void* stream);
int mi355_spmv_row_softmax_i64_f64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj,
    const double* x, double* out, double scale, void* stream);

/* ---- Fused sparse attention on the structure of a CSR matrix (MI355_SPMV_HAS_ATTENTION) --------------------------------
 * The chain mi355_spmv_sddmm -> mi355_spmv_row_softmax -> mi355_spmv_multi in ONE pass over A, for callers who need O
 * alone (inference, graph-attention layers): nothing of nnz size is written or allocated.
 *   v[n]      = scale * sum_{j < d} Q[r(n) * ldq + j] * K[Aj[n] * ldk + j]  +  bias[n]      for every stored entry n
 *   m_r       = max over row r of v;   l_r = sum over row r of exp(v - m_r)
 *   O[r, :dv] = (sum over row r of exp(v[n] - m_r) * V[Aj[n] * ldv + :dv]) / l_r
 *   lse[r]    = m_r + log(l_r)                                                  (lse NULL: not written)
 *   Q         n_rows x d, K n_cols x d, V n_cols x dv, O n_rows x dv: row-major, leading dimensions ldq, ldk >= d and
 *             ldv, ldo >= dv, all in the object's val_type; bias: nnz values in CSR order, or NULL for none.
 * scale is 1 after create (the 1 / sqrt(d) of attention: set_scale).  There is no alpha / beta: O and lse are never read.
 * bias[n] = -inf is a masked edge and contributes exactly +0 (its row of V is not multiplied in).  A row that is empty
 * or masked whole gets O[r, :dv] = +0 and lse[r] = -inf, never NaN.  A row of one unmasked entry gives O[r] = V[c] and
 * lse[r] = v exactly.  Columns >= d of Q / K and >= dv of V are never read, columns >= dv of O never written.
 * Operands may have any alignment (16-byte accesses where the pointer and ld * sizeof allow, element accesses otherwise:
 * both fill the same registers and give the same bits).  O and lse must not overlap an input or each other; this is not
 * checked.  With lse a caller who trains forms P[n] = exp(v[n] - lse[r]) from one mi355_spmv_sddmm and runs the backward
 * call by call.
 * No atomics: two executes on the same inputs give the same bits.  The bits of O depend on where the step and slice
 * edges fall in a row (states are combined by step, then by slice, in ascending order), as row softmax's do.
 * Types: {I32, I64} offsets x {F32, F64} values.  MI355_VAL_I32: MI355_SPMV_ENOTSUP; PATTERN / F16 / BF16 / unknown:
 * MI355_SPMV_EINVAL.  16-bit Q, K, V and O under fp32 everything else are an object of their own
 * (mi355_spmv_attention_create_half, below).  The fused backward is mi355_spmv_attention_bwd_* (below), heads in one call
 * mi355_spmv_attention_execute_heads (below); dist_* is not built.
 * The work is cut as the multi-vector kind's (slice_len merge items per wave, lanes_per_slot lanes per nonzero from the
 * tile of dv).  An execute launches ceil(dv / widest_tile) slice kernels (each recomputes the scores; widest_tile is 32
 * fp32 / 16 fp64 columns) and, with more than one slice, one fix-up of the rows that cross slices.
 * Life cycle: create retains Ap / Aj (not copied, not read) and allocates scratch_bytes = O(n_slices * dv_max) on the
 * current device (its only device call; none when n_rows is 0); execute is asynchronous on `stream`, allocates nothing,
 * never synchronises and decides nothing from device data (graph-capturable; no launch when n_rows is 0); one stream at a
 * time per object.  Every argument error — a null pointer, d or dv below 1 or above d_max / dv_max, a leading dimension
 * below its width, a type word that is not F32 / F64 — is refused before any device call, and the text of the last
 * error names the argument.                                                                                        */
typedef struct mi355_spmv_attention mi355_spmv_attention;
typedef struct mi355_spmv_attention_info {
    int32_t off_type, val_type;
    int32_t slice_len;       /* merge items (row ends + nonzeros) per slice = per wave                    */
    int32_t block_threads;
    int32_t d_max, dv_max;
    int32_t widest_tile;     /* columns of dv per slice pass                                              */
    int32_t passes;          /* slice kernels of an execute at dv = dv_max                                */
    int32_t lanes_per_slot;  /* C of the first pass at dv = dv_max                                        */
    int32_t reserved;
    int64_t n_slices;
    int64_t grid_blocks;     /* workgroups of a slice kernel                                              */
    int64_t scratch_bytes;   /* device memory the object owns                                             */
    char main_kernel[64];
} mi355_spmv_attention_info;
int mi355_spmv_attention_create(int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int off_type,
                                int val_type, int32_t d_max, int32_t dv_max, mi355_spmv_attention** out);
int mi355_spmv_attention_set_scale(mi355_spmv_attention* m, double scale);
int mi355_spmv_attention_execute(mi355_spmv_attention* m, int32_t d, int32_t dv, const void* Q, int64_t ldq, const void* K,
                                 int64_t ldk, const void* V, int64_t ldv, const void* bias, void* O, int64_t ldo, void* lse,
                                 void* stream);
int mi355_spmv_attention_get_info(const mi355_spmv_attention* m, mi355_spmv_attention_info* info);
int mi355_spmv_attention_destroy(mi355_spmv_attention* m);
/* One-shots: create (d_max = d, dv_max = dv), set_scale, execute, synchronise the stream, destroy — the scratch must
 * outlive the kernels, as the multi-vector one-shots' does.                                                         */
int mi355_spmv_attention_i32_f32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, const float* bias, double scale,
    float* O, int64_t ldo, float* lse, void* stream);
int mi355_spmv_attention_i32_f64(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const double* Q, int64_t ldq, const double* K, int64_t ldk, const double* V, int64_t ldv, const double* bias, double scale,
    double* O, int64_t ldo, double* lse, void* stream);
int mi355_spmv_attention_i64_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, const float* bias, double scale,
    float* O, int64_t ldo, float* lse, void* stream);
int mi355_spmv_attention_i64_f64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const double* Q, int64_t ldq, const double* K, int64_t ldk, const double* V, int64_t ldv, const double* bias, double scale,
    double* O, int64_t ldo, double* lse, void* stream);

/* ---- Fused sparse attention with 16-bit Q, K, V and O (MI355_SPMV_HAS_ATTENTION_HALF) ----------------------------------
 * For callers who keep features in 16 bits (mi355_spmv_multi_create_half, mi355_spmv_sddmm_create_half): no widening of
 * Q, K, V and no narrowing of O around the fused call.  The arithmetic is the fp32 object's, unchanged:
 *   Q, K, V, O   in ONE 16-bit type, vec_type = MI355_VAL_F16 or MI355_VAL_BF16 (2-byte elements; ld* in elements)
 *   bias, lse    float; scale, the scores, the (m, l, acc) states, the scratch and every operation are fp32
 * Every stored value is widened exactly.  An element of O is rounded to the 16-bit type exactly ONCE, from the fp32
 * acc / l, to nearest even — also in a row that crosses slices: the slices leave fp32 states and the fix-up narrows.
 * Masked edges, empty and whole-masked rows (O = +0, lse = -inf), "one live entry gives O[r] = V[c] bit for bit and
 * lse[r] = v", two executes giving the same bits, any ld* and any alignment hold as above (a row is 16-byte aligned when
 * the pointer and ld * 2 allow; both access paths fill the same registers).  No atomics, nothing of nnz size, nothing
 * decided from device data (graph-capturable).
 * A lane's 16 bytes are EIGHT columns: widest_tile = 64, lanes_per_slot from ceil(min(dv_max, 64) / 8), an execute
 * launches ceil(dv / 64) slice kernels.  info reports val_type = MI355_VAL_F32 and main_kernel =
 * "attention_half_slice_kernel"; the type of Q, K, V and O is get_types' vec_type (which equals val_type on an object
 * of mi355_spmv_attention_create).  The object is the same: set_scale, execute, get_info and destroy serve both.
 * create_half: vec_type outside {F16, BF16} is MI355_SPMV_EINVAL ("vec_type" in the text); every other check is
 * create's, before any device call, and *out stays NULL.
 * The fused backward on the same 16-bit type is mi355_spmv_attention_bwd_create_half (below).
 * Out of scope: an fp32 O under 16-bit inputs, mixed Q / K / V types, a 16-bit bias or lse, fp8, dist_*,
 * harness labels.                                                                                                   */
int mi355_spmv_attention_create_half(mi355_spmv_attention** out, int off_type, int vec_type, int32_t n_rows, int32_t n_cols,
                                     int64_t nnz, const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max);
int mi355_spmv_attention_get_types(const mi355_spmv_attention* m, int* val_type, int* vec_type);
/* One-shots (Q, K, V, O: binary16 / bfloat16 as stored): create_half (d_max = d, dv_max = dv), set_scale, execute,
 * synchronise the stream, destroy.                                                                                  */
int mi355_spmv_attention_half_i32_f16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    void* O, int64_t ldo, float* lse, void* stream);
int mi355_spmv_attention_half_i32_bf16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    void* O, int64_t ldo, float* lse, void* stream);
int mi355_spmv_attention_half_i64_f16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    void* O, int64_t ldo, float* lse, void* stream);
int mi355_spmv_attention_half_i64_bf16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    void* O, int64_t ldo, float* lse, void* stream);

/* ---- The fused backward of sparse attention (MI355_SPMV_HAS_ATTENTION_BACKWARD) ---------------------------------------
 * For a caller who trains on mi355_spmv_attention: the step saves O and lse (n_rows-sized) instead of P (nnz-sized), and
 * one object per STRUCTURE — shared by every head, layer and step — holds the transpose.  For every stored entry
 * n = (r, c) of A:
 *   v[n]     = scale * dot(Q[r, :d], K[c, :d]) + bias[n]         (rounded before + bias, as the forward)
 *   p[n]     = v[n] == -inf ? +0 : exp(v[n] - lse[r])            (the test comes before the subtraction)
 *   delta[r] = dot(dO[r, :dv], O[r, :dv]);  dp[n] = dot(dO[r, :dv], V[c, :dv]);  ds[n] = p[n] * (dp[n] - delta[r])
 *   dQ[r, :d]  = sum over row r    of (scale * ds[n]) * K[c, :d]
 *   dK[c, :d]  = sum over column c of (scale * ds[n]) * Q[r, :d]
 *   dV[c, :dv] = sum over column c of p[n] * dO[r, :dv]
 *   dbias[n]   = ds[n]                                           (optional; nnz values in A's CSR order)
 * Q, K, V, bias, O, dO and lse are inputs, all of the object's val_type; O and lse are whatever the caller passes (nothing
 * assumes they came from this library's forward).  Every matrix is row-major with its own leading dimension >= its width
 * (Q, dQ: n_rows x d; K, dK: n_cols x d; V, dV: n_cols x dv; O, dO: n_rows x dv) and may have any alignment (16-byte
 * accesses where the pointer and ld * sizeof allow, element accesses otherwise: same registers, same bits).  Outputs are
 * never read (no alpha / beta) and must not overlap an input or each other; this is not checked.
 * A masked edge (bias[n] = -inf) has p = ds = dbias = +0, and its rows of K, V, Q and dO are not loaded: a NaN there
 * contributes nothing.  A row of A without entries gets dQ[r] = +0, a column without entries dK[c] = dV[c] = +0.  Every
 * element of every requested output is written by every execute.
 * The work: one kernel for delta (into the object's scratch), then ONE slice walk in three roles — DQ on A; DK and DV on
 * A^T with bias read through the slot map — each cut as the multi-vector kind's (slice_len merge items per wave,
 * lanes_per_slot lanes per entry from the tile of the role's OUTPUT), each taking ceil(width / widest_tile) launches that
 * recompute the coefficient, and each followed, when its structure has more than one slice, by a fix-up of the lines
 * that cross slices.  A role whose output is NULL is not launched.  No atomics; nothing of nnz size is allocated or
 * written (dbias apart).  Order of addition: within a step the scan tree, then steps ascending, then slices ascending:
 * two executes give the same bits, and the bits of a line depend only on where step and slice edges fall in that line of
 * A (dQ) or A^T (dK, dV).
 * Life cycle: create builds Apt / Ajt / perm with mi355_spmv_csr_transpose on `stream` (which it synchronises) and holds
 * them in one allocation of held_bytes = 8 nnz + (n_cols + 1) offsets, allocates scratch_bytes = O(n_rows + slices *
 * max(d_max, dv_max)), and retains Ap / Aj (not copied).  2^32 or more entries: MI355_SPMV_ENOTSUP.  Type refusals as
 * mi355_spmv_attention_create (16-bit operands: mi355_spmv_attention_bwd_create_half, below).  execute is asynchronous on `stream`, launches kernels
 * only, never synchronises and decides nothing from device data (graph-capturable); one stream at a time per object.
 * Any of dQ / dK / dV may be NULL; all three NULL is MI355_SPMV_EINVAL, and so is dbias without dQ (it comes from the DQ
 * walk).  Every argument error is refused before any device call, and the text of the last error names the argument.
 * Out of scope: dist_*, harness labels, semirings, sharing the held transpose with a transposed multi-vector object
 * (DESIGN.md 3.15.2).  Heads in one call: mi355_spmv_attention_bwd_execute_heads (below).                            */
typedef struct mi355_spmv_attention_bwd mi355_spmv_attention_bwd;
typedef struct mi355_spmv_attention_bwd_info {
    int32_t off_type, val_type;
    int32_t slice_len;          /* merge items (line ends + entries) per slice = per wave                 */
    int32_t block_threads;
    int32_t d_max, dv_max;
    int32_t widest_tile;        /* columns of an output per slice pass                                    */
    int32_t reserved;
    int32_t lanes_per_slot[3];  /* C of the first pass of DQ, DK, DV at d = d_max, dv = dv_max            */
    int32_t passes[3];          /* slice kernels of DQ, DK, DV at the maxima                              */
    int64_t n_slices;           /* of A (the DQ walk)                                                     */
    int64_t grid_blocks;
    int64_t n_slices_t;         /* of A^T (the DK and DV walks)                                           */
    int64_t grid_blocks_t;
    int64_t scratch_bytes;      /* delta and the slices' pieces                                           */
    int64_t held_bytes;         /* Apt, Ajt and perm                                                      */
    char main_kernel[64];
} mi355_spmv_attention_bwd_info;
int mi355_spmv_attention_bwd_create(mi355_spmv_attention_bwd** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                    int64_t nnz, const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max, void* stream);
int mi355_spmv_attention_bwd_set_scale(mi355_spmv_attention_bwd* m, double scale);
int mi355_spmv_attention_bwd_execute(mi355_spmv_attention_bwd* m, int32_t d, int32_t dv, const void* Q, int64_t ldq, const void* K,
                                     int64_t ldk, const void* V, int64_t ldv, const void* bias, const void* O, int64_t ldo,
                                     const void* dO, int64_t lddo, const void* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk,
                                     void* dV, int64_t lddv, void* dbias, void* stream);
int mi355_spmv_attention_bwd_get_info(const mi355_spmv_attention_bwd* m, mi355_spmv_attention_bwd_info* info);
int mi355_spmv_attention_bwd_destroy(mi355_spmv_attention_bwd* m);
/* One-shots: create (d_max = d, dv_max = dv), set_scale, execute, synchronise the stream, destroy.                   */
int mi355_spmv_attention_bwd_i32_f32(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, const float* bias, double scale,
    const float* O, int64_t ldo, const float* dO, int64_t lddo, const float* lse, float* dQ, int64_t lddq, float* dK, int64_t lddk,
    float* dV, int64_t lddv, float* dbias, void* stream);
int mi355_spmv_attention_bwd_i32_f64(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const double* Q, int64_t ldq, const double* K, int64_t ldk, const double* V, int64_t ldv, const double* bias, double scale,
    const double* O, int64_t ldo, const double* dO, int64_t lddo, const double* lse, double* dQ, int64_t lddq, double* dK, int64_t lddk,
    double* dV, int64_t lddv, double* dbias, void* stream);
int mi355_spmv_attention_bwd_i64_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv, const float* bias, double scale,
    const float* O, int64_t ldo, const float* dO, int64_t lddo, const float* lse, float* dQ, int64_t lddq, float* dK, int64_t lddk,
    float* dV, int64_t lddv, float* dbias, void* stream);
int mi355_spmv_attention_bwd_i64_f64(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const double* Q, int64_t ldq, const double* K, int64_t ldk, const double* V, int64_t ldv, const double* bias, double scale,
    const double* O, int64_t ldo, const double* dO, int64_t lddo, const double* lse, double* dQ, int64_t lddq, double* dK, int64_t lddk,
    double* dV, int64_t lddv, double* dbias, void* stream);

/* ---- The fused backward with 16-bit operands (MI355_SPMV_HAS_ATTENTION_BACKWARD_HALF) ----------------------------------
 * For callers who train on mi355_spmv_attention_create_half: no widening of Q, K, V, O, dO and no narrowing of dQ, dK, dV
 * around the fused call.  The arithmetic is the fp32 object's, operation for operation:
 *   Q, K, V, O, dO, dQ, dK, dV   in ONE 16-bit type, vec_type = MI355_VAL_F16 or MI355_VAL_BF16 (2-byte elements; ld* in
 *                                elements)
 *   bias, lse, dbias             float; delta, scale, the scores, p, dp, ds, the coefficients, the per-slot partials, the
 *                                slices' pieces in scratch and every operation are fp32
 * Every stored value is widened exactly.  An element of dQ, dK or dV is rounded to the 16-bit type exactly ONCE, from the
 * fp32 sum of its line, to nearest even: by the slot that holds the line's last entry, or, for a line that crosses
 * slices, by the fix-up after it has added the fp32 pieces in slice order.  A line without a live entry is the 16-bit +0
 * bit pattern.  Masked edges (exactly +0, no row loaded), the test on v before the subtraction, every requested element
 * written by every execute, two executes giving the same bits, any ld* and any alignment (a row is 16-byte aligned when
 * the pointer and ld * 2 allow; both access paths fill the same registers, so an unaligned operand gives the aligned
 * bits), NULL roles not launched and dbias without dQ refused hold as above.  No atomics, nothing of nnz size apart from
 * dbias, kernels only (graph-capturable).
 * A lane's 16 bytes are EIGHT columns: widest_tile = 64, lanes_per_slot from ceil(min(width, 64) / 8) of each role's
 * output, ceil(width / 64) launches per role (d = dv = 64 is one pass per role).  get_info reports val_type =
 * MI355_VAL_F32 and main_kernel = "attention_bwd_half_slice_kernel"; the type of the matrices is get_types' vec_type
 * (which equals val_type on an object of mi355_spmv_attention_bwd_create).  The object is the same: set_scale, execute,
 * get_info and destroy serve both.
 * create_half: vec_type outside {F16, BF16} is MI355_SPMV_EINVAL ("vec_type" in the text); every other check is
 * mi355_spmv_attention_bwd_create's, before any device call, and *out stays NULL.
 * Out of scope: fp32 gradients under 16-bit inputs, mixed 16-bit types, a 16-bit bias / lse / dbias, fp8, dist_*,
 * harness labels, a 16-bit transposed multi-vector object.                                                           */
int mi355_spmv_attention_bwd_create_half(mi355_spmv_attention_bwd** out, int off_type, int vec_type, int32_t n_rows, int32_t n_cols,
                                         int64_t nnz, const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max, void* stream);
int mi355_spmv_attention_bwd_get_types(const mi355_spmv_attention_bwd* m, int* val_type, int* vec_type);
/* One-shots (the eight matrices: binary16 / bfloat16 as stored): create_half (d_max = d, dv_max = dv), set_scale, execute,
 * synchronise the stream, destroy.                                                                                  */
int mi355_spmv_attention_bwd_half_i32_f16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk,
    void* dV, int64_t lddv, float* dbias, void* stream);
int mi355_spmv_attention_bwd_half_i32_bf16(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk,
    void* dV, int64_t lddv, float* dbias, void* stream);
int mi355_spmv_attention_bwd_half_i64_f16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk,
    void* dV, int64_t lddv, float* dbias, void* stream);
int mi355_spmv_attention_bwd_half_i64_bf16(int32_t n_rows, int32_t n_cols, int64_t nnz, const int64_t* Ap, const int32_t* Aj, int32_t d, int32_t dv,
    const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const float* bias, double scale,
    const void* O, int64_t ldo, const void* dO, int64_t lddo, const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk,
    void* dV, int64_t lddv, float* dbias, void* stream);

/* ---- The heads of sparse attention in one call (MI355_SPMV_HAS_ATTENTION_HEADS) ---------------------------------------
 * A layer of H heads on one structure is ONE execute, forward or backward, instead of H: the same launches as one head's
 * (2 forward, up to 7 backward), each over H times the workgroups.  The structure, the cut and the backward's held
 * transpose are shared; a head is a pointer offset and a private copy of the O(slices) scratch.  The objects are the
 * existing ones, of either storage type (create and create_half): set_scale (ONE scale for all heads), get_info,
 * get_types and destroy serve them unchanged, and execute is execute_heads with n_heads = 1.
 * Strides: a stride is the number of ELEMENTS, in the operand's own type, between head h and head h + 1 of that operand;
 * the arguments behind hs are exactly execute's and describe head 0.
 *   (n, H, d) interleaved:  ld = H * d, stride = d.          (H, n, d) head-major:  ld = d, stride = n * d.
 *   bias, lse and dbias are head-major vectors: stride >= nnz (bias, dbias), >= n_rows (lse).
 *   An INPUT stride of 0 shares that operand between all heads (q, k, v, bias; in the backward also o, d_o, lse): one K and
 *   V for every head is multi-query attention, one bias a shared mask.  A negative stride is MI355_SPMV_EINVAL.
 *   With n_heads = 1 no stride is read and hs may be NULL; with n_heads > 1 a NULL hs is MI355_SPMV_EINVAL.
 * The heads of an OUTPUT may not overlap, and this is checked (a wrong stride would silently corrupt another head): for
 * a matrix of rows x width at leading dimension ld the stride must be >= width and satisfy either
 *   stride >= (rows - 1) * ld + width   (head-major)     or     ld >= (n_heads - 1) * stride + width   (interleaved);
 * lse, when asked for, needs stride >= n_rows and dbias stride >= nnz.  Anything else is MI355_SPMV_EINVAL and the text
 * names the stride (o, lse, dq, dk, dv, dbias).  An overlap between an output and an input stays unchecked, as in execute.
 * reserve_heads: after create n_heads_max is 1.  reserve_heads(n) allocates n copies of the per-head scratch (the
 * backward's: delta and every role's pieces), THEN frees the old scratch; on failure the object keeps the old scratch
 * and the old maximum.  get_info().scratch_bytes reports the new size; the backward's held_bytes (the transpose, which
 * every head shares) is not touched.  It is a device call like create (none on an object without rows): NOT for use
 * during stream capture or while an execute of the object is in flight.  n below 1: MI355_SPMV_EINVAL.
 * execute_heads: every check of execute first, in the same order and with the same messages; then n_heads must lie in
 * 1 .. n_heads_max ("n_heads" in the text); then the strides.  A grid of 2^31 workgroups or more is MI355_SPMV_ENOTSUP.
 * All checks come before any device call.  It is asynchronous on `stream`, allocates nothing, decides nothing from
 * device data and is graph-capturable; heads beyond n_heads leave their scratch unused.  In the backward a NULL role is
 * not launched for any head, and dbias without dQ is refused as in execute.
 * THE PROMISE: head h of an execute_heads equals execute on the operands offset by h strides, BIT FOR BIT, in every
 * element of every output, for any alignment and any stride.  It holds because a row takes the 16-byte path only where
 * head 0's rows are 16-byte aligned (pointer and ld * sizeof) AND the head stride in bytes is a multiple of 16 (or
 * n_heads is 1), and both paths fill the same registers; and because workgroup b of a slice kernel serves head
 * b % n_heads and slice block b / n_heads, so every head is cut exactly as one head is.
 * Out of scope: a head -> KV-head map (grouped-query attention beyond stride 0), per-head scales, one-shots with heads,
 * a sum of dK / dV over heads inside the kernel, dist_*, harness labels.                                            */
typedef struct mi355_spmv_attention_head_strides {
    int64_t q, k, v, bias, o, lse;
} mi355_spmv_attention_head_strides;
typedef struct mi355_spmv_attention_bwd_head_strides {
    int64_t q, k, v, bias, o, d_o, lse, dq, dk, dv, dbias;
} mi355_spmv_attention_bwd_head_strides;
int mi355_spmv_attention_reserve_heads(mi355_spmv_attention* m, int32_t n_heads_max);
int mi355_spmv_attention_get_heads_max(const mi355_spmv_attention* m, int32_t* n_heads_max);
int mi355_spmv_attention_execute_heads(mi355_spmv_attention* m, int32_t n_heads, const mi355_spmv_attention_head_strides* hs, int32_t d,
                                       int32_t dv, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                       const void* bias, void* O, int64_t ldo, void* lse, void* stream);
int mi355_spmv_attention_bwd_reserve_heads(mi355_spmv_attention_bwd* m, int32_t n_heads_max);
int mi355_spmv_attention_bwd_get_heads_max(const mi355_spmv_attention_bwd* m, int32_t* n_heads_max);
int mi355_spmv_attention_bwd_execute_heads(mi355_spmv_attention_bwd* m, int32_t n_heads, const mi355_spmv_attention_bwd_head_strides* hs,
                                           int32_t d, int32_t dv, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                           int64_t ldv, const void* bias, const void* O, int64_t ldo, const void* dO, int64_t lddo,
                                           const void* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv,
                                           void* dbias, void* stream);

/* ---- misc ------------------------------------------------------------------ */
int mi355_spmv_version(void);
const char* mi355_spmv_status_string(int status);
/* Message of the last failing call on this thread ("" if none).               */
const char* mi355_spmv_last_error(void);
/* Number of visible gfx950 devices (0 if none / no HIP runtime).              */
int mi355_spmv_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355_SPMV_H */
