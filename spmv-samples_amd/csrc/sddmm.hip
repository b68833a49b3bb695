// sddmm.hip — sampled dense-dense matrix product on the structure of A (mi355_spmv_sddmm_*):
//   out[n] = alpha * s[n] * sum_{j < k} U[r(n), j] * V[Aj[n], j] + beta * out[n]        for every stored entry n of A
// r(n) = the row that owns entry n, s[n] = Ax[n] (1 for a pattern: Ax == NULL).  The gradient of multi-vector SpMV with
// respect to Ax, the edge score of graph attention, the residual of a factorisation on a sparse sample.  An object of
// its own beside mi355_spmv_multi: the kernel, its launch and the extern "C" entry points, all in this unit.
//
//   sddmm_slice_kernel   one WAVE per slice of kSliceLen merge items (row ends + nonzeros): the cut of the multi-vector
//                        kind, shared with it (slice_cut.hpp, slice_cut.inc, slice_cut_row.inc).  The wave finds its two
//                        merge-path diagonals, keeps its rows' offsets in LDS relative to its first nonzero, and walks
//                        its nonzeros 64 at a time (sddmm_slice_walk.inc: the walk is ONE text, this kernel's and
//                        sddmm_half_slice_kernel's): Aj (and Ax) are loaded coalesced, one per lane, and each lane finds its
//                        nonzero's row by a binary search in LDS.  Lanes are (nonzero slot x 16-byte column group):
//                        a slot of C lanes takes one nonzero, lane c gathers its 16 bytes of V[col] and of U[row] and
//                        multiplies them into ONE scalar partial; for k wider than the tile of C groups the lane goes
//                        on to the next tile and keeps adding into the same register (A and out cross HBM once whatever
//                        k is).  An xor-shuffle tree over the C lanes of the slot gives the dot.
//   the store            the reduction runs across the column lanes of one slot, not across the slots of a row: no
//                        carries, no fix-up, no scratch, no atomics, one writer per element.  The C steps of a group of
//                        64 nonzeros hand their dots back to the lane that loaded the nonzero (one shuffle per step);
//                        that lane still holds Ax[n], so out[n0 + m] is scaled and stored once, 64 contiguous values.
//
// Order of addition: a lane adds its columns in ascending order, tile after tile, into one partial that starts at +0
// (a masked column is loaded as 0 and adds +0), and the tree adds lanes at distance 1, 2, 4, ...: an element of out is
// a function of (U[r, :k], V[c, :k], s, alpha, beta, out_old, k) only — not of where in a slice, step or slot its
// nonzero falls, and not of the alignment of U and V (the 16-byte and the element-by-element load fill the same
// registers; the arithmetic is one piece of code behind both, and behind every type of U and V: sddmm_slice_walk.inc).
//
// U and V in 16 bits under fp32 Ax, out and arithmetic (mi355_spmv_sddmm_create_half): sddmm_half_slice_kernel and its
// launch, sddmm_half_kernel.hpp, around the same walk; the object and the entry points are this unit's.
#include <new>
#include <type_traits>

#include "slice_cut.hpp"

struct mi355_spmv_sddmm {   // the opaque handle of include/mi355_spmv.h: host memory only, nothing on the device
    int off_type = 0, val_type = 0;
    int vec_type = 0;       // the type of U and V: val_type, or F16 / BF16 under F32 values (create_half)
    int32_t n_rows = 0, n_cols = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;
    double alpha = 1.0, beta = 0.0;
    int64_t n_slices = 0;
};

namespace mi355 {

// The geometry that the host simulation's tables are written for: tests/test_sddmm_sim_cpu.py reads these two lines
// and holds tests/sddmm_cases.py to them.  The kernel uses slice_cut.hpp's constants; a change there stops here.
constexpr int kSddmmSlice = 1024;
constexpr int kSddmmGroupsMax = 8;
static_assert(kSddmmSlice == kSliceLen && kSddmmGroupsMax == kSliceGroupsMax, "tests/sddmm_cases.py is tabled for this geometry");

template <typename val_t>
struct SddmmArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const val_t* Ax;        // null for a pattern kernel, which never forms an address from it
    const val_t* U;
    const val_t* V;
    val_t* out;
    int64_t ldu, ldv;
    int32_t k;
    int32_t u_vec, v_vec;   // 1 = rows of U / V are 16-byte aligned: one 16-byte load per lane and tile
    val_t alpha, beta;
};

// the arguments of an execute, Args = SddmmArgs<val_t> or SddmmHalfArgs<vec_t> (sddmm_half_kernel.hpp): the two structs
// have the same fields, of their own types
template <typename Args>
Args sddmm_args(const mi355_spmv_sddmm& m, const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out, int32_t k) {
    Args a;
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.Aj = m.Aj;
    a.Ax = static_cast<decltype(a.Ax)>(Ax);
    a.U = static_cast<decltype(a.U)>(U); a.V = static_cast<decltype(a.V)>(V);
    a.out = static_cast<decltype(a.out)>(out);
    a.ldu = ldu; a.ldv = ldv; a.k = k;
    a.u_vec = rows_aligned16<std::remove_pointer_t<decltype(a.U)>>(U, ldu) ? 1 : 0;
    a.v_vec = rows_aligned16<std::remove_pointer_t<decltype(a.V)>>(V, ldv) ? 1 : 0;
    a.alpha = decltype(a.alpha)(m.alpha); a.beta = decltype(a.beta)(m.beta);
    return a;
}

// one rounding per column whatever the compiler would otherwise choose to contract: the promise above, spelled out
__device__ __forceinline__ float sddmm_fma(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
__device__ __forceinline__ double sddmm_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }

// C = lanes per nonzero slot (16-byte column groups of a tile); the wave holds S = 64 / C slots
template <typename off_t, typename val_t, int C, bool VALUED>
__global__ __launch_bounds__(kBlock) void sddmm_slice_kernel(const SddmmArgs<val_t> a, const off_t* __restrict__ Ap) {
    using acc_t = val_t;
    constexpr int W = 16 / int(sizeof(val_t));      // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr bool kCutCarriedIn = false, kCutKeepsR1 = false;      // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = 0;
    constexpr bool kWalkFmaInPlace = false;                         // what sddmm_slice_walk.inc asks its includer
    const unsigned cut_block = blockIdx.x;
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, n0, nn, nr, rel
#include "sddmm_slice_walk.inc"     // the slice's nonzeros, 64 at a time: load_cols is slice_cut.hpp's
}

}  // namespace mi355

#include "sddmm_half_kernel.hpp"    // (down here: its launch uses the handle and sddmm_args)

using namespace mi355;

namespace {

// argument-only checks of a create (also run by the one-shots before they make anything)
int sddmm_check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                       const int32_t* Aj) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown off_type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32) {
        set_error("%s: val_type MI355_VAL_I32 is not built (fp32 / fp64 values)", who);
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) {
        set_error("%s: val_type %d is not a type of U, V and out (F32 or F64; a pattern matrix is Ax = NULL at execute)", who, val_type);
        return MI355_SPMV_EINVAL;
    }
    return check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj);
}

// argument-only checks of an execute
int sddmm_check_execute(const char* who, int64_t nnz, const void* U, int64_t ldu, const void* V, int64_t ldv, const void* out, int32_t k) {
    if (k < 1) { set_error("%s: k = %d below 1", who, k); return MI355_SPMV_EINVAL; }
    if (ldu < k) { set_error("%s: ldu = %lld below k = %d", who, (long long)ldu, k); return MI355_SPMV_EINVAL; }
    if (ldv < k) { set_error("%s: ldv = %lld below k = %d", who, (long long)ldv, k); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !U) { set_error("%s: null U", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !V) { set_error("%s: null V", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !out) { set_error("%s: null out", who); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

// the checks of create_half (and of the 16-bit one-shots): vec_type first, then what a create of fp32 values checks
int sddmm_check_create_half(const char* who, int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                            const int32_t* Aj) {
    if (vec_type != MI355_VAL_F16 && vec_type != MI355_VAL_BF16) {
        set_error("%s: vec_type %d is not a 16-bit type of U and V (MI355_VAL_F16 or MI355_VAL_BF16)", who, vec_type);
        return MI355_SPMV_EINVAL;
    }
    return sddmm_check_create(who, off_type, MI355_VAL_F32, n_rows, n_cols, nnz, Ap, Aj);
}

void sddmm_fill(mi355_spmv_sddmm& m, int off_type, int val_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                const void* Ap, const int32_t* Aj) {
    m.off_type = off_type; m.val_type = val_type; m.vec_type = vec_type;
    m.n_rows = n_rows; m.n_cols = n_cols; m.nnz = nnz;
    m.Ap = Ap; m.Aj = Aj;
    m.n_slices = slice_count(n_rows, nnz);
}

// the one launch of an execute: C from k alone, valued / pattern from Ax
template <typename off_t, typename val_t, bool VALUED>
int sddmm_launch(const mi355_spmv_sddmm& m, const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out,
                 int32_t k, hipStream_t s) {
    const SddmmArgs<val_t> a = sddmm_args<SddmmArgs<val_t>>(m, Ax, U, ldu, V, ldv, out, k);
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    constexpr int W = 16 / int(sizeof(val_t));
    with_slot_lanes((k + W - 1) / W, [&](auto lanes) {
        hipLaunchKernelGGL((sddmm_slice_kernel<off_t, val_t, decltype(lanes)::value, VALUED>), grid, block, 0, s, a, Ap);
    });
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

template <typename off_t, typename val_t>
int sddmm_launch_values(const mi355_spmv_sddmm& m, const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out,
                        int32_t k, hipStream_t s) {
    return Ax ? sddmm_launch<off_t, val_t, true>(m, Ax, U, ldu, V, ldv, out, k, s)
              : sddmm_launch<off_t, val_t, false>(m, Ax, U, ldu, V, ldv, out, k, s);
}

int sddmm_run(const mi355_spmv_sddmm& m, const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out, int32_t k,
              void* stream) {
    if (m.nnz == 0 || m.n_rows == 0) return MI355_SPMV_OK;      // no stored entry: nothing to write, nothing launched
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (m.vec_type != m.val_type) {     // 16-bit U and V under fp32 values
        const bool i32 = m.off_type == MI355_OFF_I32;
        auto run = [&](auto off, auto vec) {
            return sddmm_half_launch<decltype(off), decltype(vec)>(m, Ax, U, ldu, V, ldv, out, k, s);
        };
        if (m.vec_type == MI355_VAL_F16) return i32 ? run(int32_t(), F16()) : run(int64_t(), F16());
        return i32 ? run(int32_t(), Bf16()) : run(int64_t(), Bf16());
    }
    if (m.off_type == MI355_OFF_I32)
        return m.val_type == MI355_VAL_F64 ? sddmm_launch_values<int32_t, double>(m, Ax, U, ldu, V, ldv, out, k, s)
                                           : sddmm_launch_values<int32_t, float>(m, Ax, U, ldu, V, ldv, out, k, s);
    return m.val_type == MI355_VAL_F64 ? sddmm_launch_values<int64_t, double>(m, Ax, U, ldu, V, ldv, out, k, s)
                                       : sddmm_launch_values<int64_t, float>(m, Ax, U, ldu, V, ldv, out, k, s);
}

// the one-shots: the object lives on the caller's stack for the one launch (which copies what it reads of it into the
// kernel's arguments); every argument check comes before any device call, and nothing synchronises
int sddmm_one_shot(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                   const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out, int32_t k, void* stream) {
    set_error("%s", "");
    if (const int st = sddmm_check_create("sddmm", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    if (const int st = sddmm_check_execute("sddmm", nnz, U, ldu, V, ldv, out, k)) return st;
    mi355_spmv_sddmm m;
    sddmm_fill(m, off_type, val_type, val_type, n_rows, n_cols, nnz, Ap, Aj);
    return sddmm_run(m, Ax, U, ldu, V, ldv, out, k, stream);
}

int sddmm_half_one_shot(int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                        const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out, int32_t k, void* stream) {
    set_error("%s", "");
    if (const int st = sddmm_check_create_half("sddmm_half", off_type, vec_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    if (const int st = sddmm_check_execute("sddmm_half", nnz, U, ldu, V, ldv, out, k)) return st;
    mi355_spmv_sddmm m;
    sddmm_fill(m, off_type, MI355_VAL_F32, vec_type, n_rows, n_cols, nnz, Ap, Aj);
    return sddmm_run(m, Ax, U, ldu, V, ldv, out, k, stream);
}

}  // namespace

extern "C" {

int mi355_spmv_sddmm_create(mi355_spmv_sddmm** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                            const void* Ap, const int32_t* Aj) {
    set_error("%s", "");
    if (!out) { set_error("sddmm_create: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = sddmm_check_create("sddmm_create", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    mi355_spmv_sddmm* m = new (std::nothrow) mi355_spmv_sddmm();
    if (!m) { set_error("sddmm_create: host allocation failed"); return MI355_SPMV_ENOMEM; }
    sddmm_fill(*m, off_type, val_type, val_type, n_rows, n_cols, nnz, Ap, Aj);
    *out = m;
    return MI355_SPMV_OK;
}

int mi355_spmv_sddmm_create_half(mi355_spmv_sddmm** out, int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                 const void* Ap, const int32_t* Aj) {
    set_error("%s", "");
    if (!out) { set_error("sddmm_create_half: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = sddmm_check_create_half("sddmm_create_half", off_type, vec_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    mi355_spmv_sddmm* m = new (std::nothrow) mi355_spmv_sddmm();
    if (!m) { set_error("sddmm_create_half: host allocation failed"); return MI355_SPMV_ENOMEM; }
    sddmm_fill(*m, off_type, MI355_VAL_F32, vec_type, n_rows, n_cols, nnz, Ap, Aj);
    *out = m;
    return MI355_SPMV_OK;
}

int mi355_spmv_sddmm_get_types(const mi355_spmv_sddmm* m, int* val_type, int* vec_type) {
    if (!m) { set_error("sddmm_get_types: null object"); return MI355_SPMV_EINVAL; }
    if (val_type) *val_type = m->val_type;
    if (vec_type) *vec_type = m->vec_type;
    return MI355_SPMV_OK;
}

int mi355_spmv_sddmm_set_alpha_beta(mi355_spmv_sddmm* m, double alpha, double beta) {
    set_error("%s", "");
    if (!m) { set_error("sddmm_set_alpha_beta: null object"); return MI355_SPMV_EINVAL; }
    m->alpha = alpha;
    m->beta = beta;
    return MI355_SPMV_OK;
}

int mi355_spmv_sddmm_execute(mi355_spmv_sddmm* m, const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out,
                             int32_t k, void* stream) {
    set_error("%s", "");
    if (!m) { set_error("sddmm_execute: null object"); return MI355_SPMV_EINVAL; }
    if (const int st = sddmm_check_execute("sddmm_execute", m->nnz, U, ldu, V, ldv, out, k)) return st;
    return sddmm_run(*m, Ax, U, ldu, V, ldv, out, k, stream);
}

int mi355_spmv_sddmm_get_info(const mi355_spmv_sddmm* m, mi355_spmv_sddmm_info* info) {
    if (!m || !info) { set_error("sddmm_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->n_slices = m->n_slices;
    info->grid_blocks = slice_grid(m->n_slices);
    snprintf(info->main_kernel, sizeof(info->main_kernel), m->vec_type != m->val_type ? "sddmm_half_slice_kernel" : "sddmm_slice_kernel");
    return MI355_SPMV_OK;
}

int mi355_spmv_sddmm_destroy(mi355_spmv_sddmm* m) {
    delete m;
    return MI355_SPMV_OK;
}

#define MI355_SPMV_DEFINE_SDDMM(SUF, OFF, OFFENUM, VAL, VALENUM)                                                       \
    int mi355_spmv_sddmm_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, const VAL* Ax, \
                               const VAL* U, int64_t ldu, const VAL* V, int64_t ldv, VAL* out, int32_t k, void* stream) { \
        return sddmm_one_shot(OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, Ax, U, ldu, V, ldv, out, k, stream); \
    }
MI355_SPMV_DEFINE_SDDMM(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_SDDMM(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_SDDMM(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_SDDMM(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

#define MI355_SPMV_DEFINE_SDDMM_HALF(SUF, OFF, OFFENUM, VECENUM)                                                              \
    int mi355_spmv_sddmm_half_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, const float* Ax, \
                                    const void* U, int64_t ldu, const void* V, int64_t ldv, float* out, int32_t k, void* stream) { \
        return sddmm_half_one_shot(OFFENUM, VECENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, Ax, U, ldu, V, ldv, out, k, stream); \
    }
MI355_SPMV_DEFINE_SDDMM_HALF(i32_f16, int32_t, MI355_OFF_I32, MI355_VAL_F16)
MI355_SPMV_DEFINE_SDDMM_HALF(i32_bf16, int32_t, MI355_OFF_I32, MI355_VAL_BF16)
MI355_SPMV_DEFINE_SDDMM_HALF(i64_f16, int64_t, MI355_OFF_I64, MI355_VAL_F16)
MI355_SPMV_DEFINE_SDDMM_HALF(i64_bf16, int64_t, MI355_OFF_I64, MI355_VAL_BF16)

}  // extern "C"
