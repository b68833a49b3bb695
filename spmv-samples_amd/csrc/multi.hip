// multi.hip — multi-vector SpMV, Y = A X for k vectors in one pass over A (mi355_spmv_multi_*): the object, its host
// launch dispatch and the extern "C" entry points.  An object of its own: it shares no chunk body, planner or launch
// path with the VECTOR / LIGHT / MERGE kinds.  The kernels and launch_multi: multi_kernels.hpp; their instantiations
// per value type: the multi_<type>.hip units, which include this file with MI355_MULTI_TU set to the value type (the
// library's build, MI355_MULTI_SPLIT_UNITS; without it this unit instantiates what it launches and stands alone).
// 16-bit vectors (mi355_spmv_multi_create_half): multi_half_kernels.hpp, instantiated by multi_h16.hip, which includes
// this file with MI355_MULTI_HALF_TU set.  Permuted and transposed objects are made by multi_perm.hip and
// multi_transposed.hip on an object of this unit (multi_attach_perm) and executed here; their kernels are instantiated by
// multi_perm_f32.hip / multi_perm_f64.hip, which include this file with MI355_MULTI_PERM_TU set.  The slice geometry and the cut are the slice kinds' own, shared with SDDMM:
// slice_cut.hpp, slice_cut.inc.  DESIGN.md §3.10, §3.10.1, §3.10.2.
#include <algorithm>
#include <new>

#include "multi_kernels.hpp"
#include "multi_half_kernels.hpp"

namespace mi355 {
// The geometry that the host simulation's tables are written for: tests/test_multi_sim_cpu.py reads these two lines
// and holds tests/multi_cases.py to them.  The kernels use slice_cut.hpp's constants; a change there stops here.
constexpr int kMultiSlice = 1024;
constexpr int kMultiGroupsMax = 8;
static_assert(kMultiSlice == kSliceLen && kMultiGroupsMax == kSliceGroupsMax, "tests/multi_cases.py is tabled for this geometry");
}  // namespace mi355

#if defined(MI355_MULTI_TU)   // an instantiation unit: the launch_multi of one value type, and nothing of what follows
namespace mi355 {
MI355_MULTI_EACH_SEMIRING(MI355_MULTI_DEFINE, MI355_MULTI_TU)
}  // namespace mi355
#elif defined(MI355_MULTI_HALF_TU)   // ... or every launch_multi_half
namespace mi355 {
MI355_MULTI_HALF_EACH(MI355_MULTI_HALF_DEFINE)
}  // namespace mi355
#elif defined(MI355_MULTI_PERM_TU)   // ... or the launch_multi_perm of one value type (multi_perm_f32.hip, multi_perm_f64.hip)
namespace mi355 {
MI355_MULTI_PERM_EACH(MI355_MULTI_PERM_DEFINE, MI355_MULTI_PERM_TU)
}  // namespace mi355
#else

using namespace mi355;

struct mi355_spmv_multi {   // the opaque handle of include/mi355_spmv.h
    int off_type = 0;
    int val_type = 0;               // the type of X and Y: F32 / F64 / I32 (and of all arithmetic), or F16 / BF16 (fp32 arithmetic)
    int mat_type = 0;               // = val_type, or MI355_VAL_PATTERN (no stored values: Ax is ignored); F32 under F16 / BF16
    int semiring = MI355_SEMIRING_PLUS_TIMES;
    int32_t n_cols = 0, k_max = 0;
    MultiShape shape;               // what an execute reads (multi_kernels.hpp)
    void* scratch = nullptr;        // carry_row, then carry_val (16-bit vectors: carry_val, tail_val, then carry_row)
    size_t scratch_bytes = 0;
    // a permuted object (multi_attach_perm): shape.perm, and
    bool permuted = false;
    int64_t n_values = 0;           // values of the Ax of an execute (a plain object: nnz)
    void* held = nullptr;           // the object's copy of perm; a transposed object's perm, Aj and Ap
    size_t held_bytes = 0;
    bool owns_structure = false;    // shape.Ap / shape.Aj lie in `held`
};

namespace {

int widest_tile(int val_type) { return val_type == MI355_VAL_F64 ? 16 : is_half_matrix(val_type) ? 64 : 32; }
bool known_semiring(int semiring) { return semiring >= 0 && semiring < MI355_SEMIRING_COUNT; }

// argument-only checks of an execute (also run by the one-shots before they create anything); a pattern object has no Ax
int check_execute_args(const char* who, bool pattern, int32_t n_rows, int64_t nnz, int32_t k_max, const void* Ax, const void* X,
                       int64_t ldx, const void* Y, int64_t ldy, int32_t k) {
    if (k < 1 || k > k_max) { set_error("%s: k = %d outside 1 .. k_max = %d", who, k, k_max); return MI355_SPMV_EINVAL; }
    if (ldx < k || ldy < k) { set_error("%s: leading dimension below k (ldx %lld, ldy %lld, k %d)", who, (long long)ldx, (long long)ldy, k); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && ((!pattern && !Ax) || !X)) { set_error("%s: null Ax or X", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !Y) { set_error("%s: null Y", who); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

// mi355_spmv_multi_create: fp32 / fp64 valued matrices, as before the typed entry point existed
int check_plain_type(int val_type) {
    if (val_type == MI355_VAL_I32 || val_type == MI355_VAL_PATTERN) {
        set_error("multi_create: integer and pattern matrices are made by mi355_spmv_multi_create_typed (fp32 / fp64 here)");
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) { set_error("multi_create: unknown value type %d", val_type); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

// mi355_spmv_multi_create_typed: vec_type in {F32, F64, I32}; mat_type = vec_type or PATTERN
int check_typed_types(int mat_type, int vec_type) {
    if (vec_type != MI355_VAL_F32 && vec_type != MI355_VAL_F64 && vec_type != MI355_VAL_I32) {
        set_error("multi_create_typed: vec_type %d is not a type of X and Y (F32, F64 or I32)", vec_type);
        return MI355_SPMV_EINVAL;
    }
    if (mat_type < MI355_VAL_F32 || mat_type > MI355_VAL_BF16) { set_error("multi_create_typed: unknown matrix type %d", mat_type); return MI355_SPMV_EINVAL; }
    if (mat_type != vec_type && mat_type != MI355_VAL_PATTERN) {
        set_error("multi_create_typed: matrix type %d under vector type %d is not built (mixed precision and 16-bit matrices: "
                  "mat_type is vec_type or MI355_VAL_PATTERN)", mat_type, vec_type);
        return MI355_SPMV_ENOTSUP;
    }
    return MI355_SPMV_OK;
}

// mi355_spmv_multi_create_half: vec_type in {F16, BF16}; mat_type = vec_type or F32
int check_half_types(int mat_type, int vec_type) {
    if (!is_half_matrix(vec_type)) {
        set_error("multi_create_half: vec_type %d is not a 16-bit type of X and Y (F16 or BF16)", vec_type);
        return MI355_SPMV_EINVAL;
    }
    if (mat_type < MI355_VAL_F32 || mat_type > MI355_VAL_BF16) { set_error("multi_create_half: unknown matrix type %d", mat_type); return MI355_SPMV_EINVAL; }
    if (mat_type != vec_type && mat_type != MI355_VAL_F32) {
        set_error("multi_create_half: matrix type %d under vector type %d is not built (mat_type is vec_type or MI355_VAL_F32)",
                  mat_type, vec_type);
        return MI355_SPMV_ENOTSUP;
    }
    return MI355_SPMV_OK;
}

int check_create_args(const char* who, int off_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                      int32_t k_max) {
    // k_max is reported behind a negative size and in front of every other structure check, as it always was
    if (n_rows >= 0 && n_cols >= 0 && nnz >= 0 && (k_max < 1 || k_max > (1 << 20))) {
        set_error("%s: k_max = %d outside 1 .. 2^20", who, k_max);
        return MI355_SPMV_EINVAL;
    }
    return check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj);
}

enum CreateHow { kPlain = 0, kTyped = 1, kHalf = 2 };   // mi355_spmv_multi_create, _create_typed, _create_half

// every argument-only check of a create
int check_create(const char* who, CreateHow how, int off_type, int mat_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                 const void* Ap, const int32_t* Aj, int32_t k_max) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown offset type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (const int st = how == kHalf    ? check_half_types(mat_type, vec_type)
                       : how == kTyped ? check_typed_types(mat_type, vec_type)
                                       : check_plain_type(vec_type))
        return st;
    return check_create_args(who, off_type, n_rows, n_cols, nnz, Ap, Aj, k_max);
}

// the object of checked arguments: the slices and their carries (the only device call of a create: one hipMalloc)
int make_object(const char* who, mi355_spmv_multi** out, int off_type, int mat_type, int vec_type, int32_t n_rows, int32_t n_cols,
                int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max) {
    mi355_spmv_multi* m = new (std::nothrow) mi355_spmv_multi();
    if (!m) { set_error("%s: host allocation failed", who); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = vec_type; m->mat_type = mat_type;
    m->n_cols = n_cols; m->k_max = k_max;
    MultiShape& sh = m->shape;
    sh.n_rows = n_rows; sh.nnz = nnz; sh.Ap = Ap; sh.Aj = Aj;
    sh.n_slices = slice_count(n_rows, nnz);
    const int widest = widest_tile(vec_type);
    sh.carry_ld = int64_t(k_max + widest - 1) / widest * widest;
    if (sh.n_slices > 0) {
        const bool half = is_half_matrix(vec_type);     // fp32 carries and tails (carry_ld * 4 is a multiple of 256), then the rows
        const size_t val_bytes = vec_type == MI355_VAL_F64 ? 8 : 4;
        const size_t rows_bytes = half ? size_t(sh.n_slices) * sizeof(int32_t) : (size_t(sh.n_slices) * sizeof(int32_t) + 255) / 256 * 256;
        const size_t vals_bytes = size_t(sh.n_slices) * size_t(sh.carry_ld) * val_bytes;
        m->scratch_bytes = rows_bytes + (half ? 2 : 1) * vals_bytes;
        const hipError_t e = hipMalloc(&m->scratch, m->scratch_bytes);
        if (e != hipSuccess) {
            set_error("%s: hipMalloc(%zu) -> %s", who, m->scratch_bytes, hipGetErrorString(e));
            delete m;
            return e == hipErrorOutOfMemory ? MI355_SPMV_ENOMEM : MI355_SPMV_EHIP;
        }
        if (half) {
            sh.carry_val = m->scratch;
            sh.tail_val = static_cast<char*>(m->scratch) + vals_bytes;
            sh.carry_row = reinterpret_cast<int32_t*>(static_cast<char*>(m->scratch) + 2 * vals_bytes);
        } else {
            sh.carry_row = static_cast<int32_t*>(m->scratch);
            sh.carry_val = static_cast<char*>(m->scratch) + rows_bytes;
        }
    }
    *out = m;
    return MI355_SPMV_OK;
}

// the object's run-time choices as template arguments: the semiring, then valued / pattern
template <typename off_t, typename val_t, int SRI>
int launch_semiring(const mi355_spmv_multi& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    return m.mat_type == MI355_VAL_PATTERN ? launch_multi<off_t, val_t, SRI, true>(m.shape, Ax, X, ldx, Y, ldy, k, s)
                                           : launch_multi<off_t, val_t, SRI, false>(m.shape, Ax, X, ldx, Y, ldy, k, s);
}

template <typename off_t, typename val_t>
int launch_typed(const mi355_spmv_multi& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    switch (m.semiring) {
        case MI355_SEMIRING_PLUS_TIMES: return launch_semiring<off_t, val_t, MI355_SEMIRING_PLUS_TIMES>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_SEMIRING_MIN_PLUS: return launch_semiring<off_t, val_t, MI355_SEMIRING_MIN_PLUS>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_SEMIRING_MAX_TIMES: return launch_semiring<off_t, val_t, MI355_SEMIRING_MAX_TIMES>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_SEMIRING_MAX_PLUS: return launch_semiring<off_t, val_t, MI355_SEMIRING_MAX_PLUS>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_SEMIRING_OR_AND: return launch_semiring<off_t, val_t, MI355_SEMIRING_OR_AND>(m, Ax, X, ldx, Y, ldy, k, s);
    }
    set_error("multi_execute: unknown semiring %d", m.semiring);
    return MI355_SPMV_EINVAL;
}

// 16-bit vectors: (+, *) only, the matrix in the vectors' type or in fp32
template <typename off_t, typename vec_t>
int launch_half(const mi355_spmv_multi& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    return m.mat_type == MI355_VAL_F32 ? launch_multi_half<off_t, vec_t, float>(m.shape, Ax, X, ldx, Y, ldy, k, s)
                                       : launch_multi_half<off_t, vec_t, vec_t>(m.shape, Ax, X, ldx, Y, ldy, k, s);
}

template <typename off_t>
int launch_offsets(const mi355_spmv_multi& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    if (m.permuted)     // fp32 / fp64 under (+, *): multi_attach_perm and set_semiring see to it
        return m.val_type == MI355_VAL_F64 ? launch_multi_perm<off_t, double>(m.shape, Ax, X, ldx, Y, ldy, k, s)
                                           : launch_multi_perm<off_t, float>(m.shape, Ax, X, ldx, Y, ldy, k, s);
    switch (m.val_type) {
        case MI355_VAL_F16: return launch_half<off_t, mh::F16>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_VAL_BF16: return launch_half<off_t, Bf16>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_VAL_F32: return launch_typed<off_t, float>(m, Ax, X, ldx, Y, ldy, k, s);
        case MI355_VAL_F64: return launch_typed<off_t, double>(m, Ax, X, ldx, Y, ldy, k, s);
        default: return launch_typed<off_t, int32_t>(m, Ax, X, ldx, Y, ldy, k, s);
    }
}

int passes_for(int val_type, int32_t k) { return (k + widest_tile(val_type) - 1) / widest_tile(val_type); }

// create (k_max = k), set the semiring, execute, synchronise, destroy; every argument check comes before any device call
int multi_one_shot(const char* who, CreateHow how, int off_type, int mat_type, int vec_type, int semiring, int32_t n_rows, int32_t n_cols,
                   int64_t nnz, const void* Ap, const int32_t* Aj, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy,
                   int32_t k, void* stream) {
    set_error("%s", "");
    if (!known_semiring(semiring)) { set_error("%s: unknown semiring %d", who, semiring); return MI355_SPMV_EINVAL; }
    int st = check_create(who, how, off_type, mat_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, k < 1 ? 1 : k);
    if (st == MI355_SPMV_OK) st = check_execute_args(who, mat_type == MI355_VAL_PATTERN, n_rows, nnz, k, Ax, X, ldx, Y, ldy, k);
    if (st != MI355_SPMV_OK) return st;
    mi355_spmv_multi* m = nullptr;
    st = make_object(who, &m, off_type, mat_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, k);
    if (st != MI355_SPMV_OK) return st;
    m->semiring = semiring;         // (alpha / beta are 1 / 0: every semiring may follow)
    st = mi355_spmv_multi_execute(m, Ax, X, ldx, Y, ldy, k, stream);
    if (st == MI355_SPMV_OK) st = mi355_spmv_stream_synchronize(stream);
    const int st2 = mi355_spmv_multi_destroy(m);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace

namespace mi355 {

int multi_attach_perm(mi355_spmv_multi* m, const uint32_t* perm, int64_t n_values, void* held, size_t held_bytes, bool owns_structure) {
    if (!m || m->permuted || n_values < 0 || (m->shape.nnz > 0 && !perm)) { set_error("multi_attach_perm: bad argument"); return MI355_SPMV_EINVAL; }
    if (m->mat_type != m->val_type || (m->val_type != MI355_VAL_F32 && m->val_type != MI355_VAL_F64) ||
        m->semiring != MI355_SEMIRING_PLUS_TIMES) {
        set_error("multi_attach_perm: a permuted object is fp32 or fp64 under (+, *)");
        return MI355_SPMV_ENOTSUP;
    }
    m->permuted = true;
    m->shape.perm = perm;
    m->n_values = n_values;
    m->held = held; m->held_bytes = held_bytes; m->owns_structure = owns_structure;
    return MI355_SPMV_OK;
}

const MultiShape& multi_shape_of(const mi355_spmv_multi* m) { return m->shape; }

}  // namespace mi355

extern "C" {

int mi355_spmv_multi_create(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                            const void* Ap, const int32_t* Aj, int32_t k_max) {
    set_error("%s", "");
    if (!out) { set_error("multi_create: null object pointer"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = check_create("multi_create", kPlain, off_type, val_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k_max)) return st;
    return make_object("multi_create", out, off_type, val_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k_max);
}

int mi355_spmv_multi_create_typed(mi355_spmv_multi** out, int off_type, int mat_type, int vec_type, int32_t n_rows, int32_t n_cols,
                                  int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max) {
    set_error("%s", "");
    if (!out) { set_error("multi_create_typed: null object pointer"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = check_create("multi_create_typed", kTyped, off_type, mat_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, k_max)) return st;
    return make_object("multi_create_typed", out, off_type, mat_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, k_max);
}

int mi355_spmv_multi_create_half(mi355_spmv_multi** out, int off_type, int mat_type, int vec_type, int32_t n_rows, int32_t n_cols,
                                 int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max) {
    set_error("%s", "");
    if (!out) { set_error("multi_create_half: null object pointer"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = check_create("multi_create_half", kHalf, off_type, mat_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, k_max)) return st;
    return make_object("multi_create_half", out, off_type, mat_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, k_max);
}

int mi355_spmv_multi_set_semiring(mi355_spmv_multi* m, int semiring) {
    set_error("%s", "");
    if (!m) { set_error("multi_set_semiring: null object"); return MI355_SPMV_EINVAL; }
    if (!known_semiring(semiring)) { set_error("multi_set_semiring: unknown semiring %d", semiring); return MI355_SPMV_EINVAL; }
    if (semiring != MI355_SEMIRING_PLUS_TIMES && is_half_matrix(m->val_type)) {
        set_error("multi_set_semiring: 16-bit vectors are built under the (+, *) semiring only");
        return MI355_SPMV_ENOTSUP;
    }
    if (semiring != MI355_SEMIRING_PLUS_TIMES && m->permuted) {
        set_error("multi_set_semiring: a permuted or transposed object is built under the (+, *) semiring only");
        return MI355_SPMV_ENOTSUP;
    }
    if (semiring != MI355_SEMIRING_PLUS_TIMES && (m->shape.alpha != 1.0 || m->shape.beta != 0.0)) {
        set_error("multi_set_semiring: alpha/beta are set; they are defined for (+, *) only");
        return MI355_SPMV_ENOTSUP;
    }
    m->semiring = semiring;         // the carries are sized by k_max and the value type alone: no scratch changes
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_set_alpha_beta(mi355_spmv_multi* m, double alpha, double beta) {
    set_error("%s", "");
    if (!m) { set_error("multi_set_alpha_beta: null object"); return MI355_SPMV_EINVAL; }
    if (m->semiring != MI355_SEMIRING_PLUS_TIMES && (alpha != 1.0 || beta != 0.0)) {
        set_error("multi_set_alpha_beta: scaling is defined for the (+, *) semiring only");
        return MI355_SPMV_ENOTSUP;
    }
    if (m->val_type == MI355_VAL_I32 && (alpha != 1.0 || beta != 0.0)) {
        set_error("multi_set_alpha_beta: not for integer values");
        return MI355_SPMV_ENOTSUP;
    }
    m->shape.alpha = alpha;
    m->shape.beta = beta;
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_get_types(const mi355_spmv_multi* m, int* mat_type, int* vec_type, int* semiring) {
    if (!m) { set_error("multi_get_types: null object"); return MI355_SPMV_EINVAL; }
    if (mat_type) *mat_type = m->mat_type;
    if (vec_type) *vec_type = m->val_type;
    if (semiring) *semiring = m->semiring;
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_execute(mi355_spmv_multi* m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k,
                             void* stream) {
    set_error("%s", "");
    if (!m) { set_error("multi_execute: null object"); return MI355_SPMV_EINVAL; }
    if (const int st = check_execute_args("multi_execute", m->mat_type == MI355_VAL_PATTERN, m->shape.n_rows, m->shape.nnz, m->k_max,
                                          Ax, X, ldx, Y, ldy, k))
        return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return m->off_type == MI355_OFF_I32 ? launch_offsets<int32_t>(*m, Ax, X, ldx, Y, ldy, k, s)
                                        : launch_offsets<int64_t>(*m, Ax, X, ldx, Y, ldy, k, s);
}

int mi355_spmv_multi_get_info(const mi355_spmv_multi* m, mi355_spmv_multi_info* info) {
    if (!m || !info) { set_error("multi_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type; info->k_max = m->k_max;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->widest_tile = widest_tile(m->val_type);
    info->passes = passes_for(m->val_type, m->k_max);
    info->n_kernels = info->passes + (m->shape.n_slices > 1 ? 1 : 0);
    info->n_slices = m->shape.n_slices;
    info->grid_blocks = slice_grid(m->shape.n_slices);
    info->scratch_bytes = int64_t(m->scratch_bytes);
    snprintf(info->main_kernel, sizeof(info->main_kernel), m->permuted                    ? "multi_perm_slice_kernel"
                                                           : is_half_matrix(m->val_type) ? "multi_half_slice_kernel"
                                                                                         : "multi_slice_kernel");
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_get_perm_info(const mi355_spmv_multi* m, int64_t* n_values, int64_t* held_bytes, int* owns_structure) {
    if (!m) { set_error("multi_get_perm_info: null object"); return MI355_SPMV_EINVAL; }
    if (n_values) *n_values = m->permuted ? m->n_values : m->shape.nnz;
    if (held_bytes) *held_bytes = int64_t(m->held_bytes);
    if (owns_structure) *owns_structure = m->owns_structure ? 1 : 0;
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_destroy(mi355_spmv_multi* m) {
    if (!m) return MI355_SPMV_OK;
    int st = MI355_SPMV_OK;
    if (m->scratch) {
        const hipError_t e = hipFree(m->scratch);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    if (m->held) {
        const hipError_t e = hipFree(m->held);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    delete m;
    return st;
}

#define MI355_SPMV_DEFINE_MULTI(SUF, OFF, OFFENUM, VAL, VALENUM)                                                       \
    int mi355_spmv_multi_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, const VAL* Ax, \
                               const VAL* X, int64_t ldx, VAL* Y, int64_t ldy, int32_t k, void* stream) {              \
        return multi_one_shot("multi", kPlain, OFFENUM, VALENUM, VALENUM, MI355_SEMIRING_PLUS_TIMES, n_rows, n_cols,    \
                              (int64_t)nnz, Ap, Aj, Ax, X, ldx, Y, ldy, k, stream);                                    \
    }
MI355_SPMV_DEFINE_MULTI(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_MULTI(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

// the same under a semiring, over the three value types; and with a PATTERN matrix (no Ax)
#define MI355_SPMV_DEFINE_MULTI_GENL(SUF, OFF, OFFENUM, VAL, VALENUM)                                                  \
    int mi355_spmv_multi_genl_##SUF(int semiring, int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, \
                                    const VAL* Ax, const VAL* X, int64_t ldx, VAL* Y, int64_t ldy, int32_t k, void* stream) { \
        return multi_one_shot("multi_genl", kTyped, OFFENUM, VALENUM, VALENUM, semiring, n_rows, n_cols, (int64_t)nnz, Ap, Aj, \
                              Ax, X, ldx, Y, ldy, k, stream);                                                          \
    }                                                                                                                  \
    int mi355_spmv_multi_pattern_##SUF(int semiring, int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap,           \
                                       const int32_t* Aj, const VAL* X, int64_t ldx, VAL* Y, int64_t ldy, int32_t k,   \
                                       void* stream) {                                                                 \
        return multi_one_shot("multi_pattern", kTyped, OFFENUM, MI355_VAL_PATTERN, VALENUM, semiring, n_rows, n_cols,    \
                              (int64_t)nnz, Ap, Aj, nullptr, X, ldx, Y, ldy, k, stream);                               \
    }
MI355_SPMV_DEFINE_MULTI_GENL(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI_GENL(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_MULTI_GENL(i32_i32, int32_t, MI355_OFF_I32, int32_t, MI355_VAL_I32)
MI355_SPMV_DEFINE_MULTI_GENL(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI_GENL(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_MULTI_GENL(i64_i32, int64_t, MI355_OFF_I64, int32_t, MI355_VAL_I32)

// 16-bit vectors with the matrix in their type, (+, *): the arguments of mi355_spmv_multi_<off>_<val>
#define MI355_SPMV_DEFINE_MULTI_HALF(SUF, OFF, OFFENUM, VALENUM)                                                       \
    int mi355_spmv_multi_half_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, const void* Ax, \
                                    const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream) {       \
        return multi_one_shot("multi_half", kHalf, OFFENUM, VALENUM, VALENUM, MI355_SEMIRING_PLUS_TIMES, n_rows, n_cols, \
                              (int64_t)nnz, Ap, Aj, Ax, X, ldx, Y, ldy, k, stream);                                    \
    }
MI355_SPMV_DEFINE_MULTI_HALF(i32_f16, int32_t, MI355_OFF_I32, MI355_VAL_F16)
MI355_SPMV_DEFINE_MULTI_HALF(i32_bf16, int32_t, MI355_OFF_I32, MI355_VAL_BF16)
MI355_SPMV_DEFINE_MULTI_HALF(i64_f16, int64_t, MI355_OFF_I64, MI355_VAL_F16)
MI355_SPMV_DEFINE_MULTI_HALF(i64_bf16, int64_t, MI355_OFF_I64, MI355_VAL_BF16)

}  // extern "C"

#endif  // MI355_MULTI_TU, MI355_MULTI_HALF_TU
