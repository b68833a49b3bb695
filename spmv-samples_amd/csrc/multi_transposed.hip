// multi_transposed.hip — mi355_spmv_multi_create_transposed and its one-shots: Y = alpha * A^T X + beta * Y for k vectors,
// composed of the two layers below it: mi355_spmv_csr_transpose (coo_csr.hip) makes the structure of A^T
// and the slot map once, at create; the object is a permuted multi-vector object (multi.hip, multi_attach_perm) on that
// structure, whose executes read the caller's Ax — in A's CSR order — through the map.  No device code of its own.
#include "multi_kernels.hpp"

using namespace mi355;

namespace {

// every argument-only check of a create, in the order of mi355_spmv_multi_create's
int check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                 int32_t k_max) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown offset type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32 || val_type == MI355_VAL_PATTERN || is_half_matrix(val_type)) {
        set_error("%s: fp32 and fp64 values only (a pattern transpose is mi355_spmv_csr_transpose and mi355_spmv_multi_create_typed)", who);
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) { set_error("%s: unknown value type %d", who, val_type); return MI355_SPMV_EINVAL; }
    if (n_rows >= 0 && n_cols >= 0 && nnz >= 0 && (k_max < 1 || k_max > (1 << 20))) {
        set_error("%s: k_max = %d outside 1 .. 2^20", who, k_max);
        return MI355_SPMV_EINVAL;
    }
    if (const int st = check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    if (uint64_t(nnz) >= (1ull << 32)) { set_error("%s: 2^32 or more entries (the slot map is 32-bit)", who); return MI355_SPMV_ENOTSUP; }
    return MI355_SPMV_OK;
}

// the object of checked arguments: perm, Ajt, Apt in one allocation that the object owns, then the permuted object on them
int make_transposed(const char* who, mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                    const void* Ap, const int32_t* Aj, int32_t k_max, hipStream_t s) {
    const size_t ob = off_type == MI355_OFF_I64 ? 8 : 4;
    const size_t held_bytes = size_t(nnz) * 8 + (size_t(n_cols) + 1) * ob;   // 8 nnz is a multiple of 8: Apt is aligned
    size_t ws_bytes = 0;
    if (const int st = mi355_spmv_csr_transpose(off_type, n_rows, n_cols, nnz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ws_bytes, nullptr))
        return st;
    char* held = nullptr;
    void* ws = nullptr;
    MI355_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&held), held_bytes));
    hipError_t e = hipMalloc(&ws, ws_bytes);
    if (e != hipSuccess) {
        (void)hipFree(held);
        set_error("%s: hipMalloc(%zu) -> %s", who, ws_bytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MI355_SPMV_ENOMEM : MI355_SPMV_EHIP;
    }
    uint32_t* perm = reinterpret_cast<uint32_t*>(held);
    int32_t* Ajt = reinterpret_cast<int32_t*>(held + size_t(nnz) * 4);
    void* Apt = held + size_t(nnz) * 8;
    int st = mi355_spmv_csr_transpose(off_type, n_rows, n_cols, nnz, Ap, Aj, Apt, Ajt, perm, ws, &ws_bytes, s);   // synchronises s
    e = hipFree(ws);
    if (st == MI355_SPMV_OK && e != hipSuccess) { set_error("%s: hipFree -> %s", who, hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    mi355_spmv_multi* m = nullptr;
    if (st == MI355_SPMV_OK) st = mi355_spmv_multi_create(&m, off_type, val_type, n_cols, n_rows, nnz, Apt, Ajt, k_max);
    if (st == MI355_SPMV_OK) {
        st = multi_attach_perm(m, perm, nnz, held, held_bytes, true);
        if (st != MI355_SPMV_OK) (void)mi355_spmv_multi_destroy(m);
    }
    if (st != MI355_SPMV_OK) { (void)hipFree(held); return st; }
    *out = m;
    return MI355_SPMV_OK;
}

// create (k_max = k), execute, synchronise, destroy; every argument check comes before any device call
int transposed_one_shot(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                        const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream) {
    const char* const who = "multi_transposed";
    set_error("%s", "");
    int st = check_create(who, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k < 1 ? 1 : k);
    if (st != MI355_SPMV_OK) return st;
    if (k < 1) { set_error("%s: k = %d below 1", who, k); return MI355_SPMV_EINVAL; }
    if (ldx < k || ldy < k) { set_error("%s: leading dimension below k (ldx %lld, ldy %lld, k %d)", who, (long long)ldx, (long long)ldy, k); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && (!Ax || !X)) { set_error("%s: null Ax or X", who); return MI355_SPMV_EINVAL; }
    if (n_cols > 0 && !Y) { set_error("%s: null Y", who); return MI355_SPMV_EINVAL; }
    mi355_spmv_multi* m = nullptr;
    st = make_transposed(who, &m, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k, static_cast<hipStream_t>(stream));
    if (st != MI355_SPMV_OK) return st;
    st = mi355_spmv_multi_execute(m, Ax, X, ldx, Y, ldy, k, stream);
    if (st == MI355_SPMV_OK) st = mi355_spmv_stream_synchronize(stream);
    const int st2 = mi355_spmv_multi_destroy(m);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace

extern "C" {

int mi355_spmv_multi_create_transposed(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                       const void* Ap, const int32_t* Aj, int32_t k_max, void* stream) {
    set_error("%s", "");
    if (!out) { set_error("multi_create_transposed: null object pointer"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = check_create("multi_create_transposed", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k_max)) return st;
    return make_transposed("multi_create_transposed", out, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k_max, static_cast<hipStream_t>(stream));
}

#define MI355_SPMV_DEFINE_MULTI_TRANSPOSED(SUF, OFF, OFFENUM, VAL, VALENUM)                                            \
    int mi355_spmv_multi_transposed_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj,   \
                                          const VAL* Ax, const VAL* X, int64_t ldx, VAL* Y, int64_t ldy, int32_t k,    \
                                          void* stream) {                                                              \
        return transposed_one_shot(OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, Ax, X, ldx, Y, ldy, k, stream); \
    }
MI355_SPMV_DEFINE_MULTI_TRANSPOSED(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI_TRANSPOSED(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_MULTI_TRANSPOSED(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI_TRANSPOSED(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

}  // extern "C"
