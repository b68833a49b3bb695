// multi_perm.hip — mi355_spmv_multi_create_permuted: a multi-vector object (multi.hip) whose matrix values are read
// through a permutation, Ax[perm[n]].  This unit checks the caller's perm on the device, keeps a 4-byte
// copy of it and hands it to the object (multi_attach_perm, multi_kernels.hpp); the object, its kernels and its execute
// are multi.hip's.  A unit of its own because it copies between device and host, which multi.hip never does.
#include "multi_kernels.hpp"

namespace mi355 {
namespace {

constexpr unsigned long long kPermOk = ~0ull;

// out[i] = perm[i] in 4 bytes; *bad = the first i whose index is outside [0, n_values) (a negative one is: it is
// compared unsigned).  An index that fails is not written: out is only used when *bad stays kPermOk.
template <typename idx_t>
__global__ void __launch_bounds__(kBlock) perm_narrow(const idx_t* __restrict__ perm, uint64_t nnz, uint64_t n_values,
                                                      uint32_t* __restrict__ out, unsigned long long* bad) {
    using u_t = typename std::make_unsigned<idx_t>::type;
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < nnz; i += stride) {
        const uint64_t p = uint64_t(u_t(perm[i]));
        if (p >= n_values) atomicMin(bad, (unsigned long long)i);
        else out[i] = uint32_t(p);
    }
}

// the checked copy of perm: *copy is device memory of 4 * nnz bytes, or an error with nothing left allocated
template <typename idx_t>
int copy_checked(const idx_t* perm, int64_t nnz, int64_t n_values, uint32_t** copy, hipStream_t s) {
    *copy = nullptr;
    char* mem = nullptr;        // the copy, then the validation word
    const size_t copy_bytes = (size_t(nnz) * 4 + 255) / 256 * 256;
    MI355_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&mem), copy_bytes + 256));
    auto* bad = reinterpret_cast<unsigned long long*>(mem + copy_bytes);
    unsigned long long first_bad = kPermOk;
    long long value = 0;
    const int st = [&]() -> int {
        MI355_HIP_TRY(hipMemsetAsync(bad, 0xff, sizeof(*bad), s));
        const uint64_t blocks = (uint64_t(nnz) + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(perm_narrow<idx_t>, dim3(unsigned(blocks < 8192 ? blocks : 8192)), dim3(kBlock), 0, s, perm, uint64_t(nnz),
                           uint64_t(n_values), reinterpret_cast<uint32_t*>(mem), bad);
        MI355_HIP_TRY(hipGetLastError());
        MI355_HIP_TRY(hipMemcpyAsync(&first_bad, bad, sizeof(first_bad), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if (first_bad != kPermOk) {
            idx_t v = 0;
            MI355_HIP_TRY(hipMemcpy(&v, perm + first_bad, sizeof(v), hipMemcpyDeviceToHost));
            value = (long long)v;
        }
        return MI355_SPMV_OK;
    }();
    if (st != MI355_SPMV_OK || first_bad != kPermOk) {
        (void)hipFree(mem);
        if (st != MI355_SPMV_OK) return st;
        set_error("multi_create_permuted: perm[%llu] = %lld is outside the %lld values of Ax", first_bad, value, (long long)n_values);
        return MI355_SPMV_EINVAL;
    }
    *copy = reinterpret_cast<uint32_t*>(mem);
    return MI355_SPMV_OK;
}

}  // namespace
}  // namespace mi355

using namespace mi355;

extern "C" int mi355_spmv_multi_create_permuted(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                                int64_t nnz, const void* Ap, const int32_t* Aj, int perm_type, const void* perm,
                                                int64_t n_values, int32_t k_max, void* stream) {
    const char* const fn = "multi_create_permuted";
    set_error("%s", "");
    if (!out) { set_error("%s: null object pointer", fn); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (val_type == MI355_VAL_I32 || val_type == MI355_VAL_PATTERN || is_half_matrix(val_type)) {
        set_error("%s: fp32 and fp64 values only (a pattern matrix needs no permutation: mi355_spmv_multi_create_typed)", fn);
        return MI355_SPMV_ENOTSUP;
    }
    if (perm_type != MI355_OFF_I32 && perm_type != MI355_OFF_I64) { set_error("%s: unknown perm_type %d", fn, perm_type); return MI355_SPMV_EINVAL; }
    if (n_values < 0) { set_error("%s: negative n_values", fn); return MI355_SPMV_EINVAL; }
    if (uint64_t(n_values) >= (1ull << 32)) { set_error("%s: 2^32 or more values (the object keeps 4-byte indices)", fn); return MI355_SPMV_ENOTSUP; }
    if (nnz > 0 && !perm) { set_error("%s: null perm", fn); return MI355_SPMV_EINVAL; }
    // the type, size, pointer and k_max checks of a plain object, then its slices and carries
    mi355_spmv_multi* m = nullptr;
    int st = mi355_spmv_multi_create(&m, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k_max);
    if (st != MI355_SPMV_OK) return st;
    uint32_t* copy = nullptr;
    if (nnz > 0) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        st = perm_type == MI355_OFF_I32 ? copy_checked(static_cast<const int32_t*>(perm), nnz, n_values, &copy, s)
                                        : copy_checked(static_cast<const int64_t*>(perm), nnz, n_values, &copy, s);
    }
    if (st == MI355_SPMV_OK) {
        st = multi_attach_perm(m, copy, n_values, copy, size_t(nnz) * 4, false);
        if (st != MI355_SPMV_OK && copy) (void)hipFree(copy);
    }
    if (st != MI355_SPMV_OK) {
        (void)mi355_spmv_multi_destroy(m);      // (leaves the failure's text: it only reports a failure of its own)
        return st;
    }
    *out = m;
    return MI355_SPMV_OK;
}

// the object's Ap, Aj and perm copied to the caller's device arrays ((rows + 1) offsets, nnz int32, nnz 4-byte indices; any
// of the three may be null), asynchronously on `stream`: for a transposed object, the CSR of A^T
extern "C" int mi355_spmv_multi_copy_structure(const mi355_spmv_multi* multi, void* Ap, int32_t* Aj, uint32_t* perm, void* stream) {
    set_error("%s", "");
    if (!multi) { set_error("multi_copy_structure: null object"); return MI355_SPMV_EINVAL; }
    const MultiShape& sh = multi_shape_of(multi);
    mi355_spmv_multi_info info;
    if (const int st = mi355_spmv_multi_get_info(multi, &info)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t ob = info.off_type == MI355_OFF_I64 ? 8 : 4;
    if (Ap && sh.Ap) MI355_HIP_TRY(hipMemcpyAsync(Ap, sh.Ap, (size_t(sh.n_rows) + 1) * ob, hipMemcpyDeviceToDevice, s));
    if (sh.nnz > 0 && Aj) MI355_HIP_TRY(hipMemcpyAsync(Aj, sh.Aj, size_t(sh.nnz) * 4, hipMemcpyDeviceToDevice, s));
    if (sh.nnz > 0 && perm) {
        if (!sh.perm) { set_error("multi_copy_structure: the object has no permutation"); return MI355_SPMV_EINVAL; }
        MI355_HIP_TRY(hipMemcpyAsync(perm, sh.perm, size_t(sh.nnz) * 4, hipMemcpyDeviceToDevice, s));
    }
    return MI355_SPMV_OK;
}
