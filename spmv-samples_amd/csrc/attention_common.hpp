// attention_common.hpp — what the two directions of fused sparse attention share (attention.hip, attention_bwd.hip and their
// 16-bit kernels; DESIGN.md §3.15–§3.15.3): the device arithmetic helpers, the walk along the pieces of a line that crosses
// slices, the lane geometry of a storage type, the argument refusals of a create and of an execute, and the one loop that
// launches a slice kernel over the tiles of an output and then its fix-up.  Each entry point calls the checks in its own
// order: that order decides which message a caller with two mistakes sees.
#pragma once

#include "half_cols.hpp"
#include "slice_cut.hpp"

namespace mi355 {

#ifdef __clang__
#pragma clang fp contract(off)      // the units' reason: nothing that moves here may be fused into other arithmetic
#endif

__device__ __forceinline__ float attn_fma(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
__device__ __forceinline__ double attn_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }
__device__ __forceinline__ float attn_exp(float d) { return expf(d); }
__device__ __forceinline__ double attn_exp(double d) { return exp(d); }
__device__ __forceinline__ float attn_log(float d) { return logf(d); }
__device__ __forceinline__ double attn_log(double d) { return log(d); }

// The fix-up's walk, row[slice * 2 + piece] being the line of a slice's HEAD (0) or TAIL (1) piece, or -1.  If slice t is
// the first that carries a line, r is that line, first(piece) is called for t's TAIL and fold(piece) for the line's other
// pieces in slice order — the tails of the slices that follow, then the head of the slice it ends in; otherwise false.
template <typename First, typename Fold>
__device__ __forceinline__ bool attn_piece_chain(int64_t n_slices, const int32_t* row, int64_t t, int32_t& r, First first, Fold fold) {
    if (t >= n_slices) return false;
    r = row[t * 2 + 1];
    if (r < 0 || (t > 0 && row[(t - 1) * 2 + 1] == r)) return false;
    first(t * 2 + 1);
    int64_t u = t + 1;
    for (; u < n_slices && row[u * 2 + 1] == r; ++u) fold(u * 2 + 1);
    if (u < n_slices && row[u * 2 + 0] == r) fold(u * 2 + 0);
    return true;
}

// columns of a lane's 16 bytes of a row of the dense matrices, and the widest tile of an output
inline int attn_lane_cols(int vec_type) { return vec_type == MI355_VAL_F64 ? 2 : vec_type == MI355_VAL_F32 ? 4 : mh::kHalfV; }
inline int attn_widest(int vec_type) { return attn_lane_cols(vec_type) * kSliceGroupsMax; }

// the type refusals of a create: operands names the dense matrices, half_hint the create that takes them in 16 bits
inline int attn_check_types(const char* who, int off_type, int val_type, const char* operands, const char* half_hint) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown off_type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32) { set_error("%s: val_type MI355_VAL_I32 is not built (fp32 / fp64 values)", who); return MI355_SPMV_ENOTSUP; }
    if (val_type == MI355_VAL_F32 || val_type == MI355_VAL_F64) return MI355_SPMV_OK;
    set_error("%s: val_type %d is not a type of %s (F32 or F64; 16-bit operands: %s)", who, val_type, operands, half_hint);
    return MI355_SPMV_EINVAL;
}

inline int attn_check_half_type(const char* who, int vec_type, const char* operands) {
    if (vec_type == MI355_VAL_F16 || vec_type == MI355_VAL_BF16) return MI355_SPMV_OK;
    set_error("%s: vec_type %d is not a 16-bit type of %s (MI355_VAL_F16 or MI355_VAL_BF16)", who, vec_type, operands);
    return MI355_SPMV_EINVAL;
}

// the widths and leading dimensions of an execute, then (attn_check_inputs) its inputs that may not be null
inline int attn_check_widths(const char* who, int32_t d, int32_t dv, int32_t d_max, int32_t dv_max, int64_t ldq, int64_t ldk, int64_t ldv,
                             int64_t ldo) {
    if (d < 1) { set_error("%s: d = %d below 1", who, d); return MI355_SPMV_EINVAL; }
    if (dv < 1) { set_error("%s: dv = %d below 1", who, dv); return MI355_SPMV_EINVAL; }
    if (d > d_max) { set_error("%s: d = %d above d_max = %d", who, d, d_max); return MI355_SPMV_EINVAL; }
    if (dv > dv_max) { set_error("%s: dv = %d above dv_max = %d", who, dv, dv_max); return MI355_SPMV_EINVAL; }
    if (ldq < d) { set_error("%s: ldq = %lld below d = %d", who, (long long)ldq, d); return MI355_SPMV_EINVAL; }
    if (ldk < d) { set_error("%s: ldk = %lld below d = %d", who, (long long)ldk, d); return MI355_SPMV_EINVAL; }
    if (ldv < dv) { set_error("%s: ldv = %lld below dv = %d", who, (long long)ldv, dv); return MI355_SPMV_EINVAL; }
    if (ldo < dv) { set_error("%s: ldo = %lld below dv = %d", who, (long long)ldo, dv); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

inline int attn_check_inputs(const char* who, int32_t n_rows, int64_t nnz, const void* Q, const void* K, const void* V, const void* O) {
    if (nnz > 0 && !Q) { set_error("%s: null Q", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !K) { set_error("%s: null K", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !V) { set_error("%s: null V", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !O) { set_error("%s: null O", who); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

// The passes of a slice kernel over the tiles of an output of `width` columns (W per lane), then the fix-up when a line can
// cross slices: slice(grid, lanes) launches the kernel of lanes::value lanes per slot on a, whose col_begin and cols are
// this pass's tile, and fixup(grid) the fix-up of one thread per (slice, column).
template <int W, typename Args, typename Slice, typename Fixup>
int attn_tile_passes(Args& a, int32_t width, Slice slice, Fixup fixup) {
    constexpr int kWidest = W * kSliceGroupsMax;
    if (a.n_slices == 0) return MI355_SPMV_OK;      // no lines: nothing to write
    const dim3 grid(unsigned(slice_grid(a.n_slices)));
    for (int32_t cb = 0; cb < width; cb += kWidest) {
        a.col_begin = cb;
        a.cols = width - cb < kWidest ? width - cb : kWidest;
        with_slot_lanes((a.cols + W - 1) / W, [&](auto lanes) { slice(grid, lanes); });
        MI355_HIP_TRY(hipGetLastError());
    }
    if (a.n_slices > 1) {
        fixup(dim3(unsigned((a.n_slices * width + kBlock - 1) / kBlock)));
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

}  // namespace mi355
