// attention_common.hpp — what the two directions of fused sparse attention share (attention.hip, attention_bwd.hip and their
// 16-bit kernels; DESIGN.md §3.15–§3.15.3): the device arithmetic helpers, the walk along the pieces of a line that crosses
// slices, the lane geometry of a storage type, the argument refusals of a create and of an execute, and the one loop that
// launches a slice kernel over the tiles of an output and then its fix-up.  Each entry point calls the checks in its own
// order: that order decides which message a caller with two mistakes sees.
#pragma once

#include <utility>

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

// ---- heads in one call ------------------------------------------------------------------------------
// Head h of an operand begins h strides behind head 0, in the operand's own elements.  The kernels rebase their pointers
// in a local copy of their arguments; a null operand stays null (and null + 0 is never formed with an offset).
template <typename T>
__device__ __forceinline__ T* attn_head_ptr(T* p, int64_t head, int64_t stride) { return p ? p + head * stride : p; }
// the scratch of head h: the single-head layout at h * bytes
template <typename T>
__device__ __forceinline__ T* attn_head_scratch(T* p, int64_t head, int64_t bytes) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + head * bytes);
}

// the per-head size of a scratch of `bytes`: whole 16 bytes, so that every head's arrays are aligned as head 0's are
inline size_t attn_head_scratch_stride(size_t bytes) { return (bytes + 15) / 16 * 16; }
inline size_t attn_heads_scratch_bytes(size_t bytes, int32_t n_heads) {
    return bytes == 0 ? 0 : size_t(n_heads - 1) * attn_head_scratch_stride(bytes) + bytes;
}

// A row takes the 16-byte path only where every head's rows are aligned: rows_aligned16 of head 0 and a head stride of
// whole 16 bytes.  Both paths fill the same registers, so head h equals the single-head execute bit for bit either way.
template <typename T>
bool attn_rows_vec(const void* p, int64_t ld, int32_t n_heads, int64_t stride) {
    return rows_aligned16<T>(p, ld) && (n_heads == 1 || (size_t(stride) * sizeof(T)) % 16 == 0);
}

inline int attn_check_n_heads(const char* who, int32_t n_heads, int32_t n_heads_max, const void* hs) {
    if (n_heads < 1) { set_error("%s: n_heads = %d below 1", who, n_heads); return MI355_SPMV_EINVAL; }
    if (n_heads > n_heads_max) {
        set_error("%s: n_heads = %d above the reserved n_heads_max = %d (reserve_heads)", who, n_heads, n_heads_max);
        return MI355_SPMV_EINVAL;
    }
    if (n_heads > 1 && !hs) { set_error("%s: null head strides (hs) with n_heads = %d", who, n_heads); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

inline int attn_check_stride_sign(const char* who, const char* name, int64_t stride) {
    if (stride < 0) { set_error("%s: negative head stride %s = %lld", who, name, (long long)stride); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

// the heads of an output matrix of rows x width at leading dimension ld may not overlap: head-major or interleaved
inline int attn_check_out_stride(const char* who, const char* name, int32_t n_heads, int64_t stride, int64_t rows, int64_t width, int64_t ld) {
    if (rows <= 0) return MI355_SPMV_OK;
    // by division: no product of a caller's ld or stride is formed, so none can wrap (ld >= width >= 1 is execute's check)
    const bool head_major = stride >= width && (rows == 1 || (stride - width) / ld >= rows - 1);       // stride >= (rows - 1) ld + width
    const bool interleaved = stride >= width && (n_heads == 1 || (ld - width) / stride >= n_heads - 1);  // ld >= (n_heads - 1) stride + width
    if (head_major || interleaved) return MI355_SPMV_OK;
    set_error("%s: head stride %s = %lld lets the heads of the output overlap (%lld rows of %lld columns at leading dimension %lld, %d heads)", who,
              name, (long long)stride, (long long)rows, (long long)width, (long long)ld, n_heads);
    return MI355_SPMV_EINVAL;
}

// the heads of an output vector of n elements (lse, dbias)
inline int attn_check_out_vector_stride(const char* who, const char* name, int64_t stride, int64_t n, const char* n_name) {
    if (stride >= n) return MI355_SPMV_OK;
    set_error("%s: head stride %s = %lld below %s = %lld (the heads of the output overlap)", who, name, (long long)stride, n_name, (long long)n);
    return MI355_SPMV_EINVAL;
}

// reserve_heads of both directions: a scratch of `bytes` in place of *scratch (allocated first: on failure the object keeps
// what it has), the old one freed; *fresh is set once the object holds the new scratch.  No bytes (no rows): no device call.
inline int attn_reserve_scratch(const char* who, void** scratch, size_t bytes, void** fresh) {
    if (bytes == 0) return MI355_SPMV_OK;
    hipError_t e = hipMalloc(fresh, bytes);
    if (e != hipSuccess) {
        set_error("%s: hipMalloc(%zu) -> %s", who, bytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MI355_SPMV_ENOMEM : MI355_SPMV_EHIP;
    }
    void* old = *scratch;
    *scratch = *fresh;
    if (old) {
        e = hipFree(old);
        if (e != hipSuccess) { set_error("%s: hipFree -> %s", who, hipGetErrorString(e)); return MI355_SPMV_EHIP; }
    }
    return MI355_SPMV_OK;
}

// The fix-up and delta kernels give every head whole workgroups, the head slowest: workgroup b serves head b / per_head and
// is workgroup b % per_head of that head's threads — one scalar division per workgroup, and a thread's own index
// arithmetic is what it was with one head.
inline int64_t attn_blocks_per_head(int64_t threads) { return (threads + kBlock - 1) / kBlock; }
__device__ __forceinline__ int64_t attn_head_thread(unsigned per_head, unsigned& head) {
    head = blockIdx.x / per_head;
    return int64_t(blockIdx.x % per_head) * kBlock + threadIdx.x;
}

// the grids of n_heads heads over n_slices slices and an output of `width` columns: the slice kernel's and the fix-up's
inline int attn_check_heads_grid(const char* who, int32_t n_heads, int64_t n_slices, int64_t width) {
    constexpr int64_t kGridMax = int64_t(1) << 31;
    const int64_t slice_blocks = slice_grid(n_slices) * n_heads;
    const int64_t fixup_blocks = n_slices > 1 ? attn_blocks_per_head(n_slices * width) * n_heads : 0;
    if (slice_blocks < kGridMax && fixup_blocks < kGridMax) return MI355_SPMV_OK;
    set_error("%s: n_heads = %d makes a grid of 2^31 workgroups or more (%lld slices, %lld columns)", who, n_heads, (long long)n_slices,
              (long long)width);
    return MI355_SPMV_ENOTSUP;
}

// The passes of a slice kernel over the tiles of an output of `width` columns (W per lane), then the fix-up when a line can
// cross slices: slice(grid, lanes) launches the kernel of lanes::value lanes per slot on a, whose col_begin and cols are
// this pass's tile, and fixup(grid) the fix-up of one thread per (head, slice, column).  a.n_heads heads share each launch.
template <int W, typename Args, typename Slice, typename Fixup>
int attn_tile_passes(Args& a, int32_t width, Slice slice, Fixup fixup) {
    constexpr int kWidest = W * kSliceGroupsMax;
    if (a.n_slices == 0) return MI355_SPMV_OK;      // no lines: nothing to write
    const dim3 grid(unsigned(slice_grid(a.n_slices) * a.n_heads));     // workgroup b: head b % n_heads, slice block b / n_heads
    for (int32_t cb = 0; cb < width; cb += kWidest) {
        a.col_begin = cb;
        a.cols = width - cb < kWidest ? width - cb : kWidest;
        with_slot_lanes((a.cols + W - 1) / W, [&](auto lanes) { slice(grid, lanes); });
        MI355_HIP_TRY(hipGetLastError());
    }
    if (a.n_slices > 1) {
        fixup(dim3(unsigned(attn_blocks_per_head(a.n_slices * width) * a.n_heads)));
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

}  // namespace mi355
