// multi_half_kernels.hpp — multi-vector SpMV with X and Y stored in 16 bits (MI355_VAL_F16 / MI355_VAL_BF16) and fp32
// arithmetic (mi355_spmv_multi_create_half).  The slice walk is multi_kernels.hpp's own
// (multi_slice_walk), under the policy below; this header holds what 16-bit vectors add to it: their loads and stores, the
// policy, the fix-up, and the slice kernel that wraps the walk.  The kernels are kernels of their own, with a name and an
// argument struct of their own, because a storage type among multi_slice_kernel's template arguments would rename every
// one of the fp32 / fp64 / int32 kernels that are on record (profiles/); what a kernel calls does not enter its name.
//
// What the policy says differently from the typed kernels':
//   - a lane's 16 bytes are EIGHT columns: V = 8 with fp32 acc / p, tiles of 8 / 16 / 32 / 64 columns for C = 1 / 2 / 4 / 8
//   - every stored 16-bit value is widened exactly to fp32; products and sums are fp32, (+, *) only; Ax (vec_t or float)
//     is loaded as stored, one per lane, and widened in front of the shuffle
//   - Y is rounded to the 16-bit type ONCE per row: out = alpha * S, + beta * float(Yold) when beta != 0, then nearest
//     even (overflow to +-inf, NaN stays NaN).  A row that crosses slices is therefore never written by a slice: the
//     slices it runs through leave fp32 carries, the slice that holds its last nonzero leaves the row's fp32 partial in
//     its TAIL (tail_val[slice][carry_ld]), and the fix-up thread of the row adds the carries in slice order, then the
//     tail, reads Yold only when beta != 0 and stores the rounded row.  It is the row's only writer.
//   - every execute rewrites carry_row of every slice, and the carry / tail of every slice that has one, for the k
//     columns of the execute: the fix-up reads nothing that an earlier (wider) execute left.
// The conversions: half_convert.hpp; the widening load and the narrowing store of a lane's eight columns (mh::load_cols,
// mh::store_cols, U32x4, kHalfV): half_cols.hpp, shared with SDDMM's and fused attention's 16-bit kernels.
#pragma once

#include "half_cols.hpp"
#include "multi_kernels.hpp"

namespace mi355 {
namespace mh {

using mi355::F16;           // (binary16 as multi.hip names it)

template <typename vec_t, typename mat_t>
struct MultiHalfArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const mat_t* Ax;
    const vec_t* X;
    vec_t* Y;
    int64_t ldx, ldy;
    int32_t col_begin;      // first column of this pass's tile
    int32_t cols;           // columns of it that exist (<= tile width): the others are masked on load and store
    int32_t x_vec, y_vec;   // 1 = rows of X / Y are 16-byte aligned: one 16-byte access per lane
    float alpha, beta;
    int32_t* carry_row;     // [n_slices]: the row a slice leaves unfinished, or -1
    float* carry_val;       // [n_slices][carry_ld]
    float* tail_val;        // [n_slices][carry_ld]: the partial of the slice's first row, when that row began earlier and ends here
    int64_t carry_ld;
};

// Y[r, tile] = round(alpha * sum + beta * float(Y[r, tile])), Y read only when beta != 0: the one rounding of the row
template <typename vec_t>
__device__ __forceinline__ void store_row(vec_t* Y, int64_t ldy, int col_begin, int cols, bool vec, float alpha, float beta,
                                          int64_t r, int c, const float (&sum)[kHalfV]) {
    const int nv = min(max(cols - c * kHalfV, 0), kHalfV);
    if (nv == 0) return;
    vec_t* yp = Y + r * ldy + col_begin + c * kHalfV;
    float out[kHalfV];
#pragma unroll
    for (int j = 0; j < kHalfV; ++j) out[j] = alpha * sum[j];
    if (beta != 0.0f) {
        float old[kHalfV];
        load_cols<vec_t>(old, yp, nv, vec);
#pragma unroll
        for (int j = 0; j < kHalfV; ++j) out[j] += beta * old[j];
    }
    store_cols<vec_t>(out, yp, nv, vec);
}

// multi_slice_walk's policy (multi_kernels.hpp) for 16-bit vectors
template <typename vec_t, typename mat_t>
struct MultiHalfPolicy {
    using acc_t = float;
    using SR = Semiring<MI355_SEMIRING_PLUS_TIMES, float>;
    using Args = MultiHalfArgs<vec_t, mat_t>;
    static constexpr int V = kHalfV;
    static constexpr bool kValued = true, kMaskCombine = false, kTails = true, kPermuted = false;
    __device__ static __forceinline__ float ax(mat_t v) { return widen(v); }
    __device__ static __forceinline__ void load_cols(float (&v)[V], const vec_t* p, int nv, bool vec) { mh::load_cols<vec_t>(v, p, nv, vec); }
    static constexpr bool kFields = true;
    static constexpr float kAxFill = 0.0f;
    __device__ static __forceinline__ void store_row(vec_t* Y, int64_t ldy, int col_begin, int cols, bool vec, float alpha, float beta,
                                                     int64_t r, int c, const float (&sum)[V]) {
        mh::store_row<vec_t>(Y, ldy, col_begin, cols, vec, alpha, beta, r, c, sum);
    }
};

template <typename off_t, typename vec_t, typename mat_t, int C>
__global__ __launch_bounds__(kBlock) void multi_half_slice_kernel(const MultiHalfArgs<vec_t, mat_t> a, const off_t* __restrict__ Ap) {
    using P = MultiHalfPolicy<vec_t, mat_t>;
#include "multi_slice_walk.inc"
}

// one thread per (slice, column): the first slice that carries a row sums its carries in slice order, then the tail —
// which lies in the slice after the last one that carries the row, and that slice holds at least one nonzero of it —
// and stores the rounded row.  No slice has written it.
template <typename vec_t>
__global__ __launch_bounds__(kBlock) void multi_half_fixup_kernel(int64_t n_slices, int32_t k, const int32_t* __restrict__ carry_row,
                                                                  const float* __restrict__ carry_val,
                                                                  const float* __restrict__ tail_val, int64_t carry_ld,
                                                                  vec_t* __restrict__ Y, int64_t ldy, float alpha, float beta) {
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t = gid / k;
    const int j = int(gid % k);
    if (t >= n_slices) return;
    const int32_t r = carry_row[t];
    if (r < 0 || (t > 0 && carry_row[t - 1] == r)) return;
    float sum = carry_val[t * carry_ld + j];
    int64_t u = t + 1;
    for (; u < n_slices && carry_row[u] == r; ++u) sum += carry_val[u * carry_ld + j];
    if (u < n_slices) sum += tail_val[u * carry_ld + j];    // (always: an open row has a nonzero in the next slice)
    vec_t& y = Y[int64_t(r) * ldy + j];
    float out = alpha * sum;
    if (beta != 0.0f) out += beta * widen(y);
    y = narrow_to(out, vec_t());
}

}  // namespace mh

// the slice passes (tiles of 64 columns) and the fix-up
template <typename off_t, typename vec_t, typename mat_t>
int launch_multi_half(const MultiShape& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    static_assert(sizeof(vec_t) == 2 && (sizeof(mat_t) == 2 || sizeof(mat_t) == 4), "16-bit vectors; the matrix in their type or fp32");
    if (m.n_slices == 0) return MI355_SPMV_OK;      // no rows: nothing to write
    mh::MultiHalfArgs<vec_t, mat_t> a;
    multi_fill_args<mh::MultiHalfArgs<vec_t, mat_t>, vec_t>(a, m, X, ldx, Y, ldy);
    a.Ax = static_cast<const mat_t*>(Ax);
    a.tail_val = static_cast<float*>(m.tail_val);
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    if (const int st = multi_passes<mh::kHalfV>(a, k, [&](auto lanes) {
            hipLaunchKernelGGL((mh::multi_half_slice_kernel<off_t, vec_t, mat_t, decltype(lanes)::value>), grid, block, 0, s, a, Ap);
        }))
        return st;
    if (m.n_slices > 1) {
        const int64_t threads = m.n_slices * k;
        hipLaunchKernelGGL((mh::multi_half_fixup_kernel<vec_t>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s,
                           m.n_slices, k, m.carry_row, a.carry_val, a.tail_val, m.carry_ld, a.Y, ldy, a.alpha, a.beta);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

// MI355_MULTI_HALF_EACH(X): X(off_t, vec_t, mat_t) for both offset widths, both 16-bit types, the matrix in the vectors'
// type and in fp32 — the eight launch_multi_half (32 slice kernels) of multi_h16.hip
#define MI355_MULTI_HALF_EACH(X)                                                                          \
    X(int32_t, mh::F16, mh::F16) X(int64_t, mh::F16, mh::F16) X(int32_t, mh::F16, float) X(int64_t, mh::F16, float) \
    X(int32_t, Bf16, Bf16) X(int64_t, Bf16, Bf16) X(int32_t, Bf16, float) X(int64_t, Bf16, float)
#define MI355_MULTI_HALF_DEFINE(OFF, VEC, MAT) \
    template int launch_multi_half<OFF, VEC, MAT>(const MultiShape&, const void*, const void*, int64_t, void*, int64_t, int32_t, hipStream_t);
#define MI355_MULTI_HALF_DECLARE(OFF, VEC, MAT) extern MI355_MULTI_HALF_DEFINE(OFF, VEC, MAT)

#ifdef MI355_MULTI_SPLIT_UNITS      // the library's build: multi_h16.hip defines them
MI355_MULTI_HALF_EACH(MI355_MULTI_HALF_DECLARE)
#endif

}  // namespace mi355
