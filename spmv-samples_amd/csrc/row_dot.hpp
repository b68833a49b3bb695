// row_dot.hpp — small pieces shared by the row-based kernels: vector types, the
// nontemporal stream load, the sub-wave reduction, and the 4-byte-per-lane row dot
// product of the fallback kernels (the lanes-per-row rule: rows_plan.hip).
//
// The reference's per-row arithmetic (cusp_warp_reduce.cuh:26-57, LightSpMV.cuh:147-170):
// lane l of a T-lane vector reads one 4-byte Aj and one Ax element per step, stride T, and
// the T partial sums are folded by a shuffle tree.  On gfx950 a 4-byte-per-lane stream
// reaches roughly half the HBM rate of a 16-byte-per-lane one, so the main kernels
// (xwindow.hpp) give a lane 4 consecutive nonzeros per step — one global_load_dwordx4 of
// Aj, one or two of Ax — starting at the row start rounded DOWN to a multiple of 4 so that
// every load is 16-byte aligned, with elements outside [start, end) masked.  (The
// reference has the same idea for one case only: the aligned sweep for T == 32 and rows
// longer than 32, cusp_warp_reduce.cuh:33-44.)  Summation order: per lane ascending, then
// a shuffle-down tree over T lanes — the shape of SURVEY Appendix A.1 with T up to 64.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace mi355 {

typedef int int4v __attribute__((ext_vector_type(4)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));   // four 16-bit window indices (xwindow.hpp, PACKED)
constexpr unsigned kPackedEscape = 0xFFFFu;                    // ... and the one that says "outside the window"
typedef float float4v __attribute__((ext_vector_type(4)));
typedef double double4v __attribute__((ext_vector_type(4)));

template <typename val_t> struct Vec4;
template <> struct Vec4<float> { using type = float4v; };
template <> struct Vec4<double> { using type = double4v; };
template <> struct Vec4<int32_t> { using type = int4v; };   // (integer values: the generalized merge kind)
template <> struct Vec4<PatternOnes> { using type = PatternOnes; };   // (a pattern matrix: nothing to hold)

// 16-bit matrix values under fp32 vectors (MI355_VAL_F16 / MI355_VAL_BF16, kind VECTOR: csr_vector_h16.hip).  The chunk
// bodies take the stored type as a trailing mat_t (= val_t everywhere else): a group of four is then ONE 8-byte load,
// held as loaded and widened to four values of val_t where it is consumed; the arithmetic is val_t's.  (Bf16: common.hpp)
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
template <> struct Vec4<_Float16> { using type = uint2v; };      // (four of them as loaded)
template <> struct Vec4<Bf16> { using type = uint2v; };

// one stored value as a val_t: the hardware convert for fp16, a shift for bf16 (both exact)
template <typename val_t, typename mat_t>
__device__ __forceinline__ val_t mat_val(mat_t a) {
    if constexpr (std::is_same<mat_t, Bf16>::value) return __uint_as_float(unsigned(a.bits) << 16);
    else return val_t(a);
}
// ... and a loaded group of four
template <typename val_t, typename mat_t>
__device__ __forceinline__ typename Vec4<val_t>::type widen4(const typename Vec4<mat_t>::type& a) {
    if constexpr (std::is_same<mat_t, val_t>::value) {
        return a;
    } else if constexpr (std::is_same<mat_t, _Float16>::value) {
        return __builtin_convertvector(__builtin_bit_cast(half4v, a), float4v);
    } else {
        static_assert(std::is_same<mat_t, Bf16>::value && std::is_same<val_t, float>::value, "no such matrix type");
        return float4v{__uint_as_float(a[0] << 16), __uint_as_float(a[0] & 0xFFFF0000u), __uint_as_float(a[1] << 16),
                       __uint_as_float(a[1] & 0xFFFF0000u)};
    }
}

// Aj / Ax are read exactly once per SpMV: stream them past the caches (nontemporal) so
// that the lines of x, which ARE re-used, stay resident.  Measured on the two-stream
// read pattern of the kernels: 6.9 TB/s nontemporal vs 6.15 TB/s plain.
template <typename V>
__device__ __forceinline__ V stream_load(const V* p) {
#ifdef MI355_STREAM_PLAIN   // (A/B builds only)
    return *p;
#else
    return __builtin_nontemporal_load(p);
#endif
}

// 4-byte-per-lane partial sum of lane `lane` (0..T-1) of the vector that owns [start, end):
// the reference's form, used only when Aj/Ax/x are not 16-byte aligned.
template <int T, typename off_t, typename val_t, typename mat_t = val_t>
__device__ __forceinline__ val_t row_partial(off_t start, off_t end, int lane, const int32_t* __restrict__ Aj,
                                             const mat_t* __restrict__ Ax, const val_t* __restrict__ x) {
    val_t sum = val_t(0);
    for (off_t j = start + lane; j < end; j += T) sum += mat_val<val_t>(Ax[j]) * x[Aj[j]];
    return sum;
}

// Fold the T lane partials of every vector in the wave; lane 0 of each vector ends up
// with the row sum.  All 64 lanes must execute this.
template <int T, typename val_t>
__device__ __forceinline__ val_t vector_reduce(val_t v) {
#pragma unroll
    for (int o = T / 2; o >= 1; o >>= 1) {
        v += __shfl_down(v, o, T);
    }
    return v;
}

// The body of the plain kernels (csr_vector_kernel of csr_vector.hip, and of csr_vector_h16.hip for a 16-bit mat_t): the
// form of the reference, one row per T-lane vector of a kBlock-thread workgroup, grid = ceil(rows / vectors per
// workgroup), right for any CSR.
template <int T, typename off_t, typename val_t, typename mat_t>
__device__ __forceinline__ void plain_rows(int32_t n_rows, const off_t* __restrict__ Ap, const int32_t* __restrict__ Aj,
                                           const mat_t* __restrict__ Ax, const val_t* __restrict__ x,
                                           val_t* __restrict__ y, val_t alpha, val_t beta) {
    constexpr int ROWS_PER_BLOCK = kBlock / T;
    const unsigned blk = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & (T - 1);
    const int64_t row = int64_t(blk) * ROWS_PER_BLOCK + (threadIdx.x / T);
    const bool live = row < n_rows;
    // a vector past the last row runs as an empty row so that every lane of the
    // wave reaches the shuffles below
    off_t start = 0, end = 0;
    if (live) {
        start = Ap[row];
        end = Ap[row + 1];
    }
    val_t sum = row_partial<T, off_t, val_t>(start, end, lane, Aj, Ax, x);
    sum = vector_reduce<T, val_t>(sum);
    if (live && lane == 0) y[row] = (beta != val_t(0)) ? alpha * sum + beta * y[row] : alpha * sum;
}

}  // namespace mi355
