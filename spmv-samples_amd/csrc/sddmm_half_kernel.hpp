// sddmm_half_kernel.hpp — SDDMM with U and V stored in 16 bits (MI355_VAL_F16 / MI355_VAL_BF16) and fp32 values and
// arithmetic (mi355_spmv_sddmm_create_half):
//   out[n] = alpha * s[n] * sum_{j < k} float(U[r(n), j]) * float(V[Aj[n], j]) + beta * out[n]
// Ax (s) and out are fp32.  Every stored 16-bit value is widened exactly (half_convert.hpp's widen); products and sums
// are fp32; nothing is rounded to 16 bits anywhere.  Included by sddmm.hip, which owns the object and the entry points,
// behind its handle and sddmm_args: this header holds the kernel and its one launch.
//
//   sddmm_half_slice_kernel   sddmm_slice_kernel's walk (the same text, sddmm_slice_walk.inc) over the same cut
//                             (slice_cut.hpp, slice_cut.inc) with a lane's 16 bytes being EIGHT columns: C = 1 / 2 / 4 / 8 lanes
//                             per slot from ceil(k / 8), tiles of 8 / 16 / 32 / 64 columns, the tile loop inside the
//                             kernel for wider k.  A kernel of its own, with a name and an argument struct of its own:
//                             a storage type among sddmm_slice_kernel's template arguments would rename the kernels on
//                             record (profiles/sddmm_kernel_resources.txt).
//
// Order of addition, sddmm_slice_walk.inc's: one piece of code for this kernel and the fp32 / fp64 one, behind the 16-byte
// and the element-by-element load (both fill the same eight fp32 registers, half_cols.hpp): part = fma(u[j], v[j], part) over the lane's columns in ascending order, tile after
// tile, from +0 (a masked column is loaded as 0 and adds +0); the xor-shuffle tree over the C lanes at distance 1, 2,
// 4; the hand-back to the lane that loaded the nonzero; alpha * (ax * dot), + beta * out_old when beta != 0; one store
// of 64 contiguous fp32 values per group.  An element of out is a function of (U[r, :k], V[c, :k], s, alpha, beta,
// out_old, k) only.  The lane partition differs from the fp32 kernel's (8 columns per lane against 4), so on real data
// the two do not agree bit for bit; on data whose every partial sum is exact in fp32 they do.
#pragma once

#include "half_cols.hpp"
#include "slice_cut.hpp"

namespace mi355 {

template <typename vec_t>
struct SddmmHalfArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const float* Ax;        // null for a pattern kernel, which never forms an address from it
    const vec_t* U;
    const vec_t* V;
    float* out;
    int64_t ldu, ldv;
    int32_t k;
    int32_t u_vec, v_vec;   // 1 = rows of U / V are 16-byte aligned: one 16-byte load per lane and tile
    float alpha, beta;
};

// C = lanes per nonzero slot (16-byte column groups of a tile); the wave holds S = 64 / C slots
template <typename off_t, typename vec_t, int C, bool VALUED>
__global__ __launch_bounds__(kBlock) void sddmm_half_slice_kernel(const SddmmHalfArgs<vec_t> a, const off_t* __restrict__ Ap) {
    using acc_t = float;
    using mh::load_cols;                // the walk's load_cols: the lane's eight 16-bit columns, widened
    constexpr int W = mh::kHalfV;       // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr bool kCutCarriedIn = false, kCutKeepsR1 = false;      // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = 0;
    constexpr bool kWalkFmaInPlace = true;                          // what sddmm_slice_walk.inc asks its includer
    const unsigned cut_block = blockIdx.x;
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, n0, nn, nr, rel
#include "sddmm_slice_walk.inc"     // the slice's nonzeros, 64 at a time: sddmm_slice_kernel's walk
}

// the one launch of a 16-bit execute: C from ceil(k / 8), valued / pattern from Ax.  A caller has checked the arguments
// and that there is something to launch (nnz and n_rows above 0).
template <typename off_t, typename vec_t>
int sddmm_half_launch(const mi355_spmv_sddmm& m, const void* Ax, const void* U, int64_t ldu, const void* V, int64_t ldv, void* out,
                      int32_t k, hipStream_t s) {
    static_assert(sizeof(vec_t) == 2, "16-bit U and V");
    const SddmmHalfArgs<vec_t> a = sddmm_args<SddmmHalfArgs<vec_t>>(m, Ax, U, ldu, V, ldv, out, k);
    const off_t* ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    with_slot_lanes((k + mh::kHalfV - 1) / mh::kHalfV, [&](auto lanes) {
        constexpr int C = decltype(lanes)::value;
        if (Ax) hipLaunchKernelGGL((sddmm_half_slice_kernel<off_t, vec_t, C, true>), grid, block, 0, s, a, ap);
        else hipLaunchKernelGGL((sddmm_half_slice_kernel<off_t, vec_t, C, false>), grid, block, 0, s, a, ap);
    });
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

}  // namespace mi355
