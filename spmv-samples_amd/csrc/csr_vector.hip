// csr_vector.hip — kind VECTOR: CSR-vector SpMV with per-row sub-wave reduction.
//
// Replaces the reference's CUSP CSR-vector family on the hot path
// (include/spmv/cusp/cusp_warp_reduce.cuh:11-59 kernel, :93-133 width selection,
// include/spmv/cusp/utils.cuh:38-47 shuffle tree).  Written for gfx950:
//   * 64-lane waves, 256-thread workgroups, T lanes per row (T = 2..64);
//   * 16-byte-per-lane nontemporal loads of Aj/Ax, R rows per vector in flight;
//   * a workgroup owns a CHUNK of consecutive rows (~32 K nonzeros) and stages the
//     window of x the chunk touches through LDS (xwindow.hpp) — the plain global
//     gather is what bounds this kernel on MI355X, not the Aj/Ax stream;
//   * chunk ids are remapped so each XCD walks a contiguous range of rows and
//     neighbouring windows of x hit that XCD's L2.
// The 4-byte-per-lane kernel csr_vector_kernel is the form of the reference
// (one row per vector, grid = ceil(rows / vectors per block), cusp_warp_reduce.cuh:70-87);
// it runs small matrices of either kind (rows_plan.hip, shape_rows) and operands that are not 16-byte aligned.

#include <cstdlib>

#include "common.hpp"
#include "row_dot.hpp"
#include "row_launch.hpp"
#include "xwindow.hpp"

namespace mi355 {

// (Registers: 512-thread workgroups and the R = 2 bodies — fp64, and fp32 rows of 33+ nonzeros — are held to 128
// VGPRs, i.e. two / four workgroups per CU; the 256-thread fp32 R = 4 body needs ~135 and gets 168: three per CU,
// which is what its 36 KB window of x allows anyway.  shape_chunks sizes a small matrix's single round of chunks
// by the same numbers: a kernel that silently needs a few more registers than its plan assumed loses 30-40 %
// there — cant stand-in: 14.7 -> 19-21 us when its body went from 127 to 139 VGPRs.)  The kernel does not depend on the width
// of the row offsets: a chunk is walked with 32-bit offsets relative to its own first nonzero (xwindow.hpp).
// PACKED (NSEG == 1, equal-row chunks, the window placed from the plan's band): the loop streams the plan's 16-bit
// window indices Aj16 instead of Aj (xwindow.hpp, chunk_rows; rows_plan.hip, build_packed_index); Aj16 is unused otherwise.
template <int BLOCK, int T, int R, int NSEG, bool ADAPT, typename val_t, bool PACKED = false>
__global__ __launch_bounds__(BLOCK, (BLOCK >= kWideBlock || R == 2 ? 4 : 3)) void csr_vector_window_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz, const ApView Ap, const int32_t* __restrict__ Aj,
    const val_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y, ChunkMap cmap,
    int32_t window_cap, BandHint hint, SegmentPlan segs, const uint16_t* __restrict__ Aj16, val_t alpha, val_t beta) {
    static_assert(!PACKED || (NSEG == 1 && !ADAPT), "the packed index exists for one band-placed window and equal-row chunks");
    // NSEG: 0 = no window (plain gathers), 1 = one window of x in LDS, kMaxSegments = several bands
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window | bounds | y | flags
    __shared__ int s_red[2];
    ChunkScratch<val_t> scr(s_dyn, window_cap, cmap.rows_cap);
    scr.alpha = alpha;
    scr.beta = beta;
    scr.long_steps = cmap.long_steps;
    scr.giant_len = cmap.giant_len;
    // Equal-row chunks: each XCD walks a contiguous range (neighbouring windows of x hit that L2).  Weight-cut
    // chunks (power-law matrices, no window to share): chunk = block index, i.e. consecutive chunks go to
    // different XCDs — the chunks of the dense head of the matrix and those of its near-empty tail take very
    // different times at equal weight, and a contiguous eighth per XCD leaves the XCDs unevenly loaded.
    const unsigned chunk = cmap.table ? blockIdx.x : xcd_contiguous_id(blockIdx.x, gridDim.x);
    int64_t rb, re;
    cmap.range(chunk, n_rows, rb, re);
    if (rb >= re) return;   // (balanced plans: a hub row heavier than a chunk leaves empty chunks behind it)
    bool fits;
    const int64_t base = stage_chunk_bounds<val_t>(scr, rb, re, Ap, cmap.rel_limit, fits);
    if (!fits) {            // (uniform) more nonzeros than 32-bit chunk-relative offsets reach
        chunk_rows_wide<BLOCK, val_t>(rb, re, Ap, Aj, Ax, x, y, alpha, beta, cmap.giant_len);
        return;
    }
    __syncthreads();
    const int32_t* const Aj_c = Aj + base;       // the chunk's view: element 0 = its first 16-byte group
    const val_t* const Ax_c = Ax + base;
    const int64_t left = nnz - base;
    const int32_t nnz_c = int32_t(left < kRel32Limit + 32768 ? left : kRel32Limit + 32768);
    // the window is staged inside chunk_rows, behind the first group's stream loads
    if constexpr (NSEG > 1) {
        auto stage = [&] { return stage_x_segments<val_t>(rb, re, n_cols, x, scr.s_x, window_cap, segs); };
        chunk_rows_any<BLOCK, T, R, true, ADAPT, val_t>(rb, re, nnz_c, Aj_c, Ax_c, x, y, stage, scr);
    } else {
        auto first_last = [&](int64_t r, int& first, int& last) {
            const int32_t s = scr.s_b[r - rb], e = scr.s_b[r - rb + 1];
            if (e <= s) return false;
            first = Aj_c[s];
            last = Aj_c[e - 1];
            return true;
        };
        auto stage = [&] {
            return stage_x_window<val_t>(rb, re, n_cols, first_last, x, scr.s_x, window_cap, s_red, hint);
        };
        if constexpr (PACKED)   // (hint.use holds: the window staged is the one the index was encoded against)
            chunk_rows_any<BLOCK, T, R, true, false, val_t, decltype(stage)&, false, true>(rb, re, nnz_c, Aj_c, Ax_c, x, y, stage,
                                                                                          scr, Aj16 + base);
        else
            chunk_rows_any<BLOCK, T, R, NSEG == 1, ADAPT, val_t>(rb, re, nnz_c, Aj_c, Ax_c, x, y, stage, scr);
    }
}

// The band is wider than any window of x: one 1 024-thread workgroup per CU, a chunk = one group of rows held in
// registers, the window sweeps the band (xwindow.hpp, chunk_rows_sweep).
template <int T, int R, typename val_t>
__global__ __launch_bounds__(kHugeBlock, 4) void csr_vector_sweep_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz, const ApView Ap, const int32_t* __restrict__ Aj,
    const val_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y, ChunkMap cmap,
    int32_t window_cap, BandHint hint, val_t alpha, val_t beta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window | bounds | y | flags
    ChunkScratch<val_t> scr(s_dyn, window_cap, cmap.rows_cap);
    scr.alpha = alpha;
    scr.beta = beta;
    const unsigned chunk = xcd_contiguous_id(blockIdx.x, gridDim.x);   // (an XCD's chunks sweep neighbouring columns: its L2 holds them)
    int64_t rb, re;
    cmap.range(chunk, n_rows, rb, re);
    if (rb >= re) return;
    bool fits;
    const int64_t base = stage_chunk_bounds<val_t>(scr, rb, re, Ap, cmap.rel_limit, fits);
    if (!fits) {
        chunk_rows_wide<kHugeBlock, val_t>(rb, re, Ap, Aj, Ax, x, y, alpha, beta, 0);
        return;
    }
    __syncthreads();
    const int64_t left = nnz - base;
    const int32_t nnz_c = int32_t(left < kRel32Limit + 32768 ? left : kRel32Limit + 32768);
    // (a persistent workgroup per CU walking its share of the chunks measured WORSE, 194 vs 187 us at two passes,
    // 438 vs 358 at seven: the hardware dispatcher's refill costs less than the registers the loop does)
    chunk_rows_sweep<kHugeBlock, T, R, val_t>(rb, re, nnz_c, Aj + base, Ax + base, x, y, n_cols, window_cap, hint, scr);
}

template <int T, typename off_t, typename val_t>
__global__ __launch_bounds__(kBlock) void csr_vector_kernel(
    int32_t n_rows, off_t nnz, const off_t* __restrict__ Ap, const int32_t* __restrict__ Aj,
    const val_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y, val_t alpha, val_t beta) {
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

// VECTOR's kernels for the launch path it shares with LIGHT (row_launch.hpp): a workgroup takes the chunk of its index
struct VectorRows {
    static constexpr const char* name = "csr_vector";
    static constexpr bool kCounters = false;   // (LIGHT's kernels take its dequeue counters)
    static constexpr bool kPlainKnob = true;   // MI355_SPMV_PLAIN forces the 4-byte kernel on whole plans (LIGHT ignores it)
    static constexpr bool kPackedIndex = true; // its window kernels take the plan's packed index and have PACKED twins
    template <int BLOCK, int T, int R, int NSEG, bool ADAPT, typename val_t, bool PACKED = false>
    static auto window() { return csr_vector_window_kernel<BLOCK, T, R, NSEG, ADAPT, val_t, PACKED>; }
    template <int T, int R, typename val_t>
    static auto sweep() { return csr_vector_sweep_kernel<T, R, val_t>; }
    template <typename off_t, typename val_t>
    static int plain(const Plan& p, const off_t* Ap, const val_t* Ax, const val_t* x, val_t* y, hipStream_t s) {
        return launch_vector_plain<off_t, val_t>(p, Ap, Ax, x, y, s);
    }
};

// the plain kernel over the plan's rows, its grid from the row count (both kinds' small matrices: rows_plan.hip, shape_rows)
template <typename off_t, typename val_t>
int launch_vector_plain(const Plan& p, const off_t* Ap, const val_t* Ax, const val_t* x, val_t* y, hipStream_t s) {
    return with_lanes(p, VectorRows::name, [&](auto lanes) -> int {
        constexpr int T = decltype(lanes)::value, rows_per_block = kBlock / T;
        const dim3 grid((unsigned)((int64_t(p.n_rows) + rows_per_block - 1) / rows_per_block)), block(kBlock);
        hipLaunchKernelGGL((csr_vector_kernel<T, off_t, val_t>), grid, block, 0, s, p.n_rows, (off_t)p.nnz, Ap, p.Aj, Ax, x, y,
                           (val_t)p.alpha, (val_t)p.beta);
        MI355_HIP_TRY(hipGetLastError());
        return MI355_SPMV_OK;
    });
}

// One translation unit per value type (csr_vector_f64.hip includes this file with MI355_TU_F64): the two
// halves of the instantiations compile side by side.
#ifdef MI355_TU_PROBE      // (scripts: one kernel instantiated on its own to read its register use quickly)
#elif !defined(MI355_TU_F64)
template int launch_rows<VectorRows, int32_t, float>(const Plan&, const int32_t*, const float*, const float*, float*, hipStream_t);
template int launch_rows<VectorRows, int64_t, float>(const Plan&, const int64_t*, const float*, const float*, float*, hipStream_t);
template int launch_vector_plain<int32_t, float>(const Plan&, const int32_t*, const float*, const float*, float*, hipStream_t);
template int launch_vector_plain<int64_t, float>(const Plan&, const int64_t*, const float*, const float*, float*, hipStream_t);
#else
template int launch_rows<VectorRows, int32_t, double>(const Plan&, const int32_t*, const double*, const double*, double*, hipStream_t);
template int launch_rows<VectorRows, int64_t, double>(const Plan&, const int64_t*, const double*, const double*, double*, hipStream_t);
template int launch_vector_plain<int32_t, double>(const Plan&, const int32_t*, const double*, const double*, double*, hipStream_t);
template int launch_vector_plain<int64_t, double>(const Plan&, const int64_t*, const double*, const double*, double*, hipStream_t);
#endif

}  // namespace mi355
