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
// Here a kernel is how a workgroup gets its rows; from there to the chunk body (xwindow.hpp) the text is shared with LIGHT
// and the 16-bit kernels and included: row_chunk_window.inc, row_chunk_sweep.inc.  The plain kernel's body is
// row_dot.hpp's plain_rows, its launch row_launch.hpp's launch_plain_rows.

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
    using mat_t = val_t;
    constexpr bool kBarrierAfterWide = false;
#include "row_chunk_window.inc"
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
#include "row_chunk_sweep.inc"
}

template <int T, typename off_t, typename val_t>
__global__ __launch_bounds__(kBlock) void csr_vector_kernel(
    int32_t n_rows, off_t nnz, const off_t* __restrict__ Ap, const int32_t* __restrict__ Aj,
    const val_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y, val_t alpha, val_t beta) {
    plain_rows<T, off_t, val_t>(n_rows, Ap, Aj, Ax, x, y, alpha, beta);
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
    return launch_plain_rows(p, VectorRows::name, Ap, Ax, x, y, s,
                             [](auto lanes) { return csr_vector_kernel<decltype(lanes)::value, off_t, val_t>; });
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
