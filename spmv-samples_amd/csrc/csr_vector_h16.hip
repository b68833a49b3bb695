// csr_vector_h16.hip — kind VECTOR with the matrix stored in 16 bits (MI355_VAL_F16 / MI355_VAL_BF16) under fp32 x and y.
//
// The banded VECTOR plan is bound by the bytes it streams, and with the packed index (rows_plan.hip, build_packed_index)
// the values are 4 of the 6 bytes per nonzero.  Here Ax is _Float16 or Bf16: the chunk bodies of xwindow.hpp take the
// stored type as mat_t, load a group of four values as ONE 8-byte nontemporal load — the shape of the packed index's own
// load — and widen it to four floats (v_cvt_f32_f16, or a shift for bf16) in front of the unchanged fp32 arithmetic.
// Addresses, masks, the order of a row's additions, the pipeline depth, R and the launch bounds are the fp32 plan's: the
// plan IS the fp32 plan of the structure (capi.hip, plan_create_typed), so y equals its y on the widened values bit for bit.
//
// Built: equal-row chunks with one window of x or none (NSEG 1 / 0), 256 / 512 / 1 024 threads, with the packed index and
// without.  Every other shape (rows_plan.hip, half_matrix_chunked) and operands that are not aligned run the plain
// 4-byte-per-lane kernel below, which is right for any CSR.  The kernels are csr_vector.hip's two, for a stored type of
// their own, in a namespace of their own: a template argument is part of a kernel's name, so a mat_t on the fp32 / fp64
// kernels themselves would rename every one of them; as it is their translation units compile to the same device code
// as before.  Only the kernels' heads are written here: the window kernel's text from its rows to the chunk body is
// row_chunk_window.inc, the plain kernel's body is row_dot.hpp's plain_rows, both over mat_t.

#include "common.hpp"
#include "half_convert.hpp"
#include "row_dot.hpp"
#include "row_launch.hpp"
#include "xwindow.hpp"

namespace mi355 {
namespace h16 {

// csr_vector.hip's csr_vector_window_kernel for val_t = float and a stored type mat_t, equal-row chunks only (no chunk
// table, one vector width, no multi-band window): same LDS layout, same launch bounds, same chunk bodies.
template <int BLOCK, int T, int R, int NSEG, bool PACKED, typename mat_t>
__global__ __launch_bounds__(BLOCK, (BLOCK >= kWideBlock || R == 2 ? 4 : 3)) void csr_vector_window_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz, const ApView Ap, const int32_t* __restrict__ Aj,
    const mat_t* __restrict__ Ax, const float* __restrict__ x, float* __restrict__ y, ChunkMap cmap,
    int32_t window_cap, BandHint hint, const uint16_t* __restrict__ Aj16, float alpha, float beta) {
    static_assert(NSEG == 0 || NSEG == 1, "one window of x or none");
    static_assert(!PACKED || NSEG == 1, "the packed index exists for one band-placed window");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window | bounds | y | flags
    __shared__ int s_red[2];
    ChunkScratch<float> scr(s_dyn, window_cap, cmap.rows_cap);
    scr.alpha = alpha;
    scr.beta = beta;
    scr.long_steps = cmap.long_steps;
    scr.giant_len = cmap.giant_len;
    const unsigned chunk = xcd_contiguous_id(blockIdx.x, gridDim.x);
    int64_t rb, re;
    cmap.range(chunk, n_rows, rb, re);
    if (rb >= re) return;
    using val_t = float;
    constexpr bool ADAPT = false, kBarrierAfterWide = false;
    const SegmentPlan segs{};   // (named by the shared text where NSEG > 1, which no kernel here is)
#include "row_chunk_window.inc"
}

// ... and its csr_vector_kernel: one row per T-lane vector, 4-byte (here 2-byte) loads per lane, any CSR
template <int T, typename off_t, typename mat_t>
__global__ __launch_bounds__(kBlock) void csr_vector_kernel(
    int32_t n_rows, off_t nnz, const off_t* __restrict__ Ap, const int32_t* __restrict__ Aj,
    const mat_t* __restrict__ Ax, const float* __restrict__ x, float* __restrict__ y, float alpha, float beta) {
    plain_rows<T, off_t, float>(n_rows, Ap, Aj, Ax, x, y, alpha, beta);
}

// fp32 -> binary16 / bfloat16 (half_convert.hpp's narrow_to)
template <typename dst_t>
__global__ __launch_bounds__(kBlock) void narrow_values_kernel(int64_t n, const float* __restrict__ src, dst_t* __restrict__ dst) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock)
        dst[i] = narrow_to(src[i], dst_t());
}

struct Rows {   // (what launch_chunked asks of a kind)
    static constexpr const char* name = "csr_vector (16-bit matrix)";
    static constexpr bool kCounters = false;
};

// row_launch.hpp's launch_rows_window for the shapes built here
template <int BLOCK, typename mat_t>
static int launch_window(const RowOperands<float, mat_t>& o) {
    const Plan& p = o.p;
    if constexpr (BLOCK >= kWideBlock) {   // (a 512- / 1 024-thread plan without its window, a forced knob: the 256-thread kernel)
        if (p.window_elems <= 0) return launch_window<kBlock, mat_t>(o);
    }
    const BandHint hint{p.band_lo, p.band_hi, p.window_from_band};
    const ChunkMap cmap = chunk_map_of(p);
    auto go = [&](auto kernel) { return launch_chunked<Rows, float>(kernel, BLOCK, o, cmap, hint, (const uint16_t*)p.packed_index); };
    return with_lanes(p, Rows::name, [&](auto lanes) -> int {
        constexpr int T = decltype(lanes)::value, R = rows_in_flight(sizeof(float), T);
        if (p.packed_index && p.window_elems > 0 && p.window_from_band) return go(csr_vector_window_kernel<BLOCK, T, R, 1, true, mat_t>);
        if (p.window_elems > 0) return go(csr_vector_window_kernel<BLOCK, T, R, 1, false, mat_t>);
        if constexpr (BLOCK == kBlock) return go(csr_vector_window_kernel<BLOCK, T, R, 0, false, mat_t>);
        return MI355_SPMV_OK;
    });
}

}  // namespace h16

template <typename off_t, typename mat_t>
int launch_vector_half(const Plan& p, const off_t* Ap, const mat_t* Ax, const float* x, float* y, hipStream_t s) {
    static_assert(sizeof(mat_t) == 2, "a 16-bit stored type");
    if (p.n_rows == 0) return MI355_SPMV_OK;
    // a group of four values is one 8-byte load; Aj and x are read as the fp32 plan reads them
    const bool aligned = ((reinterpret_cast<uintptr_t>(p.Aj) | reinterpret_cast<uintptr_t>(x)) & 15u) == 0 &&
                         (reinterpret_cast<uintptr_t>(Ax) & 7u) == 0;
    if (!half_matrix_chunked(p) || !aligned || p.nnz < 4 || (p.knob.plain != 0 && !p.is_block))
        return launch_plain_rows(p, h16::Rows::name, Ap, Ax, x, y, s,
                                 [](auto lanes) { return h16::csr_vector_kernel<decltype(lanes)::value, off_t, mat_t>; });
    const RowOperands<float, mat_t> o{p, ApView{Ap, sizeof(off_t) == 8 ? 1 : 0}, Ax, x, y, s,
                                      chunk_lds_bytes(p.window_elems, p.rows_cap, sizeof(float))};
    return p.block_threads == kHugeBlock   ? h16::launch_window<kHugeBlock, mat_t>(o)
           : p.block_threads == kWideBlock ? h16::launch_window<kWideBlock, mat_t>(o)
                                           : h16::launch_window<kBlock, mat_t>(o);
}

int launch_narrow_values(int dst_type, int64_t n, const float* src, void* dst, hipStream_t s) {
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(blocks < int64_t(kCus) * 32 ? blocks : int64_t(kCus) * 32)), block(kBlock);
    if (dst_type == MI355_VAL_F16)
        hipLaunchKernelGGL((h16::narrow_values_kernel<_Float16>), grid, block, 0, s, n, src, static_cast<_Float16*>(dst));
    else
        hipLaunchKernelGGL((h16::narrow_values_kernel<Bf16>), grid, block, 0, s, n, src, static_cast<Bf16*>(dst));
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

template int launch_vector_half<int32_t, _Float16>(const Plan&, const int32_t*, const _Float16*, const float*, float*, hipStream_t);
template int launch_vector_half<int64_t, _Float16>(const Plan&, const int64_t*, const _Float16*, const float*, float*, hipStream_t);
template int launch_vector_half<int32_t, Bf16>(const Plan&, const int32_t*, const Bf16*, const float*, float*, hipStream_t);
template int launch_vector_half<int64_t, Bf16>(const Plan&, const int64_t*, const Bf16*, const float*, float*, hipStream_t);

}  // namespace mi355
