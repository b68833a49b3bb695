// attention_bwd_half_kernel.hpp — the fused attention backward with Q, K, V, O, dO, dQ, dK and dV stored in ONE 16-bit type
// (MI355_VAL_F16 / MI355_VAL_BF16) and fp32 everything else (mi355_spmv_attention_bwd_create_half): bias,
// lse, dbias, delta, scale, the scores, p, dp, ds, the coefficients, the per-slot partials, the slices' HEAD / TAIL pieces in
// scratch and every operation are fp32, exactly attention_bwd.hip's arithmetic.  Every stored 16-bit value is widened exactly
// (half_convert.hpp's widen); an element of dQ, dK or dV is rounded to the 16-bit type exactly ONCE, from the fp32 sum of its
// line (narrow_to: nearest even) — by the slot that holds the line's last entry, or, for a line that crosses slices, by the
// fix-up after it has added the fp32 pieces in slice order.  Included by attention_bwd.hip, which owns the object, the
// entry points and the one launch path of both storage types: this header holds the kernels and names them for that path.
//
//   attention_bwd_half_delta_kernel   eight lanes per row, each lane eight columns at a time (16 bytes of dO and of O, widened):
//                                     lane g takes columns 64 k + 8 g .. + 7 in one fma chain from +0, ascending, then the
//                                     fixed xor tree.  Both access paths of half_cols.hpp fill the same registers: one order
//                                     of addition per row whatever the alignment.
//   attention_bwd_half_slice_kernel   attention_bwd_slice_kernel's walk (the same text, attention_bwd_slice_walk.inc) over the
//                                     same cut with a lane's 16 bytes being EIGHT columns: C = 1 / 2 / 4 / 8 lanes per slot
//                                     from ceil(cols / 8) of the role's OUTPUT tile, tiles of 8 .. 64 columns, so d = dv = 64
//                                     is one pass per role.  An output above 64 columns: ceil(width / 64) passes, each
//                                     recomputing the coefficient; only the first DQ pass stores dbias and only the first
//                                     pass the pieces' rows.  The two dots run over C * 8 columns per round; the product of
//                                     two widened 16-bit values is exact in fp32, so each fma chain rounds no more often
//                                     than the fp32 kernel's.  A kernel of its own, with a name and an argument struct of
//                                     its own: a storage type among attention_bwd_slice_kernel's template arguments would
//                                     rename the kernels on record (profiles/attention_backward_kernel_resources.txt).
//   attention_bwd_half_fixup_kernel   attention_bwd_fixup_kernel's fold (attn_bwd_fixup_sum) and the line's one narrowing.
//
// The lane partition differs from the fp32 kernel's (8 columns per lane against 4): C and the step edges of one width
// differ, so on real data the two kinds do not agree bit for bit; where every fp32 sum is exact they do, after narrowing.
#pragma once

#include "half_cols.hpp"
#include "slice_cut.hpp"

namespace mi355 {

#ifdef __clang__
#pragma clang fp contract(off)      // attention_bwd.hip's reason: v = scale * dot, then + bias, and partial + coefficient * column stay as written
#endif

template <typename vec_t>
struct AttnBwdHalfArgs {
    int32_t n_rows;         // lines of the walked structure: A's rows (DQ) or A's columns (DK, DV)
    int64_t nnz, n_slices;
    const int32_t* Aj;      // the walked structure's gathered indices: Aj (DQ) or Ajt (DK, DV)
    const uint32_t* perm;   // DK, DV: the CSR slot of A behind a slot of A^T (bias is in A's order)
    const vec_t* Q;
    const vec_t* K;
    const vec_t* V;
    const vec_t* dO;
    const float* bias;      // null: none
    const float* lse;
    const float* delta;
    vec_t* out;             // dQ, dK or dV
    float* dbias;           // DQ only; null: not asked for
    int64_t ldq, ldk, ldv, lddo, ldout;
    int32_t d, dv;
    int32_t col_begin;      // first column of this pass's tile of out
    int32_t cols;           // columns of it that exist (<= 64): the others are masked on load and store
    int32_t q_vec, k_vec, v_vec, do_vec, out_vec;   // 1 = rows are 16-byte aligned: one 16-byte access per lane
    float scale;
    AttnBwdScratch<float> sc;
    int32_t n_heads;        // AttnBwdArgs' heads: the same members, in elements of vec_t for the matrices
    int64_t hq, hk, hv, hdo, hbias, hlse, hout, hdbias;
    int64_t hsc;
};

// delta[r] = dot(float(dO[r, :dv]), float(O[r, :dv])) in fp32: kDeltaLanes lanes per row, lane g the columns 64 k + 8 g .. + 7
template <typename vec_t>
__global__ __launch_bounds__(kBlock) void attention_bwd_half_delta_kernel(int32_t n_rows, int32_t dv, const vec_t* __restrict__ dO, int64_t lddo,
                                                                          int32_t do_vec, const vec_t* __restrict__ O, int64_t ldo, int32_t o_vec,
                                                                          float* __restrict__ delta0, const AttnBwdHeads hd) {
    constexpr int W = mh::kHalfV;
    unsigned h;
    const int64_t gid = attn_head_thread(hd.per_head, h);
    const int64_t r = gid / kDeltaLanes;
    const int g = int(gid % kDeltaLanes);
    const bool valid = r < n_rows;      // (every lane stays for the shuffles)
    float* delta = attn_head_scratch(delta0, h, hd.hsc);
    float sum = 0.0f;
    if (valid) {
        const vec_t* a = dO + h * hd.ha + r * lddo;
        const vec_t* b = O + h * hd.hb + r * ldo;
        for (int32_t cb = g * W; cb < dv; cb += kDeltaLanes * W) {
            const int nd = min(dv - cb, W);
            float x[W], y[W];
            mh::load_cols(x, a + cb, nd, do_vec != 0);
            mh::load_cols(y, b + cb, nd, o_vec != 0);
#pragma unroll
            for (int j = 0; j < W; ++j) sum = attn_fma(x[j], y[j], sum);
        }
    }
#pragma unroll
    for (int dd = 1; dd < kDeltaLanes; dd <<= 1) sum += __shfl_xor(sum, dd);
    if (valid && g == 0) delta[r] = sum;
}

// C = lanes per nonzero slot (16-byte column groups of this pass's tile of out); the wave holds S = 64 / C slots
template <typename off_t, typename vec_t, int C, int ROLE>
__global__ __launch_bounds__(kBlock) void attention_bwd_half_slice_kernel(const AttnBwdHalfArgs<vec_t> args, const off_t* __restrict__ Ap) {
    using acc_t = float;                // what attention_bwd_slice_walk.inc asks its includer
    using mh::load_cols;                // the lane's eight 16-bit columns, widened
    using mh::store_cols;               // and narrowed, once each
    constexpr int W = mh::kHalfV;       // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr float kNegInf = -std::numeric_limits<float>::infinity();
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = true;        // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
    const unsigned cut_block = blockIdx.x / unsigned(args.n_heads);     // the head varies fastest, as in attention_bwd_slice_kernel
    const AttnBwdHalfArgs<vec_t> a = attn_bwd_args_of_head(args, blockIdx.x % unsigned(args.n_heads));
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
#include "attention_bwd_slice_walk.inc"     // the slice's entries, 64 at a time: attention_bwd_slice_kernel's walk
}

// one thread per (head, slice, column), as attention_bwd_fixup_kernel: the line's only rounding to 16 bits, after the fp32 sum
template <typename vec_t>
__global__ __launch_bounds__(kBlock) void attention_bwd_half_fixup_kernel(int64_t n_slices, int32_t width, const AttnBwdScratch<float> sc0,
                                                                          vec_t* __restrict__ out0, int64_t ldout, const AttnBwdHeads hd) {
    unsigned h;
    const int64_t gid = attn_head_thread(hd.per_head, h);
    const int j = int(gid % width);
    const AttnBwdScratch<float> sc = attn_bwd_scratch_of_head(sc0, h, hd.hsc);
    vec_t* out = out0 + h * hd.ha;
    int32_t r;
    float sum;
    if (!attn_bwd_fixup_sum(n_slices, sc, gid / width, j, r, sum)) return;
    out[int64_t(r) * ldout + j] = narrow_to(sum, vec_t());
}

// the kernels as attention_bwd.hip's launch path names them (AttnBwdKernels<val_t>'s members): the passes of a role run
// over tiles of W * 8 = 64 columns
template <typename vec_t>
struct AttnBwdHalfKernels {
    static_assert(sizeof(vec_t) == 2, "16-bit Q, K, V, O, dO, dQ, dK and dV");
    using elem_t = vec_t;
    using acc_t = float;
    using Args = AttnBwdHalfArgs<vec_t>;
    static constexpr int W = mh::kHalfV;
    static void delta(dim3 grid, hipStream_t s, int32_t n_rows, int32_t dv, const vec_t* dO, int64_t lddo, const vec_t* O, int64_t ldo, float* delta,
                      const AttnBwdHeads& hd) {
        hipLaunchKernelGGL((attention_bwd_half_delta_kernel<vec_t>), grid, dim3(kBlock), 0, s, n_rows, dv, dO, lddo,
                           attn_rows_vec<vec_t>(dO, lddo, hd.n_heads, hd.ha) ? 1 : 0, O, ldo, attn_rows_vec<vec_t>(O, ldo, hd.n_heads, hd.hb) ? 1 : 0, delta,
                           hd);
    }
    template <typename off_t, int C, int ROLE>
    static void slice(dim3 grid, hipStream_t s, const Args& a, const off_t* Ap) {
        hipLaunchKernelGGL((attention_bwd_half_slice_kernel<off_t, vec_t, C, ROLE>), grid, dim3(kBlock), 0, s, a, Ap);
    }
    static void fixup(dim3 grid, hipStream_t s, const Args& a, int32_t width) {
        hipLaunchKernelGGL((attention_bwd_half_fixup_kernel<vec_t>), grid, dim3(kBlock), 0, s, a.n_slices, width, a.sc, a.out, a.ldout,
                           AttnBwdHeads{a.n_heads, uint32_t(attn_blocks_per_head(a.n_slices * width)), a.hsc, a.hout, 0});
    }
};

}  // namespace mi355
