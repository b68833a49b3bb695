// attention_half_kernel.hpp — fused sparse attention with Q, K, V and O stored in ONE 16-bit type (MI355_VAL_F16 /
// MI355_VAL_BF16) and fp32 everything else (mi355_spmv_attention_create_half): bias, lse, scale, the
// scores, the (m, l, acc) states, the scratch pieces and every operation are fp32, exactly attention.hip's arithmetic.
// Every stored 16-bit value is widened exactly (half_convert.hpp's widen); an element of O is rounded to the 16-bit type
// exactly ONCE, from the fp32 acc / l (narrow_to: nearest even) — by the slot that holds the row's last nonzero, or, for a
// row that crosses slices, by the fix-up: the slices leave fp32 states, as the fp32 kernel's do.  Included by
// attention.hip, which owns the object, the entry points and the one launch path of both storage types, behind its
// AttnScratch and fold: this header holds the kernels and names them for that path.
//
//   attention_half_slice_kernel   attention_slice_kernel's walk (the same text, attention_slice_walk.inc) over the same cut
//                                 (slice_cut.hpp, slice_cut.inc, slice_cut_row.inc) with a lane's 16 bytes being EIGHT
//                                 columns: C = 1 / 2 / 4 / 8 lanes per slot from ceil(cols / 8), tiles of 8 / 16 / 32 / 64
//                                 columns, so dv = 64 is one pass and dv = 32 runs 16 nonzeros a step.  dv above 64:
//                                 ceil(dv / 64) passes, the scores recomputed, only the first storing lse and the pieces'
//                                 (row, m, l).  d is unbounded: the tile loop runs over C * 8 columns per round.  A kernel
//                                 of its own, with a name and an argument struct of its own: a storage type among
//                                 attention_slice_kernel's template arguments would rename the kernels on record
//                                 (profiles/attention_kernel_resources.txt).
//   attention_half_fixup_kernel   attention_fixup_kernel's fold (attn_fixup_fold) and the one narrowing of a crossing row.
//
// The aligned and the element-by-element accesses fill the same eight fp32 registers (half_cols.hpp), so unaligned
// operands give the aligned bits.  The lane partition differs from the fp32 kernel's (8 columns per lane against 4): C and
// the step edges of one width differ, so on real data the two kinds do not agree bit for bit.
#pragma once

#include "half_cols.hpp"
#include "slice_cut.hpp"

namespace mi355 {

#ifdef __clang__
#pragma clang fp contract(off)      // attention.hip's reason: the walk's v = scale * dot, then + bias, and a e + a' e' stay as written
#endif

template <typename vec_t>
struct AttnHalfArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const vec_t* Q;
    const vec_t* K;
    const vec_t* V;
    const float* bias;      // null: none
    vec_t* O;
    float* lse;             // null: not asked for
    int64_t ldq, ldk, ldv, ldo;
    int32_t d;
    int32_t col_begin;      // first column of this pass's tile of dv (0: the pass that stores lse and the pieces' row, m, l)
    int32_t cols;           // columns of it that exist (<= 64): the others are masked on load and store
    int32_t q_vec, k_vec, v_vec, o_vec;     // 1 = rows are 16-byte aligned: one 16-byte access per lane
    float scale;
    AttnScratch<float> sc;
    int32_t n_heads;        // AttnArgs' heads: the same members, in elements of vec_t for Q, K, V and O
    int64_t hq, hk, hv, hbias, ho, hlse;
    int64_t hsc;
};

// C = lanes per nonzero slot (16-byte column groups of this pass's tile of dv); the wave holds S = 64 / C slots
template <typename off_t, typename vec_t, int C>
__global__ __launch_bounds__(kBlock) void attention_half_slice_kernel(const AttnHalfArgs<vec_t> args, const off_t* __restrict__ Ap) {
    using acc_t = float;                // what attention_slice_walk.inc asks its includer
    using mh::load_cols;                // the lane's eight 16-bit columns, widened
    using mh::store_cols;               // and narrowed, once each
    constexpr int W = mh::kHalfV;       // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr float kNegInf = -std::numeric_limits<float>::infinity();
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = true;        // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
    const unsigned cut_block = blockIdx.x / unsigned(args.n_heads);     // the head varies fastest, as in attention_slice_kernel
    const AttnHalfArgs<vec_t> a = attn_args_of_head(args, blockIdx.x % unsigned(args.n_heads));
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
#include "attention_slice_walk.inc"     // the slice's nonzeros, 64 at a time: attention_slice_kernel's walk
}

// one thread per (head, slice, column), as attention_fixup_kernel: the row's only rounding to 16 bits
template <typename vec_t>
__global__ __launch_bounds__(kBlock) void attention_half_fixup_kernel(int64_t n_slices, int32_t dv, const AttnScratch<float> sc0,
                                                                      vec_t* __restrict__ O0, int64_t ldo, float* __restrict__ lse0,
                                                                      const AttnFixupHeads hd) {
    unsigned h;
    const int64_t gid = attn_head_thread(hd.per_head, h);
    const int j = int(gid % dv);
    const AttnScratch<float> sc = attn_scratch_of_head(sc0, h, hd.hsc);
    vec_t* O = attn_head_ptr(O0, h, hd.ho);
    float* lse = attn_head_ptr(lse0, h, hd.hlse);
    int32_t r;
    float m, l, acc;
    if (!attn_fixup_fold(n_slices, sc, gid / dv, j, r, m, l, acc)) return;
    O[int64_t(r) * ldo + j] = narrow_to(attn_out(acc, l), vec_t());
    if (j == 0 && lse) lse[r] = attn_lse(m, l);
}

// the kernels as attention.hip's launch path names them (AttnKernels<val_t>'s members): the passes run over tiles of
// W * 8 = 64 columns
template <typename vec_t>
struct AttnHalfKernels {
    static_assert(sizeof(vec_t) == 2, "16-bit Q, K, V and O");
    using elem_t = vec_t;
    using acc_t = float;
    using Args = AttnHalfArgs<vec_t>;
    static constexpr int W = mh::kHalfV;
    template <typename off_t, int C>
    static void slice(dim3 grid, hipStream_t s, const Args& a, const off_t* Ap) {
        hipLaunchKernelGGL((attention_half_slice_kernel<off_t, vec_t, C>), grid, dim3(kBlock), 0, s, a, Ap);
    }
    static void fixup(dim3 grid, hipStream_t s, const Args& a, int32_t dv) {
        hipLaunchKernelGGL((attention_half_fixup_kernel<vec_t>), grid, dim3(kBlock), 0, s, a.n_slices, dv, a.sc, a.O, a.ldo, a.lse,
                           AttnFixupHeads{uint32_t(attn_blocks_per_head(a.n_slices * dv)), a.hsc, a.ho, a.hlse});
    }
};

}  // namespace mi355
