// attention.hip — fused sparse attention on the structure of A (mi355_spmv_attention_*): the chain
// SDDMM -> row softmax -> multi-vector SpMV in ONE pass over A, with nothing of nnz size written.
//   v[n]     = scale * dot(Q[r, :d], K[c, :d]) + bias[n]              for every stored entry n = (r, c) of A
//   m_r      = max over the row of v,   l_r = sum over the row of exp(v - m_r)
//   O[r,:dv] = (sum over the row of exp(v[n] - m_r) * V[c, :dv]) / l_r,        lse[r] = m_r + log(l_r)     (optional)
// An object of its own beside mi355_spmv_sddmm / _row_softmax / _multi: the kernels, the one launch path of both storage
// types and the extern "C" entry points, in this unit; what it shares with the backward (the checks, the pieces' walk, the
// loop over the tiles) is attention_common.hpp's.
//
// Masked edges: bias[n] = -inf contributes exactly +0 (its row of V is not multiplied in).  A row that is empty or masked
// whole gets O = +0 and lse = -inf, not NaN.  A row of one unmasked entry gives O = V[c] and lse = v exactly.
//
// The cut is the slice kinds' (slice_cut.hpp, slice_cut.inc, slice_cut_row.inc): one WAVE per slice of kSliceLen merge
// items, lanes = (nonzero slot x 16-byte column group), C lanes per slot from the width of this pass's tile of dv.
//
//   attention_slice_kernel   per step a slot takes one nonzero (column, row and bias by shuffles, as the multi-vector walk).
//                            The score: lane c gathers its 16 bytes of K[col] and Q[row] and runs SDDMM's tile loop over d
//                            (one fma chain from +0, ascending columns; then a fixed xor tree over the C lanes), v = scale *
//                            dot is rounded, then + bias.  The state of a run of one row is (m, l, acc[W per lane]) under
//                                (m, l, a) + (m', l', a') = (M = max(m, m'), l e + l' e', a e + a' e'),  e = exp(m - M), e' = exp(m' - M)
//                            with exp(0) = 1 and exp(-inf) = +0 by a branch, and a side with m = -inf contributing 0.
//                            A step inside one row that goes on folds its entries into per-slot states, no scan (hub rows).
//                            A step that holds a row end: the open row's state is folded over the slots once and joins slot
//                            0; a segmented max scan over the slots gives every run's M, each entry takes ONE exp, and the
//                            multi-vector kind's segmented sum scan carries l beside the W columns.  The slot that holds a
//                            row's last nonzero divides by l and stores O[r] (and lse[r]) contiguously.  Of the row carried
//                            in that ends here (HEAD piece) and of the row open at the slice's end (TAIL piece) only the
//                            state is written: (row, m, l, acc[whole tiles]) in the slice's two slots of scratch, row = -1
//                            for none; every slot is rewritten by every execute.  Empty rows whose end lies in the slice
//                            are written in a pass of their own at the end of the walk.
//   attention_fixup_kernel   one THREAD per (slice, column): the first slice that carries a row folds its chain with the
//                            monoid — tails in slice order, then the ending slice's head — and writes O[r] = acc / l;
//                            column 0 writes lse[r].
//
// Q, K, V and O in 16 bits under fp32 bias, lse, scale, states and arithmetic (mi355_spmv_attention_create_half, §3.15.1):
// the same object and the same walk (attention_slice_walk.inc) in a kernel of its own, attention_half_kernel.hpp.
//
// dv above the widest tile (32 fp32 / 16 fp64 / 64 16-bit columns): ceil(dv / widest) launches of the slice kernel inside the one
// execute.  Each recomputes the scores (the same bits: the score does not depend on the tile); only the first stores lse
// and the pieces' (row, m, l).  d is unbounded: the tile loop.
// No atomics, no finish pass, nothing of nnz size written, the host decides nothing from device data: an execute launches
// kernels only (graph-capturable), and two executes give the same bits.  The bits of O DO depend on where the step and
// slice edges fall in a row, as row softmax's do.  O and lse must not overlap an input (not checked).
#include <cmath>
#include <limits>
#include <new>

#include "attention_common.hpp"

struct mi355_spmv_attention {       // the opaque handle of include/mi355_spmv.h
    int off_type = 0, val_type = 0;
    int vec_type = 0;               // the type of Q, K, V and O: val_type, or F16 / BF16 under F32 everything else (create_half)
    int32_t n_rows = 0, n_cols = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;
    int32_t d_max = 0, dv_max = 0;
    double scale = 1.0;
    int64_t n_slices = 0;
    int64_t carry_ld = 0;           // dv_max rounded up to whole widest tiles
    void* scratch = nullptr;        // the slices' two pieces: rows, (m, l) and acc; n_heads_max copies, head h at h * head stride
    size_t scratch_bytes = 0;
    size_t head_bytes = 0;          // of one head's copy (what a create allocates)
    int32_t n_heads_max = 1;        // reserve_heads
};

namespace mi355 {

#ifdef __clang__
// v = scale * dot is rounded before + bias, and a e + a' e' is two products and a sum: a row of equal scores has
// v - m = 0 and e = 1 in every kernel, and the monoid gives the same bits with its sides swapped
#pragma clang fp contract(off)
#endif

// The geometry that the host simulation's table is written for: tests/test_attention_sim_cpu.py reads these two lines and
// holds tests/attention_cases.py to them.  The kernels use slice_cut.hpp's constants; a change there stops here.
constexpr int kAttentionSlice = 1024;
constexpr int kAttentionGroupsMax = 8;
static_assert(kAttentionSlice == kSliceLen && kAttentionGroupsMax == kSliceGroupsMax, "tests/attention_cases.py is tabled for this geometry");

// what a slice leaves for the fix-up: piece 0 = HEAD (the row carried in, which ends here), piece 1 = TAIL (the row open
// at the slice's end).  O(n_slices * dv_max), owned by the object.
template <typename val_t>
struct AttnScratch {
    val_t* acc;             // [n_slices][2][carry_ld]
    val_t* ml;              // [n_slices][2][2]: m, l
    int32_t* row;           // [n_slices][2]: the piece's row, or -1
    int64_t carry_ld;
};

inline size_t attn_scratch_bytes(int64_t n_slices, int64_t carry_ld, size_t val_bytes) {
    return size_t(n_slices) * 2 * (size_t(carry_ld) * val_bytes + 2 * val_bytes + sizeof(int32_t));
}

template <typename val_t>
AttnScratch<val_t> attn_scratch(void* base, int64_t n_slices, int64_t carry_ld) {
    AttnScratch<val_t> sc;
    char* p = static_cast<char*>(base);
    sc.acc = reinterpret_cast<val_t*>(p); p += size_t(n_slices) * 2 * size_t(carry_ld) * sizeof(val_t);
    sc.ml = reinterpret_cast<val_t*>(p); p += size_t(n_slices) * 4 * sizeof(val_t);
    sc.row = reinterpret_cast<int32_t*>(p);
    sc.carry_ld = carry_ld;
    return sc;
}

template <typename val_t>
struct AttnArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const val_t* Q;
    const val_t* K;
    const val_t* V;
    const val_t* bias;      // null: none
    val_t* O;
    val_t* lse;             // null: not asked for
    int64_t ldq, ldk, ldv, ldo;
    int32_t d;
    int32_t col_begin;      // first column of this pass's tile of dv (0: the pass that stores lse and the pieces' row, m, l)
    int32_t cols;           // columns of it that exist (<= tile width): the others are masked on load and store
    int32_t q_vec, k_vec, v_vec, o_vec;     // 1 = rows are 16-byte aligned: one 16-byte access per lane
    val_t scale;
    AttnScratch<val_t> sc;
    int32_t n_heads;        // heads in this launch: workgroup b serves head b % n_heads
    int64_t hq, hk, hv, hbias, ho, hlse;    // elements between two heads of an operand (0: shared; not read with one head)
    int64_t hsc;            // bytes between two heads' scratch
};

// The scratch of head h: the single-head layout at h * bytes.
template <typename acc_t>
__device__ __forceinline__ AttnScratch<acc_t> attn_scratch_of_head(AttnScratch<acc_t> sc, int64_t h, int64_t bytes) {
    sc.acc = attn_head_scratch(sc.acc, h, bytes);
    sc.ml = attn_head_scratch(sc.ml, h, bytes);
    sc.row = attn_head_scratch(sc.row, h, bytes);
    return sc;
}

// A slice kernel's local copy of its arguments, rebased to head h (AttnArgs<val_t> or AttnHalfArgs<vec_t>): the walk then
// reads a.Q, a.K, ... as it does with one head.
template <typename Args>
__device__ __forceinline__ Args attn_args_of_head(Args a, int64_t h) {
    a.Q = attn_head_ptr(a.Q, h, a.hq);
    a.K = attn_head_ptr(a.K, h, a.hk);
    a.V = attn_head_ptr(a.V, h, a.hv);
    a.bias = attn_head_ptr(a.bias, h, a.hbias);
    a.O = attn_head_ptr(a.O, h, a.ho);
    a.lse = attn_head_ptr(a.lse, h, a.hlse);
    a.sc = attn_scratch_of_head(a.sc, h, a.hsc);
    return a;
}

// exp of a difference d = m - M <= 0: exactly 1 at 0 and exactly +0 at -inf, whatever the math library gives at its ends
template <typename val_t>
__device__ __forceinline__ val_t attn_exp_diff(val_t d) {
    if (d == val_t(0)) return val_t(1);
    if (d == -std::numeric_limits<val_t>::infinity()) return val_t(0);
    return attn_exp(d);
}

// the factor of a side with maximum m under the common maximum M: a side with m = -inf contributes 0 (M may be -inf too)
template <typename val_t>
__device__ __forceinline__ val_t attn_side(val_t m, val_t M) {
    return m == -std::numeric_limits<val_t>::infinity() ? val_t(0) : attn_exp_diff(m - M);
}

// a finished row: O = acc / l and lse = m + log(l); a row without an unmasked entry (l = 0) is +0 and -inf
template <typename val_t>
__device__ __forceinline__ val_t attn_out(val_t acc, val_t l) { return l == val_t(0) ? val_t(0) : acc / l; }
template <typename val_t>
__device__ __forceinline__ val_t attn_lse(val_t m, val_t l) {
    return l == val_t(0) ? -std::numeric_limits<val_t>::infinity() : m + attn_log(l);
}

// the open row's per-slot states folded over all slots, in every lane of the column group: an xor butterfly of the monoid
// (the same bits everywhere: max and the sum of two products are commutative)
template <typename val_t, int W, int C>
__device__ __forceinline__ void attn_reduce_slots(val_t& m, val_t& l, val_t (&acc)[W]) {
#pragma unroll
    for (int d = C; d < kWave; d <<= 1) {
        const val_t m2 = __shfl_xor(m, d);
        const val_t l2 = __shfl_xor(l, d);
        const val_t M = m < m2 ? m2 : m;
        const val_t e = attn_side(m, M), e2 = attn_side(m2, M);
        l = l * e + l2 * e2;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const val_t a2 = __shfl_xor(acc[j], d);
            acc[j] = acc[j] * e + a2 * e2;
        }
        m = M;
    }
}

// C = lanes per nonzero slot (16-byte column groups of this pass's tile of dv); the wave holds S = 64 / C slots
template <typename off_t, typename val_t, int C>
__global__ __launch_bounds__(kBlock) void attention_slice_kernel(const AttnArgs<val_t> args, const off_t* __restrict__ Ap) {
    using acc_t = val_t;                            // what attention_slice_walk.inc asks its includer
    constexpr int W = 16 / int(sizeof(val_t));      // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr val_t kNegInf = -std::numeric_limits<val_t>::infinity();
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = true;        // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
    // the head varies fastest over the grid: the workgroups that read one range of Ap / Aj are dispatched together
    const unsigned cut_block = blockIdx.x / unsigned(args.n_heads);
    const AttnArgs<val_t> a = attn_args_of_head(args, blockIdx.x % unsigned(args.n_heads));
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
#include "attention_slice_walk.inc"     // the slice's nonzeros, 64 at a time, and its empty rows
}

// the fix-up's thread of (slice t, column j): if t is the first slice that carries a row, that row and its state folded
// over the row's pieces in the order of attn_piece_chain; otherwise false
template <typename acc_t>
__device__ __forceinline__ bool attn_fixup_fold(int64_t n_slices, const AttnScratch<acc_t>& sc, int64_t t, int j, int32_t& r, acc_t& m, acc_t& l,
                                                acc_t& acc) {
    return attn_piece_chain(
        n_slices, sc.row, t, r, [&](int64_t piece) { m = sc.ml[piece * 2]; l = sc.ml[piece * 2 + 1]; acc = sc.acc[piece * sc.carry_ld + j]; },
        [&](int64_t piece) {      // (m, l, acc) + the piece's state, the piece being the later side
            const acc_t m2 = sc.ml[piece * 2], l2 = sc.ml[piece * 2 + 1], a2 = sc.acc[piece * sc.carry_ld + j];
            const acc_t M = m < m2 ? m2 : m;
            const acc_t e = attn_side(m, M), e2 = attn_side(m2, M);
            l = l * e + l2 * e2;
            acc = acc * e + a2 * e2;
            m = M;
        });
}

// what the fix-up needs of the heads: how many, and what lies between two heads of the scratch, of O and of lse
struct AttnFixupHeads {
    uint32_t per_head;      // workgroups per head (attn_blocks_per_head of n_slices * dv)
    int64_t hsc, ho, hlse;
};

// one thread per (head, slice, column), every head whole workgroups: the first slice that carries a row folds the row's pieces and writes the row of O;
// column 0 writes lse
template <typename val_t>
__global__ __launch_bounds__(kBlock) void attention_fixup_kernel(int64_t n_slices, int32_t dv, const AttnScratch<val_t> sc0, val_t* __restrict__ O0,
                                                                 int64_t ldo, val_t* __restrict__ lse0, const AttnFixupHeads hd) {
    unsigned h;
    const int64_t gid = attn_head_thread(hd.per_head, h);
    const int j = int(gid % dv);
    const AttnScratch<val_t> sc = attn_scratch_of_head(sc0, h, hd.hsc);
    val_t* O = attn_head_ptr(O0, h, hd.ho);
    val_t* lse = attn_head_ptr(lse0, h, hd.hlse);
    int32_t r;
    val_t m, l, acc;
    if (!attn_fixup_fold(n_slices, sc, gid / dv, j, r, m, l, acc)) return;
    O[int64_t(r) * ldo + j] = attn_out(acc, l);
    if (j == 0 && lse) lse[r] = attn_lse(m, l);
}

// the operands of an execute as the entry points take them
struct AttnOperands {
    int32_t d, dv;
    const void* Q; int64_t ldq;
    const void* K; int64_t ldk;
    const void* V; int64_t ldv;
    const void* bias;
    void* O; int64_t ldo;
    void* lse;
};

}  // namespace mi355

#include "attention_half_kernel.hpp"    // (down here: its kernels use AttnScratch and the fold)

using namespace mi355;

namespace {

// argument-only checks of a create (also run by the one-shots before they make anything)
int attention_check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                           const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    if (const int st = attn_check_types(who, off_type, val_type, "Q, K, V and O", "mi355_spmv_attention_create_half")) return st;
    if (d_max < 1) { set_error("%s: d_max = %d below 1", who, d_max); return MI355_SPMV_EINVAL; }
    if (dv_max < 1) { set_error("%s: dv_max = %d below 1", who, dv_max); return MI355_SPMV_EINVAL; }
    return check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj);
}

// the checks of create_half (and of the 16-bit one-shots): vec_type first, then what a create of fp32 values checks
int attention_check_create_half(const char* who, int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                                const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    if (const int st = attn_check_half_type(who, vec_type, "Q, K, V and O")) return st;
    return attention_check_create(who, off_type, MI355_VAL_F32, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max);
}

// argument-only checks of an execute (bias and lse may be null)
int attention_check_execute(const char* who, int32_t n_rows, int64_t nnz, int32_t d_max, int32_t dv_max, const AttnOperands& o) {
    if (const int st = attn_check_widths(who, o.d, o.dv, d_max, dv_max, o.ldq, o.ldk, o.ldv, o.ldo)) return st;
    return attn_check_inputs(who, n_rows, nnz, o.Q, o.K, o.V, o.O);
}

// the object of checked arguments: the slices and their scratch (the only device call of a create: one hipMalloc)
int attention_make(const char* who, mi355_spmv_attention** out, int off_type, int val_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                   const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    mi355_spmv_attention* m = new (std::nothrow) mi355_spmv_attention();
    if (!m) { set_error("%s: host allocation failed", who); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = val_type; m->vec_type = vec_type;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->Ap = Ap; m->Aj = Aj;
    m->d_max = d_max; m->dv_max = dv_max;
    m->n_slices = slice_count(n_rows, nnz);
    const int widest = attn_widest(vec_type);
    m->carry_ld = (int64_t(dv_max) + widest - 1) / widest * widest;
    if (m->n_slices > 0) {      // (no rows: nothing is ever launched, nothing allocated)
        m->scratch_bytes = m->head_bytes = attn_scratch_bytes(m->n_slices, m->carry_ld, val_type == MI355_VAL_F64 ? 8 : 4);
        const hipError_t e = hipMalloc(&m->scratch, m->scratch_bytes);
        if (e != hipSuccess) {
            set_error("%s: hipMalloc(%zu) -> %s", who, m->scratch_bytes, hipGetErrorString(e));
            delete m;
            return e == hipErrorOutOfMemory ? MI355_SPMV_ENOMEM : MI355_SPMV_EHIP;
        }
    }
    *out = m;
    return MI355_SPMV_OK;
}

// The kernels of one storage type as the launch path below names them: elem_t is the type of Q, K, V and O, acc_t that of
// bias, lse, scale and the scratch, W a lane's columns.  AttnHalfKernels<vec_t> (attention_half_kernel.hpp) has the same members.
template <typename val_t>
struct AttnKernels {
    using elem_t = val_t;
    using acc_t = val_t;
    using Args = AttnArgs<val_t>;
    static constexpr int W = 16 / int(sizeof(val_t));
    template <typename off_t, int C>
    static void slice(dim3 grid, hipStream_t s, const Args& a, const off_t* Ap) {
        hipLaunchKernelGGL((attention_slice_kernel<off_t, val_t, C>), grid, dim3(kBlock), 0, s, a, Ap);
    }
    static void fixup(dim3 grid, hipStream_t s, const Args& a, int32_t dv) {
        hipLaunchKernelGGL((attention_fixup_kernel<val_t>), grid, dim3(kBlock), 0, s, a.n_slices, dv, a.sc, a.O, a.ldo, a.lse,
                           AttnFixupHeads{uint32_t(attn_blocks_per_head(a.n_slices * dv)), a.hsc, a.ho, a.hlse});
    }
};

// the passes over the tiles of dv, then the fix-up: n_heads heads in every launch (hs is not read with one head)
template <typename off_t, typename K>
int attention_launch(const mi355_spmv_attention& m, const AttnOperands& o, int32_t n_heads, const mi355_spmv_attention_head_strides* hs, hipStream_t s) {
    using elem_t = typename K::elem_t;
    using acc_t = typename K::acc_t;
    typename K::Args a;
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.Aj = m.Aj;
    a.Q = static_cast<const elem_t*>(o.Q); a.K = static_cast<const elem_t*>(o.K); a.V = static_cast<const elem_t*>(o.V);
    a.bias = static_cast<const acc_t*>(o.bias);
    a.O = static_cast<elem_t*>(o.O); a.lse = static_cast<acc_t*>(o.lse);
    a.ldq = o.ldq; a.ldk = o.ldk; a.ldv = o.ldv; a.ldo = o.ldo;
    a.d = o.d;
    const mi355_spmv_attention_head_strides h = n_heads > 1 ? *hs : mi355_spmv_attention_head_strides{0, 0, 0, 0, 0, 0};
    a.n_heads = n_heads;
    a.hq = h.q; a.hk = h.k; a.hv = h.v; a.hbias = h.bias; a.ho = h.o; a.hlse = h.lse;
    a.hsc = int64_t(attn_head_scratch_stride(m.head_bytes));
    a.q_vec = attn_rows_vec<elem_t>(o.Q, o.ldq, n_heads, h.q) ? 1 : 0;
    a.k_vec = attn_rows_vec<elem_t>(o.K, o.ldk, n_heads, h.k) ? 1 : 0;
    a.v_vec = attn_rows_vec<elem_t>(o.V, o.ldv, n_heads, h.v) ? 1 : 0;
    a.o_vec = attn_rows_vec<elem_t>(o.O, o.ldo, n_heads, h.o) ? 1 : 0;
    a.scale = acc_t(m.scale);
    a.sc = attn_scratch<acc_t>(m.scratch, m.n_slices, m.carry_ld);
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    return attn_tile_passes<K::W>(
        a, o.dv, [&](dim3 grid, auto lanes) { K::template slice<off_t, decltype(lanes)::value>(grid, s, a, Ap); },
        [&](dim3 grid) { K::fixup(grid, s, a, o.dv); });
}

int attention_run(const mi355_spmv_attention& m, const AttnOperands& o, int32_t n_heads, const mi355_spmv_attention_head_strides* hs, void* stream) {
    if (m.n_rows == 0) return MI355_SPMV_OK;        // no rows: nothing to write, nothing launched
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool i32 = m.off_type == MI355_OFF_I32;
    auto run = [&](auto off, auto kernels) { return attention_launch<decltype(off), decltype(kernels)>(m, o, n_heads, hs, s); };
    auto either = [&](auto kernels) { return i32 ? run(int32_t(), kernels) : run(int64_t(), kernels); };
    if (m.vec_type == MI355_VAL_F16) return either(AttnHalfKernels<F16>());     // 16-bit Q, K, V and O under fp32 everything else
    if (m.vec_type == MI355_VAL_BF16) return either(AttnHalfKernels<Bf16>());
    return m.val_type == MI355_VAL_F64 ? either(AttnKernels<double>()) : either(AttnKernels<float>());
}

// create, execute, synchronise, destroy (the scratch must outlive the kernels, as the multi-vector one-shots' does);
// every argument check comes before any device call
int attention_one_shot(int off_type, int val_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                       const AttnOperands& o, double scale, void* stream) {
    set_error("%s", "");
    if (const int st = attention_check_execute("attention", n_rows, nnz, o.d, o.dv, o)) return st;
    if (const int st = vec_type != val_type ? attention_check_create_half("attention_half", off_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv)
                                            : attention_check_create("attention", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv))
        return st;
    if (n_rows == 0) return MI355_SPMV_OK;
    mi355_spmv_attention* m = nullptr;
    int st = attention_make("attention", &m, off_type, val_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv);
    if (st != MI355_SPMV_OK) return st;
    m->scale = scale;
    st = attention_run(*m, o, 1, nullptr, stream);
    if (st == MI355_SPMV_OK) st = mi355_spmv_stream_synchronize(stream);
    const int st2 = mi355_spmv_attention_destroy(m);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace

extern "C" {

int mi355_spmv_attention_create(int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int off_type, int val_type,
                                int32_t d_max, int32_t dv_max, mi355_spmv_attention** out) {
    set_error("%s", "");
    if (!out) { set_error("attention_create: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = attention_check_create("attention_create", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max)) return st;
    return attention_make("attention_create", out, off_type, val_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max);
}

int mi355_spmv_attention_create_half(mi355_spmv_attention** out, int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                     const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    set_error("%s", "");
    if (!out) { set_error("attention_create_half: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = attention_check_create_half("attention_create_half", off_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max)) return st;
    return attention_make("attention_create_half", out, off_type, MI355_VAL_F32, vec_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max);
}

int mi355_spmv_attention_get_types(const mi355_spmv_attention* m, int* val_type, int* vec_type) {
    if (!m || !val_type || !vec_type) { set_error("attention_get_types: null argument"); return MI355_SPMV_EINVAL; }
    *val_type = m->val_type;
    *vec_type = m->vec_type;
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_set_scale(mi355_spmv_attention* m, double scale) {
    set_error("%s", "");
    if (!m) { set_error("attention_set_scale: null object"); return MI355_SPMV_EINVAL; }
    m->scale = scale;
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_execute(mi355_spmv_attention* m, int32_t d, int32_t dv, const void* Q, int64_t ldq, const void* K, int64_t ldk,
                                 const void* V, int64_t ldv, const void* bias, void* O, int64_t ldo, void* lse, void* stream) {
    set_error("%s", "");
    if (!m) { set_error("attention_execute: null object"); return MI355_SPMV_EINVAL; }
    const AttnOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse};
    if (const int st = attention_check_execute("attention_execute", m->n_rows, m->nnz, m->d_max, m->dv_max, o)) return st;
    return attention_run(*m, o, 1, nullptr, stream);
}

int mi355_spmv_attention_reserve_heads(mi355_spmv_attention* m, int32_t n_heads_max) {
    set_error("%s", "");
    if (!m) { set_error("attention_reserve_heads: null object"); return MI355_SPMV_EINVAL; }
    if (n_heads_max < 1) { set_error("attention_reserve_heads: n_heads_max = %d below 1", n_heads_max); return MI355_SPMV_EINVAL; }
    void* fresh = nullptr;
    const size_t bytes = attn_heads_scratch_bytes(m->head_bytes, n_heads_max);
    const int st = attn_reserve_scratch("attention_reserve_heads", &m->scratch, bytes, &fresh);
    if (bytes == 0 || fresh) { m->scratch_bytes = bytes; m->n_heads_max = n_heads_max; }
    return st;
}

int mi355_spmv_attention_get_heads_max(const mi355_spmv_attention* m, int32_t* n_heads_max) {
    if (!m || !n_heads_max) { set_error("attention_get_heads_max: null argument"); return MI355_SPMV_EINVAL; }
    *n_heads_max = m->n_heads_max;
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_execute_heads(mi355_spmv_attention* m, int32_t n_heads, const mi355_spmv_attention_head_strides* hs, int32_t d, int32_t dv,
                                       const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const void* bias, void* O,
                                       int64_t ldo, void* lse, void* stream) {
    const char* const who = "attention_execute_heads";
    set_error("%s", "");
    if (!m) { set_error("%s: null object", who); return MI355_SPMV_EINVAL; }
    const AttnOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse};
    if (const int st = attention_check_execute(who, m->n_rows, m->nnz, m->d_max, m->dv_max, o)) return st;
    if (const int st = attn_check_n_heads(who, n_heads, m->n_heads_max, hs)) return st;
    if (n_heads > 1) {
        const std::pair<const char*, int64_t> all[] = {{"q", hs->q}, {"k", hs->k}, {"v", hs->v}, {"bias", hs->bias}, {"o", hs->o}, {"lse", hs->lse}};
        for (const auto& [name, stride] : all)
            if (const int st = attn_check_stride_sign(who, name, stride)) return st;
        if (const int st = attn_check_out_stride(who, "o", n_heads, hs->o, m->n_rows, dv, ldo)) return st;
        if (lse && m->n_rows > 0)
            if (const int st = attn_check_out_vector_stride(who, "lse", hs->lse, m->n_rows, "n_rows")) return st;
    }
    if (const int st = attn_check_heads_grid(who, n_heads, m->n_slices, dv)) return st;
    return attention_run(*m, o, n_heads, hs, stream);
}

int mi355_spmv_attention_get_info(const mi355_spmv_attention* m, mi355_spmv_attention_info* info) {
    if (!m || !info) { set_error("attention_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->d_max = m->d_max; info->dv_max = m->dv_max;
    info->widest_tile = attn_widest(m->vec_type);
    info->passes = (m->dv_max + info->widest_tile - 1) / info->widest_tile;
    const int cols = m->dv_max < info->widest_tile ? m->dv_max : info->widest_tile;
    const int per_lane = info->widest_tile / kSliceGroupsMax;
    with_slot_lanes((cols + per_lane - 1) / per_lane, [&](auto lanes) { info->lanes_per_slot = decltype(lanes)::value; });
    info->n_slices = m->n_slices;
    info->grid_blocks = slice_grid(m->n_slices);
    info->scratch_bytes = int64_t(m->scratch_bytes);
    snprintf(info->main_kernel, sizeof(info->main_kernel), m->vec_type != m->val_type ? "attention_half_slice_kernel" : "attention_slice_kernel");
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_destroy(mi355_spmv_attention* m) {
    if (!m) return MI355_SPMV_OK;
    int st = MI355_SPMV_OK;
    if (m->scratch) {
        const hipError_t e = hipFree(m->scratch);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    delete m;
    return st;
}

#define MI355_SPMV_DEFINE_ATTENTION(SUF, OFF, OFFENUM, VAL, VALENUM)                                                          \
    int mi355_spmv_attention_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, int32_t d, int32_t dv, \
                                   const VAL* Q, int64_t ldq, const VAL* K, int64_t ldk, const VAL* V, int64_t ldv, const VAL* bias, \
                                   double scale, VAL* O, int64_t ldo, VAL* lse, void* stream) {                               \
        const AttnOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse};                                               \
        return attention_one_shot(OFFENUM, VALENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, o, scale, stream);                  \
    }
MI355_SPMV_DEFINE_ATTENTION(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_ATTENTION(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

#define MI355_SPMV_DEFINE_ATTENTION_HALF(SUF, OFF, OFFENUM, VECENUM)                                                          \
    int mi355_spmv_attention_half_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, int32_t d, int32_t dv, \
                                        const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,   \
                                        const float* bias, double scale, void* O, int64_t ldo, float* lse, void* stream) {    \
        const AttnOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse};                                               \
        return attention_one_shot(OFFENUM, MI355_VAL_F32, VECENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, o, scale, stream);   \
    }
MI355_SPMV_DEFINE_ATTENTION_HALF(i32_f16, int32_t, MI355_OFF_I32, MI355_VAL_F16)
MI355_SPMV_DEFINE_ATTENTION_HALF(i32_bf16, int32_t, MI355_OFF_I32, MI355_VAL_BF16)
MI355_SPMV_DEFINE_ATTENTION_HALF(i64_f16, int64_t, MI355_OFF_I64, MI355_VAL_F16)
MI355_SPMV_DEFINE_ATTENTION_HALF(i64_bf16, int64_t, MI355_OFF_I64, MI355_VAL_BF16)

}  // extern "C"
