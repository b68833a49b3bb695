// attention.hip — fused sparse attention on the structure of A (mi355_spmv_attention_*): the chain
// SDDMM -> row softmax -> multi-vector SpMV in ONE pass over A, with nothing of nnz size written.
//   v[n]     = scale * dot(Q[r, :d], K[c, :d]) + bias[n]              for every stored entry n = (r, c) of A
//   m_r      = max over the row of v,   l_r = sum over the row of exp(v - m_r)
//   O[r,:dv] = (sum over the row of exp(v[n] - m_r) * V[c, :dv]) / l_r,        lse[r] = m_r + log(l_r)     (optional)
// An object of its own beside mi355_spmv_sddmm / _row_softmax / _multi: the kernels, their launch and the extern "C" entry
// points, all in this unit.
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
// dv above the widest tile (32 fp32 / 16 fp64 columns): ceil(dv / widest) launches of the slice kernel inside the one
// execute.  Each recomputes the scores (the same bits: the score does not depend on the tile); only the first stores lse
// and the pieces' (row, m, l).  d is unbounded: the tile loop.
// No atomics, no finish pass, nothing of nnz size written, the host decides nothing from device data: an execute launches
// kernels only (graph-capturable), and two executes give the same bits.  The bits of O DO depend on where the step and
// slice edges fall in a row, as row softmax's do.  O and lse must not overlap an input (not checked).
#include <cmath>
#include <limits>
#include <new>

#include "slice_cut.hpp"

struct mi355_spmv_attention {       // the opaque handle of include/mi355_spmv.h
    int off_type = 0, val_type = 0;
    int32_t n_rows = 0, n_cols = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;
    int32_t d_max = 0, dv_max = 0;
    double scale = 1.0;
    int64_t n_slices = 0;
    int64_t carry_ld = 0;           // dv_max rounded up to whole widest tiles
    void* scratch = nullptr;        // the slices' two pieces: rows, (m, l) and acc
    size_t scratch_bytes = 0;
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
};

__device__ __forceinline__ float attn_fma(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
__device__ __forceinline__ double attn_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }
__device__ __forceinline__ float attn_exp(float d) { return expf(d); }
__device__ __forceinline__ double attn_exp(double d) { return exp(d); }
__device__ __forceinline__ float attn_log(float d) { return logf(d); }
__device__ __forceinline__ double attn_log(double d) { return log(d); }

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
__global__ __launch_bounds__(kBlock) void attention_slice_kernel(const AttnArgs<val_t> a, const off_t* __restrict__ Ap) {
    constexpr int W = 16 / int(sizeof(val_t));      // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr val_t kNegInf = -std::numeric_limits<val_t>::infinity();
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = true;        // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in

    const bool first_pass = a.col_begin == 0;
    const bool biased = a.bias != nullptr;
    const int nv = min(max(a.cols - c * W, 0), W);
    // the row carried in ends here with nonzeros of its own (a slice inside one row is a tail; a row whose last nonzero
    // was the slice before's last item has nothing here)
    const bool has_head = carried_in && nr >= 1 && rel[1] >= 1 && rel[1] <= nn;

    // per-slot state of the open row (the row whose nonzeros are not all seen yet)
    val_t m_o = kNegInf, l_o = val_t(0), acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = val_t(0);
    int open_i = -1;        // that row, relative to r0; -1 = none (the state is the identity)
    int holder = -1;        // >= 0: the state is not the identity in this slot only; -2: spread over the slots

    for (int base = 0; base < nn; base += kWave) {
        // 64 nonzeros, one per lane, coalesced; each lane finds its nonzero's row in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        val_t bias = val_t(0);
        int ie = nr * 2;    // row * 2 + (1 = this nonzero is the last of its row); nr = no nonzero
        if (m < nn) {
            col = a.Aj[n0 + m];
            if (biased) bias = a.bias[n0 + m];
#include "slice_cut_row.inc"     // leaves lo: the nonzero's row, relative to r0
            ie = lo * 2 + (rel[lo + 1] == m + 1 ? 1 : 0);
        }
        const int left = nn - base;
        const int steps = slice_group_steps<C>(left);
        for (int t = 0; t < steps; ++t) {
            // slot s takes nonzero t * S + s of the 64
            int32_t col_s = col;
            val_t bias_s = bias;
            int ie_s = ie;
            if constexpr (C > 1) {
                const int src = t * S + s;
                col_s = __shfl(col, src);
                bias_s = __shfl(bias, src);
                ie_s = __shfl(ie, src);
            }
            const int i_s = ie_s >> 1;
            const bool live = i_s < nr;

            // the score: SDDMM's tile loop over d, then a fixed tree over the slot's C lanes
            val_t part = val_t(0);
            if (live) {
                const val_t* qp = a.Q + (r0 + i_s) * a.ldq + c * W;
                const val_t* kp = a.K + int64_t(col_s) * a.ldk + c * W;
                for (int32_t cb = 0; cb < a.d; cb += C * W) {       // the tiles of d: the same register all along
                    const int nd = min(max(a.d - cb - c * W, 0), W);
                    if (nd > 0) {
                        val_t q[W], k[W];
                        load_cols<val_t, W>(q, qp + cb, nd, a.q_vec != 0);
                        load_cols<val_t, W>(k, kp + cb, nd, a.k_vec != 0);
#pragma unroll
                        for (int j = 0; j < W; ++j) part = attn_fma(q[j], k[j], part);
                    }
                }
            }
#pragma unroll
            for (int dd = 1; dd < C; dd <<= 1) part += __shfl_xor(part, dd);
            val_t v = kNegInf;
            val_t xv[W];
#pragma unroll
            for (int j = 0; j < W; ++j) xv[j] = val_t(0);
            if (live) {
                v = a.scale * part;
                if (biased) v = v + bias_s;
                // (a masked edge contributes +0 whatever its row of V holds)
                if (v != kNegInf) load_cols<val_t, W>(xv, a.V + int64_t(col_s) * a.ldv + a.col_begin + c * W, nv, a.v_vec != 0);
            }

            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one row, and the row goes on: the entry joins its slot's state, one exp
                const bool up = v > m_o;
                const val_t low = up ? m_o : v;
                const val_t f = low == kNegInf ? val_t(0) : attn_exp_diff(up ? m_o - v : v - m_o);
                const val_t e = up ? f : val_t(1), ev = v == kNegInf ? val_t(0) : up ? val_t(1) : f;
                l_o = l_o * e + ev;
#pragma unroll
                for (int j = 0; j < W; ++j) acc[j] = acc[j] * e + ev * xv[j];
                if (up) m_o = v;
                open_i = i_first;
                holder = -2;
                continue;
            }
            // a row ends in this step (or the slice does).  The open row's state, folded once, joins slot 0, whose
            // nonzero is the next of that row.
            const bool joins = open_i >= 0 && s == 0;
            if (open_i >= 0) {
                if (holder >= 0) {
                    m_o = __shfl(m_o, holder * C + c);
                    l_o = __shfl(l_o, holder * C + c);
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
                } else {
                    attn_reduce_slots<val_t, W, C>(m_o, l_o, acc);
                }
            }
            // the runs of one row over the slots, and each run's maximum M in every one of its lanes
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
            const int behind = lane - c + C;
            const unsigned long long later = behind >= kWave ? 0ull : heads >> behind;
            const int end = later ? behind + __builtin_ctzll(later) - C : kWave - C;     // lane c == 0 of its last slot
            val_t mx = joins && m_o > v ? m_o : v;
#pragma unroll
            for (int dd = C; dd < kWave; dd <<= 1) {
                const val_t o = __shfl_up(mx, dd);
                if (lane - c - dd >= start && o > mx) mx = o;
            }
            const val_t M = __shfl(mx, end + c);
            // one exp per entry; the open row's state is rescaled into slot 0
            const val_t e = attn_side(v, M);
            val_t lp = e, p[W];
#pragma unroll
            for (int j = 0; j < W; ++j) p[j] = e * xv[j];
            if (joins) {
                const val_t eo = attn_side(m_o, M);
                lp = l_o * eo + lp;
#pragma unroll
                for (int j = 0; j < W; ++j) p[j] = acc[j] * eo + p[j];
            }
            m_o = kNegInf;
            l_o = val_t(0);
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = val_t(0);
            // the segmented inclusive sum scan of the multi-vector walk, l beside the W columns
#pragma unroll
            for (int dd = C; dd < kWave; dd <<= 1) {
                const val_t ol = __shfl_up(lp, dd);
                const bool in_run = lane - c - dd >= start;
                if (in_run) lp = lp + ol;
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const val_t o = __shfl_up(p[j], dd);
                    if (in_run) p[j] = p[j] + o;
                }
            }
            if (live && lane - c == end && (ie_s & 1)) {
                if (i_s == 0 && carried_in) {
                    // the HEAD piece: the state as computed, for the fix-up (whole tiles fit carry_ld)
                    val_t* hv = a.sc.acc + (w * 2 + 0) * a.sc.carry_ld + a.col_begin + c * W;
#pragma unroll
                    for (int j = 0; j < W; ++j) hv[j] = p[j];
                    if (c == 0 && first_pass) {
                        a.sc.ml[(w * 2 + 0) * 2 + 0] = M;
                        a.sc.ml[(w * 2 + 0) * 2 + 1] = lp;
                    }
                } else {
                    const int64_t r = r0 + i_s;
                    if (nv > 0) {
                        val_t o[W];
#pragma unroll
                        for (int j = 0; j < W; ++j) o[j] = attn_out(p[j], lp);
                        store_cols<val_t, W>(o, a.O + r * a.ldo + a.col_begin + c * W, nv, a.o_vec != 0);
                    }
                    if (c == 0 && first_pass && a.lse) a.lse[r] = attn_lse(M, lp);
                }
            }
            // the last nonzero of the step: if its row goes on, its run's state is the new open state
            const int lv = min(S - 1, left - t * S - 1);
            const int ie_lv = __shfl(ie_s, lv * C);
            if (!(ie_lv & 1)) {
                open_i = ie_lv >> 1;
                holder = lv;
                if (s == lv) {
                    m_o = M;
                    l_o = lp;
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = p[j];
                }
            } else {
                open_i = -1;
                holder = -1;
            }
        }
    }

    // the TAIL piece: what this slice holds of a row that ends in a later one
    if (open_i >= 0) {
        if (holder >= 0) {
            m_o = __shfl(m_o, holder * C + c);
            l_o = __shfl(l_o, holder * C + c);
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
        } else {
            attn_reduce_slots<val_t, W, C>(m_o, l_o, acc);
        }
        if (s == 0) {
            val_t* tv = a.sc.acc + (w * 2 + 1) * a.sc.carry_ld + a.col_begin + c * W;      // (carry_ld covers whole tiles)
#pragma unroll
            for (int j = 0; j < W; ++j) tv[j] = acc[j];
        }
    }
    if (lane == 0 && first_pass) {
        a.sc.row[w * 2 + 0] = has_head ? int32_t(r0) : -1;
        a.sc.row[w * 2 + 1] = open_i >= 0 ? int32_t(r0 + open_i) : -1;
        if (open_i >= 0) {
            a.sc.ml[(w * 2 + 1) * 2 + 0] = m_o;
            a.sc.ml[(w * 2 + 1) * 2 + 1] = l_o;
        }
    }

    // empty rows whose end lies in this slice: O = +0 and lse = -inf; a row with nonzeros is stored where its last one is
    // (and a row carried in has nonzeros: an empty row is never a piece)
    if (nv > 0 || (c == 0 && first_pass && a.lse)) {
        val_t none[W];
#pragma unroll
        for (int j = 0; j < W; ++j) none[j] = val_t(0);
        for (int64_t r = r0 + s; r < r1; r += S) {
            if (Ap[r] == Ap[r + 1]) {
                if (nv > 0) store_cols<val_t, W>(none, a.O + r * a.ldo + a.col_begin + c * W, nv, a.o_vec != 0);
                if (c == 0 && first_pass && a.lse) a.lse[r] = kNegInf;
            }
        }
    }
}

// one thread per (slice, column): the first slice that carries a row folds the row's pieces in slice order — the tails,
// then the head of the slice the row ends in — and writes the row of O; column 0 writes lse
template <typename val_t>
__global__ __launch_bounds__(kBlock) void attention_fixup_kernel(int64_t n_slices, int32_t dv, const AttnScratch<val_t> sc, val_t* __restrict__ O,
                                                                 int64_t ldo, val_t* __restrict__ lse) {
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t = gid / dv;
    const int j = int(gid % dv);
    if (t >= n_slices) return;
    const int32_t r = sc.row[t * 2 + 1];
    if (r < 0 || (t > 0 && sc.row[(t - 1) * 2 + 1] == r)) return;
    val_t m = sc.ml[(t * 2 + 1) * 2], l = sc.ml[(t * 2 + 1) * 2 + 1], acc = sc.acc[(t * 2 + 1) * sc.carry_ld + j];
    const auto fold = [&](int64_t piece) {      // (m, l, acc) + the piece's state, the piece being the later side
        const val_t m2 = sc.ml[piece * 2], l2 = sc.ml[piece * 2 + 1], a2 = sc.acc[piece * sc.carry_ld + j];
        const val_t M = m < m2 ? m2 : m;
        const val_t e = attn_side(m, M), e2 = attn_side(m2, M);
        l = l * e + l2 * e2;
        acc = acc * e + a2 * e2;
        m = M;
    };
    int64_t u = t + 1;
    for (; u < n_slices && sc.row[u * 2 + 1] == r; ++u) fold(u * 2 + 1);
    if (u < n_slices && sc.row[u * 2 + 0] == r) fold(u * 2 + 0);
    O[int64_t(r) * ldo + j] = attn_out(acc, l);
    if (j == 0 && lse) lse[r] = attn_lse(m, l);
}

}  // namespace mi355

using namespace mi355;

namespace {

// argument-only checks of a create (also run by the one-shots before they make anything)
int attention_check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                           const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown off_type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32) {
        set_error("%s: val_type MI355_VAL_I32 is not built (fp32 / fp64 values)", who);
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) {
        set_error("%s: val_type %d is not a type of Q, K, V and O (F32 or F64; 16-bit values are not built)", who, val_type);
        return MI355_SPMV_EINVAL;
    }
    if (d_max < 1) { set_error("%s: d_max = %d below 1", who, d_max); return MI355_SPMV_EINVAL; }
    if (dv_max < 1) { set_error("%s: dv_max = %d below 1", who, dv_max); return MI355_SPMV_EINVAL; }
    return check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj);
}

// argument-only checks of an execute (bias and lse may be null)
int attention_check_execute(const char* who, int32_t n_rows, int64_t nnz, int32_t d_max, int32_t dv_max, int32_t d, int32_t dv, const void* Q,
                            int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const void* O, int64_t ldo) {
    if (d < 1) { set_error("%s: d = %d below 1", who, d); return MI355_SPMV_EINVAL; }
    if (dv < 1) { set_error("%s: dv = %d below 1", who, dv); return MI355_SPMV_EINVAL; }
    if (d > d_max) { set_error("%s: d = %d above d_max = %d", who, d, d_max); return MI355_SPMV_EINVAL; }
    if (dv > dv_max) { set_error("%s: dv = %d above dv_max = %d", who, dv, dv_max); return MI355_SPMV_EINVAL; }
    if (ldq < d) { set_error("%s: ldq = %lld below d = %d", who, (long long)ldq, d); return MI355_SPMV_EINVAL; }
    if (ldk < d) { set_error("%s: ldk = %lld below d = %d", who, (long long)ldk, d); return MI355_SPMV_EINVAL; }
    if (ldv < dv) { set_error("%s: ldv = %lld below dv = %d", who, (long long)ldv, dv); return MI355_SPMV_EINVAL; }
    if (ldo < dv) { set_error("%s: ldo = %lld below dv = %d", who, (long long)ldo, dv); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !Q) { set_error("%s: null Q", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !K) { set_error("%s: null K", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !V) { set_error("%s: null V", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !O) { set_error("%s: null O", who); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

int attention_widest(int val_type) { return (val_type == MI355_VAL_F64 ? 2 : 4) * kSliceGroupsMax; }

// the object of checked arguments: the slices and their scratch (the only device call of a create: one hipMalloc)
int attention_make(const char* who, mi355_spmv_attention** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                   const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    mi355_spmv_attention* m = new (std::nothrow) mi355_spmv_attention();
    if (!m) { set_error("%s: host allocation failed", who); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = val_type;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->Ap = Ap; m->Aj = Aj;
    m->d_max = d_max; m->dv_max = dv_max;
    m->n_slices = slice_count(n_rows, nnz);
    const int widest = attention_widest(val_type);
    m->carry_ld = (int64_t(dv_max) + widest - 1) / widest * widest;
    if (m->n_slices > 0) {      // (no rows: nothing is ever launched, nothing allocated)
        m->scratch_bytes = attn_scratch_bytes(m->n_slices, m->carry_ld, val_type == MI355_VAL_F64 ? 8 : 4);
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

struct AttnOperands {
    int32_t d, dv;
    const void* Q; int64_t ldq;
    const void* K; int64_t ldk;
    const void* V; int64_t ldv;
    const void* bias;
    void* O; int64_t ldo;
    void* lse;
};

// the passes over the tiles of dv, then the fix-up
template <typename off_t, typename val_t>
int attention_launch(const mi355_spmv_attention& m, const AttnOperands& o, hipStream_t s) {
    constexpr int W = 16 / int(sizeof(val_t));
    constexpr int kWidest = W * kSliceGroupsMax;
    AttnArgs<val_t> a;
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.Aj = m.Aj;
    a.Q = static_cast<const val_t*>(o.Q); a.K = static_cast<const val_t*>(o.K); a.V = static_cast<const val_t*>(o.V);
    a.bias = static_cast<const val_t*>(o.bias);
    a.O = static_cast<val_t*>(o.O); a.lse = static_cast<val_t*>(o.lse);
    a.ldq = o.ldq; a.ldk = o.ldk; a.ldv = o.ldv; a.ldo = o.ldo;
    a.d = o.d;
    a.q_vec = rows_aligned16<val_t>(o.Q, o.ldq) ? 1 : 0;
    a.k_vec = rows_aligned16<val_t>(o.K, o.ldk) ? 1 : 0;
    a.v_vec = rows_aligned16<val_t>(o.V, o.ldv) ? 1 : 0;
    a.o_vec = rows_aligned16<val_t>(o.O, o.ldo) ? 1 : 0;
    a.scale = val_t(m.scale);
    a.sc = attn_scratch<val_t>(m.scratch, m.n_slices, m.carry_ld);
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    for (int32_t cb = 0; cb < o.dv; cb += kWidest) {
        a.col_begin = cb;
        a.cols = o.dv - cb < kWidest ? o.dv - cb : kWidest;
        with_slot_lanes((a.cols + W - 1) / W, [&](auto lanes) {
            hipLaunchKernelGGL((attention_slice_kernel<off_t, val_t, decltype(lanes)::value>), grid, block, 0, s, a, Ap);
        });
        MI355_HIP_TRY(hipGetLastError());
    }
    if (m.n_slices > 1) {
        const int64_t threads = m.n_slices * o.dv;
        hipLaunchKernelGGL((attention_fixup_kernel<val_t>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s, m.n_slices, o.dv, a.sc,
                           a.O, o.ldo, a.lse);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

int attention_run(const mi355_spmv_attention& m, const AttnOperands& o, void* stream) {
    if (m.n_rows == 0) return MI355_SPMV_OK;        // no rows: nothing to write, nothing launched
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (m.off_type == MI355_OFF_I32)
        return m.val_type == MI355_VAL_F64 ? attention_launch<int32_t, double>(m, o, s) : attention_launch<int32_t, float>(m, o, s);
    return m.val_type == MI355_VAL_F64 ? attention_launch<int64_t, double>(m, o, s) : attention_launch<int64_t, float>(m, o, s);
}

// create, execute, synchronise, destroy (the scratch must outlive the kernels, as the multi-vector one-shots' does);
// every argument check comes before any device call
int attention_one_shot(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                       const AttnOperands& o, double scale, void* stream) {
    set_error("%s", "");
    if (const int st = attention_check_execute("attention", n_rows, nnz, o.d, o.dv, o.d, o.dv, o.Q, o.ldq, o.K, o.ldk, o.V, o.ldv, o.O, o.ldo))
        return st;
    if (const int st = attention_check_create("attention", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv)) return st;
    if (n_rows == 0) return MI355_SPMV_OK;
    mi355_spmv_attention* m = nullptr;
    int st = attention_make("attention", &m, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv);
    if (st != MI355_SPMV_OK) return st;
    m->scale = scale;
    st = attention_run(*m, o, stream);
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
    return attention_make("attention_create", out, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max);
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
    if (const int st = attention_check_execute("attention_execute", m->n_rows, m->nnz, m->d_max, m->dv_max, d, dv, Q, ldq, K, ldk, V, ldv, O, ldo))
        return st;
    const AttnOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse};
    return attention_run(*m, o, stream);
}

int mi355_spmv_attention_get_info(const mi355_spmv_attention* m, mi355_spmv_attention_info* info) {
    if (!m || !info) { set_error("attention_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->d_max = m->d_max; info->dv_max = m->dv_max;
    info->widest_tile = attention_widest(m->val_type);
    info->passes = (m->dv_max + info->widest_tile - 1) / info->widest_tile;
    const int cols = m->dv_max < info->widest_tile ? m->dv_max : info->widest_tile;
    const int per_lane = info->widest_tile / kSliceGroupsMax;
    with_slot_lanes((cols + per_lane - 1) / per_lane, [&](auto lanes) { info->lanes_per_slot = decltype(lanes)::value; });
    info->n_slices = m->n_slices;
    info->grid_blocks = slice_grid(m->n_slices);
    info->scratch_bytes = int64_t(m->scratch_bytes);
    snprintf(info->main_kernel, sizeof(info->main_kernel), "attention_slice_kernel");
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
        return attention_one_shot(OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, o, scale, stream);                  \
    }
MI355_SPMV_DEFINE_ATTENTION(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_ATTENTION(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

}  // extern "C"
