// attention_bwd.hip — the fused backward of sparse attention (mi355_spmv_attention_bwd_*): dQ, dK and dV
// of O = softmax(scale Q K^T + bias, on the stored entries of A) V from Q, K, V, bias, O, dO and lse, with nothing of nnz
// size written (dbias apart, when it is asked for).  For every stored entry n = (r, c) of A:
//   v[n]     = scale * dot(Q[r, :d], K[c, :d]) + bias[n]            (rounded before + bias, as the forward)
//   p[n]     = v[n] == -inf ? +0 : exp(v[n] - lse[r])               (the test comes first: -inf - -inf is never formed)
//   delta[r] = dot(dO[r, :dv], O[r, :dv]);   dp[n] = dot(dO[r, :dv], V[c, :dv]);   ds[n] = p[n] * (dp[n] - delta[r])
//   dQ[r, :d]  = sum over row r    of (scale * ds[n]) * K[c, :d]
//   dK[c, :d]  = sum over column c of (scale * ds[n]) * Q[r, :d]
//   dV[c, :dv] = sum over column c of p[n] * dO[r, :dv]
//   dbias[n]   = ds[n]                                              (optional; nnz values in CSR order)
// O and lse are whatever the caller passes: nothing here assumes they came from this library's forward.
//
//   attention_bwd_delta_kernel   eight lanes per row: delta[r] into the object's scratch; each lane one fma chain from +0 over
//                                its columns in ascending order, then a fixed xor tree (one order of addition per row).
//   attention_bwd_slice_kernel   ONE walk in three roles.  The cut is the slice kinds' (slice_cut.hpp, slice_cut.inc,
//                                slice_cut_row.inc): one wave per slice of kSliceLen merge items, lanes = (nonzero slot x
//                                16-byte column group), C lanes per slot from the tile of the role's OUTPUT.
//                                  DQ  walks A:    the line is the query r, the gathered index the key c; out = dQ, the
//                                      coefficient is scale * ds and the gathered row K[c].  Its first pass stores dbias.
//                                  DK  walks A^T:  the line is the key c, the gathered index the query r, bias is read as
//                                      bias[perm[n']]; out = dK, coefficient scale * ds, gathered row Q[r].
//                                  DV  walks A^T:  out = dV, coefficient p, gathered row dO[r].
//                                A step: two dots on the slot's C lanes — the score over d and dp over dv, each SDDMM's tile
//                                loop (one fma chain from +0, ascending columns, then a fixed xor tree) — one exp, then the
//                                multi-vector walk's accumulation: a step inside one line that goes on folds coefficient *
//                                row into the slot's own partial (no scan); a step that holds a line's end joins the open
//                                partial to slot 0 and runs the segmented inclusive sum scan over the slots; the slot that
//                                holds a line's last entry stores the line of out.  Of the line carried in that ends here
//                                (HEAD piece) and of the line open at the slice's end (TAIL piece) only the sums are
//                                written, to the slice's two slots of scratch (row = -1 for none; every slot is rewritten
//                                by every execute).  Lines without entries get +0 in a pass of their own.
//                                A masked entry (bias = -inf) loads no row of Q, K, V or dO and contributes exactly +0.
//   attention_bwd_fixup_kernel   one thread per (slice, column): the first slice that carries a line adds its pieces in
//                                slice order — the tails, then the head of the slice it ends in — and stores the line.
//
// An output wider than the widest tile (32 fp32 / 16 fp64 columns) takes ceil(width / widest) launches of its role, each
// recomputing the coefficient.  A role whose output pointer is NULL is not launched.  No atomics, nothing allocated by an
// execute, nothing decided from device data: an execute launches kernels only (graph-capturable), and two executes give
// the same bits.  Order of addition: within a step the scan tree, then steps ascending, then slices ascending; the bits of
// a line of out depend on where the step and slice edges fall in that line of A (dQ) or of A^T (dK, dV) and on nothing else.
// Outputs must not overlap an input or each other (not checked).
#include <cmath>
#include <limits>
#include <new>

#include "slice_cut.hpp"

struct mi355_spmv_attention_bwd {   // the opaque handle of include/mi355_spmv.h
    int off_type = 0, val_type = 0;
    int32_t n_rows = 0, n_cols = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;
    int32_t d_max = 0, dv_max = 0;
    double scale = 1.0;
    int64_t n_slices = 0, n_slices_t = 0;   // of A and of A^T
    int64_t carry_ld = 0;           // max(d_max, dv_max) rounded up to whole widest tiles
    char* held = nullptr;           // perm, Ajt, Apt in one allocation (multi_transposed.hip's layout)
    size_t held_bytes = 0;
    void* scratch = nullptr;        // delta, then the slices' two pieces (rows and sums), shared by the roles in stream order
    size_t scratch_bytes = 0;
};

namespace mi355 {

#ifdef __clang__
// v = scale * dot is rounded before + bias, and partial + coefficient * column is a product and a sum, as the forward's
#pragma clang fp contract(off)
#endif

// The geometry that the host simulation's table is written for: tests/test_attention_bwd_cpu.py reads these two lines and
// holds tests/attention_bwd_cases.py to them.  The kernels use slice_cut.hpp's constants; a change there stops here.
constexpr int kAttentionBwdSlice = 1024;
constexpr int kAttentionBwdGroupsMax = 8;
static_assert(kAttentionBwdSlice == kSliceLen && kAttentionBwdGroupsMax == kSliceGroupsMax, "tests/attention_bwd_cases.py is tabled for this geometry");

enum { kBwdDQ = 0, kBwdDK = 1, kBwdDV = 2 };

// what a slice leaves for the fix-up: piece 0 = HEAD (the line carried in, which ends here), piece 1 = TAIL (the line open
// at the slice's end)
template <typename val_t>
struct AttnBwdScratch {
    val_t* delta;           // [n_rows]
    val_t* acc;             // [slices][2][carry_ld]
    int32_t* row;           // [slices][2]: the piece's line, or -1
    int64_t carry_ld;
};

inline size_t attn_bwd_scratch_bytes(int32_t n_rows, int64_t slices, int64_t carry_ld, size_t val_bytes) {
    const size_t delta = (size_t(n_rows) * val_bytes + 15) / 16 * 16;
    return delta + size_t(slices) * 2 * (size_t(carry_ld) * val_bytes + sizeof(int32_t)) + 16;      // (never nothing)
}

template <typename val_t>
AttnBwdScratch<val_t> attn_bwd_scratch(void* base, int32_t n_rows, int64_t slices, int64_t carry_ld) {
    AttnBwdScratch<val_t> sc;
    char* p = static_cast<char*>(base);
    sc.delta = reinterpret_cast<val_t*>(p); p += (size_t(n_rows) * sizeof(val_t) + 15) / 16 * 16;
    sc.acc = reinterpret_cast<val_t*>(p); p += size_t(slices) * 2 * size_t(carry_ld) * sizeof(val_t);
    sc.row = reinterpret_cast<int32_t*>(p);
    sc.carry_ld = carry_ld;
    return sc;
}

template <typename val_t>
struct AttnBwdArgs {
    int32_t n_rows;         // lines of the walked structure: A's rows (DQ) or A's columns (DK, DV)
    int64_t nnz, n_slices;
    const int32_t* Aj;      // the walked structure's gathered indices: Aj (DQ) or Ajt (DK, DV)
    const uint32_t* perm;   // DK, DV: the CSR slot of A behind a slot of A^T (bias is in A's order)
    const val_t* Q;
    const val_t* K;
    const val_t* V;
    const val_t* dO;
    const val_t* bias;      // null: none
    const val_t* lse;
    const val_t* delta;
    val_t* out;             // dQ, dK or dV
    val_t* dbias;           // DQ only; null: not asked for
    int64_t ldq, ldk, ldv, lddo, ldout;
    int32_t d, dv;
    int32_t col_begin;      // first column of this pass's tile of out
    int32_t cols;           // columns of it that exist (<= tile width): the others are masked on load and store
    int32_t q_vec, k_vec, v_vec, do_vec, out_vec;   // 1 = rows are 16-byte aligned: one 16-byte access per lane
    val_t scale;
    AttnBwdScratch<val_t> sc;
};

__device__ __forceinline__ float attn_bwd_fma(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
__device__ __forceinline__ double attn_bwd_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }
__device__ __forceinline__ float attn_bwd_exp(float d) { return expf(d); }
__device__ __forceinline__ double attn_bwd_exp(double d) { return exp(d); }

// the sum over all slots of a per-slot partial, in every lane of the column group (xor butterfly: the same bits everywhere)
template <typename val_t, int W, int C>
__device__ __forceinline__ void attn_bwd_reduce_slots(val_t (&v)[W]) {
#pragma unroll
    for (int d = C; d < kWave; d <<= 1)
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = v[j] + __shfl_xor(v[j], d);
}

// delta[r] = dot(dO[r, :dv], O[r, :dv]): kDeltaLanes lanes per row, so that a wave reads whole stretches of a row.  Lane g
// takes columns g, g + kDeltaLanes, ... in one fma chain from +0, then a fixed xor tree over the row's lanes: one order of
// addition per row, whatever the alignment.
constexpr int kDeltaLanes = 8;
template <typename val_t>
__global__ __launch_bounds__(kBlock) void attention_bwd_delta_kernel(int32_t n_rows, int32_t dv, const val_t* __restrict__ dO, int64_t lddo,
                                                                     const val_t* __restrict__ O, int64_t ldo, val_t* __restrict__ delta) {
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t r = gid / kDeltaLanes;
    const int g = int(gid % kDeltaLanes);
    const bool valid = r < n_rows;      // (every lane stays for the shuffles)
    val_t sum = val_t(0);
    if (valid) {
        const val_t* a = dO + r * lddo;
        const val_t* b = O + r * ldo;
        for (int32_t j = g; j < dv; j += kDeltaLanes) sum = attn_bwd_fma(a[j], b[j], sum);
    }
#pragma unroll
    for (int dd = 1; dd < kDeltaLanes; dd <<= 1) sum += __shfl_xor(sum, dd);
    if (valid && g == 0) delta[r] = sum;
}

// C = lanes per nonzero slot (16-byte column groups of this pass's tile of out); the wave holds S = 64 / C slots
template <typename off_t, typename val_t, int C, int ROLE>
__global__ __launch_bounds__(kBlock) void attention_bwd_slice_kernel(const AttnBwdArgs<val_t> a, const off_t* __restrict__ Ap) {
    constexpr int W = 16 / int(sizeof(val_t));      // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr val_t kNegInf = -std::numeric_limits<val_t>::infinity();
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = true;        // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
    const bool first_pass = a.col_begin == 0;
    const bool biased = a.bias != nullptr;
    const int nv = min(max(a.cols - c * W, 0), W);
    // the line carried in ends here with entries of its own (a slice inside one line is a tail; a line whose last entry
    // was the slice before's last item has nothing here)
    const bool has_head = carried_in && nr >= 1 && rel[1] >= 1 && rel[1] <= nn;

    val_t acc[W];           // per-slot partial of the open line (the line whose entries are not all seen yet)
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = val_t(0);
    int open_i = -1;        // that line, relative to r0; -1 = none (acc is +0)
    int holder = -1;        // >= 0: acc is not +0 in this slot only; -2: spread over the slots

    for (int base = 0; base < nn; base += kWave) {
        // 64 entries, one per lane, coalesced; each lane finds its entry's line in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        val_t bias = val_t(0);
        int ie = nr * 2;    // line * 2 + (1 = this entry is the last of its line); nr = no entry
        if (m < nn) {
            col = a.Aj[n0 + m];
            if (biased) {
                if constexpr (ROLE == kBwdDQ) bias = a.bias[n0 + m];
                else bias = a.bias[a.perm[n0 + m]];
            }
#include "slice_cut_row.inc"     // leaves lo: the entry's line, relative to r0
            ie = lo * 2 + (rel[lo + 1] == m + 1 ? 1 : 0);
        }
        const int left = nn - base;
        const int steps = slice_group_steps<C>(left);
        for (int t = 0; t < steps; ++t) {
            // slot s takes entry t * S + s of the 64
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
            // the entry's query and key: the line and the gathered index, or the other way round on A^T
            const int64_t qi = ROLE == kBwdDQ ? r0 + i_s : int64_t(col_s);
            const int64_t ki = ROLE == kBwdDQ ? int64_t(col_s) : r0 + i_s;
            // a masked edge loads nothing and contributes exactly +0
            const bool seen = live && !(biased && bias_s == kNegInf);

            // the two dots, each SDDMM's tile loop and then a fixed tree over the slot's C lanes: the score over d, dp over dv
            val_t part = val_t(0), dpart = val_t(0);
            if (seen) {
                const val_t* qp = a.Q + qi * a.ldq + c * W;
                const val_t* kp = a.K + ki * a.ldk + c * W;
                for (int32_t cb = 0; cb < a.d; cb += C * W) {       // the tiles of d: the same register all along
                    const int nd = min(max(a.d - cb - c * W, 0), W);
                    if (nd > 0) {
                        val_t q[W], k[W];
                        load_cols(q, qp + cb, nd, a.q_vec != 0);
                        load_cols(k, kp + cb, nd, a.k_vec != 0);
#pragma unroll
                        for (int j = 0; j < W; ++j) part = attn_bwd_fma(q[j], k[j], part);
                    }
                }
                const val_t* gp = a.dO + qi * a.lddo + c * W;
                const val_t* vp = a.V + ki * a.ldv + c * W;
                for (int32_t cb = 0; cb < a.dv; cb += C * W) {      // the tiles of dv
                    const int nd = min(max(a.dv - cb - c * W, 0), W);
                    if (nd > 0) {
                        val_t g[W], x[W];
                        load_cols(g, gp + cb, nd, a.do_vec != 0);
                        load_cols(x, vp + cb, nd, a.v_vec != 0);
#pragma unroll
                        for (int j = 0; j < W; ++j) dpart = attn_bwd_fma(g[j], x[j], dpart);
                    }
                }
            }
#pragma unroll
            for (int dd = 1; dd < C; dd <<= 1) {
                part += __shfl_xor(part, dd);
                dpart += __shfl_xor(dpart, dd);
            }
            // one exp; the coefficient of this role and the lane's W columns of the row it multiplies
            val_t coef = val_t(0), ds = val_t(0);
            val_t xv[W];
#pragma unroll
            for (int j = 0; j < W; ++j) xv[j] = val_t(0);
            if (seen) {
                val_t v = a.scale * part;
                if (biased) v = v + bias_s;
                if (v != kNegInf) {     // (the test comes before the subtraction)
                    const val_t p = attn_bwd_exp(v - a.lse[qi]);
                    ds = p * (dpart - a.delta[qi]);
                    if constexpr (ROLE == kBwdDQ) {
                        coef = a.scale * ds;
                        load_cols(xv, a.K + ki * a.ldk + a.col_begin + c * W, nv, a.k_vec != 0);
                    } else if constexpr (ROLE == kBwdDK) {
                        coef = a.scale * ds;
                        load_cols(xv, a.Q + qi * a.ldq + a.col_begin + c * W, nv, a.q_vec != 0);
                    } else {
                        coef = p;
                        load_cols(xv, a.dO + qi * a.lddo + a.col_begin + c * W, nv, a.do_vec != 0);
                    }
                }
            }
            if constexpr (ROLE == kBwdDQ) {
                // one writer per element: lane 0 of the slot, on the first pass
                if (live && c == 0 && first_pass && a.dbias) a.dbias[n0 + base + t * S + s] = ds;
            }
            val_t p[W];
#pragma unroll
            for (int j = 0; j < W; ++j) p[j] = coef * xv[j];

            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one line, and the line goes on: partials stay per slot
#pragma unroll
                for (int j = 0; j < W; ++j) acc[j] = acc[j] + p[j];
                open_i = i_first;
                holder = -2;
                continue;
            }
            // a line ends in this step (or the slice does).  The open line's partial joins slot 0, whose entry is the
            // next of that line; then a segmented inclusive scan over the slots sums each line's run of products.
            if (open_i >= 0) {
                if (holder >= 0) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
                } else {
                    attn_bwd_reduce_slots<val_t, W, C>(acc);
                }
                if (s == 0) {
#pragma unroll
                    for (int j = 0; j < W; ++j) p[j] = p[j] + acc[j];
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = val_t(0);
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
#pragma unroll
            for (int dd = C; dd < kWave; dd <<= 1) {
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const val_t o = __shfl_up(p[j], dd);
                    if (lane - c - dd >= start) p[j] = p[j] + o;
                }
            }
            const bool tail = s == S - 1 || ((heads >> (lane - c + C)) & 1ull);
            if (live && tail && (ie_s & 1)) {
                if (i_s == 0 && carried_in) {
                    // the HEAD piece: as computed, for the fix-up (whole tiles fit carry_ld)
                    val_t* hv = a.sc.acc + (w * 2 + 0) * a.sc.carry_ld + a.col_begin + c * W;
#pragma unroll
                    for (int j = 0; j < W; ++j) hv[j] = p[j];
                } else if (nv > 0) {
                    store_cols(p, a.out + (r0 + i_s) * a.ldout + a.col_begin + c * W, nv, a.out_vec != 0);
                }
            }
            // the last entry of the step: if its line goes on, its run's sum is the new open partial
            const int lv = min(S - 1, left - t * S - 1);
            const int ie_lv = __shfl(ie_s, lv * C);
            if (!(ie_lv & 1)) {
                open_i = ie_lv >> 1;
                holder = lv;
                if (s == lv) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = p[j];
                }
            } else {
                open_i = -1;
                holder = -1;
            }
        }
    }

    // the TAIL piece: what this slice holds of a line that ends in a later one
    if (open_i >= 0) {
        if (holder >= 0) {
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
        } else {
            attn_bwd_reduce_slots<val_t, W, C>(acc);
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
    }

    // lines without entries whose end lies in this slice: +0; a line with entries is stored where its last one is
    if (nv > 0) {
        val_t none[W];
#pragma unroll
        for (int j = 0; j < W; ++j) none[j] = val_t(0);
        for (int64_t r = r0 + s; r < r1; r += S)
            if (Ap[r] == Ap[r + 1]) store_cols(none, a.out + r * a.ldout + a.col_begin + c * W, nv, a.out_vec != 0);
    }
}

// one thread per (slice, column): the first slice that carries a line adds the line's pieces in slice order — the tails,
// then the head of the slice the line ends in — and stores the line of out
template <typename val_t>
__global__ __launch_bounds__(kBlock) void attention_bwd_fixup_kernel(int64_t n_slices, int32_t width, const AttnBwdScratch<val_t> sc,
                                                                     val_t* __restrict__ out, int64_t ldout) {
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t = gid / width;
    const int j = int(gid % width);
    if (t >= n_slices) return;
    const int32_t r = sc.row[t * 2 + 1];
    if (r < 0 || (t > 0 && sc.row[(t - 1) * 2 + 1] == r)) return;
    val_t sum = sc.acc[(t * 2 + 1) * sc.carry_ld + j];
    int64_t u = t + 1;
    for (; u < n_slices && sc.row[u * 2 + 1] == r; ++u) sum = sum + sc.acc[(u * 2 + 1) * sc.carry_ld + j];
    if (u < n_slices && sc.row[u * 2 + 0] == r) sum = sum + sc.acc[(u * 2 + 0) * sc.carry_ld + j];
    out[int64_t(r) * ldout + j] = sum;
}

// the operands of an execute as the entry points take them
struct AttnBwdOperands {
    int32_t d, dv;
    const void* Q; int64_t ldq;
    const void* K; int64_t ldk;
    const void* V; int64_t ldv;
    const void* bias;
    const void* O; int64_t ldo;
    const void* dO; int64_t lddo;
    const void* lse;
    void* dQ; int64_t lddq;
    void* dK; int64_t lddk;
    void* dV; int64_t lddv;
    void* dbias;
};

}  // namespace mi355

using namespace mi355;

namespace {

// argument-only checks of a create (also run by the one-shots before they make anything): the type refusals of
// mi355_spmv_attention_create, then the transpose's limit
int attention_bwd_check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                               const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown off_type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32) {
        set_error("%s: val_type MI355_VAL_I32 is not built (fp32 / fp64 values)", who);
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) {
        set_error("%s: val_type %d is not a type of Q, K, V, O and dO (F32 or F64; a 16-bit backward is not built)", who, val_type);
        return MI355_SPMV_EINVAL;
    }
    if (d_max < 1) { set_error("%s: d_max = %d below 1", who, d_max); return MI355_SPMV_EINVAL; }
    if (dv_max < 1) { set_error("%s: dv_max = %d below 1", who, dv_max); return MI355_SPMV_EINVAL; }
    if (const int st = check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    if (uint64_t(nnz) >= (1ull << 32)) { set_error("%s: nnz of 2^32 or more entries (the slot map is 32-bit)", who); return MI355_SPMV_ENOTSUP; }
    return MI355_SPMV_OK;
}

// argument-only checks of an execute (bias may be null; so may any of dQ, dK, dV, but not all three)
int attention_bwd_check_execute(const char* who, int32_t n_rows, int32_t n_cols, int64_t nnz, int32_t d_max, int32_t dv_max,
                                const AttnBwdOperands& o) {
    if (o.d < 1) { set_error("%s: d = %d below 1", who, o.d); return MI355_SPMV_EINVAL; }
    if (o.dv < 1) { set_error("%s: dv = %d below 1", who, o.dv); return MI355_SPMV_EINVAL; }
    if (o.d > d_max) { set_error("%s: d = %d above d_max = %d", who, o.d, d_max); return MI355_SPMV_EINVAL; }
    if (o.dv > dv_max) { set_error("%s: dv = %d above dv_max = %d", who, o.dv, dv_max); return MI355_SPMV_EINVAL; }
    if (o.ldq < o.d) { set_error("%s: ldq = %lld below d = %d", who, (long long)o.ldq, o.d); return MI355_SPMV_EINVAL; }
    if (o.ldk < o.d) { set_error("%s: ldk = %lld below d = %d", who, (long long)o.ldk, o.d); return MI355_SPMV_EINVAL; }
    if (o.ldv < o.dv) { set_error("%s: ldv = %lld below dv = %d", who, (long long)o.ldv, o.dv); return MI355_SPMV_EINVAL; }
    if (o.ldo < o.dv) { set_error("%s: ldo = %lld below dv = %d", who, (long long)o.ldo, o.dv); return MI355_SPMV_EINVAL; }
    if (o.lddo < o.dv) { set_error("%s: lddo = %lld below dv = %d", who, (long long)o.lddo, o.dv); return MI355_SPMV_EINVAL; }
    if (!o.dQ && !o.dK && !o.dV) { set_error("%s: dQ, dK and dV are all null (nothing to compute)", who); return MI355_SPMV_EINVAL; }
    if (o.dbias && !o.dQ) { set_error("%s: dbias without dQ (dbias comes from the walk that makes dQ)", who); return MI355_SPMV_EINVAL; }
    if (o.dQ && o.lddq < o.d) { set_error("%s: lddq = %lld below d = %d", who, (long long)o.lddq, o.d); return MI355_SPMV_EINVAL; }
    if (o.dK && o.lddk < o.d) { set_error("%s: lddk = %lld below d = %d", who, (long long)o.lddk, o.d); return MI355_SPMV_EINVAL; }
    if (o.dV && o.lddv < o.dv) { set_error("%s: lddv = %lld below dv = %d", who, (long long)o.lddv, o.dv); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !o.Q) { set_error("%s: null Q", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !o.K) { set_error("%s: null K", who); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !o.V) { set_error("%s: null V", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !o.O) { set_error("%s: null O", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !o.dO) { set_error("%s: null dO", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !o.lse) { set_error("%s: null lse", who); return MI355_SPMV_EINVAL; }
    (void)n_cols;
    return MI355_SPMV_OK;
}

int attention_bwd_lane_cols(int val_type) { return val_type == MI355_VAL_F64 ? 2 : 4; }
int attention_bwd_widest(int val_type) { return attention_bwd_lane_cols(val_type) * kSliceGroupsMax; }

int attention_bwd_free(mi355_spmv_attention_bwd* m) {
    int st = MI355_SPMV_OK;
    for (void* p : {static_cast<void*>(m->held), m->scratch}) {
        if (!p) continue;
        const hipError_t e = hipFree(p);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    delete m;
    return st;
}

// the object of checked arguments: the structure of A^T and the slot map in one allocation (the transpose synchronises
// the stream), the slices of both structures and the scratch
int attention_bwd_make(const char* who, mi355_spmv_attention_bwd** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                       const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max, hipStream_t s) {
    mi355_spmv_attention_bwd* m = new (std::nothrow) mi355_spmv_attention_bwd();
    if (!m) { set_error("%s: host allocation failed", who); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = val_type;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->Ap = Ap; m->Aj = Aj;
    m->d_max = d_max; m->dv_max = dv_max;
    m->n_slices = slice_count(n_rows, nnz);
    m->n_slices_t = slice_count(n_cols, nnz);
    const int widest = attention_bwd_widest(val_type);
    const int64_t wide = d_max > dv_max ? d_max : dv_max;
    m->carry_ld = (wide + widest - 1) / widest * widest;
    const size_t ob = off_type == MI355_OFF_I64 ? 8 : 4;
    m->held_bytes = size_t(nnz) * 8 + (size_t(n_cols) + 1) * ob;    // 8 nnz is a multiple of 8: Apt is aligned
    size_t ws_bytes = 0;
    int st = mi355_spmv_csr_transpose(off_type, n_rows, n_cols, nnz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ws_bytes, nullptr);
    if (st != MI355_SPMV_OK) { delete m; return st; }
    const auto failed = [&](const char* what, size_t bytes, hipError_t e) {
        set_error("%s: %s(%zu) -> %s", who, what, bytes, hipGetErrorString(e));
        (void)attention_bwd_free(m);
        return e == hipErrorOutOfMemory ? MI355_SPMV_ENOMEM : MI355_SPMV_EHIP;
    };
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->held), m->held_bytes);
    if (e != hipSuccess) { m->held = nullptr; return failed("hipMalloc", m->held_bytes, e); }
    const int64_t slices = m->n_slices > m->n_slices_t ? m->n_slices : m->n_slices_t;
    m->scratch_bytes = attn_bwd_scratch_bytes(n_rows, slices, m->carry_ld, val_type == MI355_VAL_F64 ? 8 : 4);
    e = hipMalloc(&m->scratch, m->scratch_bytes);
    if (e != hipSuccess) { m->scratch = nullptr; return failed("hipMalloc", m->scratch_bytes, e); }
    void* ws = nullptr;
    e = hipMalloc(&ws, ws_bytes ? ws_bytes : 1);
    if (e != hipSuccess) return failed("hipMalloc", ws_bytes, e);
    uint32_t* perm = reinterpret_cast<uint32_t*>(m->held);
    int32_t* Ajt = reinterpret_cast<int32_t*>(m->held + size_t(nnz) * 4);
    void* Apt = m->held + size_t(nnz) * 8;
    st = mi355_spmv_csr_transpose(off_type, n_rows, n_cols, nnz, Ap, Aj, Apt, Ajt, perm, ws, &ws_bytes, s);    // synchronises s
    e = hipFree(ws);
    if (st == MI355_SPMV_OK && e != hipSuccess) { set_error("%s: hipFree -> %s", who, hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    if (st != MI355_SPMV_OK) { (void)attention_bwd_free(m); return st; }
    *out = m;
    return MI355_SPMV_OK;
}

// the passes of one role over the tiles of its output, then its fix-up
template <typename off_t, typename val_t, int ROLE>
int attention_bwd_role(AttnBwdArgs<val_t>& a, const off_t* Ap, int32_t width, hipStream_t s) {
    constexpr int W = 16 / int(sizeof(val_t));
    constexpr int kWidest = W * kSliceGroupsMax;
    if (a.n_slices == 0) return MI355_SPMV_OK;      // no lines: nothing to write
    const dim3 grid(unsigned(slice_grid(a.n_slices))), block(kBlock);
    for (int32_t cb = 0; cb < width; cb += kWidest) {
        a.col_begin = cb;
        a.cols = width - cb < kWidest ? width - cb : kWidest;
        with_slot_lanes((a.cols + W - 1) / W, [&](auto lanes) {
            hipLaunchKernelGGL((attention_bwd_slice_kernel<off_t, val_t, decltype(lanes)::value, ROLE>), grid, block, 0, s, a, Ap);
        });
        MI355_HIP_TRY(hipGetLastError());
    }
    if (a.n_slices > 1) {
        const int64_t threads = a.n_slices * width;
        hipLaunchKernelGGL((attention_bwd_fixup_kernel<val_t>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s, a.n_slices, width, a.sc,
                           a.out, a.ldout);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

// delta, then the roles that are asked for, one behind the other on the stream (they share the pieces' scratch)
template <typename off_t, typename val_t>
int attention_bwd_launch(const mi355_spmv_attention_bwd& m, const AttnBwdOperands& o, hipStream_t s) {
    const int64_t slices = m.n_slices > m.n_slices_t ? m.n_slices : m.n_slices_t;
    AttnBwdArgs<val_t> a;
    a.nnz = m.nnz;
    a.Q = static_cast<const val_t*>(o.Q); a.K = static_cast<const val_t*>(o.K); a.V = static_cast<const val_t*>(o.V);
    a.dO = static_cast<const val_t*>(o.dO);
    a.bias = static_cast<const val_t*>(o.bias);
    a.lse = static_cast<const val_t*>(o.lse);
    a.ldq = o.ldq; a.ldk = o.ldk; a.ldv = o.ldv; a.lddo = o.lddo;
    a.d = o.d; a.dv = o.dv;
    a.q_vec = rows_aligned16<val_t>(o.Q, o.ldq) ? 1 : 0;
    a.k_vec = rows_aligned16<val_t>(o.K, o.ldk) ? 1 : 0;
    a.v_vec = rows_aligned16<val_t>(o.V, o.ldv) ? 1 : 0;
    a.do_vec = rows_aligned16<val_t>(o.dO, o.lddo) ? 1 : 0;
    a.scale = val_t(m.scale);
    a.sc = attn_bwd_scratch<val_t>(m.scratch, m.n_rows, slices, m.carry_ld);
    a.delta = a.sc.delta;
    a.col_begin = 0; a.cols = 0;
    if (m.n_rows > 0 && m.nnz > 0) {
        hipLaunchKernelGGL((attention_bwd_delta_kernel<val_t>), dim3(unsigned((int64_t(m.n_rows) * kDeltaLanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, m.n_rows,
                           o.dv, a.dO, o.lddo, static_cast<const val_t*>(o.O), o.ldo, a.sc.delta);
        MI355_HIP_TRY(hipGetLastError());
    }
    const auto role = [&](auto which, void* out, int64_t ldout, int32_t width) {
        a.out = static_cast<val_t*>(out);
        a.ldout = ldout;
        a.out_vec = rows_aligned16<val_t>(out, ldout) ? 1 : 0;
        constexpr int ROLE = decltype(which)::value;
        if constexpr (ROLE == kBwdDQ) {
            a.n_rows = m.n_rows; a.n_slices = m.n_slices;
            a.Aj = m.Aj; a.perm = nullptr;
            a.dbias = static_cast<val_t*>(o.dbias);
            return attention_bwd_role<off_t, val_t, ROLE>(a, static_cast<const off_t*>(m.Ap), width, s);
        } else {
            a.n_rows = m.n_cols; a.n_slices = m.n_slices_t;
            a.perm = reinterpret_cast<const uint32_t*>(m.held);
            a.Aj = reinterpret_cast<const int32_t*>(m.held + size_t(m.nnz) * 4);
            a.dbias = nullptr;
            return attention_bwd_role<off_t, val_t, ROLE>(a, reinterpret_cast<const off_t*>(m.held + size_t(m.nnz) * 8), width, s);
        }
    };
    if (o.dQ)
        if (const int st = role(std::integral_constant<int, kBwdDQ>(), o.dQ, o.lddq, o.d)) return st;
    if (o.dK)
        if (const int st = role(std::integral_constant<int, kBwdDK>(), o.dK, o.lddk, o.d)) return st;
    if (o.dV)
        if (const int st = role(std::integral_constant<int, kBwdDV>(), o.dV, o.lddv, o.dv)) return st;
    return MI355_SPMV_OK;
}

int attention_bwd_run(const mi355_spmv_attention_bwd& m, const AttnBwdOperands& o, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (m.off_type == MI355_OFF_I32)
        return m.val_type == MI355_VAL_F64 ? attention_bwd_launch<int32_t, double>(m, o, s) : attention_bwd_launch<int32_t, float>(m, o, s);
    return m.val_type == MI355_VAL_F64 ? attention_bwd_launch<int64_t, double>(m, o, s) : attention_bwd_launch<int64_t, float>(m, o, s);
}

// create, execute, synchronise, destroy; every argument check comes before any device call
int attention_bwd_one_shot(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                           const AttnBwdOperands& o, double scale, void* stream) {
    const char* const who = "attention_bwd";
    set_error("%s", "");
    if (const int st = attention_bwd_check_create(who, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, o.d < 1 ? 1 : o.d, o.dv < 1 ? 1 : o.dv)) return st;
    if (const int st = attention_bwd_check_execute(who, n_rows, n_cols, nnz, o.d, o.dv, o)) return st;
    mi355_spmv_attention_bwd* m = nullptr;
    int st = attention_bwd_make(who, &m, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv, static_cast<hipStream_t>(stream));
    if (st != MI355_SPMV_OK) return st;
    m->scale = scale;
    st = attention_bwd_run(*m, o, stream);
    if (st == MI355_SPMV_OK) st = mi355_spmv_stream_synchronize(stream);
    const int st2 = attention_bwd_free(m);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace

extern "C" {

int mi355_spmv_attention_bwd_create(mi355_spmv_attention_bwd** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                    const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max, void* stream) {
    set_error("%s", "");
    if (!out) { set_error("attention_bwd_create: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = attention_bwd_check_create("attention_bwd_create", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max)) return st;
    return attention_bwd_make("attention_bwd_create", out, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max,
                              static_cast<hipStream_t>(stream));
}

int mi355_spmv_attention_bwd_set_scale(mi355_spmv_attention_bwd* m, double scale) {
    set_error("%s", "");
    if (!m) { set_error("attention_bwd_set_scale: null object"); return MI355_SPMV_EINVAL; }
    m->scale = scale;
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_bwd_execute(mi355_spmv_attention_bwd* m, int32_t d, int32_t dv, const void* Q, int64_t ldq, const void* K, int64_t ldk,
                                     const void* V, int64_t ldv, const void* bias, const void* O, int64_t ldo, const void* dO, int64_t lddo,
                                     const void* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, void* dbias,
                                     void* stream) {
    set_error("%s", "");
    if (!m) { set_error("attention_bwd_execute: null object"); return MI355_SPMV_EINVAL; }
    const AttnBwdOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, dO, lddo, lse, dQ, lddq, dK, lddk, dV, lddv, dbias};
    if (const int st = attention_bwd_check_execute("attention_bwd_execute", m->n_rows, m->n_cols, m->nnz, m->d_max, m->dv_max, o)) return st;
    return attention_bwd_run(*m, o, stream);
}

int mi355_spmv_attention_bwd_get_info(const mi355_spmv_attention_bwd* m, mi355_spmv_attention_bwd_info* info) {
    if (!m || !info) { set_error("attention_bwd_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->d_max = m->d_max; info->dv_max = m->dv_max;
    info->widest_tile = attention_bwd_widest(m->val_type);
    const int per_lane = attention_bwd_lane_cols(m->val_type);
    const int32_t widths[3] = {m->d_max, m->d_max, m->dv_max};      // the outputs of DQ, DK, DV
    for (int i = 0; i < 3; ++i) {
        info->passes[i] = (widths[i] + info->widest_tile - 1) / info->widest_tile;
        const int cols = widths[i] < info->widest_tile ? widths[i] : info->widest_tile;
        with_slot_lanes((cols + per_lane - 1) / per_lane, [&](auto lanes) { info->lanes_per_slot[i] = decltype(lanes)::value; });
    }
    info->n_slices = m->n_slices;
    info->grid_blocks = slice_grid(m->n_slices);
    info->n_slices_t = m->n_slices_t;
    info->grid_blocks_t = slice_grid(m->n_slices_t);
    info->scratch_bytes = int64_t(m->scratch_bytes);
    info->held_bytes = int64_t(m->held_bytes);
    snprintf(info->main_kernel, sizeof(info->main_kernel), "attention_bwd_slice_kernel");
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_bwd_destroy(mi355_spmv_attention_bwd* m) {
    if (!m) return MI355_SPMV_OK;
    return attention_bwd_free(m);
}

#define MI355_SPMV_DEFINE_ATTENTION_BWD(SUF, OFF, OFFENUM, VAL, VALENUM)                                                       \
    int mi355_spmv_attention_bwd_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, int32_t d, int32_t dv, \
                                       const VAL* Q, int64_t ldq, const VAL* K, int64_t ldk, const VAL* V, int64_t ldv, const VAL* bias, \
                                       double scale, const VAL* O, int64_t ldo, const VAL* dO, int64_t lddo, const VAL* lse, VAL* dQ, \
                                       int64_t lddq, VAL* dK, int64_t lddk, VAL* dV, int64_t lddv, VAL* dbias, void* stream) {  \
        const AttnBwdOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, dO, lddo, lse, dQ, lddq, dK, lddk, dV, lddv, dbias}; \
        return attention_bwd_one_shot(OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, o, scale, stream);               \
    }
MI355_SPMV_DEFINE_ATTENTION_BWD(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION_BWD(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_ATTENTION_BWD(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION_BWD(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

}  // extern "C"
