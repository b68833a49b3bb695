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
// O and lse are whatever the caller passes: nothing here assumes they came from this library's forward.  What the two
// directions share (the checks, the pieces' walk, the loop over the tiles) is attention_common.hpp's.
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
// Q, K, V, O, dO, dQ, dK and dV in 16 bits under fp32 bias, lse, dbias, delta, scale, partials, pieces and arithmetic
// (mi355_spmv_attention_bwd_create_half, §3.15.3): the same object and the same walk (attention_bwd_slice_walk.inc) in
// kernels of their own, attention_bwd_half_kernel.hpp.
//
// An output wider than the widest tile (32 fp32 / 16 fp64 / 64 16-bit columns) takes ceil(width / widest) launches of its role, each
// recomputing the coefficient.  A role whose output pointer is NULL is not launched.  No atomics, nothing allocated by an
// execute, nothing decided from device data: an execute launches kernels only (graph-capturable), and two executes give
// the same bits.  Order of addition: within a step the scan tree, then steps ascending, then slices ascending; the bits of
// a line of out depend on where the step and slice edges fall in that line of A (dQ) or of A^T (dK, dV) and on nothing else.
// Outputs must not overlap an input or each other (not checked).
#include <cmath>
#include <limits>
#include <new>

#include "attention_common.hpp"

struct mi355_spmv_attention_bwd {   // the opaque handle of include/mi355_spmv.h
    int off_type = 0, val_type = 0;
    int vec_type = 0;               // the type of Q, K, V, O, dO, dQ, dK, dV: val_type, or F16 / BF16 under F32 everything else (create_half)
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
    void* scratch = nullptr;        // delta, then the slices' two pieces (rows and sums), shared by the roles in stream order;
                                    // n_heads_max copies, head h at h * head stride
    size_t scratch_bytes = 0;
    size_t head_bytes = 0;          // of one head's copy (what a create allocates)
    int32_t n_heads_max = 1;        // reserve_heads
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
    int32_t n_heads;        // heads in this launch: workgroup b serves head b % n_heads
    int64_t hq, hk, hv, hdo, hbias, hlse, hout, hdbias;     // elements between two heads of an operand (0: shared)
    int64_t hsc;            // bytes between two heads' scratch
};

// The scratch of head h: the single-head layout at h * bytes.
template <typename acc_t>
__device__ __forceinline__ AttnBwdScratch<acc_t> attn_bwd_scratch_of_head(AttnBwdScratch<acc_t> sc, int64_t h, int64_t bytes) {
    sc.delta = attn_head_scratch(sc.delta, h, bytes);
    sc.acc = attn_head_scratch(sc.acc, h, bytes);
    sc.row = attn_head_scratch(sc.row, h, bytes);
    return sc;
}

// A slice kernel's local copy of its arguments, rebased to head h (AttnBwdArgs<val_t> or AttnBwdHalfArgs<vec_t>)
template <typename Args>
__device__ __forceinline__ Args attn_bwd_args_of_head(Args a, int64_t h) {
    a.Q = attn_head_ptr(a.Q, h, a.hq);
    a.K = attn_head_ptr(a.K, h, a.hk);
    a.V = attn_head_ptr(a.V, h, a.hv);
    a.dO = attn_head_ptr(a.dO, h, a.hdo);
    a.bias = attn_head_ptr(a.bias, h, a.hbias);
    a.lse = attn_head_ptr(a.lse, h, a.hlse);
    a.out = attn_head_ptr(a.out, h, a.hout);
    a.dbias = attn_head_ptr(a.dbias, h, a.hdbias);
    a.sc = attn_bwd_scratch_of_head(a.sc, h, a.hsc);
    a.delta = a.sc.delta;
    return a;
}

// what the delta kernel and the fix-up need of the heads: how many, and what lies between two heads of the scratch and of
// their operands (delta: dO and O; fix-up: out)
struct AttnBwdHeads {
    int32_t n_heads;
    uint32_t per_head;      // workgroups per head (attn_blocks_per_head of the head's threads)
    int64_t hsc, ha, hb;
};

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
                                                                     const val_t* __restrict__ O, int64_t ldo, val_t* __restrict__ delta0,
                                                                     const AttnBwdHeads hd) {
    unsigned h;
    const int64_t gid = attn_head_thread(hd.per_head, h);
    const int64_t r = gid / kDeltaLanes;
    const int g = int(gid % kDeltaLanes);
    const bool valid = r < n_rows;      // (every lane stays for the shuffles)
    val_t* delta = attn_head_scratch(delta0, h, hd.hsc);
    val_t sum = val_t(0);
    if (valid) {
        const val_t* a = dO + h * hd.ha + r * lddo;
        const val_t* b = O + h * hd.hb + r * ldo;
        for (int32_t j = g; j < dv; j += kDeltaLanes) sum = attn_fma(a[j], b[j], sum);
    }
#pragma unroll
    for (int dd = 1; dd < kDeltaLanes; dd <<= 1) sum += __shfl_xor(sum, dd);
    if (valid && g == 0) delta[r] = sum;
}

// C = lanes per nonzero slot (16-byte column groups of this pass's tile of out); the wave holds S = 64 / C slots
template <typename off_t, typename val_t, int C, int ROLE>
__global__ __launch_bounds__(kBlock) void attention_bwd_slice_kernel(const AttnBwdArgs<val_t> args, const off_t* __restrict__ Ap) {
    using acc_t = val_t;                            // what attention_bwd_slice_walk.inc asks its includer
    constexpr int W = 16 / int(sizeof(val_t));      // columns of a lane per tile
    constexpr int S = kWave / C;
    constexpr val_t kNegInf = -std::numeric_limits<val_t>::infinity();
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = true;        // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
    // the head varies fastest over the grid: the workgroups that read one range of Ap / Aj are dispatched together
    const unsigned cut_block = blockIdx.x / unsigned(args.n_heads);
    const AttnBwdArgs<val_t> a = attn_bwd_args_of_head(args, blockIdx.x % unsigned(args.n_heads));
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
#include "attention_bwd_slice_walk.inc"     // the slice's entries, 64 at a time, and its lines without entries
}

// the fix-up's thread of (slice t, column j): if t is the first slice that carries a line, that line and the sum of its
// pieces in the order of attn_piece_chain; otherwise false
template <typename acc_t>
__device__ __forceinline__ bool attn_bwd_fixup_sum(int64_t n_slices, const AttnBwdScratch<acc_t>& sc, int64_t t, int j, int32_t& r, acc_t& sum) {
    return attn_piece_chain(
        n_slices, sc.row, t, r, [&](int64_t piece) { sum = sc.acc[piece * sc.carry_ld + j]; },
        [&](int64_t piece) { sum = sum + sc.acc[piece * sc.carry_ld + j]; });
}

// one thread per (head, slice, column): the first slice that carries a line adds the line's pieces and stores the line of out
template <typename val_t>
__global__ __launch_bounds__(kBlock) void attention_bwd_fixup_kernel(int64_t n_slices, int32_t width, const AttnBwdScratch<val_t> sc0,
                                                                     val_t* __restrict__ out0, int64_t ldout, const AttnBwdHeads hd) {
    unsigned h;
    const int64_t gid = attn_head_thread(hd.per_head, h);
    const int j = int(gid % width);
    const AttnBwdScratch<val_t> sc = attn_bwd_scratch_of_head(sc0, h, hd.hsc);
    val_t* out = out0 + h * hd.ha;
    int32_t r;
    val_t sum;
    if (!attn_bwd_fixup_sum(n_slices, sc, gid / width, j, r, sum)) return;
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

#include "attention_bwd_half_kernel.hpp"    // (down here: its kernels use AttnBwdScratch, the fold and kDeltaLanes)

using namespace mi355;

namespace {

// argument-only checks of a create (also run by the one-shots before they make anything): the type refusals of
// mi355_spmv_attention_create, then the transpose's limit
int attention_bwd_check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                               const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    if (const int st = attn_check_types(who, off_type, val_type, "Q, K, V, O and dO", "mi355_spmv_attention_bwd_create_half")) return st;
    if (d_max < 1) { set_error("%s: d_max = %d below 1", who, d_max); return MI355_SPMV_EINVAL; }
    if (dv_max < 1) { set_error("%s: dv_max = %d below 1", who, dv_max); return MI355_SPMV_EINVAL; }
    if (const int st = check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    if (uint64_t(nnz) >= (1ull << 32)) { set_error("%s: nnz of 2^32 or more entries (the slot map is 32-bit)", who); return MI355_SPMV_ENOTSUP; }
    return MI355_SPMV_OK;
}

// the checks of create_half (and of the 16-bit one-shots): vec_type first, then what a create of fp32 values checks
int attention_bwd_check_create_half(const char* who, int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                                    const int32_t* Aj, int32_t d_max, int32_t dv_max) {
    if (const int st = attn_check_half_type(who, vec_type, "Q, K, V, O, dO, dQ, dK and dV")) return st;
    return attention_bwd_check_create(who, off_type, MI355_VAL_F32, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max);
}

// argument-only checks of an execute (bias may be null; so may any of dQ, dK, dV, but not all three)
int attention_bwd_check_execute(const char* who, int32_t n_rows, int64_t nnz, int32_t d_max, int32_t dv_max, const AttnBwdOperands& o) {
    if (const int st = attn_check_widths(who, o.d, o.dv, d_max, dv_max, o.ldq, o.ldk, o.ldv, o.ldo)) return st;
    if (o.lddo < o.dv) { set_error("%s: lddo = %lld below dv = %d", who, (long long)o.lddo, o.dv); return MI355_SPMV_EINVAL; }
    if (!o.dQ && !o.dK && !o.dV) { set_error("%s: dQ, dK and dV are all null (nothing to compute)", who); return MI355_SPMV_EINVAL; }
    if (o.dbias && !o.dQ) { set_error("%s: dbias without dQ (dbias comes from the walk that makes dQ)", who); return MI355_SPMV_EINVAL; }
    if (o.dQ && o.lddq < o.d) { set_error("%s: lddq = %lld below d = %d", who, (long long)o.lddq, o.d); return MI355_SPMV_EINVAL; }
    if (o.dK && o.lddk < o.d) { set_error("%s: lddk = %lld below d = %d", who, (long long)o.lddk, o.d); return MI355_SPMV_EINVAL; }
    if (o.dV && o.lddv < o.dv) { set_error("%s: lddv = %lld below dv = %d", who, (long long)o.lddv, o.dv); return MI355_SPMV_EINVAL; }
    if (const int st = attn_check_inputs(who, n_rows, nnz, o.Q, o.K, o.V, o.O)) return st;
    if (n_rows > 0 && !o.dO) { set_error("%s: null dO", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !o.lse) { set_error("%s: null lse", who); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

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
int attention_bwd_make(const char* who, mi355_spmv_attention_bwd** out, int off_type, int val_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                       const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max, hipStream_t s) {
    mi355_spmv_attention_bwd* m = new (std::nothrow) mi355_spmv_attention_bwd();
    if (!m) { set_error("%s: host allocation failed", who); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = val_type; m->vec_type = vec_type;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->Ap = Ap; m->Aj = Aj;
    m->d_max = d_max; m->dv_max = dv_max;
    m->n_slices = slice_count(n_rows, nnz);
    m->n_slices_t = slice_count(n_cols, nnz);
    const int widest = attn_widest(vec_type);
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
    m->scratch_bytes = m->head_bytes = attn_bwd_scratch_bytes(n_rows, slices, m->carry_ld, val_type == MI355_VAL_F64 ? 8 : 4);
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

// The kernels of one storage type as the launch path below names them: elem_t is the type of the eight matrices, acc_t that
// of bias, lse, dbias, scale and the scratch, W a lane's columns.  AttnBwdHalfKernels<vec_t> (attention_bwd_half_kernel.hpp)
// has the same members.
template <typename val_t>
struct AttnBwdKernels {
    using elem_t = val_t;
    using acc_t = val_t;
    using Args = AttnBwdArgs<val_t>;
    static constexpr int W = 16 / int(sizeof(val_t));
    static void delta(dim3 grid, hipStream_t s, int32_t n_rows, int32_t dv, const val_t* dO, int64_t lddo, const val_t* O, int64_t ldo, val_t* delta,
                      const AttnBwdHeads& hd) {
        hipLaunchKernelGGL((attention_bwd_delta_kernel<val_t>), grid, dim3(kBlock), 0, s, n_rows, dv, dO, lddo, O, ldo, delta, hd);
    }
    template <typename off_t, int C, int ROLE>
    static void slice(dim3 grid, hipStream_t s, const Args& a, const off_t* Ap) {
        hipLaunchKernelGGL((attention_bwd_slice_kernel<off_t, val_t, C, ROLE>), grid, dim3(kBlock), 0, s, a, Ap);
    }
    static void fixup(dim3 grid, hipStream_t s, const Args& a, int32_t width) {
        hipLaunchKernelGGL((attention_bwd_fixup_kernel<val_t>), grid, dim3(kBlock), 0, s, a.n_slices, width, a.sc, a.out, a.ldout,
                           AttnBwdHeads{a.n_heads, uint32_t(attn_blocks_per_head(a.n_slices * width)), a.hsc, a.hout, 0});
    }
};

// the passes of one role over the tiles of its output, then its fix-up
template <typename off_t, typename K, int ROLE>
int attention_bwd_role(typename K::Args& a, const off_t* Ap, int32_t width, hipStream_t s) {
    return attn_tile_passes<K::W>(
        a, width, [&](dim3 grid, auto lanes) { K::template slice<off_t, decltype(lanes)::value, ROLE>(grid, s, a, Ap); },
        [&](dim3 grid) { K::fixup(grid, s, a, width); });
}

// delta, then the roles that are asked for, one behind the other on the stream (they share the pieces' scratch)
template <typename off_t, typename K>
int attention_bwd_launch(const mi355_spmv_attention_bwd& m, const AttnBwdOperands& o, int32_t n_heads, const mi355_spmv_attention_bwd_head_strides* hs,
                         hipStream_t s) {
    using elem_t = typename K::elem_t;
    using acc_t = typename K::acc_t;
    const int64_t slices = m.n_slices > m.n_slices_t ? m.n_slices : m.n_slices_t;
    typename K::Args a;
    a.nnz = m.nnz;
    a.Q = static_cast<const elem_t*>(o.Q); a.K = static_cast<const elem_t*>(o.K); a.V = static_cast<const elem_t*>(o.V);
    a.dO = static_cast<const elem_t*>(o.dO);
    a.bias = static_cast<const acc_t*>(o.bias);
    a.lse = static_cast<const acc_t*>(o.lse);
    a.ldq = o.ldq; a.ldk = o.ldk; a.ldv = o.ldv; a.lddo = o.lddo;
    a.d = o.d; a.dv = o.dv;
    const mi355_spmv_attention_bwd_head_strides h = n_heads > 1 ? *hs : mi355_spmv_attention_bwd_head_strides{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    a.n_heads = n_heads;
    a.hq = h.q; a.hk = h.k; a.hv = h.v; a.hdo = h.d_o; a.hbias = h.bias; a.hlse = h.lse; a.hdbias = h.dbias;
    a.hsc = int64_t(attn_head_scratch_stride(m.head_bytes));
    a.q_vec = attn_rows_vec<elem_t>(o.Q, o.ldq, n_heads, h.q) ? 1 : 0;
    a.k_vec = attn_rows_vec<elem_t>(o.K, o.ldk, n_heads, h.k) ? 1 : 0;
    a.v_vec = attn_rows_vec<elem_t>(o.V, o.ldv, n_heads, h.v) ? 1 : 0;
    a.do_vec = attn_rows_vec<elem_t>(o.dO, o.lddo, n_heads, h.d_o) ? 1 : 0;
    a.scale = acc_t(m.scale);
    a.sc = attn_bwd_scratch<acc_t>(m.scratch, m.n_rows, slices, m.carry_ld);
    a.delta = a.sc.delta;
    a.col_begin = 0; a.cols = 0;
    if (m.n_rows > 0 && m.nnz > 0) {
        const int64_t per_head = attn_blocks_per_head(int64_t(m.n_rows) * kDeltaLanes);
        K::delta(dim3(unsigned(per_head * n_heads)), s, m.n_rows, o.dv, a.dO, o.lddo, static_cast<const elem_t*>(o.O), o.ldo, a.sc.delta,
                 AttnBwdHeads{n_heads, uint32_t(per_head), a.hsc, h.d_o, h.o});
        MI355_HIP_TRY(hipGetLastError());
    }
    const auto role = [&](auto which, void* out, int64_t ldout, int64_t hout, int32_t width) {
        a.out = static_cast<elem_t*>(out);
        a.ldout = ldout;
        a.hout = hout;
        a.out_vec = attn_rows_vec<elem_t>(out, ldout, n_heads, hout) ? 1 : 0;
        constexpr int ROLE = decltype(which)::value;
        if constexpr (ROLE == kBwdDQ) {
            a.n_rows = m.n_rows; a.n_slices = m.n_slices;
            a.Aj = m.Aj; a.perm = nullptr;
            a.dbias = static_cast<acc_t*>(o.dbias);
            return attention_bwd_role<off_t, K, ROLE>(a, static_cast<const off_t*>(m.Ap), width, s);
        } else {
            a.n_rows = m.n_cols; a.n_slices = m.n_slices_t;
            a.perm = reinterpret_cast<const uint32_t*>(m.held);
            a.Aj = reinterpret_cast<const int32_t*>(m.held + size_t(m.nnz) * 4);
            a.dbias = nullptr;
            return attention_bwd_role<off_t, K, ROLE>(a, reinterpret_cast<const off_t*>(m.held + size_t(m.nnz) * 8), width, s);
        }
    };
    if (o.dQ)
        if (const int st = role(std::integral_constant<int, kBwdDQ>(), o.dQ, o.lddq, h.dq, o.d)) return st;
    if (o.dK)
        if (const int st = role(std::integral_constant<int, kBwdDK>(), o.dK, o.lddk, h.dk, o.d)) return st;
    if (o.dV)
        if (const int st = role(std::integral_constant<int, kBwdDV>(), o.dV, o.lddv, h.dv, o.dv)) return st;
    return MI355_SPMV_OK;
}

int attention_bwd_run(const mi355_spmv_attention_bwd& m, const AttnBwdOperands& o, int32_t n_heads, const mi355_spmv_attention_bwd_head_strides* hs,
                      void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool i32 = m.off_type == MI355_OFF_I32;
    auto run = [&](auto off, auto kernels) { return attention_bwd_launch<decltype(off), decltype(kernels)>(m, o, n_heads, hs, s); };
    auto either = [&](auto kernels) { return i32 ? run(int32_t(), kernels) : run(int64_t(), kernels); };
    if (m.vec_type == MI355_VAL_F16) return either(AttnBwdHalfKernels<F16>());      // 16-bit matrices under fp32 everything else
    if (m.vec_type == MI355_VAL_BF16) return either(AttnBwdHalfKernels<Bf16>());
    return m.val_type == MI355_VAL_F64 ? either(AttnBwdKernels<double>()) : either(AttnBwdKernels<float>());
}

// create, execute, synchronise, destroy; every argument check comes before any device call
int attention_bwd_one_shot(int off_type, int val_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                           const AttnBwdOperands& o, double scale, void* stream) {
    const char* const who = vec_type != val_type ? "attention_bwd_half" : "attention_bwd";
    set_error("%s", "");
    const int32_t d1 = o.d < 1 ? 1 : o.d, dv1 = o.dv < 1 ? 1 : o.dv;
    if (const int st = vec_type != val_type ? attention_bwd_check_create_half(who, off_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, d1, dv1)
                                            : attention_bwd_check_create(who, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d1, dv1))
        return st;
    if (const int st = attention_bwd_check_execute(who, n_rows, nnz, o.d, o.dv, o)) return st;
    mi355_spmv_attention_bwd* m = nullptr;
    int st = attention_bwd_make(who, &m, off_type, val_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, o.d, o.dv, static_cast<hipStream_t>(stream));
    if (st != MI355_SPMV_OK) return st;
    m->scale = scale;
    st = attention_bwd_run(*m, o, 1, nullptr, stream);
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
    return attention_bwd_make("attention_bwd_create", out, off_type, val_type, val_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max,
                              static_cast<hipStream_t>(stream));
}

int mi355_spmv_attention_bwd_create_half(mi355_spmv_attention_bwd** out, int off_type, int vec_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                         const void* Ap, const int32_t* Aj, int32_t d_max, int32_t dv_max, void* stream) {
    set_error("%s", "");
    if (!out) { set_error("attention_bwd_create_half: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = attention_bwd_check_create_half("attention_bwd_create_half", off_type, vec_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max))
        return st;
    return attention_bwd_make("attention_bwd_create_half", out, off_type, MI355_VAL_F32, vec_type, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max,
                              static_cast<hipStream_t>(stream));
}

int mi355_spmv_attention_bwd_get_types(const mi355_spmv_attention_bwd* m, int* val_type, int* vec_type) {
    if (!m || !val_type || !vec_type) { set_error("attention_bwd_get_types: null argument"); return MI355_SPMV_EINVAL; }
    *val_type = m->val_type;
    *vec_type = m->vec_type;
    return MI355_SPMV_OK;
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
    if (const int st = attention_bwd_check_execute("attention_bwd_execute", m->n_rows, m->nnz, m->d_max, m->dv_max, o)) return st;
    return attention_bwd_run(*m, o, 1, nullptr, stream);
}

int mi355_spmv_attention_bwd_reserve_heads(mi355_spmv_attention_bwd* m, int32_t n_heads_max) {
    set_error("%s", "");
    if (!m) { set_error("attention_bwd_reserve_heads: null object"); return MI355_SPMV_EINVAL; }
    if (n_heads_max < 1) { set_error("attention_bwd_reserve_heads: n_heads_max = %d below 1", n_heads_max); return MI355_SPMV_EINVAL; }
    void* fresh = nullptr;      // (the held transpose is what every head shares: not touched)
    const size_t bytes = attn_heads_scratch_bytes(m->head_bytes, n_heads_max);
    const int st = attn_reserve_scratch("attention_bwd_reserve_heads", &m->scratch, bytes, &fresh);
    if (bytes == 0 || fresh) { m->scratch_bytes = bytes; m->n_heads_max = n_heads_max; }
    return st;
}

int mi355_spmv_attention_bwd_get_heads_max(const mi355_spmv_attention_bwd* m, int32_t* n_heads_max) {
    if (!m || !n_heads_max) { set_error("attention_bwd_get_heads_max: null argument"); return MI355_SPMV_EINVAL; }
    *n_heads_max = m->n_heads_max;
    return MI355_SPMV_OK;
}

int mi355_spmv_attention_bwd_execute_heads(mi355_spmv_attention_bwd* m, int32_t n_heads, const mi355_spmv_attention_bwd_head_strides* hs, int32_t d,
                                           int32_t dv, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                           const void* bias, const void* O, int64_t ldo, const void* dO, int64_t lddo, const void* lse, void* dQ,
                                           int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, void* dbias, void* stream) {
    const char* const who = "attention_bwd_execute_heads";
    set_error("%s", "");
    if (!m) { set_error("%s: null object", who); return MI355_SPMV_EINVAL; }
    const AttnBwdOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, dO, lddo, lse, dQ, lddq, dK, lddk, dV, lddv, dbias};
    if (const int st = attention_bwd_check_execute(who, m->n_rows, m->nnz, m->d_max, m->dv_max, o)) return st;
    if (const int st = attn_check_n_heads(who, n_heads, m->n_heads_max, hs)) return st;
    if (n_heads > 1) {
        const std::pair<const char*, int64_t> all[] = {{"q", hs->q},   {"k", hs->k},     {"v", hs->v},   {"bias", hs->bias}, {"o", hs->o},        {"d_o", hs->d_o},
                                                       {"lse", hs->lse}, {"dq", hs->dq}, {"dk", hs->dk}, {"dv", hs->dv},     {"dbias", hs->dbias}};
        for (const auto& [name, stride] : all)
            if (const int st = attn_check_stride_sign(who, name, stride)) return st;
        if (dQ)
            if (const int st = attn_check_out_stride(who, "dq", n_heads, hs->dq, m->n_rows, d, lddq)) return st;
        if (dK)
            if (const int st = attn_check_out_stride(who, "dk", n_heads, hs->dk, m->n_cols, d, lddk)) return st;
        if (dV)
            if (const int st = attn_check_out_stride(who, "dv", n_heads, hs->dv, m->n_cols, dv, lddv)) return st;
        if (dbias && m->nnz > 0)
            if (const int st = attn_check_out_vector_stride(who, "dbias", hs->dbias, m->nnz, "nnz")) return st;
    }
    const int64_t wide = d > dv ? d : dv;
    if (const int st = attn_check_heads_grid(who, n_heads, m->n_slices > m->n_slices_t ? m->n_slices : m->n_slices_t, wide)) return st;
    if (attn_blocks_per_head(int64_t(m->n_rows) * kDeltaLanes) * n_heads >= (int64_t(1) << 31)) {
        set_error("%s: n_heads = %d makes a grid of 2^31 workgroups or more (%d rows)", who, n_heads, m->n_rows);
        return MI355_SPMV_ENOTSUP;
    }
    return attention_bwd_run(*m, o, n_heads, hs, stream);
}

int mi355_spmv_attention_bwd_get_info(const mi355_spmv_attention_bwd* m, mi355_spmv_attention_bwd_info* info) {
    if (!m || !info) { set_error("attention_bwd_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->d_max = m->d_max; info->dv_max = m->dv_max;
    info->widest_tile = attn_widest(m->vec_type);
    const int per_lane = attn_lane_cols(m->vec_type);
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
    snprintf(info->main_kernel, sizeof(info->main_kernel), m->vec_type != m->val_type ? "attention_bwd_half_slice_kernel" : "attention_bwd_slice_kernel");
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
        return attention_bwd_one_shot(OFFENUM, VALENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, o, scale, stream);      \
    }
MI355_SPMV_DEFINE_ATTENTION_BWD(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION_BWD(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_ATTENTION_BWD(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ATTENTION_BWD(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

#define MI355_SPMV_DEFINE_ATTENTION_BWD_HALF(SUF, OFF, OFFENUM, VECENUM)                                                       \
    int mi355_spmv_attention_bwd_half_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, int32_t d, int32_t dv, \
                                            const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,    \
                                            const float* bias, double scale, const void* O, int64_t ldo, const void* dO, int64_t lddo, \
                                            const float* lse, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, \
                                            float* dbias, void* stream) {                                                      \
        const AttnBwdOperands o{d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, dO, lddo, lse, dQ, lddq, dK, lddk, dV, lddv, dbias}; \
        return attention_bwd_one_shot(OFFENUM, MI355_VAL_F32, VECENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, o, scale, stream); \
    }
MI355_SPMV_DEFINE_ATTENTION_BWD_HALF(i32_f16, int32_t, MI355_OFF_I32, MI355_VAL_F16)
MI355_SPMV_DEFINE_ATTENTION_BWD_HALF(i32_bf16, int32_t, MI355_OFF_I32, MI355_VAL_BF16)
MI355_SPMV_DEFINE_ATTENTION_BWD_HALF(i64_f16, int64_t, MI355_OFF_I64, MI355_VAL_F16)
MI355_SPMV_DEFINE_ATTENTION_BWD_HALF(i64_bf16, int64_t, MI355_OFF_I64, MI355_VAL_BF16)

}  // extern "C"
