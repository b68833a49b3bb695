// row_softmax.hip — softmax over the stored entries of every row of a CSR matrix, and its gradient
// (mi355_spmv_row_softmax_*): the step between SDDMM (the edge scores) and multi-vector SpMV (the
// aggregation) of sparse attention.
//   forward    v[n] = scale * x[n],  m_r = max over the row of v,  out[n] = exp(v[n] - m_r) / sum over the row of exp(v - m_r)
//   backward   t_r = sum over the row of p * dp,  dx[n] = scale * p[n] * (dp[n] - t_r)          (p = the forward's output)
// x, out, p, dp, dx are nnz values in CSR order; Aj is never read.  An object of its own beside mi355_spmv_sddmm: the
// kernels, their launch and the extern "C" entry points, all in this unit.
//
// Masked edges: an entry x[n] = -inf gives exactly +0, and a row whose entries are ALL -inf gives +0 everywhere, not NaN
// (the row's max is -inf and its sum 0: every entry takes the masked branch).  A row of one entry gives exactly 1.  Empty
// rows write nothing.  (+inf, NaN, and -inf under a scale <= 0 are not masks: they give what the arithmetic gives.)
//
// The cut is the slice kinds' (slice_cut.hpp, slice_cut.inc, slice_cut_row.inc, C = 1: one lane per nonzero, 64 per
// group, at most kRsGroups = 16 groups per slice).  Two monoids run over ONE walk (the Dir policies below):
//   forward    (m, s) + (m', s') = (M = max(m, m'), s exp(m - M) + s' exp(m' - M)); a side with m = -inf contributes 0
//   backward   a plain sum of p * dp
//
//   row_softmax_slice_kernel    one WAVE per slice.  The wave loads its at most 1 024 entries once, 16 per lane, and keeps
//                               them in registers.  Group by group, ascending, a segmented scan over the lanes (by the row
//                               that slice_cut_row.inc finds) reduces every run of one row; the run at lane 0 takes the
//                               open row's statistic of the groups before it, the run at the last lane hands it on.  Then,
//                               group by group descending, a row's final statistic flows back to its earlier groups, and
//                               every row that lies wholly inside the slice is normalised FROM THE REGISTERS and stored:
//                               x crosses HBM once and out once.  Of the row carried in (its HEAD piece: the row ends here)
//                               and of the row open at the slice's end (its TAIL piece) only the partial statistic is
//                               written, to the slice's two slots of scratch; both slots and the slice's record (n0, nn,
//                               head_len, tail_begin, tail_row = -1 for none) are rewritten by every execute.
//   row_softmax_fixup_kernel    one THREAD per slice (multi_fixup_kernel's structure): the first slice that carries a row
//                               folds that row's pieces IN SLICE ORDER, tails first and then the ending slice's head, and
//                               writes the final statistic back to every slot of the chain.
//   row_softmax_finish_kernel   one WAVE per slice: a slice with a head and / or a tail piece re-reads those entries and
//                               normalises them with the final statistic, by the main kernel's piece of arithmetic
//                               (Dir::value); other waves exit at once.  Always launched: the host decides nothing from
//                               device data, so an execute is graph-capturable and never synchronises.
//
// In place (out == x; dx == dp or dx == p): every element is read by the lane that writes it, and no element is read
// after another wave has written it — the main kernel holds its whole slice in registers before its first store and
// never stores a piece's entries, which the finish kernel reads and writes lane by lane.
// No atomics: two executes on the same inputs give the same bits.  The bits of an element DO depend on where the group
// and slice edges fall in its row (unlike SDDMM's): statistics combine by 64-nonzero group, then by slice.
#include <cmath>
#include <limits>
#include <new>

#include "slice_cut.hpp"

struct mi355_spmv_row_softmax {     // the opaque handle of include/mi355_spmv.h
    int off_type = 0, val_type = 0;
    int32_t n_rows = 0, n_cols = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;    // kept for symmetry with the other objects; never read
    double scale = 1.0;
    int64_t n_slices = 0;
    void* scratch = nullptr;        // the slices' records and their two statistic slots
    size_t scratch_bytes = 0;
};

namespace mi355 {

#ifdef __clang__
// v = scale * x is rounded before it meets a max or a difference: a row of equal entries has v - m = 0 in every kernel
#pragma clang fp contract(off)
#endif

// The geometry that the host simulation's table is written for: tests/test_row_softmax_sim_cpu.py reads these two lines
// and holds tests/row_softmax_cases.py to them.  The kernels use slice_cut.hpp's constants; a change there stops here.
constexpr int kRowSoftmaxSlice = 1024;
constexpr int kRowSoftmaxGroups = 16;
constexpr int kRsGroups = kSliceLen / kWave;    // groups of 64 nonzeros a slice can hold: 16 values per lane
static_assert(kRowSoftmaxSlice == kSliceLen && kRowSoftmaxGroups == kRsGroups, "tests/row_softmax_cases.py is tabled for this geometry");

// what the kernels keep per slice between the three launches: O(n_slices), owned by the object
template <typename val_t>
struct RsScratch {
    int64_t* n0;            // [n_slices] the slice's first nonzero
    int32_t* nn;            // its nonzeros
    int32_t* head_len;      // leading entries that are the last piece of a row carried in (0 = none)
    int32_t* tail_begin;    // first entry of the piece of the row that is open at the slice's end (nn = none)
    int32_t* tail_row;      // that row, or -1
    val_t* head_stat;       // [n_slices][2]: the head piece's partial statistic, the row's final one behind the fix-up
    val_t* tail_stat;       // [n_slices][2]: the tail piece's likewise
};

inline size_t rs_scratch_bytes(int64_t n_slices, size_t val_bytes) {
    return size_t(n_slices) * (sizeof(int64_t) + 4 * sizeof(int32_t) + 4 * val_bytes);
}

template <typename val_t>
RsScratch<val_t> rs_scratch(void* base, int64_t n_slices) {
    RsScratch<val_t> sc;
    char* p = static_cast<char*>(base);
    sc.n0 = reinterpret_cast<int64_t*>(p); p += size_t(n_slices) * sizeof(int64_t);
    sc.head_stat = reinterpret_cast<val_t*>(p); p += size_t(n_slices) * 2 * sizeof(val_t);
    sc.tail_stat = reinterpret_cast<val_t*>(p); p += size_t(n_slices) * 2 * sizeof(val_t);
    sc.nn = reinterpret_cast<int32_t*>(p); p += size_t(n_slices) * sizeof(int32_t);
    sc.head_len = reinterpret_cast<int32_t*>(p); p += size_t(n_slices) * sizeof(int32_t);
    sc.tail_begin = reinterpret_cast<int32_t*>(p); p += size_t(n_slices) * sizeof(int32_t);
    sc.tail_row = reinterpret_cast<int32_t*>(p);
    return sc;
}

template <typename val_t>
struct RowSoftmaxArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const val_t* a;         // forward: x; backward: p
    const val_t* b;         // backward: dp; forward: never read
    val_t* out;             // may be a (forward) or a or b (backward)
    val_t scale;
    RsScratch<val_t> sc;
};

__device__ __forceinline__ float rs_exp(float d) { return expf(d); }
__device__ __forceinline__ double rs_exp(double d) { return exp(d); }

// exp of a difference d = v - M <= 0: exactly 1 at 0 and exactly +0 at -inf, whatever the math library gives at its ends
template <typename val_t>
__device__ __forceinline__ val_t rs_exp_diff(val_t d) {
    if (d == val_t(0)) return val_t(1);
    if (d == -std::numeric_limits<val_t>::infinity()) return val_t(0);
    return rs_exp(d);
}

struct RsMax {
    template <typename T> __device__ __forceinline__ T operator()(T x, T y) const { return x < y ? y : x; }
};
struct RsSum {
    template <typename T> __device__ __forceinline__ T operator()(T x, T y) const { return x + y; }
};

// the reduction of a lane's run (lanes start .. end of one row) of a group, in every lane of the run: a segmented
// inclusive scan up the lanes, then the run's last lane's value
template <typename val_t, typename Op>
__device__ __forceinline__ val_t rs_run_reduce(val_t v, int lane, int start, int end, Op op) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const val_t o = __shfl_up(v, d);
        if (lane - d >= start) v = op(o, v);
    }
    return __shfl(v, end);
}

// ---- the two directions: what a Dir policy holds ---------------------------------------------------------------------
//   Stat                       a row's statistic (kN values of scratch)
//   identity()                 of combine
//   load(a, n, va, vb)         entry n into the lane's registers
//   none(va, vb)               what a lane without an entry holds: the identity under run()
//   run(va, vb, lane, s, e)    the statistic of the lane's run of one group
//   combine(x, y)              the monoid, x the earlier piece
//   value(a, va, vb, stat)     the element, from the registers and its row's final statistic: the ONE piece of arithmetic
//                              of the main and the finish kernel
template <typename val_t>
struct RsForward {
    static constexpr val_t kNegInf = -std::numeric_limits<val_t>::infinity();
    struct Stat { val_t m, s; };
    __device__ static __forceinline__ Stat identity() { return Stat{kNegInf, val_t(0)}; }
    __device__ static __forceinline__ void load(const RowSoftmaxArgs<val_t>& a, int64_t n, val_t& va, val_t&) { va = a.scale * a.a[n]; }
    __device__ static __forceinline__ void none(val_t& va, val_t& vb) { va = kNegInf; vb = val_t(0); }
    __device__ static __forceinline__ Stat run(val_t va, val_t, int lane, int start, int end) {
        Stat t;
        t.m = rs_run_reduce(va, lane, start, end, RsMax());
        const val_t e = va == kNegInf ? val_t(0) : rs_exp_diff(va - t.m);
        t.s = rs_run_reduce(e, lane, start, end, RsSum());
        return t;
    }
    __device__ static __forceinline__ Stat combine(const Stat& x, const Stat& y) {
        Stat t;
        t.m = x.m < y.m ? y.m : x.m;
        const val_t sx = x.m == kNegInf ? val_t(0) : x.s * rs_exp_diff(x.m - t.m);
        const val_t sy = y.m == kNegInf ? val_t(0) : y.s * rs_exp_diff(y.m - t.m);
        t.s = sx + sy;
        return t;
    }
    __device__ static __forceinline__ val_t value(const RowSoftmaxArgs<val_t>&, val_t va, val_t, const Stat& t) {
        return va == kNegInf ? val_t(0) : rs_exp_diff(va - t.m) / t.s;
    }
    __device__ static __forceinline__ Stat get(const val_t* p) { return Stat{p[0], p[1]}; }
    __device__ static __forceinline__ void put(val_t* p, const Stat& t) { p[0] = t.m; p[1] = t.s; }
    __device__ static __forceinline__ Stat shfl(const Stat& t, int src) { return Stat{__shfl(t.m, src), __shfl(t.s, src)}; }
};

template <typename val_t>
struct RsBackward {
    struct Stat { val_t t; };
    __device__ static __forceinline__ Stat identity() { return Stat{val_t(0)}; }
    __device__ static __forceinline__ void load(const RowSoftmaxArgs<val_t>& a, int64_t n, val_t& va, val_t& vb) { va = a.a[n]; vb = a.b[n]; }
    __device__ static __forceinline__ void none(val_t& va, val_t& vb) { va = val_t(0); vb = val_t(0); }
    __device__ static __forceinline__ Stat run(val_t va, val_t vb, int lane, int start, int end) {
        return Stat{rs_run_reduce(va * vb, lane, start, end, RsSum())};
    }
    __device__ static __forceinline__ Stat combine(const Stat& x, const Stat& y) { return Stat{x.t + y.t}; }
    __device__ static __forceinline__ val_t value(const RowSoftmaxArgs<val_t>& a, val_t va, val_t vb, const Stat& t) {
        return (a.scale * va) * (vb - t.t);
    }
    __device__ static __forceinline__ Stat get(const val_t* p) { return Stat{p[0]}; }
    __device__ static __forceinline__ void put(val_t* p, const Stat& t) { p[0] = t.t; }
    __device__ static __forceinline__ Stat shfl(const Stat& t, int src) { return Stat{__shfl(t.t, src)}; }
};

// ---- the main slice kernel ---------------------------------------------------------------------------------------------
template <typename off_t, typename val_t, typename D>
__global__ __launch_bounds__(kBlock) void row_softmax_slice_kernel(const RowSoftmaxArgs<val_t> a, const off_t* __restrict__ Ap) {
    using Stat = typename D::Stat;
    constexpr int C = 1;                                            // one lane per nonzero
    constexpr bool kCutCarriedIn = true, kCutKeepsR1 = false;       // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = 0;
    const unsigned cut_block = blockIdx.x;
#include "slice_cut.inc"            // leaves lane, c, s, w, r0, n0, nn, nr, rel, carried_in
    (void)c; (void)s;

    // the slice's entries, one per lane and group, and the row of each (relative to r0; nr = no entry)
    val_t va[kRsGroups], vb[kRsGroups];
    int row[kRsGroups];
#pragma unroll
    for (int g = 0; g < kRsGroups; ++g) {
        D::none(va[g], vb[g]);
        if (g * kWave + lane < nn) D::load(a, n0 + g * kWave + lane, va[g], vb[g]);
    }
#pragma unroll
    for (int g = 0; g < kRsGroups; ++g) {
        row[g] = nr;
        const int m = g * kWave + lane;
        if (m < nn) {
#include "slice_cut_row.inc"     // leaves lo: the nonzero's row, relative to r0
            row[g] = lo;
        }
    }
    // the last piece of a row carried in: its leading entries, when the row ends here (a slice inside one row is a tail)
    const int head_len = carried_in && nr >= 1 && rel[1] <= nn ? rel[1] : 0;

    // ascending: every run's statistic, the open row's carried from group to group
    Stat T[kRsGroups];
    Stat open = D::identity();      // of the open row, over the groups so far
    int open_row = -1;              // the row that goes on behind the last group walked, or -1
    unsigned goes = 0;              // bit g: a row goes on behind group g
#pragma unroll
    for (int g = 0; g < kRsGroups; ++g) {
        T[g] = D::identity();
        if (g * kWave < nn) {
            const int m = g * kWave + lane;
            const int prev = __shfl_up(row[g], 1);
            const unsigned long long heads = __ballot(lane == 0 || prev != row[g]);
            const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
            const unsigned long long later = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
            const int end = later ? lane + __builtin_ctzll(later) : kWave - 1;
            Stat t = D::run(va[g], vb[g], lane, start, end);
            if (open_row >= 0 && start == 0) t = D::combine(open, t);      // (groups in ascending order)
            T[g] = t;
            if (m == head_len - 1) D::put(a.sc.head_stat + w * 2, t);
            const int lv = min(kWave, nn - g * kWave) - 1;                  // the group's last entry
            const int row_lv = __shfl(row[g], lv);
            open = D::shfl(t, lv);
            const bool goes_on = rel[row_lv + 1] > g * kWave + lv + 1;
            open_row = goes_on ? row_lv : -1;
            if (goes_on) goes |= 1u << g;
        }
    }
    if (lane == 0) {
        a.sc.n0[w] = n0;
        a.sc.nn[w] = nn;
        a.sc.head_len[w] = head_len;
        a.sc.tail_begin[w] = open_row >= 0 ? rel[open_row] : nn;
        a.sc.tail_row[w] = open_row >= 0 ? int32_t(r0 + open_row) : -1;
        D::put(a.sc.tail_stat + w * 2, open_row >= 0 ? open : D::identity());
        if (head_len == 0) D::put(a.sc.head_stat + w * 2, D::identity());
    }

    // descending: a row's final statistic back to its earlier groups; the rows that lie inside the slice are stored
    const int tail_i = open_row;
    int back_row = open_row;
    Stat back = open;
#pragma unroll
    for (int g = kRsGroups - 1; g >= 0; --g) {
        if (g * kWave < nn) {
            const int m = g * kWave + lane;
            Stat f = T[g];
            if (back_row >= 0 && row[g] == back_row) f = back;
            if (m < nn && m >= head_len && row[g] != tail_i) a.out[n0 + m] = D::value(a, va[g], vb[g], f);
            if (g > 0) {
                back = D::shfl(f, 0);
                const int row_0 = __shfl(row[g], 0);
                back_row = (goes >> (g - 1)) & 1u ? row_0 : -1;
            }
        }
    }
}

// one thread per slice: the first slice that carries a row folds its pieces in slice order — the tails, then the head of
// the slice the row ends in — and hands the final statistic to every slot of the chain
template <typename val_t, typename D>
__global__ __launch_bounds__(kBlock) void row_softmax_fixup_kernel(int64_t n_slices, const RsScratch<val_t> sc) {
    using Stat = typename D::Stat;
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_slices) return;
    const int32_t r = sc.tail_row[t];
    if (r < 0 || (t > 0 && sc.tail_row[t - 1] == r)) return;
    Stat f = D::get(sc.tail_stat + t * 2);
    int64_t u = t + 1;
    for (; u < n_slices && sc.tail_row[u] == r; ++u) f = D::combine(f, D::get(sc.tail_stat + u * 2));
    if (u < n_slices) f = D::combine(f, D::get(sc.head_stat + u * 2));
    for (int64_t v = t; v < u; ++v) D::put(sc.tail_stat + v * 2, f);
    if (u < n_slices) D::put(sc.head_stat + u * 2, f);
}

// one wave per slice: the entries of its head and tail pieces, with their rows' final statistics
template <typename val_t, typename D>
__global__ __launch_bounds__(kBlock) void row_softmax_finish_kernel(const RowSoftmaxArgs<val_t> a) {
    using Stat = typename D::Stat;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = int64_t(blockIdx.x) * kSliceWaves + threadIdx.x / kWave;
    if (w >= a.n_slices) return;
    const int nn = a.sc.nn[w], head_len = a.sc.head_len[w], tail_begin = a.sc.tail_begin[w];
    if (head_len <= 0 && tail_begin >= nn) return;
    const int64_t n0 = a.sc.n0[w];
    if (head_len > 0) {
        const Stat f = D::get(a.sc.head_stat + w * 2);
        for (int m = lane; m < head_len; m += kWave) {
            val_t va, vb;
            D::none(va, vb);
            D::load(a, n0 + m, va, vb);
            a.out[n0 + m] = D::value(a, va, vb, f);
        }
    }
    if (tail_begin < nn) {
        const Stat f = D::get(a.sc.tail_stat + w * 2);
        for (int m = tail_begin + lane; m < nn; m += kWave) {
            val_t va, vb;
            D::none(va, vb);
            D::load(a, n0 + m, va, vb);
            a.out[n0 + m] = D::value(a, va, vb, f);
        }
    }
}

}  // namespace mi355

using namespace mi355;

namespace {

// argument-only checks of a create (also run by the one-shots before they make anything)
int row_softmax_check_create(const char* who, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                             const int32_t* Aj) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown off_type %d", who, off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32) {
        set_error("%s: val_type MI355_VAL_I32 is not built (fp32 / fp64 values)", who);
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) {
        set_error("%s: val_type %d is not a type of x and out (F32 or F64; 16-bit values are not built)", who, val_type);
        return MI355_SPMV_EINVAL;
    }
    return check_csr_structure(who, off_type, n_rows, n_cols, nnz, Ap, Aj);
}

// argument-only checks of an execute (b: dp of a backward, not asked of a forward)
int row_softmax_check_execute(const char* who, int64_t nnz, const void* a, const char* a_name, const void* b, const char* b_name,
                              const void* out, const char* out_name) {
    if (nnz > 0 && !a) { set_error("%s: null %s", who, a_name); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && b_name && !b) { set_error("%s: null %s", who, b_name); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !out) { set_error("%s: null %s", who, out_name); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

// the object of checked arguments: the slices and their scratch (the only device call of a create: one hipMalloc)
int row_softmax_make(const char* who, mi355_spmv_row_softmax** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                     int64_t nnz, const void* Ap, const int32_t* Aj) {
    mi355_spmv_row_softmax* m = new (std::nothrow) mi355_spmv_row_softmax();
    if (!m) { set_error("%s: host allocation failed", who); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = val_type;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->Ap = Ap; m->Aj = Aj;
    m->n_slices = slice_count(n_rows, nnz);
    if (nnz > 0 && n_rows > 0) {    // (nothing stored: nothing is ever launched, nothing allocated)
        m->scratch_bytes = rs_scratch_bytes(m->n_slices, val_type == MI355_VAL_F64 ? 8 : 4);
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

// the three launches of one direction
template <typename off_t, typename val_t, typename D>
int row_softmax_launch(const mi355_spmv_row_softmax& m, const void* a_in, const void* b_in, void* out, hipStream_t s) {
    RowSoftmaxArgs<val_t> a;
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.a = static_cast<const val_t*>(a_in); a.b = static_cast<const val_t*>(b_in); a.out = static_cast<val_t*>(out);
    a.scale = val_t(m.scale);
    a.sc = rs_scratch<val_t>(m.scratch, m.n_slices);
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    hipLaunchKernelGGL((row_softmax_slice_kernel<off_t, val_t, D>), grid, block, 0, s, a, Ap);
    MI355_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((row_softmax_fixup_kernel<val_t, D>), dim3(unsigned((m.n_slices + kBlock - 1) / kBlock)), block, 0, s, m.n_slices, a.sc);
    MI355_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((row_softmax_finish_kernel<val_t, D>), grid, block, 0, s, a);
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

template <typename off_t, typename val_t>
int row_softmax_direction(const mi355_spmv_row_softmax& m, bool backward, const void* a, const void* b, void* out, hipStream_t s) {
    return backward ? row_softmax_launch<off_t, val_t, RsBackward<val_t>>(m, a, b, out, s)
                    : row_softmax_launch<off_t, val_t, RsForward<val_t>>(m, a, b, out, s);
}

int row_softmax_run(const mi355_spmv_row_softmax& m, bool backward, const void* a, const void* b, void* out, void* stream) {
    if (m.nnz == 0 || m.n_rows == 0) return MI355_SPMV_OK;      // no stored entry: nothing to write, nothing launched
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (m.off_type == MI355_OFF_I32)
        return m.val_type == MI355_VAL_F64 ? row_softmax_direction<int32_t, double>(m, backward, a, b, out, s)
                                           : row_softmax_direction<int32_t, float>(m, backward, a, b, out, s);
    return m.val_type == MI355_VAL_F64 ? row_softmax_direction<int64_t, double>(m, backward, a, b, out, s)
                                       : row_softmax_direction<int64_t, float>(m, backward, a, b, out, s);
}

// create, execute, synchronise, destroy (the scratch must outlive the kernels, as the multi-vector one-shots' does);
// every argument check comes before any device call
int row_softmax_one_shot(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                         const void* x, void* out, double scale, void* stream) {
    set_error("%s", "");
    if (const int st = row_softmax_check_create("row_softmax", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    if (const int st = row_softmax_check_execute("row_softmax", nnz, x, "x", nullptr, nullptr, out, "out")) return st;
    if (nnz == 0 || n_rows == 0) return MI355_SPMV_OK;
    mi355_spmv_row_softmax* m = nullptr;
    int st = row_softmax_make("row_softmax", &m, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj);
    if (st != MI355_SPMV_OK) return st;
    m->scale = scale;
    st = row_softmax_run(*m, false, x, nullptr, out, stream);
    if (st == MI355_SPMV_OK) st = mi355_spmv_stream_synchronize(stream);
    const int st2 = mi355_spmv_row_softmax_destroy(m);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace

extern "C" {

int mi355_spmv_row_softmax_create(mi355_spmv_row_softmax** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                  const void* Ap, const int32_t* Aj) {
    set_error("%s", "");
    if (!out) { set_error("row_softmax_create: null object pointer (out)"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = row_softmax_check_create("row_softmax_create", off_type, val_type, n_rows, n_cols, nnz, Ap, Aj)) return st;
    return row_softmax_make("row_softmax_create", out, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj);
}

int mi355_spmv_row_softmax_set_scale(mi355_spmv_row_softmax* m, double scale) {
    set_error("%s", "");
    if (!m) { set_error("row_softmax_set_scale: null object"); return MI355_SPMV_EINVAL; }
    m->scale = scale;
    return MI355_SPMV_OK;
}

int mi355_spmv_row_softmax_execute(mi355_spmv_row_softmax* m, const void* x, void* out, void* stream) {
    set_error("%s", "");
    if (!m) { set_error("row_softmax_execute: null object"); return MI355_SPMV_EINVAL; }
    if (const int st = row_softmax_check_execute("row_softmax_execute", m->nnz, x, "x", nullptr, nullptr, out, "out")) return st;
    return row_softmax_run(*m, false, x, nullptr, out, stream);
}

int mi355_spmv_row_softmax_backward(mi355_spmv_row_softmax* m, const void* p, const void* dp, void* dx, void* stream) {
    set_error("%s", "");
    if (!m) { set_error("row_softmax_backward: null object"); return MI355_SPMV_EINVAL; }
    if (const int st = row_softmax_check_execute("row_softmax_backward", m->nnz, p, "p", dp, "dp", dx, "dx")) return st;
    return row_softmax_run(*m, true, p, dp, dx, stream);
}

int mi355_spmv_row_softmax_get_info(const mi355_spmv_row_softmax* m, mi355_spmv_row_softmax_info* info) {
    if (!m || !info) { set_error("row_softmax_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type;
    info->slice_len = kSliceLen;
    info->block_threads = kBlock;
    info->n_slices = m->n_slices;
    info->grid_blocks = slice_grid(m->n_slices);
    info->scratch_bytes = int64_t(m->scratch_bytes);
    snprintf(info->main_kernel, sizeof(info->main_kernel), "row_softmax_slice_kernel");
    return MI355_SPMV_OK;
}

int mi355_spmv_row_softmax_destroy(mi355_spmv_row_softmax* m) {
    if (!m) return MI355_SPMV_OK;
    int st = MI355_SPMV_OK;
    if (m->scratch) {
        const hipError_t e = hipFree(m->scratch);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    delete m;
    return st;
}

#define MI355_SPMV_DEFINE_ROW_SOFTMAX(SUF, OFF, OFFENUM, VAL, VALENUM)                                                   \
    int mi355_spmv_row_softmax_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, const VAL* x, \
                                     VAL* out, double scale, void* stream) {                                           \
        return row_softmax_one_shot(OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, x, out, scale, stream);    \
    }
MI355_SPMV_DEFINE_ROW_SOFTMAX(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ROW_SOFTMAX(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_ROW_SOFTMAX(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_ROW_SOFTMAX(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

}  // extern "C"
