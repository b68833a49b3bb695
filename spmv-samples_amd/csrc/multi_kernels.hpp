// multi_kernels.hpp — the device code and the launch of multi-vector SpMV (mi355_spmv_multi_*):
// Y[r, j] = reduce over the row of combine(Ax[n], X[Aj[n], j]) for k vectors in one pass over A, over a semiring SR
// (semiring.hpp), a value type in {float, double, int32_t} and a PATTERN flag (no stored values: every entry is one).
// A header: multi.hip holds the entry points; the multi_*.hip units instantiate launch_multi per value type (under
// MI355_MULTI_SPLIT_UNITS multi.hip only declares those instantiations; without it a unit that includes this header
// instantiates what it uses, which is how the host simulation compiles multi.hip alone).
//
// X is row-major (n_cols x k, leading dimension ldx): the gather of one column index pulls a whole row of X, so the
// 64/128-byte line a single-vector gather takes 4 bytes out of is used in full, and Aj / Ax cross HBM once, not k times.
//
//   multi_slice_kernel   one WAVE per slice of kSliceLen merge items (row ends + nonzeros, so that empty rows cost
//                        what they hold and a hub row is spread over as many waves as it has slices).  The wave finds
//                        its two merge-path diagonals, keeps its rows' offsets in LDS, and walks its nonzeros 64 at a
//                        time: Aj / Ax are loaded coalesced, one per lane, and handed to the (slot x column group)
//                        lanes by shuffles.  A lane gathers 16 bytes of a row of X.  Partials stay in registers: steps
//                        that lie inside one row accumulate per slot; a step that holds a row's end is reduced across
//                        the slots by a segmented scan (shuffles), and the slot that holds the end stores the row of Y.
//                        What is left of a row that runs on into the next slice goes to the slice's carry.
//                        The cut (the diagonals, the offsets in LDS, a nonzero's row) and the 16-byte column access
//                        are shared with SDDMM: slice_cut.hpp, slice_cut.inc, slice_cut_row.inc.
//   multi_fixup_kernel   reduces the carries of a row into Y in slice order (no atomics: two executes, same bits).
//
// Identity rule: wherever nothing is there — a slot past the slice's last nonzero, a masked column, the reset of the
// open partial, an empty row — the value is SR::identity(), never a combine() of zeros: under (min, +) a zero is a
// path of length 0, and INT32_MAX + x overflows.  An identity only ever meets reduce().
// What Y holds after the slice passes: every row r is written by exactly one slice — the one that holds the row's
// last nonzero (for an empty row: its row-end item) — with the reduction of the row's nonzeros that lie in that slice,
// the identity for an empty row.  Earlier slices of the row leave carries, and the fix-up sets
// Y[r, j] = reduce(Y[r, j], carries in slice order).  (+, *) on floating point keeps alpha / beta: the slice writes
// alpha * sum + beta * Y, the fix-up adds alpha * sum.  Under the other semirings, and for int32, Y is never read by
// the slice kernel and alpha / beta do not exist.
#pragma once

#include <algorithm>
#include <type_traits>

#include "semiring.hpp"
#include "slice_cut.hpp"

namespace mi355 {

template <typename val_t>
struct MultiArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const val_t* Ax;        // null for a PATTERN kernel, which never forms an address from it
    const val_t* X;
    val_t* Y;
    int64_t ldx, ldy;
    int32_t col_begin;      // first column of this pass's tile
    int32_t cols;           // columns of it that exist (<= tile width): the others are masked on load and store
    int32_t x_vec, y_vec;   // 1 = rows of X / Y are 16-byte aligned: one 16-byte access per lane
    val_t alpha, beta;      // (+, *) on floating point only
    int32_t* carry_row;     // [n_slices]: the row a slice leaves unfinished, or -1
    val_t* carry_val;       // [n_slices][carry_ld]
    int64_t carry_ld;
};

// alpha / beta exist for (+, *) on floating point; everything else stores what it reduced
template <int SRI, typename val_t>
constexpr bool kMultiScaled = SRI == MI355_SEMIRING_PLUS_TIMES && std::is_floating_point<val_t>::value;

// (+, *) on floating point: Y[r, tile] = alpha * sum + beta * Y[r, tile], Y read only when beta != 0.
// Otherwise Y[r, tile] = sum, and Y is not read.
template <int SRI, typename val_t, int V>
__device__ __forceinline__ void store_row(const MultiArgs<val_t>& a, int64_t r, int c, const val_t (&sum)[V]) {
    const int nv = min(max(a.cols - c * V, 0), V);
    if (nv == 0) return;
    val_t* yp = a.Y + r * a.ldy + a.col_begin + c * V;
    if constexpr (kMultiScaled<SRI, val_t>) {
        val_t out[V];
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = a.alpha * sum[j];
        if (a.beta != val_t(0)) {
            val_t old[V];
            load_cols<val_t, V>(old, yp, nv, a.y_vec != 0);
#pragma unroll
            for (int j = 0; j < V; ++j) out[j] += a.beta * old[j];
        }
        store_cols<val_t, V>(out, yp, nv, a.y_vec != 0);
    } else {
        store_cols<val_t, V>(sum, yp, nv, a.y_vec != 0);
    }
}

// the reduction over all slots of a per-slot partial, in every lane of the column group (xor butterfly: the same bits
// everywhere for a commutative reduce, which all five are)
template <typename SR, typename acc_t, int V, int C>
__device__ __forceinline__ void reduce_slots(acc_t (&v)[V]) {
#pragma unroll
    for (int d = C; d < kWave; d <<= 1)
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = SR::reduce(v[j], __shfl_xor(v[j], d));
}

// the typed kernels' policy (multi_slice_walk.inc says what a policy holds): everything in val_t, the values as stored or none (PATTERN), a row stored where it ends
template <typename val_t, int SRI, bool PATTERN>
struct MultiTypedPolicy {
    using acc_t = val_t;
    using SR = Semiring<SRI, val_t>;
    using Args = MultiArgs<val_t>;
    static constexpr int V = 16 / int(sizeof(val_t));
    static constexpr bool kValued = !PATTERN, kMaskCombine = SRI != MI355_SEMIRING_PLUS_TIMES, kTails = false, kPermuted = false;
    __device__ static __forceinline__ val_t ax(val_t v) { return v; }
    __device__ static __forceinline__ void load_cols(val_t (&v)[V], const val_t* p, int nv, bool vec) {
        mi355::load_cols<val_t, V>(v, p, nv, vec);
    }
    static constexpr bool kFields = false;
    static constexpr val_t kAxFill = val_t(1);
    __device__ static __forceinline__ void store_row(const Args& a, int64_t r, int c, const val_t (&sum)[V]) {
        mi355::store_row<SRI, val_t, V>(a, r, c, sum);
    }
};

template <typename off_t, typename val_t, int C, int SRI, bool PATTERN>
__global__ __launch_bounds__(kBlock) void multi_slice_kernel(const MultiArgs<val_t> a, const off_t* __restrict__ Ap) {
    using P = MultiTypedPolicy<val_t, SRI, PATTERN>;
#include "multi_slice_walk.inc"
}

// The permuted kernels (mi355_spmv_multi_create_permuted): the typed walk under (+, *) on a valued fp32 /
// fp64 matrix, with nonzero n's value read as Ax[perm[n]].  perm is the object's own validated 4-byte copy: every index
// is inside the n_values values of Ax, so the gather cannot leave the caller's array.
template <typename val_t>
struct MultiPermArgs : MultiArgs<val_t> {
    const uint32_t* perm;   // [nnz]
};
template <typename val_t>
struct MultiPermPolicy : MultiTypedPolicy<val_t, MI355_SEMIRING_PLUS_TIMES, false> {
    using Args = MultiPermArgs<val_t>;
    static constexpr bool kPermuted = true;
};

template <typename off_t, typename val_t, int C>
__global__ __launch_bounds__(kBlock) void multi_perm_slice_kernel(const MultiPermArgs<val_t> a, const off_t* __restrict__ Ap) {
    using P = MultiPermPolicy<val_t>;
#include "multi_slice_walk.inc"
}

// one thread per (slice, column): the first slice that carries a row reduces all its carries, in slice order, into Y
template <typename val_t, int SRI>
__global__ __launch_bounds__(kBlock) void multi_fixup_kernel(int64_t n_slices, int32_t k, const int32_t* __restrict__ carry_row,
                                                             const val_t* __restrict__ carry_val, int64_t carry_ld,
                                                             val_t* __restrict__ Y, int64_t ldy, val_t alpha) {
    using SR = Semiring<SRI, val_t>;
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t = gid / k;
    const int j = int(gid % k);
    if (t >= n_slices) return;
    const int32_t r = carry_row[t];
    if (r < 0 || (t > 0 && carry_row[t - 1] == r)) return;
    val_t sum = carry_val[t * carry_ld + j];
    for (int64_t u = t + 1; u < n_slices && carry_row[u] == r; ++u) sum = SR::reduce(sum, carry_val[u * carry_ld + j]);
    val_t& y = Y[int64_t(r) * ldy + j];
    if constexpr (kMultiScaled<SRI, val_t>) y += alpha * sum;
    else y = SR::reduce(y, sum);
}

// what an execute reads of the object (struct mi355_spmv_multi, multi.hip)
struct MultiShape {
    int32_t n_rows = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;
    double alpha = 1.0, beta = 0.0;
    int64_t n_slices = 0;
    int64_t carry_ld = 0;           // k_max rounded up to whole widest tiles
    int32_t* carry_row = nullptr;
    void* carry_val = nullptr;
    void* tail_val = nullptr;       // 16-bit vectors only (multi_half_kernels.hpp): [n_slices][carry_ld] fp32
    const uint32_t* perm = nullptr; // a permuted object only: [nnz] indices into the Ax of an execute, each below n_values
};

// what both argument structs (MultiArgs, mh::MultiHalfArgs) hold alike, of the object and of one execute's operands
template <typename Args, typename vec_t>
void multi_fill_args(Args& a, const MultiShape& m, const void* X, int64_t ldx, void* Y, int64_t ldy) {
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.Aj = m.Aj;
    a.X = static_cast<const vec_t*>(X); a.Y = static_cast<vec_t*>(Y);
    a.ldx = ldx; a.ldy = ldy;
    a.x_vec = rows_aligned16<vec_t>(X, ldx) ? 1 : 0;
    a.y_vec = rows_aligned16<vec_t>(Y, ldy) ? 1 : 0;
    a.alpha = decltype(a.alpha)(m.alpha); a.beta = decltype(a.beta)(m.beta);
    a.carry_row = m.carry_row; a.carry_val = static_cast<decltype(a.carry_val)>(m.carry_val); a.carry_ld = m.carry_ld;
}

// the passes of one execute: tiles of V * kSliceGroupsMax columns, the last one as narrow as fits.  slice(lanes) launches
// the slice kernel of C = lanes::value lanes per slot on the tile that a.col_begin / a.cols describe.
template <int V, typename Args, typename Slice>
int multi_passes(Args& a, int32_t k, Slice slice) {
    constexpr int kWidest = V * kSliceGroupsMax;
    for (int32_t cb = 0; cb < k; cb += kWidest) {
        a.col_begin = cb;
        a.cols = std::min<int32_t>(k - cb, kWidest);
        with_slot_lanes((a.cols + V - 1) / V, slice);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

// the slice passes and the fix-up
template <typename off_t, typename val_t, int SRI, bool PATTERN>
int launch_multi(const MultiShape& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    if (m.n_slices == 0) return MI355_SPMV_OK;      // no rows: nothing to write
    MultiArgs<val_t> a;
    multi_fill_args<MultiArgs<val_t>, val_t>(a, m, X, ldx, Y, ldy);
    a.Ax = PATTERN ? nullptr : static_cast<const val_t*>(Ax);
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    if (const int st = multi_passes<16 / int(sizeof(val_t))>(a, k, [&](auto lanes) {
            hipLaunchKernelGGL((multi_slice_kernel<off_t, val_t, decltype(lanes)::value, SRI, PATTERN>), grid, block, 0, s, a, Ap);
        }))
        return st;
    if (m.n_slices > 1) {
        const int64_t threads = m.n_slices * k;
        hipLaunchKernelGGL((multi_fixup_kernel<val_t, SRI>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s,
                           m.n_slices, k, m.carry_row, a.carry_val, m.carry_ld, a.Y, ldy, a.alpha);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

// the same for a permuted object: the permuted slice passes, then the typed fix-up of (+, *)
template <typename off_t, typename val_t>
int launch_multi_perm(const MultiShape& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    if (m.n_slices == 0) return MI355_SPMV_OK;
    MultiPermArgs<val_t> a;
    multi_fill_args<MultiPermArgs<val_t>, val_t>(a, m, X, ldx, Y, ldy);
    a.Ax = static_cast<const val_t*>(Ax);
    a.perm = m.perm;
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned(slice_grid(m.n_slices))), block(kBlock);
    if (const int st = multi_passes<16 / int(sizeof(val_t))>(a, k, [&](auto lanes) {
            hipLaunchKernelGGL((multi_perm_slice_kernel<off_t, val_t, decltype(lanes)::value>), grid, block, 0, s, a, Ap);
        }))
        return st;
    if (m.n_slices > 1) {
        const int64_t threads = m.n_slices * k;
        hipLaunchKernelGGL((multi_fixup_kernel<val_t, MI355_SEMIRING_PLUS_TIMES>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s,
                           m.n_slices, k, m.carry_row, a.carry_val, m.carry_ld, a.Y, ldy, a.alpha);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}
#define MI355_MULTI_PERM_DEFINE(OFF, VAL) \
    template int launch_multi_perm<OFF, VAL>(const MultiShape&, const void*, const void*, int64_t, void*, int64_t, int32_t, hipStream_t);
#define MI355_MULTI_PERM_EACH(X, VAL) X(int32_t, VAL) X(int64_t, VAL)
#define MI355_MULTI_PERM_DECLARE(OFF, VAL) extern MI355_MULTI_PERM_DEFINE(OFF, VAL)

// MI355_MULTI_EACH(X, val_t, SRI): X(off_t, val_t, SRI, PATTERN) for both offset widths, valued and pattern — the four
// launch_multi (sixteen slice kernels) of one value type under one semiring
#define MI355_MULTI_EACH(X, VAL, SRI) \
    X(int32_t, VAL, SRI, false) X(int64_t, VAL, SRI, false) X(int32_t, VAL, SRI, true) X(int64_t, VAL, SRI, true)
#define MI355_MULTI_EACH_SEMIRING(X, VAL)                                                                      \
    MI355_MULTI_EACH(X, VAL, MI355_SEMIRING_PLUS_TIMES) MI355_MULTI_EACH(X, VAL, MI355_SEMIRING_MIN_PLUS)      \
    MI355_MULTI_EACH(X, VAL, MI355_SEMIRING_MAX_TIMES) MI355_MULTI_EACH(X, VAL, MI355_SEMIRING_MAX_PLUS)       \
    MI355_MULTI_EACH(X, VAL, MI355_SEMIRING_OR_AND)
#define MI355_MULTI_DEFINE(OFF, VAL, SRI, PATTERN) \
    template int launch_multi<OFF, VAL, SRI, PATTERN>(const MultiShape&, const void*, const void*, int64_t, void*, int64_t, int32_t, hipStream_t);
#define MI355_MULTI_DECLARE(OFF, VAL, SRI, PATTERN) extern MI355_MULTI_DEFINE(OFF, VAL, SRI, PATTERN)

#ifdef MI355_MULTI_SPLIT_UNITS      // the library's build: multi_f32.hip, multi_f64.hip and multi_i32.hip define them
MI355_MULTI_EACH_SEMIRING(MI355_MULTI_DECLARE, float)
MI355_MULTI_EACH_SEMIRING(MI355_MULTI_DECLARE, double)
MI355_MULTI_EACH_SEMIRING(MI355_MULTI_DECLARE, int32_t)
MI355_MULTI_PERM_EACH(MI355_MULTI_PERM_DECLARE, float)      // multi_perm_f32.hip, multi_perm_f64.hip
MI355_MULTI_PERM_EACH(MI355_MULTI_PERM_DECLARE, double)
#endif

// What the units that make permuted objects (multi_perm.hip, multi_transposed.hip) ask of multi.hip, which defines both.
// multi_attach_perm turns a new object of mi355_spmv_multi_create into a permuted one: its executes read Ax[perm[n]] for
// n_values values of Ax.  `held` (device memory of held_bytes bytes that holds perm and, with owns_structure, the object's
// Ap and Aj too) becomes the object's and is freed by its destroy.  The caller has checked every index of perm.
int multi_attach_perm(::mi355_spmv_multi* m, const uint32_t* perm, int64_t n_values, void* held, size_t held_bytes,
                      bool owns_structure);
const MultiShape& multi_shape_of(const ::mi355_spmv_multi* m);

}  // namespace mi355
