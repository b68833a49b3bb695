// multi.hip — multi-vector SpMV, Y = alpha * A X + beta * Y for k vectors in one pass over A (mi355_spmv_multi_*).
// An object of its own: it shares no chunk body, planner or launch path with the VECTOR / LIGHT / MERGE kinds, and
// this translation unit holds all of it — kernels, host launch, the extern "C" entry points.  DESIGN.md §3.10.
//
// X is row-major (n_cols x k, leading dimension ldx): the gather of one column index pulls a whole row of X, so the
// 64/128-byte line a single-vector gather takes 4 bytes out of is used in full, and Aj / Ax cross HBM once, not k times.
//
//   multi_slice_kernel   one WAVE per slice of kMultiSlice merge items (row ends + nonzeros, so that empty rows cost
//                        what they hold and a hub row is spread over as many waves as it has slices).  The wave finds
//                        its two merge-path diagonals, keeps its rows' offsets in LDS, and walks its nonzeros 64 at a
//                        time: Aj / Ax are loaded coalesced, one per lane, and handed to the (slot x column group)
//                        lanes by shuffles.  A lane gathers 16 bytes of a row of X.  Sums stay in registers: steps that
//                        lie inside one row accumulate per slot; a step that holds a row's end is reduced across the
//                        slots by a segmented scan (shuffles), and the slot that holds the end stores the row of Y.
//                        What is left of a row that runs on into the next slice goes to the slice's carry.
//   multi_fixup_kernel   adds the carries of a row to Y in slice order (no float atomics: two executes, same bits).

#include <algorithm>
#include <new>

#include "common.hpp"

namespace mi355 {

constexpr int kMultiSlice = 1024;               // merge items per slice (= per wave)
constexpr int kMultiWaves = kBlock / kWave;     // slices per workgroup
constexpr int kMultiGroupsMax = 8;              // most 16-byte column groups of a tile: 32 fp32 / 16 fp64 columns

template <typename val_t>
struct MultiArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const val_t* Ax;
    const val_t* X;
    val_t* Y;
    int64_t ldx, ldy;
    int32_t col_begin;      // first column of this pass's tile
    int32_t cols;           // columns of it that exist (<= tile width): the others are masked on load and store
    int32_t x_vec, y_vec;   // 1 = rows of X / Y are 16-byte aligned: one 16-byte access per lane
    val_t alpha, beta;
    int32_t* carry_row;     // [n_slices]: the row a slice leaves unfinished, or -1
    val_t* carry_val;       // [n_slices][carry_ld]
    int64_t carry_ld;
};

template <typename val_t> struct Pack16;
template <> struct Pack16<float> { using type = float4; };
template <> struct Pack16<double> { using type = double2; };

// the lane's V columns of a row: one 16-byte access when the row is aligned and all V exist, else the nv that do
template <typename val_t, int V>
__device__ __forceinline__ void load_cols(val_t (&v)[V], const val_t* p, int nv, bool vec) {
    if (vec && nv == V) {
        const auto t = *reinterpret_cast<const typename Pack16<val_t>::type*>(p);
        v[0] = t.x; v[1] = t.y;
        if constexpr (V == 4) { v[2] = t.z; v[3] = t.w; }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = j < nv ? p[j] : val_t(0);
    }
}

template <typename val_t, int V>
__device__ __forceinline__ void store_cols(const val_t (&v)[V], val_t* p, int nv, bool vec) {
    if (vec && nv == V) {
        typename Pack16<val_t>::type t;
        t.x = v[0]; t.y = v[1];
        if constexpr (V == 4) { t.z = v[2]; t.w = v[3]; }
        *reinterpret_cast<typename Pack16<val_t>::type*>(p) = t;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < nv) p[j] = v[j];
    }
}

// Y[r, tile] = alpha * sum + beta * Y[r, tile]; Y is read only when beta != 0
template <typename val_t, int V>
__device__ __forceinline__ void store_row(const MultiArgs<val_t>& a, int64_t r, int c, const val_t (&sum)[V]) {
    const int nv = min(max(a.cols - c * V, 0), V);
    if (nv == 0) return;
    val_t* yp = a.Y + r * a.ldy + a.col_begin + c * V;
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
}

// the sum over all slots of a per-slot partial, in every lane of the column group (xor butterfly: the same bits everywhere)
template <typename val_t, int V, int C>
__device__ __forceinline__ void reduce_slots(val_t (&v)[V]) {
#pragma unroll
    for (int d = C; d < kWave; d <<= 1)
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] += __shfl_xor(v[j], d);
}

// C = lanes per nonzero slot (16-byte column groups of the tile); the wave holds S = 64 / C slots
template <typename off_t, typename val_t, int C>
__global__ __launch_bounds__(kBlock) void multi_slice_kernel(const MultiArgs<val_t> a, const off_t* __restrict__ Ap) {
    constexpr int V = 16 / int(sizeof(val_t));
    constexpr int S = kWave / C;
    // row offsets of the slice relative to its first nonzero, clamped to [0, nn + 1]: entry i belongs to row r0 + i
    __shared__ int32_t rel_all[kMultiWaves][kMultiSlice + 2];
    const int lane = threadIdx.x & (kWave - 1);
    const int c = lane % C, s = lane / C;
    int32_t* rel = rel_all[threadIdx.x / kWave];
    const int64_t w = int64_t(blockIdx.x) * kMultiWaves + threadIdx.x / kWave;
    const bool active = w < a.n_slices;
    int64_t r0 = 0, r1 = 0, n0 = 0;
    int nr = -1, nn = 0;
    if (active) {
        // merge-path diagonals of the slice: lanes 0..31 search its start, lanes 32..63 its end.  Row end r comes before
        // nonzero n iff Ap[r + 1] <= n; (r, n) = row ends and nonzeros in front of the diagonal.
        const int64_t items = int64_t(a.n_rows) + a.nnz;
        int64_t d = (lane < 32 ? w : w + 1) * kMultiSlice;
        if (d > items) d = items;
        int64_t lo = d > a.nnz ? d - a.nnz : 0, hi = d < a.n_rows ? d : a.n_rows;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (int64_t(Ap[mid + 1]) <= d - mid - 1) lo = mid + 1; else hi = mid;
        }
        const int64_t n = d - lo;
        r0 = __shfl(lo, 0); r1 = __shfl(lo, 32);
        n0 = __shfl(n, 0);
        nn = int(__shfl(n, 32) - n0);
        // rows r0 .. r_last have nonzeros or their end here (row r1, when there is one, does not end in this slice)
        const int64_t r_last = r1 < a.n_rows ? r1 : int64_t(a.n_rows) - 1;
        nr = int(r_last - r0) + 1;
        for (int i = lane; i <= nr; i += kWave) {
            const int64_t v = int64_t(Ap[r0 + i]) - n0;
            rel[i] = v < 0 ? 0 : v > nn ? nn + 1 : int32_t(v);
        }
    }
    __syncthreads();
    if (!active) return;

    val_t acc[V];           // per-slot partial of the open row (the row whose nonzeros are not all seen yet)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = val_t(0);
    int open_i = -1;        // that row, relative to r0; -1 = none (acc is zero)
    int holder = -1;        // >= 0: acc is non-zero in this slot only; -2: spread over the slots
    const int nv = min(max(a.cols - c * V, 0), V);

    for (int base = 0; base < nn; base += kWave) {
        // 64 nonzeros, one per lane, coalesced; each lane finds its nonzero's row in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        val_t ax = val_t(0);
        int ie = nr * 2;    // row * 2 + (1 = this nonzero is the last of its row); nr = no nonzero
        if (m < nn) {
            col = a.Aj[n0 + m];
            ax = a.Ax[n0 + m];
            int lo = 0, hi = nr - 1;
            while (lo < hi) {           // the last i with rel[i] <= m (empty rows repeat an offset: the last is the owner)
                const int mid = (lo + hi + 1) >> 1;
                if (rel[mid] <= m) lo = mid; else hi = mid - 1;
            }
            ie = lo * 2 + (rel[lo + 1] == m + 1 ? 1 : 0);
        }
        const int left = nn - base;
        const int steps = left >= kWave ? C : (left + S - 1) / S;
        for (int t = 0; t < steps; ++t) {
            // slot s takes nonzero t * S + s of the 64
            int32_t col_s = col;
            val_t ax_s = ax;
            int ie_s = ie;
            if constexpr (C > 1) {
                const int src = t * S + s;
                col_s = __shfl(col, src);
                ax_s = __shfl(ax, src);
                ie_s = __shfl(ie, src);
            }
            const int i_s = ie_s >> 1;
            val_t p[V];
            if (i_s < nr) {
                val_t xv[V];
                load_cols<val_t, V>(xv, a.X + int64_t(col_s) * a.ldx + a.col_begin + c * V, nv, a.x_vec != 0);
#pragma unroll
                for (int j = 0; j < V; ++j) p[j] = ax_s * xv[j];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) p[j] = val_t(0);
            }
            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one row, and the row goes on: sums stay per slot
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] += p[j];
                open_i = i_first;
                holder = -2;
                continue;
            }
            // a row ends in this step (or the slice does).  The open row's partial joins slot 0, whose nonzero is the
            // next of that row; then a segmented inclusive scan over the slots sums each row's run of products.
            if (open_i >= 0) {
                if (holder >= 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = __shfl(acc[j], holder * C + c);
                } else {
                    reduce_slots<val_t, V, C>(acc);
                }
                if (s == 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) p[j] += acc[j];
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = val_t(0);
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
#pragma unroll
            for (int d = C; d < kWave; d <<= 1) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const val_t o = __shfl_up(p[j], d);
                    if (lane - c - d >= start) p[j] += o;
                }
            }
            const bool tail = s == S - 1 || ((heads >> (lane - c + C)) & 1ull);
            if (i_s < nr && tail && (ie_s & 1)) store_row<val_t, V>(a, r0 + i_s, c, p);
            // the last nonzero of the step: if its row goes on, its run's sum is the new open partial
            const int lv = min(S - 1, left - t * S - 1);
            const int ie_lv = __shfl(ie_s, lv * C);
            if (!(ie_lv & 1)) {
                open_i = ie_lv >> 1;
                holder = lv;
                if (s == lv) {
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = p[j];
                }
            } else {
                open_i = -1;
                holder = -1;
            }
        }
    }

    // the carry: what this slice holds of a row that ends in a later one
    if (open_i >= 0) {
        if (holder >= 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = __shfl(acc[j], holder * C + c);
        } else {
            reduce_slots<val_t, V, C>(acc);
        }
        if (s == 0) {
            val_t* cv = a.carry_val + w * a.carry_ld + a.col_begin + c * V;    // (carry_ld covers whole tiles)
#pragma unroll
            for (int j = 0; j < V; ++j) cv[j] = acc[j];
        }
    }
    if (lane == 0) a.carry_row[w] = open_i >= 0 ? int32_t(r0 + open_i) : -1;

    // empty rows whose end lies in this slice: Y = beta * Y (a row with nonzeros is stored where its last one is)
    val_t zero[V];
#pragma unroll
    for (int j = 0; j < V; ++j) zero[j] = val_t(0);
    for (int64_t r = r0 + s; r < r1; r += S)
        if (Ap[r] == Ap[r + 1]) store_row<val_t, V>(a, r, c, zero);
}

// one thread per (slice, column): the first slice that carries a row adds all its carries, in slice order
template <typename val_t>
__global__ __launch_bounds__(kBlock) void multi_fixup_kernel(int64_t n_slices, int32_t k, const int32_t* __restrict__ carry_row,
                                                             const val_t* __restrict__ carry_val, int64_t carry_ld,
                                                             val_t* __restrict__ Y, int64_t ldy, val_t alpha) {
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t = gid / k;
    const int j = int(gid % k);
    if (t >= n_slices) return;
    const int32_t r = carry_row[t];
    if (r < 0 || (t > 0 && carry_row[t - 1] == r)) return;
    val_t sum = carry_val[t * carry_ld + j];
    for (int64_t u = t + 1; u < n_slices && carry_row[u] == r; ++u) sum += carry_val[u * carry_ld + j];
    Y[int64_t(r) * ldy + j] += alpha * sum;
}

}  // namespace mi355

using namespace mi355;

struct mi355_spmv_multi {   // the opaque handle of include/mi355_spmv.h
    int off_type = 0, val_type = 0;
    int32_t n_rows = 0, n_cols = 0, k_max = 0;
    int64_t nnz = 0;
    const void* Ap = nullptr;
    const int32_t* Aj = nullptr;
    double alpha = 1.0, beta = 0.0;
    int64_t n_slices = 0;
    int64_t carry_ld = 0;           // k_max rounded up to whole widest tiles
    void* scratch = nullptr;        // carry_row, then carry_val
    size_t scratch_bytes = 0;
    int32_t* carry_row = nullptr;
    void* carry_val = nullptr;
};

namespace {

int widest_tile(int val_type) { return val_type == MI355_VAL_F64 ? 16 : 32; }

// argument-only checks of an execute (also run by the one-shots before they create anything)
int check_execute_args(const char* who, int32_t n_rows, int64_t nnz, int32_t k_max, const void* Ax, const void* X, int64_t ldx,
                       const void* Y, int64_t ldy, int32_t k) {
    if (k < 1 || k > k_max) { set_error("%s: k = %d outside 1 .. k_max = %d", who, k, k_max); return MI355_SPMV_EINVAL; }
    if (ldx < k || ldy < k) { set_error("%s: leading dimension below k (ldx %lld, ldy %lld, k %d)", who, (long long)ldx, (long long)ldy, k); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && (!Ax || !X)) { set_error("%s: null Ax or X", who); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !Y) { set_error("%s: null Y", who); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

int check_create_args(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                      const int32_t* Aj, int32_t k_max) {
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("multi_create: unknown offset type %d", off_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32 || val_type == MI355_VAL_PATTERN) {
        set_error("multi_create: integer and pattern matrices are built for the merge kind only (fp32 / fp64 here)");
        return MI355_SPMV_ENOTSUP;
    }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64) { set_error("multi_create: unknown value type %d", val_type); return MI355_SPMV_EINVAL; }
    if (n_rows < 0 || n_cols < 0 || nnz < 0) { set_error("multi_create: negative size"); return MI355_SPMV_EINVAL; }
    if (k_max < 1 || k_max > (1 << 20)) { set_error("multi_create: k_max = %d outside 1 .. 2^20", k_max); return MI355_SPMV_EINVAL; }
    if (off_type == MI355_OFF_I32 && nnz > INT32_MAX) { set_error("multi_create: nnz does not fit 32-bit offsets"); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !Ap) { set_error("multi_create: null Ap"); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !Aj) { set_error("multi_create: null Aj"); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && (n_cols == 0 || n_rows == 0)) { set_error("multi_create: nonzeros but no rows or no columns"); return MI355_SPMV_EINVAL; }
    return MI355_SPMV_OK;
}

template <typename off_t, typename val_t>
int launch_multi(const mi355_spmv_multi& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k,
                 hipStream_t s) {
    if (m.n_slices == 0) return MI355_SPMV_OK;      // no rows: nothing to write
    constexpr int V = 16 / int(sizeof(val_t));
    constexpr int kWidest = V * kMultiGroupsMax;
    MultiArgs<val_t> a;
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.Aj = m.Aj; a.Ax = static_cast<const val_t*>(Ax); a.X = static_cast<const val_t*>(X); a.Y = static_cast<val_t*>(Y);
    a.ldx = ldx; a.ldy = ldy;
    a.x_vec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && (size_t(ldx) * sizeof(val_t)) % 16 == 0) ? 1 : 0;
    a.y_vec = (reinterpret_cast<uintptr_t>(Y) % 16 == 0 && (size_t(ldy) * sizeof(val_t)) % 16 == 0) ? 1 : 0;
    a.alpha = val_t(m.alpha); a.beta = val_t(m.beta);
    a.carry_row = m.carry_row; a.carry_val = static_cast<val_t*>(m.carry_val); a.carry_ld = m.carry_ld;
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned((m.n_slices + kMultiWaves - 1) / kMultiWaves)), block(kBlock);
    for (int32_t cb = 0; cb < k; cb += kWidest) {       // passes: tiles of the widest width, the last one as narrow as fits
        a.col_begin = cb;
        a.cols = std::min<int32_t>(k - cb, kWidest);
        const int groups = (a.cols + V - 1) / V;
        if (groups <= 1) hipLaunchKernelGGL((multi_slice_kernel<off_t, val_t, 1>), grid, block, 0, s, a, Ap);
        else if (groups <= 2) hipLaunchKernelGGL((multi_slice_kernel<off_t, val_t, 2>), grid, block, 0, s, a, Ap);
        else if (groups <= 4) hipLaunchKernelGGL((multi_slice_kernel<off_t, val_t, 4>), grid, block, 0, s, a, Ap);
        else hipLaunchKernelGGL((multi_slice_kernel<off_t, val_t, 8>), grid, block, 0, s, a, Ap);
        MI355_HIP_TRY(hipGetLastError());
    }
    if (m.n_slices > 1) {
        const int64_t threads = m.n_slices * k;
        hipLaunchKernelGGL((multi_fixup_kernel<val_t>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s, m.n_slices,
                           k, m.carry_row, static_cast<const val_t*>(m.carry_val), m.carry_ld, a.Y, ldy, a.alpha);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

int passes_for(int val_type, int32_t k) { return (k + widest_tile(val_type) - 1) / widest_tile(val_type); }

int multi_one_shot(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj,
                   const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, void* stream) {
    set_error("%s", "");
    int st = check_create_args(off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k < 1 ? 1 : k);
    if (st == MI355_SPMV_OK) st = check_execute_args("multi", n_rows, nnz, k, Ax, X, ldx, Y, ldy, k);
    if (st != MI355_SPMV_OK) return st;
    mi355_spmv_multi* m = nullptr;
    st = mi355_spmv_multi_create(&m, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k);
    if (st != MI355_SPMV_OK) return st;
    st = mi355_spmv_multi_execute(m, Ax, X, ldx, Y, ldy, k, stream);
    if (st == MI355_SPMV_OK) st = mi355_spmv_stream_synchronize(stream);
    const int st2 = mi355_spmv_multi_destroy(m);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace

extern "C" {

int mi355_spmv_multi_create(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                            const void* Ap, const int32_t* Aj, int32_t k_max) {
    set_error("%s", "");
    if (!out) { set_error("multi_create: null object pointer"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (const int st = check_create_args(off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, k_max)) return st;
    mi355_spmv_multi* m = new (std::nothrow) mi355_spmv_multi();
    if (!m) { set_error("multi_create: host allocation failed"); return MI355_SPMV_ENOMEM; }
    m->off_type = off_type; m->val_type = val_type;
    m->n_rows = n_rows; m->n_cols = n_cols; m->k_max = k_max; m->nnz = nnz; m->Ap = Ap; m->Aj = Aj;
    const int64_t items = int64_t(n_rows) + nnz;
    m->n_slices = (items + kMultiSlice - 1) / kMultiSlice;
    const int widest = widest_tile(val_type);
    m->carry_ld = int64_t(k_max + widest - 1) / widest * widest;
    if (m->n_slices > 0) {
        const size_t val_bytes = val_type == MI355_VAL_F64 ? 8 : 4;
        const size_t rows_bytes = (size_t(m->n_slices) * sizeof(int32_t) + 255) / 256 * 256;
        m->scratch_bytes = rows_bytes + size_t(m->n_slices) * size_t(m->carry_ld) * val_bytes;
        const hipError_t e = hipMalloc(&m->scratch, m->scratch_bytes);
        if (e != hipSuccess) {
            set_error("multi_create: hipMalloc(%zu) -> %s", m->scratch_bytes, hipGetErrorString(e));
            delete m;
            return e == hipErrorOutOfMemory ? MI355_SPMV_ENOMEM : MI355_SPMV_EHIP;
        }
        m->carry_row = static_cast<int32_t*>(m->scratch);
        m->carry_val = static_cast<char*>(m->scratch) + rows_bytes;
    }
    *out = m;
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_set_alpha_beta(mi355_spmv_multi* m, double alpha, double beta) {
    set_error("%s", "");
    if (!m) { set_error("multi_set_alpha_beta: null object"); return MI355_SPMV_EINVAL; }
    m->alpha = alpha;
    m->beta = beta;
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_execute(mi355_spmv_multi* m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k,
                             void* stream) {
    set_error("%s", "");
    if (!m) { set_error("multi_execute: null object"); return MI355_SPMV_EINVAL; }
    if (const int st = check_execute_args("multi_execute", m->n_rows, m->nnz, m->k_max, Ax, X, ldx, Y, ldy, k)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (m->off_type == MI355_OFF_I32)
        return m->val_type == MI355_VAL_F32 ? launch_multi<int32_t, float>(*m, Ax, X, ldx, Y, ldy, k, s)
                                            : launch_multi<int32_t, double>(*m, Ax, X, ldx, Y, ldy, k, s);
    return m->val_type == MI355_VAL_F32 ? launch_multi<int64_t, float>(*m, Ax, X, ldx, Y, ldy, k, s)
                                        : launch_multi<int64_t, double>(*m, Ax, X, ldx, Y, ldy, k, s);
}

int mi355_spmv_multi_get_info(const mi355_spmv_multi* m, mi355_spmv_multi_info* info) {
    if (!m || !info) { set_error("multi_get_info: null argument"); return MI355_SPMV_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->off_type = m->off_type; info->val_type = m->val_type; info->k_max = m->k_max;
    info->slice_len = kMultiSlice;
    info->block_threads = kBlock;
    info->widest_tile = widest_tile(m->val_type);
    info->passes = passes_for(m->val_type, m->k_max);
    info->n_kernels = info->passes + (m->n_slices > 1 ? 1 : 0);
    info->n_slices = m->n_slices;
    info->grid_blocks = (m->n_slices + kMultiWaves - 1) / kMultiWaves;
    info->scratch_bytes = int64_t(m->scratch_bytes);
    snprintf(info->main_kernel, sizeof(info->main_kernel), "multi_slice_kernel");
    return MI355_SPMV_OK;
}

int mi355_spmv_multi_destroy(mi355_spmv_multi* m) {
    if (!m) return MI355_SPMV_OK;
    int st = MI355_SPMV_OK;
    if (m->scratch) {
        const hipError_t e = hipFree(m->scratch);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    delete m;
    return st;
}

#define MI355_SPMV_DEFINE_MULTI(SUF, OFF, OFFENUM, VAL, VALENUM)                                                       \
    int mi355_spmv_multi_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, const int32_t* Aj, const VAL* Ax, \
                               const VAL* X, int64_t ldx, VAL* Y, int64_t ldy, int32_t k, void* stream) {              \
        return multi_one_shot(OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, Ax, X, ldx, Y, ldy, k, stream);  \
    }
MI355_SPMV_DEFINE_MULTI(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_MULTI(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_MULTI(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

}  // extern "C"
