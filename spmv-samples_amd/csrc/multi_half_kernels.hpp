// multi_half_kernels.hpp — multi-vector SpMV with X and Y stored in 16 bits (MI355_VAL_F16 / MI355_VAL_BF16) and fp32
// arithmetic (mi355_spmv_multi_create_half).  The geometry is multi_kernels.hpp's: one wave per slice
// of kMultiSlice merge items, the wave searches its own diagonals, row offsets in LDS, lanes = (slot x 16-byte column
// group), the same segmented scan and open-row state machine.  The kernels live in a namespace of their own — a
// template argument is part of a kernel's name, so a storage type on multi_slice_kernel itself would rename every one
// of the fp32 / fp64 / int32 kernels; as it is their units compile to the device code they compiled to before.
//
// What differs from multi_slice_kernel:
//   - a lane's 16 bytes are EIGHT columns: V = 8 with fp32 acc / p, tiles of 8 / 16 / 32 / 64 columns for C = 1 / 2 / 4 / 8
//   - every stored 16-bit value is widened exactly to fp32; products and sums are fp32; Ax (vec_t or float) is loaded as
//     stored, one per lane, and widened in front of the shuffle
//   - Y is rounded to the 16-bit type ONCE per row: out = alpha * S, + beta * float(Yold) when beta != 0, then nearest
//     even (overflow to +-inf, NaN stays NaN).  A row that crosses slices is therefore never written by a slice: the
//     slices it runs through leave fp32 carries, the slice that holds its last nonzero leaves the row's fp32 partial in
//     its TAIL (tail_val[slice][carry_ld]), and the fix-up thread of the row adds the carries in slice order, then the
//     tail, reads Yold only when beta != 0 and stores the rounded row.  It is the row's only writer.
//   - every execute rewrites carry_row of every slice, and the carry / tail of every slice that has one, for the k
//     columns of the execute: the fix-up reads nothing that an earlier (wider) execute left.
// The conversions are plain C++ (casts and integer bit operations), as in csr_vector_h16.hip; where the compiler has no
// _Float16 (the host compiler of the lane-by-lane simulation) binary16 is held as uint16_t and converted in software.
#pragma once

#include "multi_kernels.hpp"

namespace mi355 {
namespace mh {

#ifdef __FLT16_MANT_DIG__
using F16 = _Float16;
__host__ __device__ __forceinline__ float widen(F16 v) { return float(v); }                           // (v_cvt_f32_f16)
__host__ __device__ __forceinline__ F16 narrow_to(float v, F16) { return F16(v); }                    // (v_cvt_f16_f32)
__host__ __device__ __forceinline__ uint16_t bits_of(F16 v) { return __builtin_bit_cast(uint16_t, v); }
__host__ __device__ __forceinline__ F16 from_bits(uint16_t b, F16) { return __builtin_bit_cast(F16, b); }
#else
struct F16 { uint16_t bits; };
inline float widen(F16 h) {
    const uint32_t s = uint32_t(h.bits & 0x8000u) << 16, e = (h.bits >> 10) & 31u, m = h.bits & 0x3FFu;
    if (e == 0) {       // zero or subnormal: m * 2^-24, exact in fp32
        const float v = float(m) * 5.9604644775390625e-08f;
        return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | s);
    }
    if (e == 31) return __builtin_bit_cast(float, s | 0x7F800000u | (m << 13));
    return __builtin_bit_cast(float, s | ((e + 112u) << 23) | (m << 13));
}
inline F16 narrow_to(float v, F16) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v), s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return F16{uint16_t(s | 0x7E00u | ((a >> 13) & 0x3FFu))};      // NaN stays NaN (quiet)
    if (a >= 0x47800000u) return F16{uint16_t(s | 0x7C00u)};                            // 65 536 and beyond: inf
    if (a >= 0x38800000u) {                                                             // normal: nearest, ties to even
        uint32_t r = a - (112u << 23);
        r += 0xFFFu + ((r >> 13) & 1u);                                                 // (65 520 and beyond carry into inf)
        return F16{uint16_t(s | (r >> 13))};
    }
    if (a <= 0x33000000u) return F16{uint16_t(s)};                                      // up to 2^-25 (a tie to even): zero
    const uint32_t mant = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - (a >> 23);        // 14 .. 24
    uint32_t h = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u))) ++h;                                   // (0x400 = the smallest normal)
    return F16{uint16_t(s | h)};
}
inline uint16_t bits_of(F16 v) { return v.bits; }
inline F16 from_bits(uint16_t b, F16) { return F16{b}; }
#endif

// bfloat16 is the upper half of an fp32; narrowing is csr_vector_h16.hip's narrow_to
__host__ __device__ __forceinline__ float widen(Bf16 v) { return __builtin_bit_cast(float, uint32_t(v.bits) << 16); }
__host__ __device__ __forceinline__ Bf16 narrow_to(float v, Bf16) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) u |= 0x00400000u;      // NaN: keep it one (quiet) when the payload's low bits go
    else u += 0x7FFFu + ((u >> 16) & 1u);                       // nearest, ties to even; carries into the exponent up to inf
    return Bf16{uint16_t(u >> 16)};
}
__host__ __device__ __forceinline__ uint16_t bits_of(Bf16 v) { return v.bits; }
__host__ __device__ __forceinline__ Bf16 from_bits(uint16_t b, Bf16) { return Bf16{b}; }
__host__ __device__ __forceinline__ float widen(float v) { return v; }      // an fp32 matrix under 16-bit vectors

constexpr int kHalfV = 8;   // columns of a lane: 16 bytes of a row of X / Y

template <typename vec_t, typename mat_t>
struct MultiHalfArgs {
    int32_t n_rows;
    int64_t nnz, n_slices;
    const int32_t* Aj;
    const mat_t* Ax;
    const vec_t* X;
    vec_t* Y;
    int64_t ldx, ldy;
    int32_t col_begin;      // first column of this pass's tile
    int32_t cols;           // columns of it that exist (<= tile width): the others are masked on load and store
    int32_t x_vec, y_vec;   // 1 = rows of X / Y are 16-byte aligned: one 16-byte access per lane
    float alpha, beta;
    int32_t* carry_row;     // [n_slices]: the row a slice leaves unfinished, or -1
    float* carry_val;       // [n_slices][carry_ld]
    float* tail_val;        // [n_slices][carry_ld]: the partial of the slice's first row, when that row began earlier and ends here
    int64_t carry_ld;
};

struct __attribute__((aligned(16), may_alias)) U32x4 { uint32_t x, y, z, w; };   // eight 16-bit columns per lane

// the lane's 8 columns of a row, widened: one 16-byte access when the row is aligned and all 8 exist, else the nv that do
template <typename vec_t>
__device__ __forceinline__ void load_cols(float (&v)[kHalfV], const vec_t* p, int nv, bool vec) {
    if (vec && nv == kHalfV) {
        const U32x4 t = *reinterpret_cast<const U32x4*>(p);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[2 * q] = widen(from_bits(uint16_t(w[q] & 0xFFFFu), vec_t()));
            v[2 * q + 1] = widen(from_bits(uint16_t(w[q] >> 16), vec_t()));
        }
    } else {
#pragma unroll
        for (int j = 0; j < kHalfV; ++j) v[j] = j < nv ? widen(p[j]) : 0.0f;
    }
}

template <typename vec_t>
__device__ __forceinline__ void store_cols(const float (&v)[kHalfV], vec_t* p, int nv, bool vec) {
    if (vec && nv == kHalfV) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = uint32_t(bits_of(narrow_to(v[2 * q], vec_t()))) | (uint32_t(bits_of(narrow_to(v[2 * q + 1], vec_t()))) << 16);
        *reinterpret_cast<U32x4*>(p) = U32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
        for (int j = 0; j < kHalfV; ++j)
            if (j < nv) p[j] = narrow_to(v[j], vec_t());
    }
}

// Y[r, tile] = round(alpha * sum + beta * float(Y[r, tile])), Y read only when beta != 0: the one rounding of the row
template <typename vec_t>
__device__ __forceinline__ void store_row(vec_t* Y, int64_t ldy, int col_begin, int cols, bool vec, float alpha, float beta,
                                          int64_t r, int c, const float (&sum)[kHalfV]) {
    const int nv = min(max(cols - c * kHalfV, 0), kHalfV);
    if (nv == 0) return;
    vec_t* yp = Y + r * ldy + col_begin + c * kHalfV;
    float out[kHalfV];
#pragma unroll
    for (int j = 0; j < kHalfV; ++j) out[j] = alpha * sum[j];
    if (beta != 0.0f) {
        float old[kHalfV];
        load_cols<vec_t>(old, yp, nv, vec);
#pragma unroll
        for (int j = 0; j < kHalfV; ++j) out[j] += beta * old[j];
    }
    store_cols<vec_t>(out, yp, nv, vec);
}

template <int C>
__device__ __forceinline__ void reduce_slots(float (&v)[kHalfV]) {
#pragma unroll
    for (int d = C; d < kWave; d <<= 1)
#pragma unroll
        for (int j = 0; j < kHalfV; ++j) v[j] += __shfl_xor(v[j], d);
}

// C = lanes per nonzero slot (16-byte column groups of the tile); the wave holds S = 64 / C slots
template <typename off_t, typename vec_t, typename mat_t, int C>
__global__ __launch_bounds__(kBlock) void multi_half_slice_kernel(const MultiHalfArgs<vec_t, mat_t> a, const off_t* __restrict__ Ap) {
    constexpr int V = kHalfV;
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
    bool carried_in = false;    // row r0 began in an earlier slice: its partial here goes to the tail, never to Y
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
        carried_in = int64_t(Ap[r0]) < n0;
    }
    __syncthreads();
    if (!active) return;

    float acc[V];           // per-slot partial of the open row (the row whose nonzeros are not all seen yet)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0f;
    int open_i = -1;        // that row, relative to r0; -1 = none (acc is zero)
    int holder = -1;        // >= 0: acc is not zero in this slot only; -2: spread over the slots
    const int nv = min(max(a.cols - c * V, 0), V);

    for (int base = 0; base < nn; base += kWave) {
        // 64 nonzeros, one per lane, coalesced (2 or 4 bytes of Ax); each lane finds its nonzero's row in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        float ax = 0.0f;
        int ie = nr * 2;    // row * 2 + (1 = this nonzero is the last of its row); nr = no nonzero
        if (m < nn) {
            col = a.Aj[n0 + m];
            ax = widen(a.Ax[n0 + m]);
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
            float ax_s = ax;
            int ie_s = ie;
            if constexpr (C > 1) {
                const int src = t * S + s;
                col_s = __shfl(col, src);
                ax_s = __shfl(ax, src);
                ie_s = __shfl(ie, src);
            }
            const int i_s = ie_s >> 1;
            float p[V];
            if (i_s < nr) {
                float xv[V];
                load_cols<vec_t>(xv, a.X + int64_t(col_s) * a.ldx + a.col_begin + c * V, nv, a.x_vec != 0);
                // a masked column was loaded as 0 and its product is the zero of the sum already
#pragma unroll
                for (int j = 0; j < V; ++j) p[j] = ax_s * xv[j];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) p[j] = 0.0f;
            }
            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one row, and the row goes on: partials stay per slot
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
                    reduce_slots<C>(acc);
                }
                if (s == 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) p[j] += acc[j];
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.0f;
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
#pragma unroll
            for (int d = C; d < kWave; d <<= 1) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float o = __shfl_up(p[j], d);
                    if (lane - c - d >= start) p[j] += o;
                }
            }
            const bool tail = s == S - 1 || ((heads >> (lane - c + C)) & 1ull);
            if (i_s < nr && tail && (ie_s & 1)) {
                if (i_s == 0 && carried_in) {
                    // the last piece of a row that crossed slices: fp32, for the fix-up (whole tiles fit carry_ld)
                    float* tv = a.tail_val + w * a.carry_ld + a.col_begin + c * V;
#pragma unroll
                    for (int j = 0; j < V; ++j) tv[j] = p[j];
                } else {
                    store_row<vec_t>(a.Y, a.ldy, a.col_begin, a.cols, a.y_vec != 0, a.alpha, a.beta, r0 + i_s, c, p);
                }
            }
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
            reduce_slots<C>(acc);
        }
        if (s == 0) {
            float* cv = a.carry_val + w * a.carry_ld + a.col_begin + c * V;    // (carry_ld covers whole tiles)
#pragma unroll
            for (int j = 0; j < V; ++j) cv[j] = acc[j];
        }
    }
    if (lane == 0) a.carry_row[w] = open_i >= 0 ? int32_t(r0 + open_i) : -1;

    // empty rows whose end lies in this slice: Y = beta * Y, rounded once; a row with nonzeros is stored where its last
    // one is (a row carried in has nonzeros)
    float none[V];
#pragma unroll
    for (int j = 0; j < V; ++j) none[j] = 0.0f;
    for (int64_t r = r0 + s; r < r1; r += S)
        if (Ap[r] == Ap[r + 1]) store_row<vec_t>(a.Y, a.ldy, a.col_begin, a.cols, a.y_vec != 0, a.alpha, a.beta, r, c, none);
}

// one thread per (slice, column): the first slice that carries a row sums its carries in slice order, then the tail —
// which lies in the slice after the last one that carries the row, and that slice holds at least one nonzero of it —
// and stores the rounded row.  No slice has written it.
template <typename vec_t>
__global__ __launch_bounds__(kBlock) void multi_half_fixup_kernel(int64_t n_slices, int32_t k, const int32_t* __restrict__ carry_row,
                                                                  const float* __restrict__ carry_val,
                                                                  const float* __restrict__ tail_val, int64_t carry_ld,
                                                                  vec_t* __restrict__ Y, int64_t ldy, float alpha, float beta) {
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t = gid / k;
    const int j = int(gid % k);
    if (t >= n_slices) return;
    const int32_t r = carry_row[t];
    if (r < 0 || (t > 0 && carry_row[t - 1] == r)) return;
    float sum = carry_val[t * carry_ld + j];
    int64_t u = t + 1;
    for (; u < n_slices && carry_row[u] == r; ++u) sum += carry_val[u * carry_ld + j];
    if (u < n_slices) sum += tail_val[u * carry_ld + j];    // (always: an open row has a nonzero in the next slice)
    vec_t& y = Y[int64_t(r) * ldy + j];
    float out = alpha * sum;
    if (beta != 0.0f) out += beta * widen(y);
    y = narrow_to(out, vec_t());
}

}  // namespace mh

// the passes of one execute (tiles of 64 columns, the last one as narrow as fits) and the fix-up
template <typename off_t, typename vec_t, typename mat_t>
int launch_multi_half(const MultiShape& m, const void* Ax, const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t k, hipStream_t s) {
    static_assert(sizeof(vec_t) == 2 && (sizeof(mat_t) == 2 || sizeof(mat_t) == 4), "16-bit vectors; the matrix in their type or fp32");
    if (m.n_slices == 0) return MI355_SPMV_OK;      // no rows: nothing to write
    constexpr int V = mh::kHalfV;
    constexpr int kWidest = V * kMultiGroupsMax;
    mh::MultiHalfArgs<vec_t, mat_t> a;
    a.n_rows = m.n_rows; a.nnz = m.nnz; a.n_slices = m.n_slices;
    a.Aj = m.Aj; a.Ax = static_cast<const mat_t*>(Ax);
    a.X = static_cast<const vec_t*>(X); a.Y = static_cast<vec_t*>(Y);
    a.ldx = ldx; a.ldy = ldy;
    a.x_vec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && (size_t(ldx) * sizeof(vec_t)) % 16 == 0) ? 1 : 0;
    a.y_vec = (reinterpret_cast<uintptr_t>(Y) % 16 == 0 && (size_t(ldy) * sizeof(vec_t)) % 16 == 0) ? 1 : 0;
    a.alpha = float(m.alpha); a.beta = float(m.beta);
    a.carry_row = m.carry_row; a.carry_val = static_cast<float*>(m.carry_val); a.tail_val = static_cast<float*>(m.tail_val);
    a.carry_ld = m.carry_ld;
    const off_t* Ap = static_cast<const off_t*>(m.Ap);
    const dim3 grid(unsigned((m.n_slices + kMultiWaves - 1) / kMultiWaves)), block(kBlock);
    for (int32_t cb = 0; cb < k; cb += kWidest) {
        a.col_begin = cb;
        a.cols = std::min<int32_t>(k - cb, kWidest);
        const int groups = (a.cols + V - 1) / V;
        if (groups <= 1) hipLaunchKernelGGL((mh::multi_half_slice_kernel<off_t, vec_t, mat_t, 1>), grid, block, 0, s, a, Ap);
        else if (groups <= 2) hipLaunchKernelGGL((mh::multi_half_slice_kernel<off_t, vec_t, mat_t, 2>), grid, block, 0, s, a, Ap);
        else if (groups <= 4) hipLaunchKernelGGL((mh::multi_half_slice_kernel<off_t, vec_t, mat_t, 4>), grid, block, 0, s, a, Ap);
        else hipLaunchKernelGGL((mh::multi_half_slice_kernel<off_t, vec_t, mat_t, 8>), grid, block, 0, s, a, Ap);
        MI355_HIP_TRY(hipGetLastError());
    }
    if (m.n_slices > 1) {
        const int64_t threads = m.n_slices * k;
        hipLaunchKernelGGL((mh::multi_half_fixup_kernel<vec_t>), dim3(unsigned((threads + kBlock - 1) / kBlock)), block, 0, s,
                           m.n_slices, k, m.carry_row, a.carry_val, a.tail_val, m.carry_ld, a.Y, ldy, a.alpha, a.beta);
        MI355_HIP_TRY(hipGetLastError());
    }
    return MI355_SPMV_OK;
}

// MI355_MULTI_HALF_EACH(X): X(off_t, vec_t, mat_t) for both offset widths, both 16-bit types, the matrix in the vectors'
// type and in fp32 — the eight launch_multi_half (32 slice kernels) of multi_h16.hip
#define MI355_MULTI_HALF_EACH(X)                                                                          \
    X(int32_t, mh::F16, mh::F16) X(int64_t, mh::F16, mh::F16) X(int32_t, mh::F16, float) X(int64_t, mh::F16, float) \
    X(int32_t, Bf16, Bf16) X(int64_t, Bf16, Bf16) X(int32_t, Bf16, float) X(int64_t, Bf16, float)
#define MI355_MULTI_HALF_DEFINE(OFF, VEC, MAT) \
    template int launch_multi_half<OFF, VEC, MAT>(const MultiShape&, const void*, const void*, int64_t, void*, int64_t, int32_t, hipStream_t);
#define MI355_MULTI_HALF_DECLARE(OFF, VEC, MAT) extern MI355_MULTI_HALF_DEFINE(OFF, VEC, MAT)

#ifdef MI355_MULTI_SPLIT_UNITS      // the library's build: multi_h16.hip defines them
MI355_MULTI_HALF_EACH(MI355_MULTI_HALF_DECLARE)
#endif

}  // namespace mi355
