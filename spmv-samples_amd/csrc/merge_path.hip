// merge_path.hip — kind MERGE: merge-path load-balanced CSR SpMV for gfx950.
//
// Replaces the reference's vendored CUB pipeline:
//   search   include/spmv/merge_based/thread_search.cuh:15-49,
//            dispatch_spmv_orig.cuh:104-148            -> merge_search_kernel
//   tile     include/spmv/merge_based/agent_spmv_orig.cuh:454-757,
//            dispatch_spmv_orig.cuh:154-191            -> merge_tile_kernel
//   fix-up   include/spmv/merge_based/agent_segment_fixup.cuh:97-384,
//            dispatch_spmv_orig.cuh:197-229            -> merge_fixup_kernel
// and the offset_t-typed twin include/spmv/merge_genl/ (the only reference merge
// variant that accepts 64-bit offsets): both offset widths are instantiated here.
//
// The decomposition is the reference's: the merge of the row-end offsets
// Ap[1..n_rows] with the counting sequence 0..nnz-1 is cut into tiles of equal item
// count; a tile owns the rows that END inside it and the nonzeros inside it,
// whatever the row lengths.  What is rebuilt for MI355X:
//  * a workgroup walks a RUN of consecutive tiles (a "super-tile", ~32 K items) so
//    that (a) the window of x those tiles touch is staged through LDS once
//    (xwindow.hpp — the plain global gather, not the Aj/Ax stream, bounds SpMV on
//    this chip), (b) the next tile's Aj/Ax are already in flight in registers while
//    the current tile is walked, (c) the partial sum of a row that crosses tiles is
//    carried in a register instead of through memory: only one carry per
//    super-tile reaches the fix-up kernel;
//  * nonzeros are streamed with 16-byte-per-lane loads from the tile start
//    rounded down to a multiple of 4 (the reference reads 4 bytes per lane,
//    strided by the block, agent_spmv_orig.cuh:474-506);
//  * row ends are staged tile-relative as 32-bit integers whatever offset_t is,
//    so a 64-bit-offset matrix costs no extra LDS;
//  * the walk bounds each thread by the tile's real item count instead of
//    padding the row-end list and clamping the carry (agent_spmv_orig.cuh:543-548,
//    :744-753);
//  * the reference's cub::BlockScan of (key, value) pairs with ReduceByKeyOp
//    (agent_spmv_orig.cuh:616-629) becomes a flag-segmented wave64 scan
//    (six __shfl_up steps) plus a 4-entry cross-wave pass, written here;
//  * a row closed inside one thread is stored to y straight from the walk (no
//    per-item key/value register arrays, no LDS scatter pass);
//  * the fix-up is deterministic: one thread per distinct carried row sums that
//    row's carries in order and adds once, instead of float atomics
//    (agent_segment_fixup.cuh:228-271), so results do not change
//    from run to run;
//  * super-tile ids are remapped so each XCD walks a contiguous range of the matrix.
//
// n_cols == 1 (the reference's special kernel, dispatch_spmv_orig.cuh:68-96,
// :572-597) needs no special case here.
//
// This file is a header: the device code a value-type translation unit instantiates (merge_path_*.hip, through
// merge_launch.hpp).  The search and fix-up kernels, which do not depend on the matrix type, and the plan's shape:
// merge_plan.hip.

#pragma once

#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "row_dot.hpp"
#include "semiring.hpp"
#include "xwindow.hpp"

namespace mi355 {

// merge items per thread (IPT) is 8 or 16; a tile has kBlock * IPT - 4 items so that
// (tile nnz + 3) / 4 <= kBlock * IPT / 4 sixteen-byte groups, IPT / 4 per thread
constexpr int kMergeSuperItems = 32768;                   // items one workgroup walks at most

// ---- semirings: Extreme / Semiring<S, val_t> live in semiring.hpp (shared with the multi-vector kernels) ------------
// host: f(std::integral_constant<int, S>()) for a plan's semiring S, which the kernels take as a template argument
template <typename F>
static int with_semiring(int semiring, F&& f) {
    switch (semiring) {
        case MI355_SEMIRING_PLUS_TIMES: return f(std::integral_constant<int, MI355_SEMIRING_PLUS_TIMES>());
        case MI355_SEMIRING_MIN_PLUS: return f(std::integral_constant<int, MI355_SEMIRING_MIN_PLUS>());
        case MI355_SEMIRING_MAX_TIMES: return f(std::integral_constant<int, MI355_SEMIRING_MAX_TIMES>());
        case MI355_SEMIRING_MAX_PLUS: return f(std::integral_constant<int, MI355_SEMIRING_MAX_PLUS>());
        case MI355_SEMIRING_OR_AND: return f(std::integral_constant<int, MI355_SEMIRING_OR_AND>());
    }
    set_error("merge: unknown semiring %d", semiring);
    return MI355_SPMV_EINVAL;
}

// ---- K6: tile start coordinates ------------------------------------------------
// The split of diagonal d is the first p in [lo, hi] with Ap[p + 1] > d - p - 1.  The reference finds it
// by bisection, one thread per diagonal (thread_search.cuh:15-49): ~log2(n_rows) DEPENDENT loads, and the
// few workgroups that hold all the diagonals issue them uncoalesced.  Here L lanes share a diagonal: one
// probe per lane cuts the range (L+1)-fold per round (the predicate is monotone, so the number of probes
// below the split, a popcount of the group's ballot bits, names the sub-range), the chain is
// log_{L+1}(n_rows) + 1 loads long and the probes of a round are spread over L times as many CUs.
// L = 16 for a few thousand diagonals (latency-bound), smaller L as the diagonals alone fill the chip
// (L = 1 is the bisection); launch_merge picks L from the measured crossovers.
// The split of diagonal `diag`, searched by a group of kSearchLanes consecutive lanes (k = lane's index in its
// group, shift = the group's first lane in the wave).  Every lane of the wave must call; groups whose search has
// ended probe nothing new.  Returns the rows consumed (lo); the nonzeros consumed are nnz_begin + diag - lo.
template <int kSearchLanes, typename off_t>
__device__ __forceinline__ int64_t merge_search_group(int64_t diag, int32_t n_rows, int64_t nnz_begin, int64_t nnz,
                                                      const off_t* __restrict__ Ap, int k, int shift) {
    const int64_t count = nnz - nnz_begin;
    int64_t lo = diag - count > 0 ? diag - count : 0;
    int64_t hi = diag < n_rows ? diag : n_rows;
    while (__any(lo < hi)) {                                    // a finished group probes nothing new: c = 0
        const int64_t n = hi - lo;
        const bool last = n <= kSearchLanes;                    // every remaining position probed: c is the answer
        auto probe = [&](int j) { return last ? lo + j : lo + (int64_t(j + 1) * n) / (kSearchLanes + 1); };
        const int64_t q = probe(k);
        const int64_t qc = q < hi ? q : hi - 1;                 // clamped into [-1, n_rows): the load is in range
        const bool below = (q < hi) & (int64_t(Ap[qc + 1]) - nnz_begin <= diag - qc - 1);
        const int c = __popcll((__ballot(below) >> shift) & ((kSearchLanes == 64 ? ~0ull : (1ull << kSearchLanes) - 1)));
        if (last) {
            lo += c;
            hi = lo;
        } else {
            const int64_t new_lo = c > 0 ? probe(c - 1) + 1 : lo;
            hi = c < kSearchLanes ? probe(c) : hi;
            lo = new_lo;
        }
    }
    return lo;
}

// The stored value of a nonzero as val_t: element e of a prefetched 16-byte group, or entry k of Ax.  A pattern matrix
// (mat_t = PatternOnes, common.hpp) stores none: the value is one and neither the group nor the pointer is touched.
template <typename val_t, typename m4>
__device__ __forceinline__ val_t mat_elem(const m4& a, int e) {
    if constexpr (std::is_same<m4, PatternOnes>::value) return val_t(1);
    else return val_t(a[e]);
}
template <typename val_t, typename mat_t>
__device__ __forceinline__ val_t mat_at(const mat_t* __restrict__ Ax, int64_t k) {
    if constexpr (std::is_same<mat_t, PatternOnes>::value) return val_t(1);
    else return val_t(Ax[k]);
}

// ---- K7: one run of consecutive tiles per workgroup ---------------------------------
// SEARCH: the run's tile coordinates are found HERE (16 lanes per diagonal, up to 16 diagonals at once by the
// whole workgroup) instead of by a search kernel in front: one launch and one kernel boundary fewer per SpMV
// (the reference has the same option, agent_spmv_orig.cuh:697-719).  The workgroup's first lane group also stores
// them where the search kernel would have, so plan_merge_coords / MI355_PLAN_REUSE_STRUCTURE see the same arrays.
// mat_t: the type the matrix values are STORED in — val_t, or float under double vectors (the reference keeps the
// matrix / x / y types apart, include/spmv.h:29-34; its generalized merge kind computes in the y type,
// merge_genl.cuh:29-31): a value is widened when it meets x, products and sums are val_t throughout.  PatternOnes: the
// matrix stores no values (MI355_VAL_PATTERN) — the Ax stream is not issued, a[] takes no registers and every product is
// combine(1, x); tiles, walk, scan and carries are those of the valued kernel, so the sums come out in the same order.
template <int BLOCK, int IPT, bool VEC, bool WINDOW, int S, bool SEARCH, typename off_t, typename val_t, typename mat_t = val_t>
__global__ __launch_bounds__(BLOCK) void merge_tile_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz_begin, int64_t nnz, const off_t* __restrict__ Ap, const int32_t* __restrict__ Aj,
    const mat_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y,
    int32_t* __restrict__ tile_row_g, int64_t* __restrict__ tile_nnz_g, int64_t tile_items,
    int32_t* __restrict__ carry_row, val_t* __restrict__ carry_val, int64_t n_tiles, int32_t tiles_per_super,
    int32_t window_cap, BandHint hint, val_t alpha, val_t beta) {
    constexpr int G = IPT / 4;
    using v4 = typename Vec4<val_t>::type;
    using m4 = typename Vec4<mat_t>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window_cap values of x
    val_t* s_x = reinterpret_cast<val_t*>(s_dyn);
    __shared__ __attribute__((aligned(32))) val_t s_nz[BLOCK * IPT];   // products, index = nnz - (y0 & ~3)
    __shared__ int s_re[BLOCK * IPT + 1];                               // tile-relative row ends
    __shared__ val_t s_wave_sum[BLOCK / kWave];
    __shared__ int s_wave_flag[BLOCK / kWave];
    __shared__ int s_red[2];

    const unsigned sup = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int tid = threadIdx.x;
    const int lane64 = tid & (kWave - 1);
    const int wave = tid / kWave;
    const int64_t first = int64_t(sup) * tiles_per_super;
    const int64_t last = min(first + tiles_per_super, n_tiles);

    // tile coordinates first .. last of this run: from the search kernel's arrays, or searched here
    constexpr int kMaxRun = 32;                       // (launch_merge: tiles_per_super < kMaxRun when SEARCH)
    __shared__ int32_t s_tile_row[SEARCH ? kMaxRun + 1 : 1];
    __shared__ int64_t s_tile_nnz[SEARCH ? kMaxRun + 1 : 1];
    if constexpr (SEARCH) {
        const int64_t items = int64_t(n_rows) + (nnz - nnz_begin);
        const int n_diag = int(last - first) + 1;
        // one pass of the whole workgroup: 16 lanes per diagonal for up to BLOCK / 16 diagonals, else 8 lanes
        auto pass = [&](auto lanes_tag) {
            constexpr int L = decltype(lanes_tag)::value;
            const int d = tid / L;
            int64_t diag = (first + min(d, n_diag - 1)) * tile_items;           // surplus groups repeat the last diagonal
            if (diag > items) diag = items;
            const int64_t lo = merge_search_group<L, off_t>(diag, n_rows, nnz_begin, nnz, Ap, tid & (L - 1),
                                                            (tid & (kWave - 1)) & ~(L - 1));
            if ((tid & (L - 1)) == 0 && d < n_diag) {
                s_tile_row[d] = int32_t(lo);
                s_tile_nnz[d] = nnz_begin + diag - lo;
                if (d < n_diag - 1 || last == n_tiles) {                        // (the next run stores its own first one)
                    tile_row_g[first + d] = int32_t(lo);
                    tile_nnz_g[first + d] = nnz_begin + diag - lo;
                }
            }
        };
        if (n_diag <= BLOCK / 16) pass(std::integral_constant<int, 16>{});      // (uniform over the workgroup)
        else pass(std::integral_constant<int, 8>{});
        __syncthreads();
    }
    const int32_t* const tile_row = SEARCH ? s_tile_row - first : tile_row_g;   // (indexed by absolute tile number below)
    const int64_t* const tile_nnz = SEARCH ? s_tile_nnz - first : tile_nnz_g;

    int x0 = tile_row[first], x1 = tile_row[first + 1];
    int64_t y0 = tile_nnz[first], y1 = tile_nnz[first + 1];
    const int64_t row_lo = x0;
    const int64_t row_hi = min(int64_t(tile_row[last]) + 1, int64_t(n_rows));

    // registers holding the Aj/Ax groups of the tile about to be processed
    int4v c[G];
    [[maybe_unused]] m4 a[G];
    // branch-free: addresses are clamped below the last whole 16-byte group of the arrays (hipcc
    // serialises loads it finds in branches); the few nonzeros at or past nnz_vec are redone below
    const int64_t nnz_vec = nnz & ~int64_t(3);
    const int64_t j_max = nnz_vec - 4;                 // VEC launches guarantee nnz >= 4
    auto issue = [&](int64_t ya) {
        const int64_t base = ya & ~int64_t(3);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            int64_t j = base + 4 * int64_t(tid + g * BLOCK);
            j = j < j_max ? j : j_max;
            c[g] = stream_load(reinterpret_cast<const int4v*>(Aj + j));
            if constexpr (!std::is_same<mat_t, PatternOnes>::value) a[g] = stream_load(reinterpret_cast<const m4*>(Ax + j));
        }
    };
    if constexpr (VEC) issue(y0);
    // the window of x for all rows this run touches (incl. the row left open at its end), staged while the
    // first tile's stream is in flight
    auto first_last = [&](int64_t r, int& fc, int& lc) {
        const off_t s = Ap[r], e = Ap[r + 1];
        if (e <= s) return false;
        fc = Aj[s];
        lc = Aj[e - 1];
        return true;
    };
    const XWindow<val_t> win =
        stage_x_window<val_t>(row_lo, row_hi, n_cols, first_last, x, s_x, window_cap, s_red, hint);
    // the first BLOCK row ends of a tile are fetched one tile ahead as well (a tile with more
    // rows than that — mean row length below 8 — loads the rest when it gets there)
    auto fetch_row_end = [&](int xa, int xe) -> int64_t {
        return (tid < xe - xa) ? int64_t(Ap[int64_t(xa) + tid + 1]) : int64_t(0);
    };
    int64_t re_next = fetch_row_end(x0, x1);

    using SR = Semiring<S, val_t>;  // S = 0: the ordinary (+, *) of every other kind
    // y = alpha * (A x) + beta * y for the ordinary semiring (the fix-up adds alpha * carry); 1, 0 otherwise
    auto put = [&](int64_t row, val_t v) {
        if constexpr (S == MI355_SEMIRING_PLUS_TIMES) {
            v = alpha * v;
            if (beta != val_t(0)) v += beta * y[row];
        }
        y[row] = v;
    };
    val_t block_carry = SR::identity();   // sum so far of the row left open by the previous tile of this run
    for (int64_t t = first; t < last; ++t) {
        int x2 = x1;
        int64_t y2 = y1;
        if (t + 1 < last) {
            x2 = tile_row[t + 2];
            y2 = tile_nnz[t + 2];
        }
        const int tr = x1 - x0;            // rows that end in this tile
        const int tn = int(y1 - y0);       // nonzeros in this tile
        const int shift = VEC ? int(y0 & 3) : 0;

        // (1) products a*x for the tile's nonzeros
        if constexpr (VEC) {
            if constexpr (WINDOW) {
                // (this kernel is bound by instruction issue: the lookup is a clamp (v_min), an address and one
                // compare per element; which elements are REAL nonzeros of the tile is only worked out in the rare
                // branch where some column fell outside the window)
                const unsigned len_m1 = unsigned(win.len > 0 ? win.len - 1 : 0);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    v4 p;
                    bool any_out = false;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned rel = unsigned(c[g][e] - win.lo);
                        any_out |= rel >= unsigned(win.len);
                        p[e] = SR::combine(mat_elem<val_t>(a[g], e), win.s_x[min(rel, len_m1)]);
                    }
                    if (any_out) {                       // rare: loaded and consumed inside the branch
                        const int rel0 = 4 * (tid + g * BLOCK) - shift;   // tile-relative index of element 0
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool out = unsigned(c[g][e] - win.lo) >= unsigned(win.len);
                            if (out && (rel0 + e >= 0) && (rel0 + e < tn)) p[e] = SR::combine(mat_elem<val_t>(a[g], e), x[c[g][e]]);
                        }
                    }
                    *reinterpret_cast<v4*>(&s_nz[4 * (tid + g * BLOCK)]) = p;
                }
            } else {
                val_t xv[G][4];
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xv[g][e] = x[c[g][e]];   // every column is a loaded Aj entry: in range
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    v4 p;
#pragma unroll
                    for (int e = 0; e < 4; ++e) p[e] = SR::combine(mat_elem<val_t>(a[g], e), xv[g][e]);
                    *reinterpret_cast<v4*>(&s_nz[4 * (tid + g * BLOCK)]) = p;
                }
            }
            if (y1 > nnz_vec) {   // uniform, at most one tile: the nonzeros past the last whole group
                // Their slots were just written — with the products of the clamped group — by the thread whose
                // 16-byte store covers them, usually in another wave: the corrective stores must come after
                // that store, hence the barrier (without it the last row of a matrix with nnz % 4 != 0 was
                // wrong about once in 25 processes).
                __syncthreads();
                const int64_t k = (y0 > nnz_vec ? y0 : nnz_vec) + tid;
                if (k < y1) s_nz[int(k - y0) + shift] = SR::combine(mat_at<val_t>(Ax, k), x[Aj[k]]);
            }
            // the next tile's stream goes in flight now and lands while this tile is walked
            if (t + 1 < last) issue(y1);
        } else {
            // Aj / Ax not 16-byte aligned (an offset view): 4-byte-per-lane form
            for (int i = tid; i < tn; i += BLOCK) {
                const int32_t col = Aj[y0 + i];
                s_nz[i] = SR::combine(mat_at<val_t>(Ax, y0 + i), window_gather<val_t>(win, x, col, true));
            }
        }
        // (2) row ends, relative to y0; the row still open at the tile end never ends here
        if (tid <= tr) s_re[tid] = (tid < tr) ? int(re_next - y0) : INT_MAX;
        for (int i = tid + BLOCK; i <= tr; i += BLOCK) {
            s_re[i] = (i < tr) ? int(int64_t(Ap[int64_t(x0) + i + 1]) - y0) : INT_MAX;
        }
        if (t + 1 < last) re_next = fetch_row_end(x1, x2);
        __syncthreads();

        // (3) this thread's piece of the merge path: items [d0, d1) of the tile
        const int items = tr + tn;
        const int d0 = min(tid * IPT, items);
        const int d1 = min(d0 + IPT, items);
        int lo = max(d0 - tn, 0), hi = min(d0, tr);
        while (lo < hi) {
            const int p = (lo + hi) >> 1;
            if (s_re[p] <= d0 - p - 1) lo = p + 1;
            else hi = p;
        }
        int cx = lo, cy = d0 - lo;

        // (4) walk: a nonzero extends the running row sum, a row end closes it
        val_t run = SR::identity(), first_val = SR::identity();
        int first_end = -1;
        int re = s_re[cx];
        const int cnt = d1 - d0;
        // Rows longer than a thread's IPT items (the banded target, FEM matrices, stencils) put at most ONE row
        // end among them: the items are then `before` nonzeros, the row end, and the rest nonzeros of the next
        // row — contiguous in s_nz.  When that holds for every thread of the wave, the item-by-item walk (IPT
        // dependent LDS reads and branches) is replaced by IPT independent reads and two masked sums, in the
        // same order, so the result is the same bit for bit.  Otherwise the wave walks.
        const int before = re - cy;                                   // nonzeros ahead of my first row end
        const bool has_end = before < cnt;
        const int re2 = (has_end && cx + 1 <= tr) ? s_re[cx + 1] : INT_MAX;
        const bool simple = !has_end || (re2 - re >= cnt - before - 1);
        if (__all(simple)) {
            const int n_nz = cnt - (has_end ? 1 : 0);                 // my nonzeros: s_nz[cy + shift .. + n_nz)
            val_t v[IPT];
#pragma unroll
            for (int k = 0; k < IPT; ++k) v[k] = s_nz[min(cy + shift + k, BLOCK * IPT - 1)];
            val_t head = SR::identity(), tail = SR::identity();
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                head = (k < before && k < n_nz) ? SR::reduce(head, v[k]) : head;
                tail = (k >= before && k < n_nz) ? SR::reduce(tail, v[k]) : tail;
            }
            if (has_end) {
                first_end = cx;                           // may continue a row opened by earlier threads
                first_val = head;
                run = tail;
            } else {
                run = head;
            }
        } else {
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                if (k < cnt) {
                    if (cy < re) {
                        run = SR::reduce(run, s_nz[cy + shift]);
                        ++cy;
                    } else {
                        if (first_end < 0) {
                            first_end = cx;                   // may continue a row opened by earlier threads
                            first_val = run;
                        } else {
                            put(int64_t(x0) + cx, run);       // opened and closed inside this thread
                        }
                        run = SR::identity();
                        ++cx;
                        re = s_re[cx];
                    }
                }
            }
        }

        // (5) carry-in = sum of the open-row tails of the preceding threads back to the
        //     last thread that closed a row (or the previous tile's carry): a
        //     flag-segmented inclusive scan
        val_t sv = run;
        int sf = first_end >= 0 ? 1 : 0;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const val_t ov = __shfl_up(sv, d, kWave);
            const int of = __shfl_up(sf, d, kWave);
            if (lane64 >= d) {
                if (!sf) sv = SR::reduce(ov, sv);
                sf |= of;
            }
        }
        if (lane64 == kWave - 1) {
            s_wave_sum[wave] = sv;
            s_wave_flag[wave] = sf;
        }
        __syncthreads();
        val_t prefix = block_carry;  // block-inclusive value at the end of the previous wave
        val_t total = block_carry;   // ... and at the end of the last wave: the row still open at the end of the tile
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) {
            const val_t ws = s_wave_sum[w];
            total = s_wave_flag[w] ? ws : SR::reduce(total, ws);
            if (w + 1 == wave) prefix = total;
        }
        const val_t incl = sf ? sv : SR::reduce(prefix, sv);
        val_t carry_in = __shfl_up(incl, 1, kWave);
        if (lane64 == 0) carry_in = prefix;
        if (first_end >= 0) put(int64_t(x0) + first_end, SR::reduce(carry_in, first_val));
        // No third barrier (round 1 passed the tile's carry through one more LDS word): every thread folds the
        // wave totals itself, and the next tile cannot disturb this one — it writes s_nz / s_re before ITS first
        // barrier and the wave totals after it, and no wave gets there before every wave has left the second
        // barrier of this tile with its reads of s_nz / s_re done (they precede that barrier).
        block_carry = total;
        x0 = x1; y0 = y1;
        x1 = x2; y1 = y2;
    }
    if (tid == 0) {
        // the row still open at the end of the run: x0 now holds tile_row[last] (== n_rows: none)
        carry_row[sup] = x0;
        carry_val[sup] = block_carry;
    }
}

// ---- K7r: a run of a REGULAR matrix, row-parallel ------------------------------------------------------
// The merge-path cut decides WHICH nonzeros and row ends a workgroup owns (the run: a fixed number of merge items,
// whatever the row lengths — the reference's decomposition, agent_spmv_orig.cuh:697-719); how the workgroup sums them
// is free.  On a matrix whose rows are alike and not short (plan: shape_merge, merge_rows) the item-by-item machinery
// of K7 — products through LDS, a search per thread, a segmented scan per tile — costs ~460 instructions per wave and
// tile and holds the kernel at 4.4 TB/s.  Here the run is handed to the row-chunk body of the CSR-vector kind
// (xwindow.hpp: T lanes per row, 16-byte loads straight into registers, window of x, results swept from LDS): the
// rows that END in the run are stored, the partial sum of the row still open at its end becomes the run's carry, and a
// row that began in an earlier run contributes the part that lies in this one (the fix-up adds the earlier carries,
// exactly as for K7).  The workgroup finds its two diagonals itself.  Runs with more rows than the LDS layout holds
// (stretches of empty rows) are walked in pieces.
constexpr int kMergeRowsCap = 1984;    // rows per piece: bounds + results fit 16 KB next to the window

// SEARCH: the workgroup finds its two diagonals itself (grids of a few rounds); else run_row / run_nnz hold the run
// boundaries, found by the search kernel on n_super + 1 diagonals (every workgroup of a big grid would otherwise pay
// the chain of dependent loads at its start).
// TS > 0: the band is wider than any window (plan: shape_merge, mr_sweep_lanes) — a piece is then ONE group of rows of the
// 1 024-thread workgroup, TS lanes per row and R rows per vector held in registers, and the window sweeps the band
// (xwindow.hpp, chunk_rows_sweep: the CSR-vector kind's body for such bands; plain gathers ran the run at 1.6 TB/s).
// NSEG > 1: the columns sit in several far-apart bands (the 3-D stencil) — each band gets its own segment of the window,
// staged per piece of the run (xwindow.hpp, stage_x_segments: the CSR-vector kind's multi-band plan).
struct NoSegments {};   // (the one-window variants take no segment list: 68 bytes of kernel arguments cost the sweep variants their last scalar registers)
template <int BLOCK, int R, bool WINDOW, bool SEARCH, typename off_t, typename val_t, int TS = 0, int NSEG = 1>
__global__ __launch_bounds__(BLOCK, (BLOCK >= kWideBlock ? 4 : 3)) void merge_rows_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz_begin, int64_t nnz, const off_t* __restrict__ Ap,
    const int32_t* __restrict__ Aj_arg, const val_t* __restrict__ Ax_arg, const val_t* __restrict__ x_arg,
    val_t* __restrict__ y_arg, int64_t tile_items, const int32_t* __restrict__ run_row, const int64_t* __restrict__ run_nnz,
    int32_t* __restrict__ carry_row, val_t* __restrict__ carry_val,
    int64_t n_tiles, int32_t tiles_per_super, int32_t window_cap, BandHint hint, val_t alpha, val_t beta, int32_t piece_rows,
    typename std::conditional<(NSEG > 1), SegmentPlan, NoSegments>::type segs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window | bounds | y | flags
    __shared__ int s_red[2];
    __shared__ int64_t s_diag[4];            // (row, nnz) of the run's first and last diagonal
    ChunkScratch<val_t> scr(s_dyn, window_cap, piece_rows);
    scr.alpha = alpha;
    scr.beta = beta;
    const unsigned sup = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int tid = threadIdx.x;
    const int64_t first = int64_t(sup) * tiles_per_super;
    const int64_t last = min(first + tiles_per_super, n_tiles);
    if constexpr (!SEARCH) {
        if (tid == 0) {
            s_diag[0] = run_row[sup];
            s_diag[1] = run_nnz[sup];
            s_diag[2] = run_row[sup + 1];
            s_diag[3] = run_nnz[sup + 1];
        }
        __syncthreads();
    } else {   // the two diagonals, 16 lanes each (lanes 0..31 of wave 0; the other lanes of that wave repeat the second)
        const int64_t items = int64_t(n_rows) + (nnz - nnz_begin);
        if (tid < kWave) {
            const int which = min(tid / 16, 1);
            int64_t diag = (which ? last : first) * tile_items;
            if (diag > items) diag = items;
            const int64_t lo = merge_search_group<16, off_t>(diag, n_rows, nnz_begin, nnz, Ap, tid & 15, tid & 48);
            if ((tid & 15) == 0 && tid < 32) {
                s_diag[2 * which] = lo;
                s_diag[2 * which + 1] = nnz_begin + diag - lo;
            }
        }
        __syncthreads();
    }
    // rows [row_lo, row_last) END in this run; row_last (if it exists) is open at its end.  The four coordinates stay in
    // LDS and are read again by every piece (scalar loads): held in scalar registers across the pieces they were what
    // pushed the eight-row sweeping variants past their register budget.  Row counts of a run fit 32 bits.
    int n_store_all, n_all;
    {
        const int64_t row_lo0 = uniform_i64(s_diag[0]), row_last0 = uniform_i64(s_diag[2]);
        n_store_all = int(row_last0 - row_lo0);
        n_all = n_store_all + (row_last0 < n_rows ? 1 : 0);
    }
    val_t carry = val_t(0);
    for (int pb = 0; pb < n_all; pb += piece_rows) {                 // (uniform; one piece unless the run holds more rows than the layout)
        const int pe = min(pb + piece_rows, n_all);
        const int rows = pe - pb;
        const int64_t row_lo = uniform_i64(s_diag[0]), y_first = uniform_i64(s_diag[1]), y_last = uniform_i64(s_diag[3]);
        const int64_t base = y_first & ~int64_t(3);
        const int64_t left = nnz - base;
        // (not xwindow.hpp's chunk_nnz_reach, which caps 32 768 higher: a run spans kMergeSuperItems nonzeros at most, far
        // below either cap, so both are right; this one stays as the kernels on record were compiled)
        const int32_t nnz_c = int32_t(left < kRel32Limit ? left : kRel32Limit);
        // opaque copies of the operand pointers, once per piece (see light_rows.hip: keeps per-thread addresses from
        // being hoisted out of this loop and spilled)
        int zero = 0;
        asm volatile("" : "+v"(zero));
        zero = __builtin_amdgcn_readfirstlane(zero);
        const int32_t* const Aj_c = Aj_arg + zero + base;
        const val_t* const Ax_c = Ax_arg + zero + base;
        const val_t* const x = x_arg + zero;
        val_t* const y = y_arg + zero;
        // bounds of the piece's rows, clipped to the run's nonzeros [y_first, y_last), relative to base
        int t2 = tid;
        asm volatile("" : "+v"(t2));
        for (int i = t2; i <= rows; i += BLOCK) {
            int64_t b = int64_t(Ap[min(row_lo + pb + i, int64_t(n_rows))]);
            b = b < y_first ? y_first : (b > y_last ? y_last : b);
            scr.s_b[i] = int32_t(b - base);
        }
        for (int i = t2; i < rows / 32 + 1; i += BLOCK) scr.long_map[i] = 0u;
        scr.store_rows = min(pe, n_store_all) - pb;                   // the open row's partial stays in s_y
        __syncthreads();
        const int64_t rb = row_lo + pb, re = row_lo + pe;
        if constexpr (TS > 0) {
            chunk_rows_sweep<BLOCK, TS, R, val_t>(rb, re, nnz_c, Aj_c, Ax_c, x, y, n_cols, window_cap, hint, scr);
            __syncthreads();
            if (pe == n_all && n_all > n_store_all) carry = uniform_val(scr.s_y[rows - 1]);
            __syncthreads();
            continue;
        }
        if constexpr (NSEG > 1) {
            auto stage = [&] { return stage_x_segments<val_t>(rb, re, n_cols, x, scr.s_x, window_cap, segs); };
            chunk_rows_any<BLOCK, 2, R, true, true, val_t, decltype(stage)&, true>(rb, re, nnz_c, Aj_c, Ax_c, x, y, stage, scr);
        } else {
            auto first_last = [&](int64_t r, int& fc, int& lc) {
                const int32_t s = scr.s_b[r - rb], e = scr.s_b[r - rb + 1];
                if (e <= s) return false;
                fc = Aj_c[s];
                lc = Aj_c[e - 1];
                return true;
            };
            auto stage = [&] { return stage_x_window<val_t>(rb, re, n_cols, first_last, x, scr.s_x, window_cap, s_red, hint); };
            chunk_rows_any<BLOCK, 2, R, WINDOW, true, val_t, decltype(stage)&, true>(rb, re, nnz_c, Aj_c, Ax_c, x, y, stage, scr);
        }
        __syncthreads();
        if (pe == n_all && n_all > n_store_all) carry = uniform_val(scr.s_y[rows - 1]);   // (one LDS word: scalar register)
        __syncthreads();                                                       // ... read before the next piece refills it
    }
    if (tid == 0) {
        carry_row[sup] = int32_t(s_diag[2]);      // the run's last row; == n_rows: no row is open (the fix-up skips it)
        carry_val[sup] = carry;
    }
}

}  // namespace mi355
