// row_launch.hpp — the launch path of the chunked row kinds, VECTOR (csr_vector.hip) and LIGHT (light_rows.hip).
// Both run the same chunk bodies (xwindow.hpp) under the same plan (rows_plan.hip: shape_rows, set_rows_launch); they
// differ only in how a workgroup gets its chunk — by block index, or from LIGHT's sharded counters — and so in their
// kernels.  A kind names those in a traits type (VectorRows, LightRows) and instantiates launch_rows with it in its own
// translation units, so that each kernel is compiled where it is defined.

#pragma once

#include <type_traits>

#include "common.hpp"
#include "giant_rows.hpp"
#include "xwindow.hpp"

namespace mi355 {

// f(std::integral_constant<int, T>()) for the plan's lanes per row T, which the kernels take as a template argument
template <typename F>
static int with_lanes(const Plan& p, const char* kind, F&& f) {
    switch (p.lanes_per_row) {
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        case 64: return f(std::integral_constant<int, 64>());
    }
    set_error("%s: bad lanes_per_row %d", kind, p.lanes_per_row);
    return MI355_SPMV_EINVAL;
}

// A plain kernel (row_dot.hpp, plain_rows) over the plan's rows, its grid from the row count; kernel_of(lanes) names the
// kernel for the plan's lanes per row.
template <typename off_t, typename val_t, typename mat_t, typename KernelOf>
static int launch_plain_rows(const Plan& p, const char* kind, const off_t* Ap, const mat_t* Ax, const val_t* x, val_t* y,
                             hipStream_t s, KernelOf kernel_of) {
    return with_lanes(p, kind, [&](auto lanes) -> int {
        constexpr int rows_per_block = kBlock / decltype(lanes)::value;
        const dim3 grid((unsigned)((int64_t(p.n_rows) + rows_per_block - 1) / rows_per_block)), block(kBlock);
        hipLaunchKernelGGL(kernel_of(lanes), grid, block, 0, s, p.n_rows, (off_t)p.nnz, Ap, p.Aj, Ax, x, y, (val_t)p.alpha,
                           (val_t)p.beta);
        MI355_HIP_TRY(hipGetLastError());
        return MI355_SPMV_OK;
    });
}

// what every launch of a chunked kernel of a plan passes
template <typename val_t, typename mat_t = val_t>   // (mat_t: the type Ax is stored in, xwindow.hpp chunk_rows)
struct RowOperands {
    const Plan& p;
    ApView Ap;
    const mat_t* Ax;
    const val_t* x;
    val_t* y;
    hipStream_t s;
    size_t lds;   // dynamic LDS: window | bounds | y | flags
};

// One launch of a chunked kernel on the plan's grid (LIGHT's kernels take the counters after y).  A launch that asks for
// more than the default 64 KB of LDS raises the kernel's limit first.
template <typename Kind, typename val_t, typename K, typename mat_t, typename... Tail>
static int launch_chunked(K kernel, int threads, const RowOperands<val_t, mat_t>& o, const ChunkMap& cmap, const BandHint& hint,
                          Tail... tail) {
    const Plan& p = o.p;
    if (const int st = allow_dynamic_lds((const void*)kernel, o.lds)) return st;
    const dim3 grid((unsigned)p.grid_blocks), block(threads);
    if constexpr (Kind::kCounters)
        hipLaunchKernelGGL(kernel, grid, block, o.lds, o.s, p.n_rows, p.n_cols, p.nnz_read, o.Ap, p.Aj, o.Ax, o.x, o.y,
                           p.counters, cmap, (int32_t)p.window_elems, hint, tail..., (val_t)p.alpha, (val_t)p.beta);
    else
        hipLaunchKernelGGL(kernel, grid, block, o.lds, o.s, p.n_rows, p.n_cols, p.nnz_read, o.Ap, p.Aj, o.Ax, o.x, o.y,
                           cmap, (int32_t)p.window_elems, hint, tail..., (val_t)p.alpha, (val_t)p.beta);
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

template <typename Kind, int BLOCK, typename off_t, typename val_t>
static int launch_rows_window(const RowOperands<val_t>& o, const off_t* Ap) {
    const Plan& p = o.p;
    if constexpr (BLOCK >= kWideBlock) {
        // a 512- / 1 024-thread plan is only ever shaped around ONE window of x; without it (a forced knob) the
        // 256-thread kernel walks the same chunks (any workgroup size walks any chunk)
        if (p.window_elems <= 0 || p.n_seg >= 2) return launch_rows_window<Kind, kBlock>(o, Ap);
    }
    const BandHint hint{p.band_lo, p.band_hi, p.window_from_band};
    const ChunkMap cmap = chunk_map_of(p);
    SegmentPlan segs;
    segs.n = p.n_seg;
    for (int i = 0; i < kMaxSegments; ++i) { segs.lo[i] = p.seg_lo[i]; segs.hi[i] = p.seg_hi[i]; }
    auto go = [&](auto kernel) {
        if constexpr (Kind::kPackedIndex)
            return launch_chunked<Kind, val_t>(kernel, BLOCK, o, cmap, hint, segs, (const uint16_t*)p.packed_index);
        else
            return launch_chunked<Kind, val_t>(kernel, BLOCK, o, cmap, hint, segs);
    };
    if constexpr (BLOCK == kBlock) if (p.balanced) {   // vector width per chunk (chunk_rows_any); the T of the template is not used
        // (the weight-cut layout holds up to 2 K rows of bounds and results next to the window: may pass 64 KB)
        constexpr int R = rows_in_flight(sizeof(val_t), 2);
        const int st = p.window_elems > 0 ? go(Kind::template window<kBlock, 2, R, 1, true, val_t>())
                                          : go(Kind::template window<kBlock, 2, R, 0, true, val_t>());
        if (st != MI355_SPMV_OK) return st;
        return launch_giant_rows<off_t, val_t>(p, Ap, o.Ax, o.x, o.y, o.s);   // (rows too long for one workgroup, if any)
    }
    return with_lanes(p, Kind::name, [&](auto lanes) -> int {
        constexpr int T = decltype(lanes)::value, R = rows_in_flight(sizeof(val_t), T);
        if (p.window_elems > 0 && p.n_seg >= 2) {
            // (several bands: shape_chunks keeps those plans on 256 threads)
            if constexpr (BLOCK == kBlock) return go(Kind::template window<BLOCK, T, R, kMaxSegments, false, val_t>());
            set_error("%s: no 512-thread kernel for a multi-band window", Kind::name);
            return MI355_SPMV_EINVAL;
        }
        if constexpr (Kind::kPackedIndex) {
            // the plan holds 16-bit window indices (build_packed_index made sure of the shape: one window placed from
            // the band, equal-row chunks; the operands' alignment was checked by launch_rows): the twin that streams them
            if (p.packed_index && p.window_elems > 0 && p.window_from_band)
                return go(Kind::template window<BLOCK, T, R, 1, false, val_t, true>());
        }
        if (p.window_elems > 0) return go(Kind::template window<BLOCK, T, R, 1, false, val_t>());
        if constexpr (BLOCK == kBlock) return go(Kind::template window<BLOCK, T, R, 0, false, val_t>());
        return MI355_SPMV_OK;
    });
}

template <typename Kind, typename val_t>
static int launch_rows_sweep(const RowOperands<val_t>& o) {
    const Plan& p = o.p;
    const BandHint hint{p.band_lo, p.band_hi, true};
    const ChunkMap cmap{nullptr, (int32_t)p.rows_per_chunk, (int32_t)p.rows_cap, p.n_chunks, 0, int64_t(0),
                        p.knob.rel32_limit > 0 ? p.knob.rel32_limit : kRel32Limit, p.light_dequeue_once ? 1 : 0};
    // rows a vector holds: 4, or 8 (fp32; sweep_rows_for) — the plan's rows per chunk say which
    const int64_t vectors = kHugeBlock / p.lanes_per_row;
    const int held = int(p.rows_per_chunk / vectors);
    constexpr bool kHasEight = sizeof(val_t) == 4;
    if (p.rows_per_chunk != vectors * held || !(held == kSweepRows || (kHasEight && held == 8 && p.lanes_per_row >= 4)) ||
        p.rows_cap < p.rows_per_chunk || p.window_elems < int(kHugeBlock * 16 / sizeof(val_t))) {
        set_error("%s: sweep plan with %lld rows per chunk at %d lanes per row", Kind::name, (long long)p.rows_per_chunk,
                  p.lanes_per_row);
        return MI355_SPMV_EINVAL;
    }
    return with_lanes(p, Kind::name, [&](auto lanes) -> int {
        constexpr int T = decltype(lanes)::value;
        auto go = [&](auto kernel) { return launch_chunked<Kind, val_t>(kernel, kHugeBlock, o, cmap, hint); };
        if constexpr (kHasEight && T >= 4) if (held == 8) return go(Kind::template sweep<T, 8, val_t>());
        return go(Kind::template sweep<T, kSweepRows, val_t>());
    });
}

template <typename Kind, typename off_t, typename val_t>
int launch_rows(const Plan& p, const off_t* Ap, const val_t* Ax, const val_t* x, val_t* y, hipStream_t s) {
    if (p.n_rows == 0) return MI355_SPMV_OK;
    // a small matrix: the plain one-pass kernel of the CSR-vector kind, whichever the plan's kind (rows_plan.hip,
    // shape_rows; handing rows out cost LIGHT 29-133 us where this takes 3-6).  A block inherits the choice with its
    // lanes per row: the same sums bit for bit.
    if (p.small_plain) return launch_vector_plain<off_t, val_t>(p, Ap, Ax, x, y, s);
    // 16-byte loads need 16-byte-aligned Aj / Ax / x (hipMalloc gives 256); a caller that passes an offset view gets the
    // kind's 4-byte-per-lane kernel instead, as does a whole VECTOR plan under MI355_SPMV_PLAIN (tuning / tests — a
    // block keeps the whole plan's order)
    const bool aligned = ((reinterpret_cast<uintptr_t>(p.Aj) | reinterpret_cast<uintptr_t>(Ax) |
                           reinterpret_cast<uintptr_t>(x)) & 15u) == 0;
    if (!aligned || p.nnz < 4 || (Kind::kPlainKnob && p.knob.plain != 0 && !p.is_block))
        return Kind::plain(p, Ap, Ax, x, y, s);
    const RowOperands<val_t> o{p, ApView{Ap, sizeof(off_t) == 8 ? 1 : 0}, Ax, x, y, s,
                               chunk_lds_bytes(p.window_elems, p.rows_cap, sizeof(val_t))};
    if (p.sweep) return launch_rows_sweep<Kind>(o);
    return p.block_threads == kHugeBlock   ? launch_rows_window<Kind, kHugeBlock>(o, Ap)
           : p.block_threads == kWideBlock ? launch_rows_window<Kind, kWideBlock>(o, Ap)
                                           : launch_rows_window<Kind, kBlock>(o, Ap);
}

}  // namespace mi355
