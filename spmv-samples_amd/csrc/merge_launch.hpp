// merge_launch.hpp — the launch path of the MERGE kind's tile and run kernels (merge_path.hip), under the plan that
// merge_plan.hip shaped.  A translation unit per value type (merge_path_*.hip) instantiates launch_merge for its types, so
// that each kernel is compiled where it is launched; the search and fix-up kernels are launched through merge_plan.hip.

#pragma once

#include "merge_path.hip"

namespace mi355 {

// what every launch of a plan's execute passes
template <typename off_t, typename val_t, typename mat_t>
struct MergeOperands {
    Plan& p;
    const off_t* Ap;
    const mat_t* Ax;
    const val_t* x;
    val_t* y;
    hipStream_t s;
    static constexpr int kOffType = sizeof(off_t) == 8 ? MI355_OFF_I64 : MI355_OFF_I32;   // (of Ap, for launch_merge_search)
};

// f(tag) with a run-time choice as a template argument: a flag, the sweeping body's lanes per row (with_semiring: merge_path.hip)
template <typename F>
static int with_bool(bool flag, F&& f) {
    return flag ? f(std::true_type()) : f(std::false_type());
}
template <typename F>
static int with_sweep_lanes(int lanes, F&& f) {
    switch (lanes) {
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
    }
    set_error("merge: bad sweep width %d", lanes);
    return MI355_SPMV_EINVAL;
}

// One launch of a run kernel, one workgroup per run.
template <int BLOCK, int R, bool WIN, bool SEARCH, int TS, int NSEG, typename off_t, typename val_t>
static int launch_merge_run(const MergeOperands<off_t, val_t, val_t>& o, size_t lds, const BandHint& hint) {
    const Plan& p = o.p;
    const auto kernel = merge_rows_kernel<BLOCK, R, WIN, SEARCH, off_t, val_t, TS, NSEG>;
    if (const int st = allow_dynamic_lds((const void*)kernel, lds + 1024)) return st;
    typename std::conditional<(NSEG > 1), SegmentPlan, NoSegments>::type segs{};
    if constexpr (NSEG > 1) {
        segs.n = p.n_seg;
        for (int i = 0; i < kMaxSegments; ++i) { segs.lo[i] = p.seg_lo[i]; segs.hi[i] = p.seg_hi[i]; }
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.n_super), dim3(BLOCK), lds, o.s, p.n_rows, p.n_cols, p.nnz_begin, p.nnz, o.Ap,
                       p.Aj, o.Ax, o.x, o.y, p.tile_items, p.tile_row, p.tile_nnz, p.carry_row,
                       static_cast<val_t*>(p.carry_val), p.n_tiles, (int32_t)p.tiles_per_super, (int32_t)p.window_elems, hint,
                       (val_t)p.alpha, (val_t)p.beta, (int32_t)p.mr_piece_rows, segs);
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

// One launch of a tile kernel, one workgroup per run, with a window of `cap` values of x.
template <int BLOCK, int IPT, bool VEC, bool WIN, int S, bool SEARCH, typename off_t, typename val_t, typename mat_t>
static int launch_merge_tile(const MergeOperands<off_t, val_t, mat_t>& o, int32_t cap, const BandHint& hint) {
    const Plan& p = o.p;
    const auto kernel = merge_tile_kernel<BLOCK, IPT, VEC, WIN, S, SEARCH, off_t, val_t, mat_t>;
    const size_t dyn = size_t(cap) * sizeof(val_t);
    if (dyn > 40 * 1024)   // (dynamic + the kernel's own LDS may pass 64 KB)
        if (const int st = allow_dynamic_lds((const void*)kernel, dyn + 24 * 1024)) return st;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.n_super), dim3(BLOCK), dyn, o.s, p.n_rows, p.n_cols, p.nnz_begin, p.nnz, o.Ap,
                       p.Aj, o.Ax, o.x, o.y, p.tile_row, p.tile_nnz, p.tile_items, p.carry_row,
                       static_cast<val_t*>(p.carry_val), p.n_tiles, (int32_t)p.tiles_per_super, cap, hint, (val_t)p.alpha,
                       (val_t)p.beta);
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

// regular matrix: row-parallel runs (plus-times, one value type, 16-byte path), then the fix-up
template <typename off_t, typename val_t>
static int launch_merge_runs(const MergeOperands<off_t, val_t, val_t>& o) {
    Plan& p = o.p;
    const int32_t capw = (int32_t)p.window_elems;
    const size_t lds = chunk_lds_bytes(capw, p.mr_piece_rows, sizeof(val_t));
    // run boundaries: searched in the kernel on small grids, by the search kernel (n_super + 1 diagonals of
    // tiles_per_super tiles each; the last one clamps to the end of the merge) on big ones
    const bool in_kernel = merge_search_in_kernel(p);
    if (!in_kernel) {
        if (const int st = launch_merge_search(o.kOffType, 4, p.n_super + 1, p.tile_items * p.tiles_per_super, p, o.Ap, o.s))
            return st;
        p.coords_valid = false;       // (the arrays now hold RUN boundaries, not tile coordinates)
    }
    const bool sweep = p.mr_sweep_lanes > 0 && capw > 0;   // the window sweeps the band: one group of rows per piece
    // rows a vector keeps in flight: 8 when sweeping in fp32; else the 512-thread kernel is held to 128 VGPRs, which the
    // fp32 body with 4 rows exceeds, and with several bands that body spills
    constexpr int RS = sizeof(val_t) == 4 ? 8 : kSweepRows, RR = sizeof(val_t) == 4 ? 4 : 2;
    if (sweep && (p.mr_piece_rows != (kHugeBlock / p.mr_sweep_lanes) * RS || capw < int32_t(kHugeBlock * 16 / sizeof(val_t)))) {
        set_error("merge: sweep plan with %d rows per piece at %d lanes per row", p.mr_piece_rows, p.mr_sweep_lanes);
        return MI355_SPMV_EINVAL;
    }
    const BandHint hint{p.band_lo, p.band_hi, sweep || p.window_from_band};
    const int st = with_bool(in_kernel, [&](auto search) {
        constexpr bool SEARCH = decltype(search)::value;
        if (sweep)
            return with_sweep_lanes(p.mr_sweep_lanes, [&](auto lanes) {
                return launch_merge_run<kHugeBlock, RS, true, SEARCH, decltype(lanes)::value, 1>(o, lds, hint);
            });
        // (the wide run kernels exist around ONE window of x)
        if (p.mr_block == kHugeBlock && capw > 0) return launch_merge_run<kHugeBlock, 2, true, SEARCH, 0, 1>(o, lds, hint);
        if (p.mr_block == kWideBlock && capw > 0) return launch_merge_run<kWideBlock, 2, true, SEARCH, 0, 1>(o, lds, hint);
        // several bands: a segment of the window each
        if (capw > 0 && p.n_seg >= 2) return launch_merge_run<kBlock, 2, true, SEARCH, 0, kMaxSegments>(o, lds, hint);
        if (capw > 0) return launch_merge_run<kBlock, RR, true, SEARCH, 0, 1>(o, lds, hint);
        return launch_merge_run<kBlock, RR, false, SEARCH, 0, 1>(o, lds, hint);
    });
    if (st != MI355_SPMV_OK) return st;
    return launch_merge_fixup<val_t>(MI355_SEMIRING_PLUS_TIMES, p, o.y, o.s);
}

template <typename off_t, typename val_t, typename mat_t>
int launch_merge(Plan& p, const off_t* Ap, const mat_t* Ax, const val_t* x, val_t* y, hipStream_t s) {
    if (p.n_rows == 0 || p.n_tiles == 0) return MI355_SPMV_OK;
    const MergeOperands<off_t, val_t, mat_t> o{p, Ap, Ax, x, y, s};
    // (a pattern matrix has no Ax: whatever the caller passed, NULL included, is neither read nor counted here)
    const uintptr_t ax_bits = std::is_same<mat_t, PatternOnes>::value ? uintptr_t(0) : reinterpret_cast<uintptr_t>(Ax);
    const bool aligned = ((reinterpret_cast<uintptr_t>(p.Aj) | ax_bits | reinterpret_cast<uintptr_t>(x)) & 15u) == 0;
    const bool reuse = (p.flags & MI355_PLAN_REUSE_STRUCTURE) && p.coords_valid;
    const bool vec = aligned && p.nnz >= 4;
    const bool wide = p.block_threads == kWideBlock && p.semiring == MI355_SEMIRING_PLUS_TIMES;
    // (no run kernels for integers, mixed value types or pattern matrices)
    if constexpr (std::is_same<val_t, mat_t>::value && std::is_floating_point<val_t>::value) {
        if (p.merge_rows && vec && p.semiring == MI355_SEMIRING_PLUS_TIMES) return launch_merge_runs(o);
    }
    // the tile kernel finds its run's coordinates itself (no search kernel in front) on the 16-byte path with 256 threads
    const bool fused = !reuse && vec && !wide && merge_search_in_kernel(p);
    if (!reuse && !fused) {
        const int64_t diagonals = p.n_tiles + 1;
        // measured (us, L = 1 / 4 / 16): 2 946 diagonals 7.3 / 6.0 / 4.4, 68 K 11.9 / 8.5 / 13.3, 139 K 14.0 / 16.0 / 30.9
        const int forced = p.knob.merge_search_lanes;
        const int lanes = forced > 0 ? forced : diagonals <= 16384 ? 16 : diagonals <= 98304 ? 4 : 1;
        if (const int st = launch_merge_search(o.kOffType, lanes, diagonals, p.tile_items, p, Ap, s)) return st;
    }
    if (!reuse) p.coords_valid = true;
    // a window sized for the row-parallel run kernel (512 / 1 024 threads, a swept band, a segment per band: up to
    // ~155 KB) is not one for the tile kernel, which needs its own ~24 KB next to it: those plans' other executes
    // (another semiring, an fp32 matrix under fp64 vectors) walk their tiles on plain gathers
    const bool rows_window = p.merge_rows && (p.mr_block != kBlock || p.mr_sweep_lanes > 0 || p.n_seg >= 2);
    const int32_t cap = (vec && !rows_window) ? (int32_t)p.window_elems : 0;
    const BandHint hint{p.band_lo, p.band_hi, p.window_from_band};
    return with_semiring(p.semiring, [&](auto semiring) {
        constexpr int S = decltype(semiring)::value;
        // 512 threads x 4 items under plus-times only; the searching kernel on the 16-byte path only
        auto tile = [&](auto vec_tag, auto win_tag) {
            constexpr bool VEC = decltype(vec_tag)::value, WIN = decltype(win_tag)::value;
            if constexpr (S == MI355_SEMIRING_PLUS_TIMES)
                if (wide) return launch_merge_tile<kWideBlock, 4, VEC, WIN, S, false>(o, cap, hint);
            if constexpr (VEC)
                if (fused) return launch_merge_tile<kBlock, 8, VEC, WIN, S, true>(o, cap, hint);
            return launch_merge_tile<kBlock, 8, VEC, WIN, S, false>(o, cap, hint);
        };
        const int st = !vec      ? tile(std::false_type(), std::false_type())
                       : cap > 0 ? tile(std::true_type(), std::true_type())
                                 : tile(std::true_type(), std::false_type());
        if (st != MI355_SPMV_OK) return st;
        return launch_merge_fixup<val_t>(S, p, y, s);
    });
}

}  // namespace mi355
