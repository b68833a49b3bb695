// merge_plan.hip — kind MERGE, everything that does not depend on the type of the matrix values: the shape of a plan
// (shape_merge), the predicates the shaper and the launcher share, and the search and fix-up kernels with their host
// launchers.  Compiled once; the tile and run kernels are instantiated per value type in merge_path_*.hip
// (merge_path.hip, merge_launch.hpp).

#include <algorithm>

#include "merge_path.hip"

namespace mi355 {

template <int kSearchLanes, typename off_t>
__global__ __launch_bounds__(kBlock) void merge_search_kernel(
    int32_t n_rows, int64_t nnz_begin, int64_t nnz, const off_t* __restrict__ Ap, int64_t tile_items, int64_t n_tiles,
    int32_t* __restrict__ tile_row, int64_t* __restrict__ tile_nnz) {
    // (nnz_begin = Ap[0], nnz = Ap[n_rows]: the counting sequence of the merge is nnz_begin .. nnz - 1; a
    // row-block view of a larger CSR starts at 1..3, everything else at 0)
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t t_raw = gid / kSearchLanes;
    const int64_t t = t_raw <= n_tiles ? t_raw : n_tiles;       // surplus groups repeat the last diagonal
    const int k = int(gid) & (kSearchLanes - 1);
    const int shift = (threadIdx.x & (kWave - 1)) & ~(kSearchLanes - 1);
    const int64_t items = int64_t(n_rows) + (nnz - nnz_begin);
    int64_t diag = t * tile_items;
    if (diag > items) diag = items;
    const int64_t lo = merge_search_group<kSearchLanes, off_t>(diag, n_rows, nnz_begin, nnz, Ap, k, shift);
    if (k == 0 && t_raw <= n_tiles) {
        tile_row[t] = int32_t(lo);
        tile_nnz[t] = nnz_begin + diag - lo;
    }
}

int launch_merge_search(int off_type, int lanes, int64_t diagonals, int64_t tile_items, const Plan& p, const void* Ap,
                        hipStream_t s) {
    const unsigned g = unsigned((diagonals * lanes + kBlock - 1) / kBlock);
    auto go = [&](auto* ap) {
        using off_t = typename std::remove_cv<typename std::remove_pointer<decltype(ap)>::type>::type;
        const auto kernel = lanes >= 16 ? merge_search_kernel<16, off_t> : lanes >= 4 ? merge_search_kernel<4, off_t> : merge_search_kernel<1, off_t>;
        hipLaunchKernelGGL(kernel, dim3(g), dim3(kBlock), 0, s, p.n_rows, p.nnz_begin, p.nnz, ap, tile_items, diagonals - 1,
                           p.tile_row, p.tile_nnz);
    };
    if (off_type == MI355_OFF_I32) go(static_cast<const int32_t*>(Ap));
    else go(static_cast<const int64_t*>(Ap));
    MI355_HIP_TRY(hipGetLastError());
    return MI355_SPMV_OK;
}

// ---- K8: add the carries of rows that straddle runs ------------------------------------
template <int S, typename val_t>
__global__ __launch_bounds__(kBlock) void merge_fixup_kernel(
    int64_t n_carries, int32_t n_rows, const int32_t* __restrict__ carry_row,
    const val_t* __restrict__ carry_val, val_t* __restrict__ y, val_t alpha) {
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_carries) return;
    // the neighbours and the value are fetched with carry_row[t]: two dependent round trips (then y[r]), not four
    const int32_t r = carry_row[t];
    const int32_t r_prev = t > 0 ? carry_row[t - 1] : -1;
    const int32_t r_next = t + 1 < n_carries ? carry_row[t + 1] : -1;
    val_t s = carry_val[t];
    if (r >= n_rows || r_prev == r) return;      // no carry, or not the first run carrying row r
    using SR = Semiring<S, val_t>;
    if (r_next == r)
        for (int64_t u = t + 1; u < n_carries && carry_row[u] == r; ++u) s = SR::reduce(s, carry_val[u]);
    if constexpr (S == MI355_SEMIRING_PLUS_TIMES) s = alpha * s;
    y[r] = SR::reduce(y[r], s);
}

template <typename val_t>
int launch_merge_fixup(int semiring, const Plan& p, val_t* y, hipStream_t s) {
    if (p.n_super <= 1) return MI355_SPMV_OK;
    return with_semiring(semiring, [&](auto sr) -> int {
        hipLaunchKernelGGL((merge_fixup_kernel<decltype(sr)::value, val_t>), dim3(unsigned((p.n_super + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, s, p.n_super, p.n_rows, p.carry_row, static_cast<const val_t*>(p.carry_val), y,
                           (val_t)p.alpha);
        MI355_HIP_TRY(hipGetLastError());
        return MI355_SPMV_OK;
    });
}
template int launch_merge_fixup<float>(int, const Plan&, float*, hipStream_t);
template int launch_merge_fixup<double>(int, const Plan&, double*, hipStream_t);
template int launch_merge_fixup<int32_t>(int, const Plan&, int32_t*, hipStream_t);

// ---- host side -----------------------------------------------------------------------
// Whether the tile kernel searches its own coordinates (MI355_MERGE_FUSED = 0 | 1 overrides): always, when a run
// is short enough for the workgroup to search all its diagonals in two passes.
bool merge_search_in_kernel(const Plan& p) {
    if (p.knob.merge_fused == 0) return false;
    if (p.tiles_per_super + 1 > 32) return false;         // (one pass of 256 threads searches 32 diagonals)
    if (p.knob.merge_fused > 0) return true;
    // Measured (us, fused / search kernel in front): web-Google stand-in (1 473 runs) 46.6 / 49.5, cant stand-in 19.3 /
    // 20.3 — but S32-band (4 233 runs of 16 tiles) 282 / 258 and R-MAT-24 (8 700 runs) 2 516 / 2 483: on a grid of
    // many rounds every workgroup pays the search's chain of dependent loads at its start, and the search kernel's
    // ~9 us are a few per cent.  Fused where the grid is at most ~two rounds of the chip.
    return p.n_super <= int64_t(kCus) * 8;
}

// Row-parallel runs (merge_rows_kernel) for a matrix whose rows all but fill ONE step of a vector of 2, 4, 8, 16 or 32
// lanes (the widths the run body picks from: 8, 16, 32, 64, 128 nonzeros per step) — the probe's 256 sampled rows all
// hold between three quarters of such a step and the whole of it — and big enough for runs of 16 K+ items (on a small
// matrix a run is a tile or two: the window and the two diagonals cost more than they are worth — cant stand-in 40.6 us
// against 19.5 with the item walk).  Measured on 2^27 nonzeros (us, runs / item walk; scripts/gpu_r02_merge_regular.py,
// profiles/r02_row_length_scan.txt): fixed 8 per row 347 / 410, 16: 285 / 315, 27: 251 / 275, 32: 218 / 257, 48: 239 / 256,
// 64: 205 / 245, 100: 229 / 242, 128: 195 / 237 — but 40: 262 / 256 (a step of 64 is 62 % full), and rows of VARYING length
// lose at every mean (24 +- 6: 415 / 341, 64 +- 16: 479 / 381, 128 +- 32: 502 / 380): those keep the item walk, at
// 4.8-5.5 TB/s.  MI355_MERGE_ROWS = 0 | 1 overrides.
bool merge_rows_wanted(const Plan& p) {
    if (p.knob.merge_rows >= 0) return p.knob.merge_rows != 0;
    if (p.tiles_per_super * p.tile_items < 16000) return false;      // (8 tiles of 2 044 items and up)
    return merge_rows_regular(p);
}
bool merge_rows_regular(const Plan& p) {
    if (!p.probe_ok || p.n_rows <= 0 || p.val_type == MI355_VAL_I32) return false;
    // (... or all but an eighth of them do: the boundary rows of a stencil — the nlpkkt stand-in's 27-point rows are
    // 18, 12 or 8 long on the faces, edges and corners of its box — cost their vectors a few idle lanes, nothing more)
    for (const int64_t step : {8, 16, 32, 64, 128})
        if (p.probe_len_max <= step && (p.probe_len_min * 4 >= step * 3 || p.probe_short_rows * 8 <= kBlock)) return true;
    return false;
}

// ---- the shape of a plan ----------------------------------------------------------------------------------------
static void set_runs(Plan& p, int64_t tps) {
    p.tiles_per_super = tps;
    p.n_super = (p.n_tiles + tps - 1) / tps;
    p.grid_blocks = p.n_super;
}

// Tiles of a run that is one piece of `rows` rows of the matrix's mean length (mean1 = that length + 1: a row is its
// nonzeros and its end), at most kMergeSuperItems items.  0 when the piece does not fill a tile.
static int64_t tiles_for_rows(const Plan& p, int64_t rows, int64_t mean1) {
    return std::min(rows * mean1 / p.tile_items, kMergeSuperItems / p.tile_items);
}

// the search kernel in front unless the main kernel searches its own coordinates, the main kernel, and the fix-up
// behind it when there is more than one run (a row-parallel plan is a 256-thread plan)
static int merge_kernel_count(const Plan& p) {
    return (p.n_super > 1 ? 2 : 1) + ((merge_search_in_kernel(p) && p.block_threads == kBlock) ? 0 : 1);
}

// a window of x only pays when a run is long enough to amortise staging it, and
// when the band the probe saw (plus the rows of a run) fits
static int run_window_elems(Plan& p, ProbeSamples& probe, int64_t tps, int64_t mean1) {
    return (tps * p.tile_items >= 8192) ? pick_window_elems(p, probe, tps * p.tile_items / mean1 + 1) : 0;
}

// Several far-apart bands (the 3-D stencil).  A REGULAR matrix of that kind takes row-parallel runs with a segment
// of the window per band, staged per piece of a run — the CSR-vector kind's multi-band plan: the piece is as many
// rows as the bands leave room for, a run is one piece.  (Round 2 had this at 681 us against the item walk's 727
// on the C4 stand-in, with spilling kernels, and dropped it; the chunk body of round 3 fits its registers.)
// MI355_MERGE_SEGMENTS=0 keeps the item walk on plain gathers, as every other several-band matrix does.
// Returns the rows per piece; 0, with p untouched, when the plan is not taken.
static int try_segmented_runs(Plan& p, int64_t mean1) {
    if (!(p.n_seg >= 2 && p.block_threads == kBlock && p.knob.merge_segments != 0 && p.knob.merge_tps <= 0 &&
          p.knob.window < 0 && merge_rows_wanted(p)))
        return 0;
    int64_t piece = segment_rows_fit(p);
    if (piece > kMergeRowsCap) piece = kMergeRowsCap;
    piece &= ~int64_t(3);
    const int64_t tps = tiles_for_rows(p, piece, mean1);
    if (!(piece >= 256 && tps >= 1 && (p.n_tiles + tps - 1) / tps >= int64_t(kCus) * 2)) return 0;
    int64_t need = 0;                         // (LDS is occupancy: what the bands need with that many rows)
    for (int i = 0; i < p.n_seg; ++i) need += p.seg_hi[i] - p.seg_lo[i] + 1 + 4 + piece;
    need = (need + 3) & ~int64_t(3);
    if (need < p.window_elems) p.window_elems = int(need);
    set_runs(p, tps);
    return int(piece);
}

// The band does not fit the window of a 256-thread workgroup (fp64 on the S32-band shape: 8 193 columns + the rows of a run):
// two workgroups of 512 threads per CU may take ~78 KB each, as the CSR-vector kind's wide plan does; the run is then
// as long as the rows the band leaves room for, and walked in one piece.
// ... and a band too wide for that gets ONE workgroup of 1 024 threads per CU with ~155 KB (the CSR-vector kind's
// third plan): fp32, 32 769 columns, 32 per row: 343 -> see profiles/r02_shape_sweep.txt
// One such try: true when the plan is taken; else p is as it was.
static bool try_wide_window(Plan& p, ProbeSamples& probe, int block, int64_t lds, int64_t min_piece, int64_t mean1) {
    const int64_t vb = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const int64_t band = p.band_hi - p.band_lo + 1;
    int64_t piece = (lds - vb * (band + 8) - 4) * 8 / (8 * (2 * vb + 4) + 1);   // val (band + rows + 8) + 4 (rows + 1) + val rows + rows / 8
    piece &= ~int64_t(3);
    if (piece > kMergeRowsCap) piece = kMergeRowsCap;
    if (!(band > 0 && piece >= min_piece)) return false;
    const int64_t tps = std::max<int64_t>(tiles_for_rows(p, piece, mean1), 1);
    // what pick_window_elems writes, to put back if the try fails (a budget that holds the band and the piece never
    // reaches the several-band search, so the segment list stays as it is)
    const int bytes = p.window_bytes, elems = p.window_elems, n_seg = p.n_seg;
    const bool from_band = p.window_from_band;
    p.window_bytes = int(vb * (band + piece + 8));
    p.window_elems = pick_window_elems(p, probe, piece);
    if (!(p.window_elems > 0 && p.n_seg < 2 && p.window_from_band && (p.n_tiles + tps - 1) / tps >= int64_t(kCus) * 2)) {
        p.window_bytes = bytes; p.window_elems = elems; p.n_seg = n_seg; p.window_from_band = from_band;
        return false;
    }
    set_runs(p, tps);
    p.mr_block = block;
    p.mr_piece_rows = int(piece);
    return true;
}

// Still no window: the band is wider than one CU's LDS.  The CSR-vector kind sweeps such a band with the window
// (rows_plan.hip, shape_sweep); a run here does the same — a piece = one group of rows of a 1 024-thread workgroup held in
// registers, 4 T nonzeros per row in one step — under the same rule: the staged bytes of a piece stay below half the
// line fills its nonzeros would cost as plain gathers.  Rows of up to 8 nonzeros (T = 2) keep the gathers.
static void try_sweep(Plan& p, int64_t mean1) {
    if (!(p.merge_rows && p.window_elems == 0 && p.probe_ok && p.knob.sweep != 0 && p.knob.window < 0 && p.knob.merge_tps <= 0 &&
          p.knob.merge_wide_window != 0 && p.probe_len_max > 8 && p.probe_len_max <= 128))
        return;
    const int64_t vb = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const int64_t band = p.band_hi - p.band_lo + 1;
    int t = 4;
    while (t < 32 && 4 * t < p.probe_len_max) t *= 2;
    const int64_t piece = int64_t(kHugeBlock / t) * sweep_rows_for(p.val_type, t);
    const int64_t fixed = int64_t(chunk_lds_bytes(0, int(piece), size_t(vb)));
    const int64_t cap = sweep_window_cap(vb, fixed);
    const int64_t span = band + piece + 8;
    const int64_t passes = cap > 0 ? (span + cap - 1) / cap : 0;
    const int64_t tps = std::max<int64_t>(tiles_for_rows(p, piece, mean1), 1);
    const bool pays = span * vb <= 64 * (mean1 - 1) * piece;
    if (!(band > 0 && passes >= 1 && passes <= 16 && (p.n_tiles + tps - 1) / tps >= int64_t(kCus) * 2 && (pays || p.knob.sweep == 1)))
        return;
    set_runs(p, tps);
    p.mr_block = kHugeBlock;
    p.mr_piece_rows = int(piece);
    p.mr_sweep_lanes = t;
    p.window_bytes = int(cap * vb);
    p.window_elems = int(cap);
    p.window_from_band = true;
    p.n_seg = 0;
}

void shape_merge(Plan& p, ProbeSamples& probe) {
    // tuning knobs: MI355_MERGE_TPS = tiles per run (and MI355_SPMV_WINDOW = 0|1, analyze.hip)
    // 256 threads x 8 items or (MI355_MERGE_BLOCK=512) 512 threads x 4 items: the same 2 044-item tiles
    p.block_threads = p.knob.merge_block == kWideBlock ? kWideBlock : kBlock;
    const int ipt = p.block_threads == kWideBlock ? 4 : 8;   // (16: S32-band 251 vs 259 us, web-Google stand-in 52.4 vs 46.4: not kept)
    p.lanes_per_row = 0;
    p.elems_per_lane = ipt;            // reported as items per thread for this kind
    p.tile_items = int64_t(p.block_threads) * ipt - 4;
    const int64_t items = int64_t(p.n_rows) + (p.nnz - p.nnz_begin);
    p.n_tiles = (items + p.tile_items - 1) / p.tile_items;
    const int64_t mean1 = 1 + (p.n_rows > 0 ? (p.nnz - p.nnz_begin) / p.n_rows : 0);
    // runs of up to ~32 K items, but at least ~4 runs per CU when the matrix allows
    int64_t tps_small = p.n_tiles / (int64_t(kCus) * 4);
    const int64_t cap = kMergeSuperItems / p.tile_items;
    if (tps_small > cap) tps_small = cap;
    if (p.knob.merge_tps > 0) tps_small = p.knob.merge_tps;
    if (tps_small < 1) tps_small = 1;
    // A REGULAR mid-size matrix (one to four runs of 8 tiles per CU) takes runs of 8 tiles rather than the two to seven
    // the rule above gives it: 16 K items are what the row-parallel runs and their window of x need to pay
    // (S32-band shape, us, before / after: 2^17 rows 20.5 / 19.4, 2^18 37.0 / 25.1, 2^19 47.7 / 41.3 — that one by the
    // threshold in merge_rows_wanted alone).  Taken back below if no window placed from the band serves such a run.
    const bool bumped = p.knob.merge_tps <= 0 && p.knob.merge_rows < 0 && tps_small < 8 && p.n_tiles >= 8 * int64_t(kCus) &&
                        p.block_threads == kBlock && merge_rows_regular(p);
    const int64_t tps = bumped ? 8 : tps_small;
    set_runs(p, tps);
    p.window_elems = run_window_elems(p, probe, tps, mean1);
    // fp64 halves what the 36 KB budget (three workgroups per CU) holds: the S32-band shape in fp64 ran on plain
    // gathers at 2.4 TB/s.  Second try with 56 KB (two workgroups per CU next to the kernel's 16-24 KB of own LDS).
    if (p.window_elems == 0 && p.n_seg < 2 && p.val_type == MI355_VAL_F64 && p.knob.window < 0 && tps * p.tile_items >= 8192 &&
        p.knob.merge_wide_window != 0) {
        p.window_bytes = 56 * 1024;
        p.window_elems = pick_window_elems(p, probe, tps * p.tile_items / mean1 + 1);
        if (p.window_elems == 0 || p.n_seg >= 2) p.window_bytes = 0;
    }
    int segment_piece = try_segmented_runs(p, mean1);   // rows per piece of a run with one window segment per band (0: not that plan)
    if (bumped && !(p.window_elems > 0 && p.n_seg < 2 && p.window_from_band)) {   // no window for runs of 8 tiles: the shorter runs
        set_runs(p, tps_small);
        p.window_bytes = 0;
        p.window_elems = run_window_elems(p, probe, tps_small, mean1);
        segment_piece = 0;
    }
    const bool several_bands = p.n_seg >= 2 && segment_piece == 0;
    if (several_bands) { p.window_elems = 0; p.n_seg = 0; }   // several bands: the item walk keeps to global gathers
    p.n_kernels = merge_kernel_count(p);
    // (a matrix whose columns sit in several far-apart bands — the 3-D stencil — keeps the item walk: row-parallel runs
    // on plain gathers measured 720 us against 650-700 on the C4 stand-in, and with the bands staged per piece of a run
    // 681 against 727 on one box, with four spilling kernels: not kept)
    p.merge_rows = p.block_threads == kBlock && !several_bands && merge_rows_wanted(p);
    p.mr_block = kBlock;
    p.mr_piece_rows = segment_piece > 0 ? segment_piece : kMergeRowsCap;
    if (segment_piece > 0 && !p.merge_rows) { p.window_elems = 0; p.n_seg = 0; }   // (cannot happen: merge_rows_wanted held above)
    if (p.merge_rows && segment_piece == 0 && p.knob.merge_wide_window != 0 && p.knob.window < 0 && p.knob.merge_tps <= 0 && p.probe_ok &&
        !(p.window_elems > 0 && p.window_from_band)) {
        if (!try_wide_window(p, probe, kWideBlock, 78 * 1024, 256, mean1)) try_wide_window(p, probe, kHugeBlock, 155 * 1024, 512, mean1);
    }
    p.mr_sweep_lanes = 0;
    try_sweep(p, mean1);
    if (p.merge_rows) {
        p.n_kernels = merge_kernel_count(p);
        snprintf(p.main_kernel, sizeof(p.main_kernel), "merge_rows_kernel");
        return;
    }
    p.coords_valid = false;
    snprintf(p.main_kernel, sizeof(p.main_kernel), "merge_tile_kernel");
}

// What a plan reports when every one of its executes walks the tiles whatever shape_merge shaped it around (a pattern
// matrix: merge_rows_kernel has no pattern form).  The shape itself — tiles, runs, window — stays as it is.
void merge_report_tile_walk(Plan& p) {
    p.n_kernels = merge_kernel_count(p);
    snprintf(p.main_kernel, sizeof(p.main_kernel), "merge_tile_kernel");
}

// The tile coordinates on demand (mi355_spmv_plan_merge_coords on a plan whose executes do not produce them: the
// row-parallel run kernel only ever finds its own two diagonals).
int merge_compute_coords(Plan& p) {
    if (p.n_rows == 0 || p.n_tiles == 0) return MI355_SPMV_OK;
    if (const int st = launch_merge_search(p.off_type, 4, p.n_tiles + 1, p.tile_items, p, p.Ap, nullptr)) return st;
    MI355_HIP_TRY(hipStreamSynchronize(nullptr));
    return MI355_SPMV_OK;
}

}  // namespace mi355
