// analyze.hip — what both planners (rows_plan.hip, merge_plan.hip) use at plan creation: the knobs, the structure
// probe, the per-device analysis buffer, allow_dynamic_lds, the window pick with its band clustering, and the
// partition into row blocks.
//
// The probe decides ONE launch-shape question: is an LDS window of x worth its LDS?  A window
// costs 36 KB per workgroup (occupancy) and pays only if it can hold most of the
// columns a chunk of rows touches.  256 rows spread over the matrix are sampled
// (first and last column of each); the band [min(col - row), max(col - row)] over
// the samples, plus the rows a workgroup owns, is the span a window would have to
// cover.  The result never affects correctness: the kernels range-check every
// column against the window they actually staged (xwindow.hpp).
// The reference has no counterpart (no plan, no LDS staging of x).

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <new>
#include <unordered_map>

#include "common.hpp"
#include "xwindow.hpp"

namespace mi355 {

// ---- knobs --------------------------------------------------------------------------------------
static std::mutex g_knobs_mutex;
static Knobs g_knobs;
static bool g_knobs_ready = false;

static void parse_knobs(Knobs& k) {
    k = Knobs();
    size_t used = 0;
    auto note = [&](const char* name, const char* v) {
        const int w = snprintf(k.text + used, sizeof(k.text) - used, "%s%s=%s", used ? " " : "", name, v);
        if (w > 0) used = std::min(sizeof(k.text) - 1, used + size_t(w));
    };
    auto geti = [&](const char* name, int& dst) {
        if (const char* v = getenv(name)) { dst = atoi(v); note(name, v); }
    };
    auto getl = [&](const char* name, int64_t& dst) {
        if (const char* v = getenv(name)) { dst = atoll(v); note(name, v); }
    };
    geti("MI355_SPMV_LANES", k.lanes);
    geti("MI355_SPMV_BLOCK", k.block);
    getl("MI355_SPMV_ROWS_PER_CHUNK", k.rows_per_chunk);
    geti("MI355_SPMV_WINDOW", k.window);
    geti("MI355_SPMV_WINDOW_FROM_BAND", k.window_from_band);
    geti("MI355_SPMV_SEGMENTS", k.segments);
    geti("MI355_SPMV_SWEEP", k.sweep);
    geti("MI355_SPMV_BALANCE", k.balance);
    geti("MI355_SPMV_LONG_STEPS", k.long_steps);
    geti("MI355_SPMV_GIANT", k.giant);
    getl("MI355_SPMV_GIANT_ROW", k.giant_row);
    geti("MI355_SPMV_PLAIN", k.plain);
    geti("MI355_SPMV_SMALL", k.small);
    geti("MI355_SPMV_PACK", k.pack);
    getl("MI355_SPMV_REL32_LIMIT", k.rel32_limit);
    geti("MI355_LIGHT_BLOCKS_PER_CU", k.light_blocks_per_cu);
    geti("MI355_LIGHT_CHUNK_DIV", k.light_chunk_div);
    geti("MI355_MERGE_BLOCK", k.merge_block);
    geti("MI355_MERGE_TPS", k.merge_tps);
    geti("MI355_MERGE_SEARCH_LANES", k.merge_search_lanes);
    geti("MI355_MERGE_FUSED", k.merge_fused);
    geti("MI355_MERGE_WIDE_WINDOW", k.merge_wide_window);
    geti("MI355_MERGE_SEGMENTS", k.merge_segments);
    geti("MI355_SPMV_PLAN_CACHE", k.plan_cache);
    geti("MI355_MERGE_ROWS", k.merge_rows);
    geti("MI355_DIST_TRIALS", k.dist_trials);
    geti("MI355_DIST_SHARED_DEVICE", k.dist_shared_device);
    if (const char* v = getenv("MI355_DIST_EXCHANGE")) {
        k.dist_exchange = !strcmp(v, "bcast") ? MI355_DIST_EXCHANGE_BCAST : !strcmp(v, "sendrecv") ? MI355_DIST_EXCHANGE_SENDRECV
                          : !strcmp(v, "allgather") ? MI355_DIST_EXCHANGE_ALLGATHER : MI355_DIST_EXCHANGE_AUTO;
        note("MI355_DIST_EXCHANGE", v);
    }
    if (const char* v = getenv("MI355_SPMV_RCCL_LIB")) {
        snprintf(k.rccl_lib, sizeof(k.rccl_lib), "%s", v);
        note("MI355_SPMV_RCCL_LIB", strrchr(v, '/') ? strrchr(v, '/') + 1 : v);
    }
    if (k.window > 1) k.window = 1;
    if (k.balance > 1) k.balance = 1;
}

const Knobs& knobs() {
    std::lock_guard<std::mutex> lock(g_knobs_mutex);
    if (!g_knobs_ready) { parse_knobs(g_knobs); g_knobs_ready = true; }
    return g_knobs;
}

void knobs_reload() {
    std::lock_guard<std::mutex> lock(g_knobs_mutex);
    parse_knobs(g_knobs);
    g_knobs_ready = true;
}

template <typename off_t>
__global__ __launch_bounds__(kBlock) void probe_kernel(int32_t n_rows, const off_t* __restrict__ Ap,
                                                       const int32_t* __restrict__ Aj, long long* out) {
    // out[0], out[1]: band [lo, hi] over the first/last column of 256 rows;
    // out[2 + 32 t + i]: (column - row) at 32 positions spread over row t's nonzeros (LLONG_MAX = none);
    // out[2 + 32 * 256], out[3 + 32 * 256]: shortest / longest of the 256 rows
    __shared__ long long s_lo[kBlock / kWave], s_hi[kBlock / kWave], s_lmin[kBlock / kWave], s_lmax[kBlock / kWave];
    __shared__ int s_short;
    const int tid = threadIdx.x;
    long long lo = LLONG_MAX, hi = LLONG_MIN, lmin = LLONG_MAX, lmax = 0, mine = 0;
    for (int i = 0; i < kProbePerRow; ++i) out[2 + tid * kProbePerRow + i] = LLONG_MAX;
    if (n_rows > 0) {
        const int64_t r = (int64_t(n_rows - 1) * tid) / (kBlock - 1);
        const off_t s = Ap[r], e = Ap[r + 1];
        lmin = lmax = mine = (long long)(e - s);
        if (e > s) {
            const long long first = Aj[s], last = Aj[e - 1];
            lo = min(first, last) - r;
            hi = max(first, last) - r;
            const off_t len = e - s;
            const int take = len < kProbePerRow ? int(len) : kProbePerRow;
            for (int i = 0; i < take; ++i) {
                const off_t k = take > 1 ? s + ((len - 1) * i) / (take - 1) : s;
                out[2 + tid * kProbePerRow + i] = (long long)Aj[k] - r;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, kWave));
        hi = max(hi, __shfl_xor(hi, o, kWave));
        lmin = min(lmin, __shfl_xor(lmin, o, kWave));
        lmax = max(lmax, __shfl_xor(lmax, o, kWave));
    }
    if ((tid & (kWave - 1)) == 0) {
        s_lo[tid / kWave] = lo;
        s_hi[tid / kWave] = hi;
        s_lmin[tid / kWave] = lmin;
        s_lmax[tid / kWave] = lmax;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) {
            lo = min(lo, s_lo[w]);
            hi = max(hi, s_hi[w]);
            lmin = min(lmin, s_lmin[w]);
            lmax = max(lmax, s_lmax[w]);
        }
        out[0] = lo;
        out[1] = hi;
        out[2 + kBlock * kProbePerRow] = lmin;
        out[3 + kBlock * kProbePerRow] = lmax;
        s_lmax[0] = lmax;
        s_short = 0;
    }
    // how many of the sampled rows fill less than three quarters of the step (8, 16, 32, 64 or 128 nonzeros: the widths
    // a vector of lanes covers at once) that the longest of them needs: a stencil's boundary rows are a few per cent
    // of the sample, a matrix of VARYING row lengths half of it (merge_plan.hip, merge_rows_wanted)
    __syncthreads();
    {
        const long long longest = s_lmax[0];
        long long step = 8;
        while (step < longest && step < 128) step *= 2;
        const bool is_short = n_rows > 0 && mine * 4 < step * 3;
        const int n = __popcll(__ballot(is_short));
        if ((tid & (kWave - 1)) == 0 && n) atomicAdd(&s_short, n);
    }
    __syncthreads();
    if (tid == 0) out[4 + kBlock * kProbePerRow] = s_short;
}

static std::mutex g_analysis_mutex;   // (common.hpp, AnalysisBuffer)
static long long* g_analysis_buf[64] = {};

static long long* analysis_words() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!g_analysis_buf[dev]) {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, kAnalysisWords * sizeof(long long)) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        g_analysis_buf[dev] = static_cast<long long*>(ptr);
    }
    return g_analysis_buf[dev];
}

AnalysisBuffer::AnalysisBuffer() : lock_(g_analysis_mutex), words(analysis_words()) {}

int probe_structure(Plan& p, ProbeSamples& probe) {
    p.probe_ok = false;
    p.band_lo = p.band_hi = 0;
    probe.n = 0;
    p.n_seg = 0;
    if (p.n_rows <= 0 || p.nnz <= 0) return MI355_SPMV_OK;
    constexpr size_t NS = 2 + size_t(kBlock) * kProbePerRow;   // band + samples
    constexpr size_t N = NS + 3;                                // + shortest / longest sampled row, + the count of short ones
    static_assert(size_t(kBlock) * kProbePerRow <= sizeof(probe.off) / sizeof(probe.off[0]), "probe buffer");
    p.probe_len_min = p.probe_len_max = 0;
    p.probe_short_rows = 0;
    const AnalysisBuffer buf;
    long long* d_out = buf.words;
    if (!d_out) { set_error("probe_structure: no device scratch"); return MI355_SPMV_ENOMEM; }
    with_offsets(p, [&](auto* Ap) { hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(kBlock), 0, nullptr, p.n_rows, Ap, p.Aj, d_out); });
    long long* h = new (std::nothrow) long long[N];
    hipError_t e = h ? hipGetLastError() : hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpy(h, d_out, N * sizeof(long long), hipMemcpyDeviceToHost);   // synchronises
    if (e != hipSuccess) {
        delete[] h;
        set_error("probe_structure: %s", hipGetErrorString(e));
        return MI355_SPMV_EHIP;
    }
    if (h[0] <= h[1]) {
        p.band_lo = h[0];
        p.band_hi = h[1];
        p.probe_ok = true;
        for (size_t i = 2; i < NS; ++i)
            if (h[i] != LLONG_MAX) probe.off[probe.n++] = h[i];
        p.probe_len_min = h[NS];
        p.probe_len_max = h[NS + 1];
        p.probe_short_rows = int(h[NS + 2]);
        probe.sorted = false;    // sorted on first use (cluster_bands): most plans never need the samples
    }
    delete[] h;
    return MI355_SPMV_OK;
}

int allow_dynamic_lds(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return MI355_SPMV_OK;
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> allowed;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = allowed[kernel];
    if (have >= bytes) return MI355_SPMV_OK;
    MI355_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
    have = bytes;
    return MI355_SPMV_OK;
}

// ---- partition into row blocks (multi-GPU; include/mi355_spmv.h "row-block plans") -----------------
// Boundary b of `parts` blocks: the first UNIT whose first row starts at or after nonzero b * nnz / parts.
// A unit is a chunk of the plan (VECTOR / LIGHT: a block then owns whole chunks, so it can reproduce the whole
// plan's per-chunk decisions) or 4 rows (MERGE: any multiple of 4 rows keeps the 16-byte phase rule simple).
template <typename off_t>
__global__ __launch_bounds__(kBlock) void partition_kernel(int32_t n_rows, const off_t* __restrict__ Ap,
                                                           const int32_t* __restrict__ table, int64_t rows_per_unit,
                                                           int64_t n_units, int parts, long long* out) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b > parts) return;
    auto unit_row = [&](int64_t u) -> int64_t {
        if (u >= n_units) return n_rows;
        return table ? int64_t(table[u]) : min(u * rows_per_unit, int64_t(n_rows));
    };
    const int64_t first = int64_t(Ap[0]), last = int64_t(Ap[n_rows]);
    int64_t u = 0;
    if (b == parts) u = n_units;
    else if (b > 0) {
        const int64_t target = first + int64_t((__int128)(last - first) * b / parts);
        int64_t lo = 0, hi = n_units;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (int64_t(Ap[unit_row(mid)]) >= target) hi = mid;
            else lo = mid + 1;
        }
        u = lo;
    }
    const int64_t r = unit_row(u);
    out[3 * b + 0] = r;
    out[3 * b + 1] = u;
    out[3 * b + 2] = int64_t(Ap[r]);
}

int partition_plan(const Plan& p, int parts, int64_t* row_cuts, int64_t* chunk_cuts, int64_t* nnz_cuts) {
    if (p.n_rows <= 0) {
        for (int b = 0; b <= parts; ++b) { row_cuts[b] = 0; chunk_cuts[b] = 0; nnz_cuts[b] = p.nnz_begin; }
        return MI355_SPMV_OK;
    }
    if (size_t(parts + 1) * 3 > kAnalysisWords) { set_error("plan_partition: too many parts"); return MI355_SPMV_EINVAL; }
    const bool chunked = p.kind != MI355_KIND_MERGE;
    const int32_t* table = (chunked && p.balanced) ? p.chunk_row : nullptr;
    const int64_t rows_per_unit = chunked ? (p.rows_per_chunk > 0 ? p.rows_per_chunk : 4) : 4;
    const int64_t n_units = table ? p.n_chunks : (int64_t(p.n_rows) + rows_per_unit - 1) / rows_per_unit;
    const AnalysisBuffer scratch;
    long long* buf = scratch.words;
    if (!buf) { set_error("plan_partition: no device scratch"); return MI355_SPMV_ENOMEM; }
    const unsigned g = unsigned((parts + 1 + kBlock - 1) / kBlock);
    with_offsets(p, [&](auto* Ap) {
        hipLaunchKernelGGL(partition_kernel, dim3(g), dim3(kBlock), 0, nullptr, p.n_rows, Ap, table, rows_per_unit, n_units, parts, buf);
    });
    hipError_t e = hipGetLastError();
    long long* h = new (std::nothrow) long long[size_t(parts + 1) * 3];
    if (!h) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpy(h, buf, size_t(parts + 1) * 3 * sizeof(long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        delete[] h;
        set_error("plan_partition: %s", hipGetErrorString(e));
        return MI355_SPMV_EHIP;
    }
    for (int b = 0; b <= parts; ++b) {
        row_cuts[b] = h[3 * b];
        chunk_cuts[b] = chunked ? h[3 * b + 1] : 0;
        nnz_cuts[b] = h[3 * b + 2];
        if (b > 0 && row_cuts[b] < row_cuts[b - 1]) {   // (monotone by construction; keep it so whatever Ap holds)
            row_cuts[b] = row_cuts[b - 1]; chunk_cuts[b] = chunk_cuts[b - 1]; nnz_cuts[b] = nnz_cuts[b - 1];
        }
    }
    delete[] h;
    return MI355_SPMV_OK;
}

// Cluster the sampled offsets into bands: a gap wider than the rows a workgroup owns starts a
// new band (splitting costs `rows` extra columns per band, keeping the gap costs the gap).
// Returns the columns a workgroup would have to hold: sum of (band width + rows).
static int64_t cluster_bands(Plan& p, ProbeSamples& probe, int64_t rows) {
    p.n_seg = 0;
    if (probe.n == 0) return 0;
    if (!probe.sorted) {
        std::sort(probe.off, probe.off + probe.n);
        probe.sorted = true;
    }
    int64_t lo[64], hi[64];
    int n = 0;
    lo[0] = hi[0] = probe.off[0];
    for (int i = 1; i < probe.n; ++i) {
        if (probe.off[i] - hi[n] > rows && n + 1 < 64) {
            ++n;
            lo[n] = probe.off[i];
        }
        hi[n] = probe.off[i];
    }
    ++n;
    while (n > kMaxSegments) {   // merge across the narrowest gap
        int best = 0;
        for (int i = 1; i + 1 < n; ++i)
            if (lo[i + 1] - hi[i] < lo[best + 1] - hi[best]) best = i;
        hi[best] = hi[best + 1];
        for (int i = best + 1; i + 1 < n; ++i) { lo[i] = lo[i + 1]; hi[i] = hi[i + 1]; }
        --n;
    }
    int64_t need = 0;
    for (int i = 0; i < n; ++i) {
        // the samples may miss a band's edges: widen each by 1/16 of its width + 8 columns
        const int64_t pad = (hi[i] - lo[i]) / 16 + 8;
        p.seg_lo[i] = lo[i] - pad;
        p.seg_hi[i] = hi[i] + pad;
        need += (p.seg_hi[i] - p.seg_lo[i] + 1) + rows;
    }
    p.n_seg = n;
    return need;
}

// Window size (elements) for a workgroup that owns `rows_per_workgroup` consecutive rows: what the
// sampled band plus those rows needs, up to the plan's LDS budget (p.window_bytes), when that is within
// 1.5x of the budget (the kernels centre a too-small window on the span); else several narrow bands; else
// none.  MI355_SPMV_WINDOW=0|1 forces the choice (tuning / tests).
int pick_window_elems(Plan& p, ProbeSamples& probe, int64_t rows_per_workgroup) {
    const int val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const int cap = (p.window_bytes > 0 ? p.window_bytes : kWindowBytes) / val_bytes;
    p.window_from_band = false;
    if (p.knob.window >= 0) return p.knob.window ? cap : 0;
    if (!p.probe_ok) return 0;
    const int64_t span = (p.band_hi - p.band_lo + 1) + rows_per_workgroup;
    // the band (plus the chunk's rows) all but fits: no need to sample every chunk
    p.window_from_band = p.knob.window_from_band >= 0 ? p.knob.window_from_band != 0 : span <= int64_t(cap) * 9 / 8;
    p.n_seg = 0;
    if (span <= int64_t(cap) * 3 / 2) {
        // LDS is occupancy: take what the span needs (a sampled window is widened by an eighth + 64 per side)
        const int64_t want = p.window_from_band ? span + 8 : span + 2 * (span / 8 + 64) + 8;
        const int64_t elems = (std::min<int64_t>(want, cap) + 3) & ~int64_t(3);
        return int(std::min<int64_t>(elems, cap));
    }
    // one window cannot hold the band: do a few narrow ones?  (MI355_SPMV_SEGMENTS=0 disables)
    if (p.knob.segments != 0) {
        const int64_t need = cluster_bands(p, probe, rows_per_workgroup);
        // up to 1.25x: the tail of the last band is cut and falls back to global loads; the
        // row-based kinds then shrink their chunk so that everything fits (segment_rows_fit)
        if (p.n_seg >= 2 && need <= int64_t(cap) * 5 / 4) return cap;
    }
    p.n_seg = 0;
    return 0;
}

// Rows per workgroup for which the plan's bands fit the window exactly:
// sum_k (width_k + rows) <= cap.  0 when there are no segments.
int64_t segment_rows_fit(const Plan& p) {
    if (p.n_seg < 2 || p.window_elems <= 0) return 0;
    int64_t width = 0;
    for (int i = 0; i < p.n_seg; ++i) width += p.seg_hi[i] - p.seg_lo[i] + 1 + 4;   // +4: 16-byte rounding
    const int64_t fit = (int64_t(p.window_elems) - width) / p.n_seg;
    return fit > 0 ? fit : 0;
}

}  // namespace mi355
