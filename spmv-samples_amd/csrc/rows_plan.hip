// rows_plan.hip — kinds VECTOR and LIGHT, the plan unit: the shape of a plan (shape_rows: lanes per row, workgroup
// size, chunks and the window of x in shape_chunks, equal-row or weight-cut chunks in decide_balance, the sweeping window
// in shape_sweep, giant rows, the small-matrix rule), the launch that follows from it (set_rows_launch), what a row block
// inherits of it (export_rows_shape / inherit_rows_shape), and the plan-time kernels with their host side: the heaviest
// chunk, the chunk table, the giant-row scan and the packed index.  Compiled once; the kinds' kernels are launched
// through row_launch.hpp.  The probe, the window pick and the analysis buffer are shared with the merge planner
// (analyze.hip).

#include <algorithm>
#include <utility>

#include "common.hpp"
#include "row_dot.hpp"
#include "xwindow.hpp"

namespace mi355 {

// Workgroups of the plan's size a CU holds by REGISTERS (the launch bounds of the VECTOR / LIGHT kernels): two of
// 512 threads; four of 256 when the body keeps 2 rows per vector in flight (fp64; fp32 with 16+ lanes per row),
// three with 4 rows (fp32, up to 8 lanes per row, and the per-chunk-width kernels of weight-cut plans).
static int workgroups_per_cu_by_registers(const Plan& p) {
    if (p.block_threads == kHugeBlock) return 1;
    if (p.block_threads == kWideBlock) return 2;
    if (p.balanced) return p.val_type == MI355_VAL_F64 ? 4 : 3;
    return (p.val_type == MI355_VAL_F64 || p.lanes_per_row >= 16) ? 4 : 3;
}

int long_steps_for(const Plan& p) {
    if (p.knob.long_steps > 0) return p.knob.long_steps;
    // measured on the power-law stand-ins (us, 1 / 2 / 4 / 8 / 16 steps): web-Google 139 / 120 / 99 / 104 / 105,
    // R-MAT-24 light 2 820 at 4 vs 3 200 at 16; uniform plans keep the long chain (their rows rarely need it)
    return p.balanced ? 4 : kLongSteps;
}

// T (lanes per row) from the mean row length.  With 4 nonzeros per lane per step a T-lane
// vector covers 4T nonzeros per step; pick the smallest T whose step covers the mean row,
// so that a typical row is one load per lane and a wave holds 64/T rows in flight.
// (Reference rule, 1 element per lane and T <= 32: cusp_warp_reduce.cuh:100-127;
// LightSpMV.cuh:354-370.)
static int pick_lanes_per_row(int64_t nnz, int64_t n_rows, int elems) {
    const int64_t mean = n_rows > 0 ? (nnz + n_rows - 1) / n_rows : 0;
    int t = 2;
    while (t < 64 && int64_t(t) * elems < mean) t <<= 1;
    return t;
}

// Rows per workgroup chunk: ~32 K nonzeros (256 KB of fp32 stream) per chunk, a
// multiple of the rows one pass of the workgroup covers.
static int64_t pick_rows_per_chunk(int64_t nnz, int64_t n_rows, int lanes_per_row, int rows_in_flight, int block_threads,
                                   int64_t nnz_per_chunk, int per_cu) {
    const int64_t pass = int64_t(block_threads / lanes_per_row) * rows_in_flight;
    const int64_t mean = n_rows > 0 ? (nnz + n_rows - 1) / n_rows : 1;
    int64_t rows = nnz_per_chunk / (mean > 0 ? mean : 1);
    // small matrices: prefer one chunk per workgroup slot (per_cu a CU) over long chunks
    const int64_t fill = (n_rows + int64_t(kCus) * per_cu - 1) / (int64_t(kCus) * per_cu);
    if (rows > fill) rows = fill;
    rows = (rows + pass - 1) / pass * pass;
    if (rows < pass) rows = pass;
    if (rows > kMaxChunkRows) rows = kMaxChunkRows / pass * pass > 0 ? kMaxChunkRows / pass * pass : pass;
    return rows;
}

// ---- uniform or nnz-balanced chunks (VECTOR, LIGHT) ---------------------------------------------
// Chunks of equal ROW count are right for matrices whose rows are alike (the S32-band target, FEM
// matrices, stencils): no table, no extra load.  On a power-law matrix they are not: the 2 048 rows
// that hold the hubs of the web-Google stand-in carry 8 % of all nonzeros, one workgroup walks them
// while the chip idles (vector 763 us, light 575 us vs merge 49 us; R-MAT-24: 20.4 / 14.4 ms vs 2.4 ms).
// The plan therefore measures the heaviest uniform chunk once (two reads of Ap per chunk) and, when it is
// more than twice the mean,
// cuts the rows by WEIGHT instead: a row weighs (its nonzeros + k), k = mean row length, and chunk c
// starts at the first row r with Ap[r] + k r >= c Q.  That is the merge-path diagonal cut with rows
// weighted k instead of 1 (thread_search.cuh:15-49) at chunk granularity: a chunk holds at most Q / k rows
// and at most Q nonzeros plus one row's overshoot, and the boundaries come from a binary search per
// chunk at plan creation (chunk_table_kernel) instead of a per-launch search kernel.
template <typename off_t>
__global__ __launch_bounds__(kBlock) void chunk_max_kernel(int32_t n_rows, const off_t* __restrict__ Ap,
                                                           int64_t rows_per_chunk, int64_t n_chunks,
                                                           unsigned long long* out) {
    unsigned long long m = 0;
    for (int64_t c = int64_t(blockIdx.x) * kBlock + threadIdx.x; c < n_chunks; c += int64_t(gridDim.x) * kBlock) {
        const int64_t rb = c * rows_per_chunk;
        const int64_t re = min(rb + rows_per_chunk, int64_t(n_rows));
        const unsigned long long w = (unsigned long long)(Ap[re] - Ap[rb]);
        m = w > m ? w : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(m, o, kWave);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicMax(out, m);
}

template <typename off_t>
__global__ __launch_bounds__(kBlock) void chunk_table_kernel(int32_t n_rows, const off_t* __restrict__ Ap, int64_t k,
                                                             int64_t q, int64_t n_chunks,
                                                             int32_t* __restrict__ chunk_row, int64_t weight_off,
                                                             int64_t chunk_off) {
    // weight_off / chunk_off: a row-block plan numbers weights and chunks as the WHOLE matrix's plan does
    // (weight of local row r = Ap[r] + k r + weight_off, local chunk c = whole chunk c + chunk_off), so that its
    // boundaries are the whole plan's; both 0 otherwise.  A block starts on a multiple of 4 rows of the whole.
    const int64_t c = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (c > n_chunks) return;
    if (c == n_chunks) {
        chunk_row[c] = n_rows;
        return;
    }
    const int64_t target = (c + chunk_off) * q - weight_off;   // first r in [0, n_rows] with Ap[r] + k r >= target
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (int64_t(Ap[mid]) + k * mid >= target) hi = mid;
        else lo = mid + 1;
    }
    chunk_row[c] = int32_t(lo & ~int64_t(3));   // multiples of 4 rows keep the y sweep on 16-byte stores
}

static int decide_balance(Plan& p) {
    p.balanced = false;
    p.chunk_row = nullptr;
    p.rows_cap = int(p.rows_per_chunk);
    p.n_chunks = p.rows_per_chunk > 0 ? (int64_t(p.n_rows) + p.rows_per_chunk - 1) / p.rows_per_chunk : 0;
    if (p.n_chunks < 1) p.n_chunks = 1;
    const int ev = p.knob.balance;                          // 0 = never, 1 = always, -1 = measure
    if (p.n_rows <= 0 || p.nnz <= 0 || ev == 0) return MI355_SPMV_OK;
    bool want = ev > 0;
    if (!want && p.n_chunks >= 2) {
        const AnalysisBuffer buf;
        if (!buf.words) { set_error("decide_balance: no device scratch"); return MI355_SPMV_ENOMEM; }
        unsigned long long* d_max = reinterpret_cast<unsigned long long*>(buf.words + kAnalysisWords - 1);
        hipError_t e = hipMemsetAsync(d_max, 0, sizeof(unsigned long long), nullptr);
        const unsigned g = unsigned(std::min<int64_t>((p.n_chunks + kBlock - 1) / kBlock, 1024));
        if (e == hipSuccess) {
            with_offsets(p, [&](auto* Ap) {
                hipLaunchKernelGGL(chunk_max_kernel, dim3(g), dim3(kBlock), 0, nullptr, p.n_rows, Ap, p.rows_per_chunk, p.n_chunks, d_max);
            });
            e = hipGetLastError();
        }
        unsigned long long h_max = 0;
        if (e == hipSuccess) e = hipMemcpy(&h_max, d_max, sizeof(h_max), hipMemcpyDeviceToHost);   // synchronises
        if (e != hipSuccess) {
            set_error("decide_balance: %s", hipGetErrorString(e));
            return MI355_SPMV_EHIP;
        }
        const double mean = double(p.nnz) / double(p.n_chunks);
        want = double(h_max) > 2.0 * mean + 1024.0;
    }
    if (!want) return MI355_SPMV_OK;
    // chunk weight: twice what a chunk of rows_per_chunk mean rows weighs, rows capped so that the LDS
    // layout (bounds + results of rows_cap rows) stays what a uniform plan of kMaxChunkRows rows takes
    int64_t r0 = p.rows_per_chunk;
    if (r0 > kMaxChunkRows / 2) r0 = kMaxChunkRows / 2;
    if (r0 < 4) r0 = 4;
    p.bal_k = (p.nnz - p.nnz_begin + p.n_rows - 1) / p.n_rows;
    if (p.bal_k < 1) p.bal_k = 1;
    p.bal_q = 2 * p.bal_k * r0;
    const int64_t weight = (p.nnz - p.nnz_begin) + p.bal_k * int64_t(p.n_rows);
    p.n_chunks = (weight + p.bal_q - 1) / p.bal_q;
    if (p.n_chunks < 1) p.n_chunks = 1;
    p.rows_cap = int(2 * r0 + 4);              // Q / k rows, + 3 for the round-down of the boundaries
    p.balanced = true;
    // Whole rounds (as shape_chunks does for equal-row chunks): 862 chunks on 768 workgroup slots are two rounds of
    // full-size chunks, the second one an eighth full; cut the same weight into 2 x 768 smaller chunks instead.
    // Only ever makes chunks smaller, so rows_cap holds.
    if (p.knob.rows_per_chunk <= 0) {
        const int64_t slots = int64_t(kCus) * workgroups_per_cu_by_registers(p);
        const int64_t rounds = (p.n_chunks + slots - 1) / slots;
        if (rounds <= 4 && p.n_chunks > slots / 2 && p.n_chunks % slots != 0) {
            int64_t q = (weight + rounds * slots - 1) / (rounds * slots);
            if (q < 8 * p.bal_k) q = 8 * p.bal_k;
            if (q < p.bal_q) {
                p.bal_q = q;
                p.n_chunks = (weight + q - 1) / q;
            }
        }
    }
    return MI355_SPMV_OK;
}

// ---- giant rows (giant_rows.hpp) ------------------------------------------------------------------
template <typename off_t>
__global__ __launch_bounds__(kBlock) void giant_scan_kernel(int32_t n_rows, const off_t* __restrict__ Ap, int cap,
                                                            int64_t giant_len, long long* out) {   // out[0] = count, then (row, length) pairs
    for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < n_rows; r += int64_t(gridDim.x) * kBlock) {
        const int64_t len = int64_t(Ap[r + 1]) - int64_t(Ap[r]);
        if (len > giant_len) {
            const unsigned long long i = atomicAdd(reinterpret_cast<unsigned long long*>(out), 1ull);
            if (i < (unsigned long long)cap) {
                out[1 + 2 * i] = r;
                out[2 + 2 * i] = len;
            }
        }
    }
}

int find_giant_rows(Plan& p, GiantRowList& giants) {
    p.n_giant = 0;
    p.n_giant_slices = 0;
    // (a row-block plan does what the whole matrix's plan decided: p.giant_enabled / p.giant_len are inherited)
    if (!p.balanced || (p.is_block ? !p.giant_enabled : p.knob.giant == 0)) { p.giant_enabled = false; return MI355_SPMV_OK; }
    // an empty row block of a weight-cut plan (a row heavier than a block's share of the nonzeros leaves the cuts behind
    // it without rows): nothing to scan, and a grid of no workgroups is not a launch
    if (p.n_rows <= 0) return MI355_SPMV_OK;
    // A row is giant when it alone is more than an eighth of a CU's fair share of the matrix (a hub of 30 K nonzeros in a
    // 4 M-nonzero R-MAT kept ONE workgroup busy for most of the kernel: 75 us against merge's 30), between 4 K and 64 K.
    if (!p.is_block) {
        int64_t fair = ((p.nnz - p.nnz_begin) / (int64_t(kCus) * 8) + 1023) & ~int64_t(1023);
        fair = fair < 4096 ? 4096 : (fair > kGiantRow ? kGiantRow : fair);
        p.giant_len = p.knob.giant_row >= 4096 ? p.knob.giant_row : fair;
    }
    p.giant_enabled = false;
    const AnalysisBuffer scratch;
    long long* buf = scratch.words;   // (1 + 2 kMaxGiantRows words of it: common.hpp)
    if (!buf) { set_error("find_giant_rows: no device scratch"); return MI355_SPMV_ENOMEM; }
    static thread_local long long h[1 + 2 * kMaxGiantRows];
    auto scan = [&](int64_t giant_len) -> int {          // rows longer than giant_len -> h (count, then (row, length) pairs)
        hipError_t e = hipMemsetAsync(buf, 0, sizeof(long long), nullptr);
        if (e == hipSuccess) {
            const unsigned g = unsigned(std::min<int64_t>((int64_t(p.n_rows) + kBlock - 1) / kBlock, 2048));
            with_offsets(p, [&](auto* Ap) {
                hipLaunchKernelGGL(giant_scan_kernel, dim3(g), dim3(kBlock), 0, nullptr, p.n_rows, Ap, kMaxGiantRows, giant_len, buf);
            });
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost);   // synchronises
        if (e != hipSuccess) {
            set_error("find_giant_rows: %s", hipGetErrorString(e));
            return MI355_SPMV_EHIP;
        }
        return MI355_SPMV_OK;
    };
    if (const int st = scan(p.giant_len)) return st;
    // The slices cost two more launches (~6 us).  With the threshold lowered for a small matrix they are only taken when the
    // longest row is on the critical path by more than that: a workgroup walks ~1 K nonzeros of a hub per us, so the hub must
    // outweigh a workgroup slot's share of the whole matrix (nonzeros + mean-row-length per row, over the slots in use) by 10 K+.
    // R-MAT-18 (30 K hub, share 11 K): 75 -> 55 us; R-MAT-20 (69 K, 44 K): 200 -> 173; R-MAT-16 (13 K, 8 K) and the web-Google
    // stand-in lost 6 us each with the slices and keep the default threshold.
    if (!p.is_block && p.knob.giant_row < 4096 && p.giant_len < kGiantRow) {
        long long longest = 0;
        if (h[0] > 0 && h[0] <= kMaxGiantRows)
            for (long long i = 0; i < h[0]; ++i) longest = std::max(longest, h[2 + 2 * i]);
        const int64_t nnz = p.nnz - p.nnz_begin;
        const int64_t slots = std::max<int64_t>(1, std::min<int64_t>(p.n_chunks, int64_t(kCus) * 3));   // (a small matrix has fewer chunks than slots)
        const int64_t share = (nnz + (p.n_rows > 0 ? nnz / p.n_rows : 0) * int64_t(p.n_rows)) / slots;
        if (longest < share + 10240) {
            p.giant_len = kGiantRow;
            if (const int st = scan(p.giant_len)) return st;
        }
    }
    const long long count = h[0];
    if (count > kMaxGiantRows) return MI355_SPMV_OK;   // too many to be "a few dense rows": they stay with their workgroups
    p.giant_enabled = true;                            // (a block of this matrix may hold some even if this one holds none)
    if (count <= 0) return MI355_SPMV_OK;
    const int64_t slice = giant_slice_for(p.giant_len);
    static thread_local std::pair<long long, long long> rows[kMaxGiantRows];
    for (long long i = 0; i < count; ++i) rows[i] = {h[1 + 2 * i], h[2 + 2 * i]};
    std::sort(rows, rows + count);                                // the device appended them in any order
    giants.slice_first[0] = 0;
    for (long long i = 0; i < count; ++i) {
        giants.row[i] = int32_t(rows[i].first);
        giants.slice_first[i + 1] = giants.slice_first[i] + (rows[i].second + slice - 1) / slice;
    }
    p.n_giant = int(count);
    p.n_giant_slices = giants.slice_first[count];
    return MI355_SPMV_OK;
}

int build_chunk_table(Plan& p, const GiantRowList& giants) {
    if (p.n_giant > 0) {
        MI355_HIP_TRY(hipMemcpy(p.giant_row, giants.row, sizeof(int32_t) * size_t(p.n_giant), hipMemcpyHostToDevice));
        MI355_HIP_TRY(hipMemcpy(p.giant_slice_first, giants.slice_first, sizeof(int64_t) * size_t(p.n_giant + 1),
                                hipMemcpyHostToDevice));
    }
    if (!p.balanced) return MI355_SPMV_OK;
    const unsigned g = unsigned((p.n_chunks + 1 + kBlock - 1) / kBlock);
    with_offsets(p, [&](auto* Ap) {
        hipLaunchKernelGGL(chunk_table_kernel, dim3(g), dim3(kBlock), 0, nullptr, p.n_rows, Ap, p.bal_k, p.bal_q, p.n_chunks, p.chunk_row,
                           p.is_block ? p.block_weight_off : -p.nnz_begin, p.is_block ? p.block_chunk_begin : int64_t(0));
    });
    MI355_HIP_TRY(hipGetLastError());
    MI355_HIP_TRY(hipStreamSynchronize(nullptr));   // the first execute may come on any stream
    return MI355_SPMV_OK;
}

// ---- the packed index of a banded VECTOR plan -----------------------------------------------------------
// On the flagship (S32-band, 2^22 rows x 32, fp32) Aj is 537 MB of the 1 124 MB an execute reads, and all the kernel
// does with a column is subtract the start of its chunk's window and range-check the difference (XWindow::find).  When
// every chunk's window is placed from the plan's band — a function of the chunk's rows and the plan alone
// (xwindow.hpp, band_window) — that difference can be stored once: 16 bits per nonzero, kPackedEscape for a column
// outside the window (the kernel then reads the real column from Aj, as it reads x from memory for it today).
// One workgroup per chunk of the plan's ChunkMap; it writes exactly the elements [Ap[rb], Ap[re]) of its rows.
template <typename val_t>
__global__ __launch_bounds__(kBlock) void pack_index_kernel(int32_t n_rows, int32_t n_cols, const ApView Ap,
                                                            const int32_t* __restrict__ Aj, uint16_t* __restrict__ out,
                                                            ChunkMap cmap, int32_t window_cap, BandHint hint,
                                                            unsigned long long* escapes) {
    int64_t rb, re;
    cmap.range(blockIdx.x, n_rows, rb, re);
    if (rb >= re) return;
    const int64_t s = Ap.at(rb), e = Ap.at(re);
    const WindowSpan w = band_window<val_t>(rb, re, n_cols, window_cap, hint);
    unsigned escaped = 0;
    auto encode = [&](int32_t col) -> unsigned {
        const unsigned rel = unsigned(col - w.lo);
        const bool in = rel < unsigned(w.len);
        escaped += in ? 0u : 1u;
        return in ? rel : kPackedEscape;
    };
    // whole 16-byte groups of Aj -> 8-byte groups of the index; the elements before the first and after the last singly
    const int64_t s4 = min((s + 3) & ~int64_t(3), e), e4 = max(e & ~int64_t(3), s4);
    const int tid = threadIdx.x;
    if (tid < s4 - s) out[s + tid] = uint16_t(encode(Aj[s + tid]));
    if (tid < e - e4) out[e4 + tid] = uint16_t(encode(Aj[e4 + tid]));
    for (int64_t k = s4 + int64_t(tid) * 4; k < e4; k += int64_t(kBlock) * 4) {
        const int4v c = stream_load(reinterpret_cast<const int4v*>(Aj + k));
        uint2v v;
        v[0] = encode(c[0]) | (encode(c[1]) << 16);
        v[1] = encode(c[2]) | (encode(c[3]) << 16);
        *reinterpret_cast<uint2v*>(out + k) = v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) escaped += __shfl_xor(escaped, o, kWave);
    if ((tid & (kWave - 1)) == 0 && escaped) atomicAdd(escapes, (unsigned long long)escaped);
}

// Which plans hold one: kind VECTOR on the chunked kernels with ONE window of at most 65 535 elements that every chunk
// places from the band, equal-row chunks, a 16-byte-aligned Aj, and neither MI355_PLAN_NO_INDEX_COPY nor
// MI355_SPMV_PACK=0.  No device memory for it: the plan stays unpacked, which is not an error.  Synchronises (the first
// execute may come on any stream; the escape count comes back with it).
int build_packed_index(Plan& p) {
    p.packed_index = nullptr;
    p.packed_bytes = 0;
    p.packed_escapes = 0;
    if (p.kind != MI355_KIND_VECTOR || (p.flags & MI355_PLAN_NO_INDEX_COPY) || p.knob.pack == 0) return MI355_SPMV_OK;
    if (p.small_plain || p.sweep || p.balanced || (p.knob.plain != 0 && !p.is_block)) return MI355_SPMV_OK;
    if (p.window_elems <= 0 || p.window_elems > 65535 || p.n_seg >= 2 || !p.window_from_band) return MI355_SPMV_OK;
    if (p.n_rows <= 0 || p.nnz < 4 || p.nnz <= p.nnz_begin || p.n_chunks < 1 || p.n_chunks > int64_t(UINT32_MAX)) return MI355_SPMV_OK;
    if ((reinterpret_cast<uintptr_t>(p.Aj) & 15u) != 0) return MI355_SPMV_OK;
    // every 8-byte group the kernels address lies below nnz_read rounded up to a group (their clamped loads included:
    // j_max = the last whole group); one group more, and the allocation is 256-byte aligned
    const size_t bytes = (((size_t(p.nnz_read) + 3) & ~size_t(3)) + 4) * sizeof(uint16_t);
    void* ptr = nullptr;
    if (hipMalloc(&ptr, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return MI355_SPMV_OK;
    }
    const AnalysisBuffer buf;
    unsigned long long* d_escapes = reinterpret_cast<unsigned long long*>(buf.words);
    hipError_t e = d_escapes ? hipSuccess : hipErrorOutOfMemory;
    // elements that belong to no row of this plan (a block's phase, the tail of its last group, the padding) escape
    if (e == hipSuccess) e = hipMemsetAsync(ptr, 0xFF, bytes, nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(d_escapes, 0, sizeof(unsigned long long), nullptr);
    if (e == hipSuccess) {
        const ApView Ap{p.Ap, p.off_type == MI355_OFF_I64 ? 1 : 0};
        const BandHint hint{p.band_lo, p.band_hi, true};
        const dim3 grid((unsigned)p.n_chunks), block(kBlock);
        if (p.val_type == MI355_VAL_F64)
            hipLaunchKernelGGL((pack_index_kernel<double>), grid, block, 0, nullptr, p.n_rows, p.n_cols, Ap, p.Aj,
                               static_cast<uint16_t*>(ptr), chunk_map_of(p), (int32_t)p.window_elems, hint, d_escapes);
        else
            hipLaunchKernelGGL((pack_index_kernel<float>), grid, block, 0, nullptr, p.n_rows, p.n_cols, Ap, p.Aj,
                               static_cast<uint16_t*>(ptr), chunk_map_of(p), (int32_t)p.window_elems, hint, d_escapes);
        e = hipGetLastError();
    }
    unsigned long long escaped = 0;
    if (e == hipSuccess) e = hipMemcpy(&escaped, d_escapes, sizeof(escaped), hipMemcpyDeviceToHost);   // synchronises
    if (e != hipSuccess) {
        (void)hipFree(ptr);
        set_error("build_packed_index: %s", hipGetErrorString(e));
        return MI355_SPMV_EHIP;
    }
    p.packed_index = static_cast<uint16_t*>(ptr);
    p.packed_bytes = bytes;
    p.packed_escapes = int64_t(escaped);
    return MI355_SPMV_OK;
}

// LDS a workgroup may take: 3 workgroups of 256 threads per CU (what the 36 KB window was sized for),
// or 2 of 512 threads (up to 64 KB each, ~1 KB of it static).
static int window_budget(const Plan& p, int block_threads, int64_t rows) {
    if (block_threads == kBlock) return kWindowBytes;
    const size_t val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const int64_t avail = 63 * 1024 - int64_t(chunk_lds_bytes(0, int(rows), val_bytes));   // <= 64 KB per launch
    return int(avail < 0 ? 0 : avail);
}

static int rows_in_flight_of(const Plan& p) { return rows_in_flight(p.val_type == MI355_VAL_F64 ? 8 : 4, p.lanes_per_row); }
// ONE window of x, placed from the band, serves the chunk: what the 512- and 1 024-thread kernels are built around
static bool one_band_window(const Plan& p) { return p.window_elems > 0 && p.n_seg < 2 && p.window_from_band; }

// Whole rounds: with a few chunks per workgroup slot, a last round that is a third full costs a quarter
// of the kernel (2^20 rows: 1 024 chunks on 768 slots).  Shrink the chunk so that the count is a multiple
// of the slots the plan's LDS and registers leave on the chip.
static void shrink_to_whole_rounds(Plan& p, int64_t pass) {
    if (p.knob.rows_per_chunk > 0 || p.n_seg >= 2) return;
    const size_t val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const size_t lds = chunk_lds_bytes(p.window_elems, int(p.rows_per_chunk), val_bytes) + 1024;
    int64_t per_cu = int64_t(160 * 1024 / lds);
    const int64_t reg_bound = workgroups_per_cu_by_registers(p);
    if (per_cu > reg_bound) per_cu = reg_bound;
    const int64_t slots = int64_t(kCus) * (per_cu > 0 ? per_cu : 1);
    const int64_t n_chunks = (int64_t(p.n_rows) + p.rows_per_chunk - 1) / p.rows_per_chunk;
    const int64_t rounds = (n_chunks + slots - 1) / slots;
    if (!(n_chunks > slots / 2 && rounds < 8 && n_chunks % slots != 0)) return;
    int64_t r = (int64_t(p.n_rows) + rounds * slots - 1) / (rounds * slots);
    r = (r + 3) & ~int64_t(3);
    if (r >= pass && r < p.rows_per_chunk) {
        const int64_t shrink = p.rows_per_chunk - r;
        p.rows_per_chunk = r;
        if (p.window_elems > shrink && p.window_from_band) p.window_elems -= int(shrink & ~int64_t(3));
    }
}

// The plan for workgroups of block_threads threads and chunks of ~nnz_per_chunk nonzeros (or of rows_wanted rows): rows
// per chunk, the window's budget and the window.  div = the kind's chunk divisor (LIGHT's tuning knob).  Returns the
// rows of a chunk before it was shrunk to whole rounds.
static int64_t shape_for_block(Plan& p, ProbeSamples& probe, int64_t div, int block_threads, int64_t nnz_per_chunk,
                               int64_t rows_wanted = 0) {
    const int R = rows_in_flight_of(p);
    p.block_threads = block_threads;
    const int64_t pass = int64_t(block_threads / p.lanes_per_row) * R;
    int64_t rows = pick_rows_per_chunk(p.nnz, p.n_rows, p.lanes_per_row, R, block_threads, nnz_per_chunk,
                                       workgroups_per_cu_by_registers(p));
    if (div > 1) rows = (rows / div + pass - 1) / pass * pass;
    if (rows_wanted > 0) rows = std::min<int64_t>((rows_wanted + 3) & ~int64_t(3), kMaxChunkRows);
    if (p.knob.rows_per_chunk > 0) {
        int64_t r = p.knob.rows_per_chunk;
        r = (r + pass - 1) / pass * pass;
        if (r >= pass && r <= kMaxChunkRows) rows = r;
    }
    if (rows < pass) rows = pass;
    p.rows_per_chunk = rows;
    p.window_bytes = window_budget(p, block_threads, rows);
    p.window_elems = pick_window_elems(p, probe, rows);
    if (const int64_t fit = segment_rows_fit(p)) {   // several bands: shrink the chunk until they all fit
        if (fit < p.rows_per_chunk && fit >= pass) p.rows_per_chunk = fit / pass * pass;
        // ... and take only the LDS the bands need with that many rows (LDS is occupancy)
        int64_t need = 0;
        for (int i = 0; i < p.n_seg; ++i) need += p.seg_hi[i] - p.seg_lo[i] + 1 + 4 + p.rows_per_chunk;
        need = (need + 3) & ~int64_t(3);
        if (need < p.window_elems) p.window_elems = int(need);
    }
    shrink_to_whole_rounds(p, pass);
    return rows;
}

// Whether the 512-thread plan that shape_for_block just made stays (rows_before_rounding: what it returned).
static bool keep_wide_block(Plan& p, ProbeSamples& probe, int64_t div, bool force, int64_t rows_before_rounding) {
    const int64_t mean = p.n_rows > 0 ? (p.nnz + p.n_rows - 1) / p.n_rows : 1;
    // keep it when (a) the ">= 4 chunks per CU" rule left the chunk long and (b) one window placed from the
    // band serves it (with 64-bit offsets / fp64 / several bands the 64 KB a launch may take is better spent
    // on three workgroups of 256: C4 stand-in 660 us vs 824 us)
    // ("long" is judged before the chunk was shrunk to whole rounds: rows of 20-24 nonzeros reach the 2 048-row cap
    // at 41-49 K nonzeros, were shrunk a little, then failed the 48 K test and fell to 256 threads — 302 us against
    // 245 / 201 for 18 / 26 per row on either side)
    const bool long_chunk = p.rows_per_chunk * mean >= 49152 || rows_before_rounding >= kMaxChunkRows;
    // (a forced 512 is honoured unless the window needs several bands: those kernels exist for 256 threads only)
    if ((force && p.n_seg < 2) || (long_chunk && one_band_window(p))) return true;
    // A small matrix whose chunks all run at once — one round of the chip — also keeps the 512 threads when its rows
    // are long (16+ lanes per row: the R = 2 bodies): the same rows by half as many workgroups, i.e. half the
    // prologues (bounds, window, barriers) in a kernel that is nothing but its prologue and four groups of rows.
    // cant stand-in: 10.7-10.8 us against 10.9-11.2 with 976 workgroups of 256 (rounds 2 and 3, three boxes).
    // ... and whatever the row length when every workgroup still gets TWO groups of rows or more to pipeline: two
    // workgroups of 512 per CU — or, where that leaves them a single group each, one per CU with twice the rows.
    // S32-band shape, fp32, T = 8 (us, rule / the 256-thread plan with ~3 workgroups per CU it replaces;
    // scripts/probes/mid_size_knobs.sh): 2^17 rows 10.6 / 11.6, 2^18 15.9 / 19.0, 2^19 27.4 / 29.2 — the
    // mid-size matrices (35-140 MB) where a kernel is one round of the chip.
    if (force || p.knob.rows_per_chunk > 0 || div > 1 || !one_band_window(p)) return false;
    const int64_t pass = int64_t(kWideBlock / p.lanes_per_row) * rows_in_flight_of(p);
    const int64_t n_chunks = p.rows_per_chunk > 0 ? (int64_t(p.n_rows) + p.rows_per_chunk - 1) / p.rows_per_chunk : 0;
    if (n_chunks < kCus || n_chunks > int64_t(kCus) * 2) return false;
    if (p.lanes_per_row >= 16 || p.rows_per_chunk >= 2 * pass) return true;
    const int64_t twice = (int64_t(p.n_rows) + kCus - 1) / kCus;
    if (twice < 2 * pass || twice > kMaxChunkRows) return false;
    shape_for_block(p, probe, div, kWideBlock, 65536, twice);
    return one_band_window(p);
}

// One try of a bigger workgroup around ONE window that holds the whole band: block_threads threads with lds_bytes of
// LDS, the chunk as long as the band leaves room for — at least min_rows rows, in at least min_chunks chunks.  True when
// the plan is taken; else p is as it was.
static bool try_wide_window(Plan& p, ProbeSamples& probe, int block_threads, int64_t lds_bytes, int64_t min_rows,
                            int64_t min_chunks, bool shorter_chunks) {
    const int64_t off_bytes = 4, val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;   // (bounds are chunk-relative int32 in LDS)
    const int64_t band = p.band_hi - p.band_lo + 1;
    const int64_t pass = int64_t(block_threads / p.lanes_per_row) * rows_in_flight_of(p);
    // val (band + rows + 8) + off (rows + 1) + val rows + rows / 8 <= lds_bytes
    int64_t rows = (lds_bytes - val_bytes * (band + 8) - off_bytes) * 8 / (8 * (2 * val_bytes + off_bytes) + 1);
    rows = rows / pass * pass;
    if (rows > kMaxChunkRows) rows = kMaxChunkRows / pass * pass;
    // (a matrix too small for a full round of such chunks takes shorter ones — the band still fits: 2^18 rows x 64
    // in fp64 fell to the 1 024-thread plan at 3.9 TB/s for want of 512 chunks of 704 rows)
    if (shorter_chunks && rows > 0 && (p.n_rows + rows - 1) / rows < int64_t(kCus) * 2) {
        const int64_t fewer = ((int64_t(p.n_rows) + int64_t(kCus) * 2 - 1) / (int64_t(kCus) * 2) + pass - 1) / pass * pass;
        if (fewer < rows) rows = fewer;
    }
    const int64_t n_chunks = rows > 0 ? (p.n_rows + rows - 1) / rows : 0;
    if (!(band > 0 && rows >= pass && rows >= min_rows && n_chunks >= min_chunks)) return false;
    // what this try and pick_window_elems write (n_seg: it zeroes a multi-band plan's), to put back if the try fails;
    // a budget that holds the band and the chunk never reaches the several-band search, so the bands stay as they are
    const int threads = p.block_threads, bytes = p.window_bytes, elems = p.window_elems, n_seg = p.n_seg;
    const int64_t rows_per_chunk = p.rows_per_chunk;
    const bool from_band = p.window_from_band;
    p.block_threads = block_threads;
    p.rows_per_chunk = rows;
    p.window_bytes = int(val_bytes * (band + rows + 8));
    p.window_elems = pick_window_elems(p, probe, rows);
    if (one_band_window(p)) return true;
    p.block_threads = threads; p.rows_per_chunk = rows_per_chunk; p.window_bytes = bytes; p.window_elems = elems;
    p.n_seg = n_seg; p.window_from_band = from_band;   // (several bands etc.: keep the 256-thread plan)
    return false;
}

// VECTOR / LIGHT: workgroup size, rows per chunk and the window of x.  div = the kind's chunk divisor (LIGHT's tuning knob).
// Workgroup size: 512 threads own a chunk twice as long (64 K nonzeros) — the window of x is staged half as
// often per row and 2 x 8 waves sit on a CU instead of 3 x 4 (LDS-bound either way): 190 -> 178 us on the
// S32-band target (LIGHT: 199 -> 195 us once its kernel is held to 128 VGPRs; at 151 only one such workgroup
// fits a CU and it lost, 237 us).
static void shape_chunks(Plan& p, ProbeSamples& probe, int64_t div) {
    const bool force = p.knob.block > 0;
    if (!force || p.knob.block == kWideBlock) {   // (the knob cannot force a workgroup size the kind has no kernel for)
        // (3 072- and 3 584-row chunks with 79 KB of LDS measured worse: 189-194 vs 180 us)
        const int64_t rows_before_rounding = shape_for_block(p, probe, div, kWideBlock, 65536);
        if (keep_wide_block(p, probe, div, force, rows_before_rounding)) return;
    }
    shape_for_block(p, probe, div, kBlock, 32768);
    if (force || !p.probe_ok || p.knob.window >= 0 || p.knob.rows_per_chunk > 0 || one_band_window(p)) return;
    // (several bands with two 512-thread workgroups of 78 KB per CU and 1 664-row chunks: measured 722 vs 700 us on the
    // C4 stand-in — the 256-thread plan stays)
    // A band too wide for either budget (fp64 halves what 36 KB holds: the S32-band shape in fp64 ran on plain
    // gathers, 704 us): gfx950 lets a workgroup take more than the default 64 KB of LDS, and two workgroups of
    // 512 threads with ~78 KB each still fit a CU.  The chunk is then as long as the band leaves room for,
    // in at least one full round of the chip.
    if (try_wide_window(p, probe, kWideBlock, 78 * 1024, 256, int64_t(kCus) * 2 - 8, true)) return;
    // Still no window: the band is wider than two workgroups per CU can hold (round 1: every kind fell to the
    // plain-gather rate, 1.6-2.5 TB/s, once the band passed ~17 K columns in fp32 / ~9 K in fp64).  ONE workgroup
    // of 1 024 threads per CU can take ~155 of the CU's 160 KB: twice the band.  Its prologue is not hidden by a
    // neighbour, so this is only worth it where the alternative is the plain gather.
    if (p.window_elems == 0) try_wide_window(p, probe, kHugeBlock, 155 * 1024, 512, int64_t(kCus) * 2, false);
}

// VECTOR / LIGHT, after decide_balance said "equal-row chunks" and no window of x was found: the band is wider than one
// CU's LDS — let the window sweep it (chunk_rows_sweep).  A chunk is one group of rows of the 1 024-thread
// workgroup, every row one step of its vector (T from the longest row the probe saw), and the chunk's band is
// staged in `passes` windows.  Worth it while the staged bytes stay well below the line fills the same
// nonzeros cost as plain gathers (128 bytes each, some of them L1 hits).  MI355_SPMV_SWEEP=0|1 forces the choice.
static void shape_sweep(Plan& p) {
    p.sweep = false;
    if (p.balanced || p.knob.block > 0 || !p.probe_ok || p.window_elems != 0 || p.knob.window >= 0 ||
        p.knob.rows_per_chunk > 0 || p.knob.sweep == 0 || p.probe_len_max <= 0 || p.probe_len_max > 4 * kWave)
        return;
    const int64_t val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const int64_t band = p.band_hi - p.band_lo + 1;
    int t = p.lanes_per_row;
    while (t < kWave && 4 * t < p.probe_len_max) t *= 2;
    const int64_t rows = int64_t(kHugeBlock / t) * sweep_rows_for(p.val_type, t);
    const int64_t fixed = int64_t(chunk_lds_bytes(0, int(rows), size_t(val_bytes)));
    const int64_t cap = sweep_window_cap(val_bytes, fixed);
    const int64_t span = band + rows + 8;
    const int64_t passes = cap > 0 ? (span + cap - 1) / cap : 0;
    const int64_t mean = p.n_rows > 0 ? (p.nnz - p.nnz_begin) / p.n_rows : 0;
    const int64_t n_chunks = (p.n_rows + rows - 1) / rows;
    const bool pays = span * val_bytes <= 64 * mean * rows;     // staged bytes vs half the gathers' line fills
    if (!(band > 0 && passes >= 1 && passes <= 16 && n_chunks >= int64_t(kCus) * 2 && (pays || p.knob.sweep == 1))) return;
    p.sweep = true;
    p.lanes_per_row = t;
    p.block_threads = kHugeBlock;
    p.rows_per_chunk = rows;
    p.rows_cap = int(rows);
    p.n_chunks = n_chunks;
    p.window_bytes = int(cap * val_bytes);
    p.window_elems = int(cap);
    p.window_from_band = true;
    p.n_seg = 0;
}

// LIGHT: workgroups that stay resident on the chip.  A swept plan's: one per CU.  Otherwise bounded by LDS (160 KB: the
// chunk's layout + ~1 KB static) and by registers (3 workgroups of 256 threads, 2 of 512).  Asking for more than fits
// leaves the surplus workgroups to start when the others have finished everything (4 asked / 3 resident: 207 vs 200 us).
static int64_t light_resident(const Plan& p) {
    if (p.sweep) return kCus;
    if (p.knob.light_blocks_per_cu > 0) return int64_t(kCus) * p.knob.light_blocks_per_cu;
    const size_t val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;
    const size_t lds = chunk_lds_bytes(p.window_elems, p.balanced ? p.rows_cap : int(p.rows_per_chunk), val_bytes) + 1024;
    int64_t per_cu = int64_t(160 * 1024 / lds);
    const int64_t reg_bound = workgroups_per_cu_by_registers(p);
    if (per_cu > reg_bound) per_cu = reg_bound;
    if (per_cu < 1) per_cu = 1;
    return int64_t(kCus) * per_cu;
}

// VECTOR / LIGHT: the launch that follows from the plan's shape — the kernel, its grid and the number of kernels — for
// whole plans (end of shape_rows) and for row-block plans (after they inherit the whole plan's shape and find their
// giant rows).
void set_rows_launch(Plan& p) {
    p.n_tiles = p.n_chunks;
    p.n_kernels = p.n_giant > 0 ? 3 : 1;   // (+ the giant rows' slices and their sums)
    p.light_dequeue_once = false;
    const char* kernel;
    if (p.small_plain) {   // either kind: the plain CSR-vector kernel over the plan's rows, no window
        p.window_elems = 0;
        p.n_seg = 0;
        const int64_t rows_per_block = kBlock / p.lanes_per_row;
        p.grid_blocks = (int64_t(p.n_rows) + rows_per_block - 1) / rows_per_block;
        kernel = "csr_vector_kernel";
    } else if (p.kind == MI355_KIND_LIGHT) {
        // Equal-row chunks: one workgroup per chunk, which takes the chunk of its index while there are at most two
        // chunks per workgroup slot and makes one dequeue beyond.  Weight-cut chunks: the same up to two per slot (the
        // dequeue — two dependent atomics and a poll per workgroup — then costs more than it can balance away), else
        // the persistent grid of what stays resident.
        const int64_t resident = light_resident(p);
        p.grid_blocks = (!p.balanced || p.n_chunks <= 2 * resident) ? p.n_chunks : resident;
        p.light_dequeue_once = !p.balanced && p.n_chunks > 2 * resident;
        kernel = p.sweep ? "light_rows_sweep_kernel" : "light_rows_window_kernel";
    } else {
        p.grid_blocks = p.n_chunks;
        kernel = p.sweep ? "csr_vector_sweep_kernel" : "csr_vector_window_kernel";
    }
    snprintf(p.main_kernel, sizeof(p.main_kernel), "%s", kernel);
}

// VECTOR / LIGHT, whole plans: lanes per row, chunks and window (shape_chunks), equal-row or weight-cut chunks
// (decide_balance), a window that sweeps a band too wide for one (shape_sweep), giant rows, the small-matrix rule, and
// the launch that follows (set_rows_launch).  Synchronises (decide_balance, find_giant_rows).
int shape_rows(Plan& p, ProbeSamples& probe, GiantRowList& giants) {
    p.lanes_per_row = pick_lanes_per_row(p.nnz - p.nnz_begin, p.n_rows, p.elems_per_lane);
    const int t = p.knob.lanes;                                // tuning knob
    if (t == 2 || t == 4 || t == 8 || t == 16 || t == 32 || t == 64) p.lanes_per_row = t;
    // LIGHT's chunks: VECTOR's size unless its knob divides them (halving them cost 6 % on the S32-band target: the
    // window of x is staged per chunk), never below one pass of the workgroup
    const int div = p.kind == MI355_KIND_LIGHT ? p.knob.light_chunk_div : 0;
    shape_chunks(p, probe, div > 0 ? div : 1);
    if (const int st = decide_balance(p)) return st;   // heaviest uniform chunk vs the mean
    if (p.balanced) {   // weight-cut chunks are sized for 256 threads, the window for the rows a chunk may hold
        p.block_threads = kBlock;
        p.window_bytes = kWindowBytes;
        p.window_elems = pick_window_elems(p, probe, p.rows_cap);
        if (p.n_seg >= 2) { p.window_elems = 0; p.n_seg = 0; }   // (the multi-band plan is sized for uniform chunks)
    }
    shape_sweep(p);
    if (const int st = find_giant_rows(p, giants)) return st;   // balanced plans: rows too long for one workgroup
    // a small, regular matrix: the plain one-pass kernel (common.hpp, kSmallPlainNnz)
    if (p.knob.small != 0 && p.knob.plain == 0 && !p.balanced && !p.sweep && p.n_giant == 0 && p.n_rows > 0 &&
        (p.nnz - p.nnz_begin) <= kSmallPlainNnz) {
        const int64_t mean = (p.nnz - p.nnz_begin) / p.n_rows;
        // lanes per row: two 4-byte elements per lane and row up to 32 per row, four beyond (measured: 32 per row 16 lanes
        // over 8 and 32; 64 per row 16 lanes over 32 and 64)
        const int64_t per_lane = mean <= 32 ? 2 : 4;
        int lanes = 2;
        while (lanes < kWave && per_lane * lanes < mean) lanes *= 2;
        p.small_plain = true;
        p.lanes_per_row = lanes;
        p.block_threads = kBlock;
    }
    set_rows_launch(p);
    return MI355_SPMV_OK;
}

// A VECTOR plan whose matrix is stored in 16 bits (capi.hip, plan_create_typed) keeps the fp32 plan's shape, but the
// 16-bit chunked kernels exist only for equal-row chunks with one window of x or none (csr_vector_h16.hip).  Every
// other shape — weight-cut chunks (with their giant rows), several bands, the swept window, a small matrix — runs the
// plain one-pass kernel with the shape's lanes per row, and the plan's report says so; the shape itself
// (export_rows_shape) stays the fp32 plan's.
bool half_matrix_chunked(const Plan& p) {
    return !p.small_plain && !p.sweep && !p.balanced && p.n_seg < 2 && p.n_giant == 0;
}

void set_half_matrix_launch(Plan& p) {
    if (half_matrix_chunked(p)) return;
    const int64_t rows_per_block = kBlock / p.lanes_per_row;
    p.grid_blocks = (int64_t(p.n_rows) + rows_per_block - 1) / rows_per_block;
    p.n_kernels = 1;
    snprintf(p.main_kernel, sizeof(p.main_kernel), "%s", "csr_vector_kernel");
}

// ---- a row block's inherited shape: out of the whole plan, into the block's ---------------------------------
// The two directions side by side: a field added to one belongs in the other.
void export_rows_shape(const Plan& p, mi355_spmv_plan_shape* sh) {
    memset(sh, 0, sizeof(*sh));
    sh->struct_bytes = int32_t(sizeof(*sh));
    sh->kind = p.kind; sh->off_type = p.off_type; sh->val_type = p.val_type;
    sh->n_rows = p.n_rows; sh->n_cols = p.n_cols; sh->nnz = p.nnz;
    sh->lanes_per_row = p.lanes_per_row; sh->elems_per_lane = p.elems_per_lane;
    sh->block_threads = p.block_threads > 0 ? p.block_threads : kBlock;
    sh->balanced_chunks = p.balanced ? 1 : 0;
    sh->rows_cap = p.rows_cap;
    sh->giant_rows_enabled = p.giant_enabled ? 1 : 0;
    sh->rows_per_chunk = p.rows_per_chunk; sh->n_chunks = p.n_chunks;
    sh->bal_k = p.bal_k; sh->bal_q = p.bal_q; sh->giant_len = p.giant_len;
    sh->window_elems = p.window_elems; sh->window_bytes = p.window_bytes;
    sh->window_from_band = p.window_from_band ? 1 : 0;
    sh->window_sweep = p.sweep ? 1 : 0;
    sh->small_plain = p.small_plain ? 1 : 0;
    sh->window_segments = p.n_seg >= 2 ? p.n_seg : (p.window_elems > 0 ? 1 : 0);
    sh->probe_ok = p.probe_ok ? 1 : 0;
    sh->long_steps = p.knob.long_steps;
    // bands in whole-matrix row numbering (a block plan stores them shifted by its first row)
    sh->band_lo = p.band_lo - p.block_row_begin; sh->band_hi = p.band_hi - p.block_row_begin;
    for (int i = 0; i < 4; ++i) { sh->seg_lo[i] = p.seg_lo[i] - p.block_row_begin; sh->seg_hi[i] = p.seg_hi[i] - p.block_row_begin; }
}

// p: the block's plan with its own sizes, types and arrays set (plan_create_impl).  VECTOR / LIGHT blocks take the
// launch shape of the whole matrix's plan so that every row is summed exactly as there.
int inherit_rows_shape(Plan& p, const mi355_spmv_plan_shape& w, const BlockSpec& blk) {
    if (w.struct_bytes != int32_t(sizeof(mi355_spmv_plan_shape)) || w.kind != p.kind || w.off_type != p.off_type ||
        w.val_type != p.val_type) {
        set_error("plan_create_block: the shape is of another kind / type / library version");
        return MI355_SPMV_EINVAL;
    }
    if (p.n_rows > 0 && ((blk.row_begin & 3) != 0 ||
                         (w.balanced_chunks == 0 && w.rows_per_chunk > 0 && blk.row_begin % w.rows_per_chunk != 0))) {
        set_error("plan_create_block: row_begin is not a chunk boundary of the whole plan");
        return MI355_SPMV_EINVAL;
    }
    p.is_block = true;
    // not the last block: the tail of its last row is read in whole 16-byte groups, as the whole plan reads it — but
    // never past the end of the whole arrays (a block that ends inside their last, partial group)
    if ((blk.nnz_begin_whole & ~int64_t(3)) + p.nnz < w.nnz)
        p.nnz_read = std::min((p.nnz + 3) & ~int64_t(3), w.nnz - (blk.nnz_begin_whole & ~int64_t(3)));
    p.block_row_begin = blk.row_begin;
    p.block_chunk_begin = blk.chunk_begin;
    p.lanes_per_row = w.lanes_per_row; p.elems_per_lane = w.elems_per_lane;
    p.block_threads = w.block_threads;
    p.balanced = w.balanced_chunks != 0;
    p.rows_cap = w.rows_cap;
    p.giant_enabled = w.giant_rows_enabled != 0;
    p.rows_per_chunk = w.rows_per_chunk;
    p.n_chunks = p.balanced ? blk.n_chunks
                            : (p.rows_per_chunk > 0 ? (int64_t(p.n_rows) + p.rows_per_chunk - 1) / p.rows_per_chunk : 0);
    if (p.n_chunks < 1) p.n_chunks = 1;
    p.bal_k = w.bal_k; p.bal_q = w.bal_q; p.giant_len = w.giant_len;
    p.block_weight_off = (blk.nnz_begin_whole - blk.phase) + w.bal_k * blk.row_begin;
    p.window_elems = w.window_elems; p.window_bytes = w.window_bytes;
    p.window_from_band = w.window_from_band != 0;
    p.sweep = w.window_sweep != 0;
    p.small_plain = w.small_plain != 0;
    p.n_seg = w.window_segments >= 2 ? w.window_segments : 0;
    p.probe_ok = w.probe_ok != 0;
    p.knob.long_steps = w.long_steps;          // (0 = the default rule, which depends on `balanced` only)
    // (column - row) bands were measured with whole-matrix row numbers; this plan's rows start at 0
    p.band_lo = w.band_lo + blk.row_begin; p.band_hi = w.band_hi + blk.row_begin;
    for (int i = 0; i < 4; ++i) { p.seg_lo[i] = w.seg_lo[i] + blk.row_begin; p.seg_hi[i] = w.seg_hi[i] + blk.row_begin; }
    return MI355_SPMV_OK;
}

}  // namespace mi355
