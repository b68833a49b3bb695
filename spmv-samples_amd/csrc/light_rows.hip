// light_rows.hip — kind LIGHT: dynamic row distribution (LightSpMV rebuilt for gfx950).
//
// Replaces include/spmv/LightSpMV.cuh:111-263 (csrDynamicVector / csrDynamicWarp)
// and its per-call setup (:266-316).  The idea kept from the reference: a
// persistent grid that fetches rows from a global atomic counter, so that rows of
// very different lengths balance across the chip.
//
// What changes for MI355X:
//  * the unit handed out by one atomic is a CHUNK of consecutive rows (equal row counts,
//    or equal weight on a power-law matrix: rows_plan.hip, decide_balance) taken by a
//    whole workgroup (the reference hands 1 row to a vector or 32/T rows to a warp,
//    LightSpMV.cuh:128-132, :205-209).  One returning device-scope atomic on a
//    single word saturates near 88 dequeues/us on this chip; 1 row per atomic would
//    cost ~10^5 us for 8.3 M rows.  A chunk also gives the workgroup a window of x
//    worth staging through LDS (xwindow.hpp), which is what lifts the gather limit;
//  * the counter is SHARDED: 8 counters, each on its own 128-byte line, each
//    covering one contiguous eighth of the chunks.  A workgroup starts on the shard of
//    its XCD (blockIdx % 8 shares an L2) and walks the other shards when its own
//    runs dry, so placement only affects speed, never results;
//  * lane 0 of the workgroup dequeues, the chunk index reaches the other waves
//    through LDS + barrier; all lanes stay in the loops and rows past the chunk are
//    predicated (the reference's warp-level kernel lets finished vectors leave a
//    loop whose siblings still shuffle, LightSpMV.cuh:212, :246, :260);
//  * the counters live in the plan's scratch, zeroed once at plan creation, and are
//    RE-ARMED BY THE KERNEL: the last workgroup to leave (a ninth counter counts the
//    leavers) stores zeros, so an execute is a single launch with no memset in front
//    of it and can be captured in a hipGraph (the reference mallocs, memsets and frees
//    the counter per call, LightSpMV.cuh:274-276, :314).  A plan therefore serves one
//    stream at a time;
//  * x is read with plain loads / the LDS window (no texture path on CDNA; the
//    reference's texture fetch, LightSpMV.cuh:59-88, has no counterpart).
//
// A chunk's way from its rows to the chunk body is the text VECTOR's kernels include (row_chunk_window.inc,
// row_chunk_sweep.inc), here behind opaque copies of the operand pointers; the single dequeue of equal-row chunks is
// light_dequeue_once, for the window and the sweep kernel.
//
// Exit condition: a workgroup drains its own shard, asks once which other shards still
// hold rows, visits those and leaves; a visit ends on the first dequeue at or past the
// shard's end, which every workgroup reaches whatever the interleaving, so the grid
// always drains.

#include <cstdlib>

#include "common.hpp"
#include "row_dot.hpp"
#include "row_launch.hpp"
#include "xwindow.hpp"

namespace mi355 {

constexpr int kCounterStride = 16;  // unsigned long long per 128-byte line

__device__ __forceinline__ unsigned long long wave_broadcast_u64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(v));
    const unsigned hi = __builtin_amdgcn_readfirstlane(unsigned(v >> 32));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}


// Bit s set = shard s still had rows to hand out a moment ago.  Called by a whole wave: lanes 0..7 read
// the eight counters with one returning atomic each, in flight together, so a workgroup whose own shard
// ran dry pays ONE round trip to learn which other shards are worth a visit instead of one failed
// dequeue (a dependent ~2 us round trip) per shard.  A counter only grows during an execute, so "dry" is
// final; a shard reported busy is visited and drained with ordinary dequeues.
__device__ __forceinline__ unsigned shards_with_rows(unsigned long long* __restrict__ counters, int64_t n_units) {
    int lane = threadIdx.x & (kWave - 1);
    // (opaque to the optimiser: the per-lane address and shard size below are loop invariants that it would
    // otherwise compute once, keep in VGPRs across the whole chunk body of the persistent loop, and spill)
    asm volatile("" : "+v"(lane));
    bool has = false;
    if (lane < kXcds) {
        const int64_t size = n_units * (lane + 1) / kXcds - n_units * lane / kXcds;
        has = int64_t(atomicAdd(&counters[lane * kCounterStride], 0ull)) < size;
    }
    return unsigned(__ballot(has)) & ((1u << kXcds) - 1u);
}

// The workgroup has made its last dequeue (on every shard it visited one returned past the shard's end,
// and the issuing thread waited for every returned value).  The last of the gridDim.x workgroups to get here re-arms
// the counters for the next execute.
__device__ __forceinline__ void light_leave(unsigned long long* __restrict__ counters) {
    __syncthreads();
    // Relaxed device-scope atomics are enough (and a fence here would write the XCD's L2 back, +10 us):
    // the counters are only ever touched by atomics, and this thread has consumed the value returned by
    // every dequeue it issued, so they all precede this increment.
    if (threadIdx.x == 0) {
        const unsigned long long left = atomicAdd(&counters[kXcds * kCounterStride], 1ull);
        if (left == gridDim.x - 1)
            for (int i = 0; i <= kXcds; ++i) atomicExch(&counters[i * kCounterStride], 0ull);
    }
}

// Equal-row chunks, one dequeue per workgroup (light_rows_window_kernel without ADAPT, light_rows_sweep_kernel): the
// workgroup's chunk, or -1.  static_mode: the chunk of its index, the counters are not touched.  Otherwise it starts on
// the shard of its XCD (neighbouring chunks share windows of x in that L2) and tries the other shards if that one is dry;
// there are exactly as many workgroups as chunks, so everybody finds one.  All threads call; s_got is the kernel's LDS word.
__device__ __forceinline__ int64_t light_dequeue_once(const ChunkMap& cmap, unsigned long long* __restrict__ counters,
                                                      unsigned long long& s_got, bool static_mode) {
    const int home = blockIdx.x % kXcds;
    int64_t chunk = -1;
    if (static_mode) {
        chunk = xcd_contiguous_id(blockIdx.x, gridDim.x);
        if (chunk >= cmap.n_chunks) chunk = -1;
    } else {
        for (int visit = 0; visit < kXcds && chunk < 0; ++visit) {   // (uniform over the workgroup)
            const int shard = (home + visit) % kXcds;
            const int64_t shard_begin = cmap.n_chunks * shard / kXcds;          // in chunks
            const int64_t shard_end = cmap.n_chunks * (shard + 1) / kXcds;
            if (threadIdx.x == 0) s_got = atomicAdd(&counters[shard * kCounterStride], 1ull);
            __syncthreads();
            const int64_t c = shard_begin + int64_t(wave_broadcast_u64(s_got));
            if (c < shard_end) chunk = c;
            __syncthreads();          // s_got read by all before the next shard's dequeue overwrites it
        }
    }
    return chunk;
}

// (512 threads: two workgroups per CU need 4 waves per SIMD, i.e. <= 128 VGPRs; 256 threads: three workgroups
// per CU need 3 waves per SIMD, <= 168 VGPRs.)  Like the CSR-vector kernel this one does not depend on the
// width of the row offsets: a chunk is walked with 32-bit offsets relative to its first nonzero.
template <int BLOCK, int T, int R, int NSEG, bool ADAPT, typename val_t>
__global__ __launch_bounds__(BLOCK, (BLOCK >= kWideBlock || R == 2 ? 4 : 3)) void light_rows_window_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz, const ApView Ap, const int32_t* __restrict__ Aj_arg,
    const val_t* __restrict__ Ax_arg, const val_t* __restrict__ x_arg, val_t* __restrict__ y_arg,
    unsigned long long* __restrict__ counters, ChunkMap cmap, int32_t window_cap, BandHint hint,
    SegmentPlan segs, val_t alpha, val_t beta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window | bounds | y | flags
    __shared__ int s_red[2];
    __shared__ unsigned long long s_got;
    __shared__ unsigned s_busy;
    ChunkScratch<val_t> scr(s_dyn, window_cap, cmap.rows_cap);
    scr.alpha = alpha;
    scr.beta = beta;
    scr.long_steps = cmap.long_steps;
    scr.giant_len = cmap.giant_len;
    // the body of one chunk (all threads; ends with the results swept to y)
    auto run_chunk = [&](int64_t rb, int64_t re) {
        // Opaque copies of the operand pointers, once per chunk: without them every per-thread address the chunk
        // body derives from a kernel argument is a loop invariant of the persistent loop, gets computed once up
        // front, lives in VGPRs across the whole body and is spilled (the same body in the one-chunk-per-workgroup
        // CSR-vector kernel needs ~130 VGPRs; here it needed more than 256).
        int zero = 0;
        asm volatile("" : "+v"(zero));
        zero = __builtin_amdgcn_readfirstlane(zero);     // (a scalar the optimiser cannot see through)
        const int32_t* Aj = Aj_arg + zero;
        const val_t* Ax = Ax_arg + zero;
        const val_t* x = x_arg + zero;
        val_t* y = y_arg + zero;
        using mat_t = val_t;
        constexpr bool PACKED = false, kBarrierAfterWide = true;
        const uint16_t* const Aj16 = nullptr;   // (VECTOR only: LIGHT plans hold no packed index)
#include "row_chunk_window.inc"
    };
    // static_mode — few chunks per workgroup slot (small matrices): there is nothing to balance, every workgroup
    // takes the chunk of its index and the counters are not touched (the dequeue costs two dependent atomics
    // and a shard poll per workgroup: 32 vs 14 us on 2^17 rows).
    const bool static_mode = cmap.n_chunks <= int64_t(gridDim.x) && !cmap.dequeue_once;
    if constexpr (!ADAPT) {
        // Equal-row chunks (uniform matrices): ONE dequeue per workgroup, as many workgroups as chunks.  The
        // rows are still handed out by the global counters in arrival order — LightSpMV's scheme — but the loop
        // that keeps a persistent workgroup alive is the hardware dispatcher's: the body then compiles like the
        // CSR-vector kernel's (no loop-carried state: 127 instead of 168+ VGPRs, so the 512-thread plan fits
        // two workgroups per CU), and chunks of equal cost need no stealing.
        const int64_t chunk = light_dequeue_once(cmap, counters, s_got, static_mode);
        if (chunk >= 0) {
            int64_t chunk_begin, chunk_end;
            cmap.range(chunk, n_rows, chunk_begin, chunk_end);
            if (chunk_begin < chunk_end) run_chunk(chunk_begin, chunk_end);
        }
        if (!static_mode) light_leave(counters);
        return;
    } else {
    // Weight-cut chunks (power-law matrices): a PERSISTENT grid that keeps dequeuing, own shard first, then the
    // shards that still hold chunks — chunks of the same weight take different times (2 000 near-empty rows vs
    // 100 long ones), and stealing across the XCDs' shards is what balances them (R-MAT-24: 2.6 ms against
    // 3.7 ms for one workgroup per chunk in index order).
    // ONE loop with ONE call of the chunk body (two call sites made the compiler keep the body as a real
    // function for the biggest instantiations: captures through scratch memory, a call per chunk).  Its dequeue is its
    // own text, not light_dequeue_once: it goes on from the shard it stopped at and asks once which others are busy.
    const int home = blockIdx.x % kXcds;
    unsigned busy = 1u << home;
    int visit = 0;
    bool took_static = false;
    for (;;) {
        int64_t chunk = -1;
        if (static_mode) {
            if (took_static) break;
            took_static = true;
            chunk = xcd_contiguous_id(blockIdx.x, gridDim.x);
            if (chunk >= cmap.n_chunks) break;
        } else {
            while (visit < kXcds) {                              // (everything here is uniform over the workgroup)
                const int shard = (home + visit) % kXcds;
                if ((busy >> shard) & 1u) {
                    const int64_t shard_begin = cmap.n_chunks * shard / kXcds;          // in chunks
                    const int64_t shard_end = cmap.n_chunks * (shard + 1) / kXcds;
                    if (threadIdx.x == 0) s_got = atomicAdd(&counters[shard * kCounterStride], 1ull);
                    __syncthreads();
                    const int64_t c = shard_begin + int64_t(wave_broadcast_u64(s_got));
                    if (c < shard_end) { chunk = c; break; }
                    __syncthreads();      // s_got read by all before the next shard's dequeue overwrites it
                }
                ++visit;
                if (visit == 1) {         // own shard dry: ask the others once, all at the same time
                    if (threadIdx.x < kWave) {
                        const unsigned b = shards_with_rows(counters, cmap.n_chunks);
                        if (threadIdx.x == 0) s_busy = b;
                    }
                    __syncthreads();
                    // (LDS contents are the same for every lane, but the compiler cannot know: a VGPR here would
                    // make the branches on `busy` divergent)
                    busy = __builtin_amdgcn_readfirstlane(s_busy);
                }
            }
            if (chunk < 0) break;
        }
        int64_t chunk_begin, chunk_end;
        cmap.range(chunk, n_rows, chunk_begin, chunk_end);
        if (chunk_begin >= chunk_end) {   // a hub row heavier than a chunk leaves empty chunks behind it
            __syncthreads();              // s_got read by all before the next dequeue overwrites it
            continue;
        }
        run_chunk(chunk_begin, chunk_end);
        __syncthreads();                  // every wave is done with the window before it is refilled
    }
    if (!static_mode) light_leave(counters);
    }
}

// 4-byte-per-lane form for operands that are not 16-byte aligned: one dequeue per wave.
template <int T, typename off_t, typename val_t>
__global__ __launch_bounds__(kBlock) void light_rows_kernel(
    int32_t n_rows, off_t nnz, const off_t* __restrict__ Ap, const int32_t* __restrict__ Aj,
    const val_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y,
    unsigned long long* __restrict__ counters, int32_t rows_per_chunk, val_t alpha, val_t beta) {
    constexpr int ROWS_PER_STEP = kWave / T;
    const int lane64 = threadIdx.x & (kWave - 1);
    const int lane = threadIdx.x & (T - 1);
    const int vec_in_wave = lane64 / T;
    const int home = blockIdx.x % kXcds;
    unsigned busy = 1u << home;
    for (int visit = 0; visit < kXcds; ++visit) {
        const int shard = (home + visit) % kXcds;
        if (visit == 1) busy = shards_with_rows(counters, n_rows);   // (this kernel's unit is the row)
        if (!((busy >> shard) & 1u)) continue;      // wave-uniform
        const int64_t shard_begin = int64_t(n_rows) * shard / kXcds;
        const int64_t shard_end = int64_t(n_rows) * (shard + 1) / kXcds;
        while (true) {
            unsigned long long got = 0;
            if (lane64 == 0) {
                got = atomicAdd(&counters[shard * kCounterStride], (unsigned long long)rows_per_chunk);
            }
            got = wave_broadcast_u64(got);
            const int64_t chunk_begin = shard_begin + int64_t(got);
            if (chunk_begin >= shard_end) break;  // wave-uniform
            const int64_t chunk_end = min(chunk_begin + rows_per_chunk, shard_end);
            for (int64_t base = chunk_begin; base < chunk_end; base += ROWS_PER_STEP) {
                const int64_t row = base + vec_in_wave;
                const bool live = row < chunk_end;
                off_t start = 0, end = 0;
                if (live) {
                    start = Ap[row];
                    end = Ap[row + 1];
                }
                val_t sum = row_partial<T, off_t, val_t>(start, end, lane, Aj, Ax, x);
                sum = vector_reduce<T, val_t>(sum);
                if (live && lane == 0) y[row] = (beta != val_t(0)) ? alpha * sum + beta * y[row] : alpha * sum;
            }
        }
    }
    light_leave(counters);
}

// The band is wider than any window of x (xwindow.hpp, chunk_rows_sweep; csr_vector.hip has the static twin): one
// 1 024-thread workgroup per CU, a chunk = one group of rows held in registers, handed out by the counters exactly
// as the equal-row chunks of light_rows_window_kernel are (one dequeue per workgroup).
template <int T, int R, typename val_t>
__global__ __launch_bounds__(kHugeBlock, 4) void light_rows_sweep_kernel(
    int32_t n_rows, int32_t n_cols, int64_t nnz, const ApView Ap, const int32_t* __restrict__ Aj,
    const val_t* __restrict__ Ax, const val_t* __restrict__ x, val_t* __restrict__ y,
    unsigned long long* __restrict__ counters, ChunkMap cmap, int32_t window_cap, BandHint hint, val_t alpha, val_t beta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // window | bounds | y | flags
    __shared__ unsigned long long s_got;
    ChunkScratch<val_t> scr(s_dyn, window_cap, cmap.rows_cap);
    scr.alpha = alpha;
    scr.beta = beta;
    const bool static_mode = cmap.n_chunks <= int64_t(gridDim.x) && !cmap.dequeue_once;
    const int64_t chunk = light_dequeue_once(cmap, counters, s_got, static_mode);
    int64_t rb = 0, re = 0;
    if (chunk >= 0) cmap.range(chunk, n_rows, rb, re);
    if (rb < re) {
#include "row_chunk_sweep.inc"
    }
    if (!static_mode) light_leave(counters);
}

// LIGHT's kernels for the launch path it shares with VECTOR (row_launch.hpp): chunks handed out by the counters
struct LightRows {
    static constexpr const char* name = "light_rows";
    static constexpr bool kCounters = true;
    static constexpr bool kPlainKnob = false;
    template <int BLOCK, int T, int R, int NSEG, bool ADAPT, typename val_t>
    static auto window() { return light_rows_window_kernel<BLOCK, T, R, NSEG, ADAPT, val_t>; }
    static constexpr bool kPackedIndex = false;   // (VECTOR only: LIGHT plans hold no packed index)
    template <int T, int R, typename val_t>
    static auto sweep() { return light_rows_sweep_kernel<T, R, val_t>; }
    // unaligned operands: light_rows_kernel on the plan's grid, a dequeue of rows_per_chunk rows per wave
    template <typename off_t, typename val_t>
    static int plain(const Plan& p, const off_t* Ap, const val_t* Ax, const val_t* x, val_t* y, hipStream_t s) {
        return with_lanes(p, name, [&](auto lanes) -> int {
            constexpr int T = decltype(lanes)::value;
            hipLaunchKernelGGL((light_rows_kernel<T, off_t, val_t>), dim3((unsigned)p.grid_blocks), dim3(kBlock), 0, s, p.n_rows,
                               (off_t)p.nnz, Ap, p.Aj, Ax, x, y, p.counters, (int32_t)p.rows_per_chunk, (val_t)p.alpha,
                               (val_t)p.beta);
            MI355_HIP_TRY(hipGetLastError());
            return MI355_SPMV_OK;
        });
    }
};

// One translation unit per value type (light_rows_f64.hip includes this file with MI355_TU_F64).
#ifdef MI355_TU_PROBE      // (scripts: one kernel instantiated on its own to read its register use quickly)
#elif !defined(MI355_TU_F64)
template int launch_rows<LightRows, int32_t, float>(const Plan&, const int32_t*, const float*, const float*, float*, hipStream_t);
template int launch_rows<LightRows, int64_t, float>(const Plan&, const int64_t*, const float*, const float*, float*, hipStream_t);
#else
template int launch_rows<LightRows, int32_t, double>(const Plan&, const int32_t*, const double*, const double*, double*, hipStream_t);
template int launch_rows<LightRows, int64_t, double>(const Plan&, const int64_t*, const double*, const double*, double*, hipStream_t);
#endif

}  // namespace mi355
