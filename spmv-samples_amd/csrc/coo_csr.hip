// coo_csr.hip — COO -> CSR on the device with the result of the reference's ToCsr (include/load.hpp:420-474; the
// product's host twin is host/load.hpp ToCsr): Ap[r] = entries whose row is below r, entries of a row in their input
// order, duplicates kept, columns not sorted.  mi355_spmv_coo_to_csr (include/mi355_spmv.h) is the entry point.
//
// The row is the key of an LSD radix sort with the source index as its payload; the sort is stable, so the sorted
// payload is the CSR slot -> source index map (`perm`) and everything else is a gather through it.  Per pass of
// 8 bits (ceil(bit_width(n_rows - 1) / 8) passes: 0 for one row, 3 up to 2^24 rows) it is reduce-then-scan:
//   count_digits  each tile counts its 256 digits                          -> counts[digit][tile]
//   scan_*        an exclusive scan over that array, digit-major            -> where (digit, tile) starts
//   scatter       stable ranks inside the tile, the tile in digit order in LDS, then key and payload to their places
// Every kernel finishes on its own: no workgroup waits for another (no look-back, no grid barrier).  Stable ranks:
// the four waves of a tile each walk a contiguous quarter in steps of 64 entries, so (wave, step, lane) is source
// order; the lanes of one step that share a digit are found with 8 ballots, a lane's rank among them is the popcount
// of the peers below it, and a running count per (wave, digit) in LDS carries it from step to step.  No atomics: the
// order in which they land cannot reach the result.
//
// Validation runs first and records the smallest entry whose row or column is out of range; every later kernel reads
// that word and returns at once if it is set, so no index that failed the check is ever used as an address and the
// caller's output buffers are not written.
//
// mi355_spmv_coo_to_csr_symmetric takes the STORED entries of a `symmetric` Matrix Market file and gives ToCsr of what
// LoadCoo makes of them (reference include/load.hpp:362-403; host/load.hpp ExpandSymmetric): entry i, then its mirror
// if it is off the diagonal.  The expanded COO is never built: stored entry i goes to expanded place
// i + (off-diagonal entries before i), found by reduce-then-scan over tiles of stored entries (offdiag_count ->
// scan_sums -> expand), and only the sort's key (the row) and payload (2 i + mirror bit) are written there; the last
// gather reads cols[i] or rows[i] by the bit, and vals[i], from the stored arrays.  check_count compares the true
// expanded count with the caller's before anything is sized by it and stops every later kernel through the same word
// the validation uses.
//
// mi355_spmv_csr_transpose gives the structure of A^T from the CSR structure of A by the same sort with the COLUMN as key
// and the CSR slot as payload: Apt from the sorted keys, perm = the sorted payload, and Ajt = each slot's
// row, found in Ap by slot_rows.  Inside a column the slots ascend: the sort is stable.
#include "common.hpp"

namespace mi355 {
namespace coo {

constexpr int kSteps = 16;                        // 64-entry steps a wave walks per tile
constexpr int kTile = kBlock * kSteps;             // 4 096 entries per tile
constexpr int kScanItems = 16;                     // counts a thread of the scan kernels sums
constexpr int kScanChunk = kBlock * kScanItems;   // counts per workgroup of the scan kernels
constexpr unsigned long long kNoBad = ~0ull;
constexpr unsigned long long kBadCount = ~0ull - 1;   // symmetric: nnz_expanded is not the true count (no entry index gets here: nnz < 2^32)

constexpr size_t align_up(size_t v) { return (v + 255) / 256 * 256; }

inline int radix_passes(int32_t n_rows) {
    int bits = 0;
    for (uint32_t m = n_rows > 1 ? uint32_t(n_rows - 1) : 0u; m; m >>= 1) ++bits;
    return (bits + 7) / 8;
}

// Workspace: the validation word, two key and two payload buffers (one of each for a single pass), the tile counts
// and the scan's per-workgroup sums.
struct Layout {
    int passes = 0;
    uint64_t n_tiles = 0, n_counts = 0, n_scan_blocks = 0;
    size_t o_keys[2] = {0, 0}, o_pay[2] = {0, 0}, o_counts = 0, o_bsum = 0, bytes = 0;
};

// both_pairs: two buffer pairs for a single pass too (the symmetric call sorts out of a buffer of its own making).
inline Layout layout(int32_t n_rows, uint64_t nnz, bool both_pairs = false) {
    Layout L;
    L.passes = nnz ? radix_passes(n_rows) : 0;
    size_t off = 256;   // the validation word
    if (L.passes > 0) {
        L.n_tiles = (nnz + kTile - 1) / kTile;
        L.n_counts = 256 * L.n_tiles;
        L.n_scan_blocks = (L.n_counts + kScanChunk - 1) / kScanChunk;
        const int bufs = L.passes > 1 || both_pairs ? 2 : 1;
        for (int b = 0; b < bufs; ++b) {
            L.o_keys[b] = off; off = align_up(off + 4 * nnz);
            L.o_pay[b] = off;  off = align_up(off + 4 * nnz);
        }
        L.o_counts = off; off = align_up(off + 4 * L.n_counts);
        L.o_bsum = off;   off = align_up(off + 4 * L.n_scan_blocks);
    }
    L.bytes = off;
    return L;
}

__global__ void __launch_bounds__(kBlock) validate(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                   uint64_t nnz, uint32_t n_rows, uint32_t n_cols,
                                                   unsigned long long* bad) {
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += stride)
        if (uint32_t(rows[k]) >= n_rows || uint32_t(cols[k]) >= n_cols) atomicMin(bad, (unsigned long long)k);
}

// Digits of one wave's quarter of a tile: cnt[wave][digit] ends as the wave's count of each digit.  With RANKS, rank[s]
// is the entry's place among the wave's entries of its digit, in source order.  `keys` is the tile's first entry.
template <bool RANKS>
__device__ inline void wave_digits(const uint32_t* __restrict__ keys, uint64_t n_left, int shift, uint32_t (*cnt)[256],
                                   uint32_t* key, uint32_t* rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    const uint64_t first = uint64_t(wave) * kSteps * 64 + lane;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t i = first + uint64_t(s) * 64;
        key[s] = i < n_left ? keys[i] : 0u;
    }
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const bool valid = first + uint64_t(s) * 64 < n_left;
        const uint32_t d = (key[s] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const uint32_t before = cnt[wave][d];
        const uint32_t r = uint32_t(__popcll(peers & below));
        if (RANKS) rank[s] = before + r;
        // the last of the peers advances the count; every lane has read it above, in this wave's program order
        if (valid && (peers >> lane) == 1ull) cnt[wave][d] = before + r + 1;
    }
}

// Upsweep: counts[digit * n_tiles + tile] = entries of the tile with that digit.
__global__ void __launch_bounds__(kBlock) count_digits(const uint32_t* __restrict__ keys, uint64_t nnz, int shift,
                                                       uint64_t n_tiles, uint32_t* __restrict__ counts,
                                                       const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    __shared__ uint32_t cnt[4][256];
    for (int i = threadIdx.x; i < 4 * 256; i += kBlock) cnt[i >> 8][i & 255] = 0;
    __syncthreads();
    const uint64_t base = uint64_t(blockIdx.x) * kTile;
    uint32_t key[kSteps];
    wave_digits<false>(keys + base, nnz - base, shift, cnt, key, nullptr);
    __syncthreads();
    const int d = threadIdx.x;
    counts[uint64_t(d) * n_tiles + blockIdx.x] = cnt[0][d] + cnt[1][d] + cnt[2][d] + cnt[3][d];
}

// Exclusive scan of `count` per-thread items held in v[], over the workgroup; returns the workgroup total.
__device__ inline uint32_t block_exclusive_scan(uint32_t* v, int count) {
    __shared__ uint32_t wave_sum[4];
    uint32_t own = 0;
    for (int i = 0; i < count; ++i) { const uint32_t t = v[i]; v[i] = own; own += t; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t before = inc - own, total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    __syncthreads();   // wave_sum is reused by the next call
    for (int i = 0; i < count; ++i) v[i] += before;
    return total;
}

// Reduce: bsum[b] = sum of the counts of scan workgroup b.
__global__ void __launch_bounds__(kBlock) scan_reduce(const uint32_t* __restrict__ counts, uint64_t n,
                                                      uint32_t* __restrict__ bsum, const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    __shared__ uint32_t part[kBlock / 64];
    const uint64_t base = uint64_t(blockIdx.x) * kScanChunk;
    uint32_t s = 0;
    for (int i = 0; i < kScanItems; ++i) {
        const uint64_t k = base + uint64_t(i) * kBlock + threadIdx.x;
        if (k < n) s += counts[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// One workgroup: exclusive scan of the per-workgroup sums, in place, in chunks with a running carry.
__global__ void __launch_bounds__(kBlock) scan_sums(uint32_t* bsum, uint64_t n, const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < n; base += kScanChunk) {
        uint32_t v[kScanItems];
        const uint64_t first = base + uint64_t(threadIdx.x) * kScanItems;
        for (int i = 0; i < kScanItems; ++i) v[i] = first + i < n ? bsum[first + i] : 0u;
        const uint32_t total = block_exclusive_scan(v, kScanItems);
        for (int i = 0; i < kScanItems; ++i)
            if (first + i < n) bsum[first + i] = v[i] + carry;
        carry += total;
    }
}

// Apply: the counts of scan workgroup b become their exclusive prefix, starting at bsum[b].
__global__ void __launch_bounds__(kBlock) scan_apply(uint32_t* counts, uint64_t n, const uint32_t* __restrict__ bsum,
                                                     const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    const uint64_t first = uint64_t(blockIdx.x) * kScanChunk + uint64_t(threadIdx.x) * kScanItems;
    uint32_t v[kScanItems];
    for (int i = 0; i < kScanItems; ++i) v[i] = first + i < n ? counts[first + i] : 0u;
    (void)block_exclusive_scan(v, kScanItems);
    const uint32_t carry = bsum[blockIdx.x];
    for (int i = 0; i < kScanItems; ++i)
        if (first + i < n) counts[first + i] = v[i] + carry;
}

// Downsweep: each entry of the tile goes to start(digit, tile) + entries of that digit before it in the tile.  The
// tile is first put in digit order in LDS, so that consecutive lanes write consecutive places of a digit's run (a
// store instruction then touches a few runs, not up to 64 of them).  pay_in == nullptr: the payload is the source
// index (the first pass).
__global__ void __launch_bounds__(kBlock) scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ pay_in,
                                                  uint64_t nnz, int shift, uint64_t n_tiles,
                                                  const uint32_t* __restrict__ starts, uint32_t* __restrict__ keys_out,
                                                  uint32_t* __restrict__ pay_out, const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    __shared__ uint32_t cnt[4][256];
    __shared__ uint32_t digit_at[256];    // where digit d's run starts in the tile, in digit order
    __shared__ uint32_t digit_out[256];   // ... and in the output
    __shared__ uint32_t staged_key[kTile], staged_pay[kTile];
    for (int i = threadIdx.x; i < 4 * 256; i += kBlock) cnt[i >> 8][i & 255] = 0;
    __syncthreads();
    const uint64_t base = uint64_t(blockIdx.x) * kTile;
    const uint64_t n_left = nnz - base;
    uint32_t key[kSteps], rank[kSteps];
    wave_digits<true>(keys_in + base, n_left, shift, cnt, key, rank);
    __syncthreads();
    {   // cnt[w][d] becomes where wave w's entries of digit d start inside the digit's run
        const int d = threadIdx.x;
        uint32_t total = 0;
        for (int w = 0; w < 4; ++w) { const uint32_t c = cnt[w][d]; cnt[w][d] = total; total += c; }
        (void)block_exclusive_scan(&total, 1);
        digit_at[d] = total;
        digit_out[d] = starts[uint64_t(d) * n_tiles + blockIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t first = uint64_t(wave) * kSteps * 64 + lane;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t i = first + uint64_t(s) * 64;
        if (i < n_left) {
            const uint32_t d = (key[s] >> shift) & 255u;
            const uint32_t at = digit_at[d] + cnt[wave][d] + rank[s];
            staged_key[at] = key[s];
            staged_pay[at] = pay_in ? pay_in[base + i] : uint32_t(base + i);
        }
    }
    __syncthreads();
    const uint32_t n_here = n_left < kTile ? uint32_t(n_left) : uint32_t(kTile);
    for (uint32_t i = threadIdx.x; i < n_here; i += kBlock) {
        const uint32_t k = staged_key[i];
        const uint32_t d = (k >> shift) & 255u;
        const uint32_t dst = digit_out[d] + (i - digit_at[d]);
        keys_out[dst] = k;
        pay_out[dst] = staged_pay[i];
    }
}

// Ap[r] = first place of a key >= r in the sorted keys (keys == nullptr: every key is 0, one row).
template <typename off_t>
__global__ void __launch_bounds__(kBlock) row_offsets(const uint32_t* __restrict__ keys, uint64_t nnz, uint32_t n_rows,
                                                      off_t* __restrict__ Ap, const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x; r <= n_rows; r += stride) {
        uint64_t lo = 0, hi = nnz;
        if (!keys) {
            lo = r == 0 ? 0 : nnz;
        } else {
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (keys[mid] < r) lo = mid + 1; else hi = mid;
            }
        }
        Ap[r] = off_t(lo);
    }
}

// Aj[k] = cols[perm[k]], Ax[k] = vals[perm[k]] (elem_t: the value's bits), perm out as int64 if asked for.
// pay == nullptr: the identity (no pass ran).
template <typename elem_t>
__global__ void __launch_bounds__(kBlock) gather(const uint32_t* __restrict__ pay, uint64_t nnz,
                                                 const int32_t* __restrict__ cols, const elem_t* __restrict__ vals,
                                                 int32_t* __restrict__ Aj, elem_t* __restrict__ Ax,
                                                 int64_t* __restrict__ perm, const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += stride) {
        const uint64_t p = pay ? pay[k] : k;
        Aj[k] = cols[p];
        if (Ax) Ax[k] = vals[p];
        if (perm) perm[k] = int64_t(p);
    }
}

// ---- symmetric: the stored entries of a `symmetric` file -------------------------------------------------------
// The sort's workspace for nnz_expanded entries, then one count per tile of stored entries (+ 1: the total).
struct SymLayout {
    Layout sort;
    uint64_t n_etiles = 0;
    size_t o_esum = 0, bytes = 0;
};

inline SymLayout sym_layout(int32_t n_rows, uint64_t nnz_stored, uint64_t nnz_expanded) {
    SymLayout S;
    S.sort = layout(n_rows, nnz_expanded, true);
    S.n_etiles = (nnz_stored + kTile - 1) / kTile;
    S.o_esum = S.sort.bytes;
    S.bytes = align_up(S.o_esum + 4 * (S.n_etiles + 1));
    return S;
}

// The mirror (col, row) is stored too: both indices inside both dimensions (the loader's rule, host/load.hpp).
__global__ void __launch_bounds__(kBlock) validate_symmetric(const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ cols, uint64_t nnz,
                                                             uint32_t n_square, unsigned long long* bad) {
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += stride)
        if (uint32_t(rows[k]) >= n_square || uint32_t(cols[k]) >= n_square) atomicMin(bad, (unsigned long long)k);
}

// Reduce: esum[t] = off-diagonal entries of tile t of the stored entries (0 for the one workgroup past the last tile,
// which the exclusive scan turns into the total).  Compares only: no index is used as an address.
__global__ void __launch_bounds__(kBlock) offdiag_count(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                        uint64_t nnz, uint32_t* __restrict__ esum) {
    __shared__ uint32_t part[kBlock / 64];
    const uint64_t base = uint64_t(blockIdx.x) * kTile;
    uint32_t s = 0;
    for (int i = 0; i < kSteps; ++i) {
        const uint64_t k = base + uint64_t(i) * kBlock + threadIdx.x;
        if (k < nnz) s += rows[k] != cols[k];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) esum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// After the scan esum[n_etiles] is the number of off-diagonal entries.  word[1] = the true expanded count; if it is
// not the caller's, word[0] (the validation word) stops everything that follows.
__global__ void __launch_bounds__(kBlock) check_count(const uint32_t* __restrict__ esum, uint64_t n_etiles,
                                                      uint64_t nnz_stored, uint64_t nnz_expanded,
                                                      unsigned long long* word) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || word[0] != kNoBad) return;
    const unsigned long long expanded = nnz_stored + esum[n_etiles];
    word[1] = expanded;
    if (expanded != nnz_expanded) word[0] = kBadCount;
}

// Downsweep: stored entry i goes to expanded place i + (off-diagonal entries before it), its mirror right after it.
// The four waves each walk a contiguous quarter of the tile in steps of 64, as the sort does, so one ballot per step
// counts the off-diagonal entries before a lane.  Key = the row of the expanded entry, payload = 2 i + mirror.
__global__ void __launch_bounds__(kBlock) expand(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                 uint64_t nnz, const uint32_t* __restrict__ esum,
                                                 uint32_t* __restrict__ keys_out, uint32_t* __restrict__ pay_out,
                                                 const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    __shared__ uint32_t wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    const uint64_t base = uint64_t(blockIdx.x) * kTile;
    const uint64_t n_left = nnz - base;
    const uint64_t first = uint64_t(wave) * kSteps * 64 + lane;
    uint32_t r[kSteps], c[kSteps], before[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t i = first + uint64_t(s) * 64;
        r[s] = i < n_left ? uint32_t(rows[base + i]) : 0u;
        c[s] = i < n_left ? uint32_t(cols[base + i]) : 0u;   // (past the end: r == c, counts as nothing)
    }
    uint32_t run = 0;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const unsigned long long m = __ballot(r[s] != c[s]);
        before[s] = run + uint32_t(__popcll(m & below));
        run += uint32_t(__popcll(m));
    }
    if (lane == 0) wave_total[wave] = run;
    __syncthreads();
    uint64_t shift = base + esum[blockIdx.x];   // expanded place of the tile's first entry, minus its stored place
    for (int w = 0; w < wave; ++w) shift += wave_total[w];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t i = first + uint64_t(s) * 64;
        if (i < n_left) {
            const uint64_t at = shift + i + before[s];
            const uint32_t p = uint32_t(base + i) << 1;
            keys_out[at] = r[s];
            pay_out[at] = p;
            if (r[s] != c[s]) {
                keys_out[at + 1] = c[s];
                pay_out[at + 1] = p | 1u;
            }
        }
    }
}

// Aj[k] = cols[i] (rows[i] for a mirror), Ax[k] = vals[i], perm[k] = i, with 2 i + mirror = the sorted payload.
// pay == nullptr: the identity (no pass ran: at most one row, so no entry has a mirror).
template <typename elem_t>
__global__ void __launch_bounds__(kBlock) gather_symmetric(const uint32_t* __restrict__ pay, uint64_t nnz,
                                                           const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ cols,
                                                           const elem_t* __restrict__ vals, int32_t* __restrict__ Aj,
                                                           elem_t* __restrict__ Ax, int64_t* __restrict__ perm,
                                                           const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += stride) {
        const uint64_t p = pay ? pay[k] : k << 1;
        const uint64_t i = p >> 1;
        Aj[k] = (p & 1) ? rows[i] : cols[i];
        if (Ax) Ax[k] = vals[i];
        if (perm) perm[k] = int64_t(i);
    }
}

// Off-diagonal entries of the whole list (mi355_spmv_coo_symmetric_nnz): one integer add per wave, so the total does
// not depend on the order in which they land.
__global__ void __launch_bounds__(kBlock) offdiag_total(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                        uint64_t nnz, unsigned long long* total) {
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    uint32_t s = 0;
    for (uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += stride) s += rows[k] != cols[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, (unsigned long long)s);
}

inline unsigned grid_for(uint64_t items) {
    const uint64_t g = (items + kBlock - 1) / kBlock;
    return unsigned(g < 8192 ? (g ? g : 1) : 8192);
}

#define MI355_COO_LAUNCH(kernel, grid, ...)                     \
    do {                                                        \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, __VA_ARGS__); \
        MI355_HIP_TRY(hipGetLastError());                       \
    } while (0)

template <typename off_t>
static int run(const Layout& L, int val_bytes, int32_t n_rows, int32_t n_cols, uint64_t nnz, const int32_t* rows,
               const int32_t* cols, const void* vals, void* Ap, int32_t* Aj, void* Ax, int64_t* perm, char* ws,
               hipStream_t s) {
    auto* bad = reinterpret_cast<unsigned long long*>(ws);
    MI355_HIP_TRY(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), s));
    if (nnz) MI355_COO_LAUNCH(validate, grid_for(nnz), rows, cols, nnz, uint32_t(n_rows), uint32_t(n_cols), bad);
    const uint32_t* keys = nullptr;
    const uint32_t* pay = nullptr;
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws + L.o_counts);
    uint32_t* bsum = reinterpret_cast<uint32_t*>(ws + L.o_bsum);
    for (int p = 0; p < L.passes; ++p) {
        const int shift = 8 * p;
        const uint32_t* keys_in = p == 0 ? reinterpret_cast<const uint32_t*>(rows) : keys;
        uint32_t* keys_out = reinterpret_cast<uint32_t*>(ws + L.o_keys[p & 1]);
        uint32_t* pay_out = reinterpret_cast<uint32_t*>(ws + L.o_pay[p & 1]);
        MI355_COO_LAUNCH(count_digits, unsigned(L.n_tiles), keys_in, nnz, shift, L.n_tiles, counts, bad);
        MI355_COO_LAUNCH(scan_reduce, unsigned(L.n_scan_blocks), counts, L.n_counts, bsum, bad);
        MI355_COO_LAUNCH(scan_sums, 1u, bsum, L.n_scan_blocks, bad);
        MI355_COO_LAUNCH(scan_apply, unsigned(L.n_scan_blocks), counts, L.n_counts, bsum, bad);
        MI355_COO_LAUNCH(scatter, unsigned(L.n_tiles), keys_in, pay, nnz, shift, L.n_tiles, counts, keys_out, pay_out, bad);
        keys = keys_out;
        pay = pay_out;
    }
    MI355_COO_LAUNCH(row_offsets<off_t>, grid_for(uint64_t(n_rows) + 1), keys, nnz, uint32_t(n_rows),
                     static_cast<off_t*>(Ap), bad);
    if (nnz) {
        if (val_bytes == 8)
            MI355_COO_LAUNCH(gather<uint64_t>, grid_for(nnz), pay, nnz, cols, static_cast<const uint64_t*>(vals), Aj,
                             static_cast<uint64_t*>(Ax), perm, bad);
        else
            MI355_COO_LAUNCH(gather<uint32_t>, grid_for(nnz), pay, nnz, cols, static_cast<const uint32_t*>(vals), Aj,
                             static_cast<uint32_t*>(Ax), perm, bad);
    }
    // the one synchronisation: the validation word
    unsigned long long first_bad = kNoBad;
    MI355_HIP_TRY(hipMemcpyAsync(&first_bad, bad, sizeof(first_bad), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if (first_bad != kNoBad) {
        int32_t r = 0, c = 0;
        MI355_HIP_TRY(hipMemcpy(&r, rows + first_bad, sizeof(r), hipMemcpyDeviceToHost));
        MI355_HIP_TRY(hipMemcpy(&c, cols + first_bad, sizeof(c), hipMemcpyDeviceToHost));
        set_error("coo_to_csr: entry %llu is (row %d, col %d), outside the %d x %d matrix", first_bad, r, c, n_rows,
                  n_cols);
        return MI355_SPMV_EINVAL;
    }
    return MI355_SPMV_OK;
}

template <typename off_t>
static int run_symmetric(const SymLayout& S, int val_bytes, int32_t n_rows, int32_t n_cols, uint64_t nnz_stored,
                         uint64_t nnz_expanded, const int32_t* rows, const int32_t* cols, const void* vals, void* Ap,
                         int32_t* Aj, void* Ax, int64_t* perm, char* ws, hipStream_t s) {
    const Layout& L = S.sort;
    auto* bad = reinterpret_cast<unsigned long long*>(ws);   // [0] the validation word, [1] the true expanded count
    uint32_t* esum = reinterpret_cast<uint32_t*>(ws + S.o_esum);
    MI355_HIP_TRY(hipMemsetAsync(bad, 0xff, 2 * sizeof(unsigned long long), s));
    if (nnz_stored)
        MI355_COO_LAUNCH(validate_symmetric, grid_for(nnz_stored), rows, cols, nnz_stored,
                         uint32_t(n_rows < n_cols ? n_rows : n_cols), bad);
    MI355_COO_LAUNCH(offdiag_count, unsigned(S.n_etiles + 1), rows, cols, nnz_stored, esum);
    MI355_COO_LAUNCH(scan_sums, 1u, esum, S.n_etiles + 1, bad);
    MI355_COO_LAUNCH(check_count, 1u, esum, S.n_etiles, nnz_stored, nnz_expanded, bad);
    uint32_t* keys_buf[2] = {reinterpret_cast<uint32_t*>(ws + L.o_keys[0]), reinterpret_cast<uint32_t*>(ws + L.o_keys[1])};
    uint32_t* pay_buf[2] = {reinterpret_cast<uint32_t*>(ws + L.o_pay[0]), reinterpret_cast<uint32_t*>(ws + L.o_pay[1])};
    const uint32_t* keys = nullptr;
    const uint32_t* pay = nullptr;
    if (L.passes > 0) {
        MI355_COO_LAUNCH(expand, unsigned(S.n_etiles), rows, cols, nnz_stored, esum, keys_buf[0], pay_buf[0], bad);
        keys = keys_buf[0];
        pay = pay_buf[0];
    }
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws + L.o_counts);
    uint32_t* bsum = reinterpret_cast<uint32_t*>(ws + L.o_bsum);
    for (int p = 0; p < L.passes; ++p) {
        const int shift = 8 * p;
        uint32_t* keys_out = keys_buf[(p + 1) & 1];
        uint32_t* pay_out = pay_buf[(p + 1) & 1];
        MI355_COO_LAUNCH(count_digits, unsigned(L.n_tiles), keys, nnz_expanded, shift, L.n_tiles, counts, bad);
        MI355_COO_LAUNCH(scan_reduce, unsigned(L.n_scan_blocks), counts, L.n_counts, bsum, bad);
        MI355_COO_LAUNCH(scan_sums, 1u, bsum, L.n_scan_blocks, bad);
        MI355_COO_LAUNCH(scan_apply, unsigned(L.n_scan_blocks), counts, L.n_counts, bsum, bad);
        MI355_COO_LAUNCH(scatter, unsigned(L.n_tiles), keys, pay, nnz_expanded, shift, L.n_tiles, counts, keys_out, pay_out, bad);
        keys = keys_out;
        pay = pay_out;
    }
    MI355_COO_LAUNCH(row_offsets<off_t>, grid_for(uint64_t(n_rows) + 1), keys, nnz_expanded, uint32_t(n_rows),
                     static_cast<off_t*>(Ap), bad);
    if (nnz_expanded) {
        if (val_bytes == 8)
            MI355_COO_LAUNCH(gather_symmetric<uint64_t>, grid_for(nnz_expanded), pay, nnz_expanded, rows, cols,
                             static_cast<const uint64_t*>(vals), Aj, static_cast<uint64_t*>(Ax), perm, bad);
        else
            MI355_COO_LAUNCH(gather_symmetric<uint32_t>, grid_for(nnz_expanded), pay, nnz_expanded, rows, cols,
                             static_cast<const uint32_t*>(vals), Aj, static_cast<uint32_t*>(Ax), perm, bad);
    }
    // the one synchronisation: the validation word and the true count
    unsigned long long word[2] = {kNoBad, 0};
    MI355_HIP_TRY(hipMemcpyAsync(word, bad, sizeof(word), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if (word[0] == kBadCount) {
        set_error("coo_to_csr_symmetric: nnz_expanded is %llu, the stored entries expand to %llu",
                  (unsigned long long)nnz_expanded, word[1]);
        return MI355_SPMV_EINVAL;
    }
    if (word[0] != kNoBad) {
        int32_t r = 0, c = 0;
        MI355_HIP_TRY(hipMemcpy(&r, rows + word[0], sizeof(r), hipMemcpyDeviceToHost));
        MI355_HIP_TRY(hipMemcpy(&c, cols + word[0], sizeof(c), hipMemcpyDeviceToHost));
        set_error("coo_to_csr_symmetric: entry %llu is (row %d, col %d); it or its mirror is outside the %d x %d matrix",
                  word[0], r, c, n_rows, n_cols);
        return MI355_SPMV_EINVAL;
    }
    return MI355_SPMV_OK;
}

}  // namespace coo
}  // namespace mi355

extern "C" int mi355_spmv_coo_to_csr(int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                                     const int32_t* rows, const int32_t* cols, const void* vals, void* Ap, int32_t* Aj,
                                     void* Ax, int64_t* perm, void* workspace, size_t* workspace_bytes, void* stream) {
    using namespace mi355;
    set_error("%s", "");
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("coo_to_csr: unknown offset type %d", off_type); return MI355_SPMV_EINVAL; }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64 && val_type != MI355_VAL_I32) { set_error("coo_to_csr: unknown value type %d", val_type); return MI355_SPMV_EINVAL; }
    if (n_rows < 0 || n_cols < 0 || nnz < 0) { set_error("coo_to_csr: negative size"); return MI355_SPMV_EINVAL; }
    if (off_type == MI355_OFF_I32 && nnz > INT32_MAX) { set_error("coo_to_csr: nnz does not fit 32-bit offsets (use 64-bit offsets)"); return MI355_SPMV_EINVAL; }
    if (uint64_t(nnz) >= (1ull << 32)) { set_error("coo_to_csr: 2^32 or more entries (the sort's payload is 32-bit)"); return MI355_SPMV_ENOTSUP; }
    if (!workspace_bytes) { set_error("coo_to_csr: null workspace_bytes"); return MI355_SPMV_EINVAL; }
    const coo::Layout L = coo::layout(n_rows, uint64_t(nnz));
    if (!workspace) { *workspace_bytes = L.bytes; return MI355_SPMV_OK; }
    if (*workspace_bytes < L.bytes) { set_error("coo_to_csr: workspace of %zu bytes, %zu needed", *workspace_bytes, L.bytes); return MI355_SPMV_EINVAL; }
    if (!Ap) { set_error("coo_to_csr: null Ap"); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && (!rows || !cols || !Aj)) { set_error("coo_to_csr: null rows, cols or Aj"); return MI355_SPMV_EINVAL; }
    if ((vals == nullptr) != (Ax == nullptr)) { set_error("coo_to_csr: Ax and vals must be both given or both null"); return MI355_SPMV_EINVAL; }
    const int val_bytes = val_type == MI355_VAL_F64 ? 8 : 4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    return off_type == MI355_OFF_I32
               ? coo::run<int32_t>(L, val_bytes, n_rows, n_cols, uint64_t(nnz), rows, cols, vals, Ap, Aj, Ax, perm, ws, s)
               : coo::run<int64_t>(L, val_bytes, n_rows, n_cols, uint64_t(nnz), rows, cols, vals, Ap, Aj, Ax, perm, ws, s);
}

// ---- the structure of A^T: a stable sort of the CSR slots by column ------------------------------------------------
namespace mi355 {
namespace coo {

constexpr unsigned long long kBadOffsets = ~0ull - 1;   // csr_transpose: Ap is not 0 .. nnz ascending (word[1] names the place)

// word[1] = the first i with Ap[i] out of order: Ap[0] != 0, Ap[i] < Ap[i - 1], or Ap[n_rows] != nnz (i = n_rows);
// word[0] then stops every later kernel.  Compares only: no offset is used as an address.
template <typename off_t>
__global__ void __launch_bounds__(kBlock) validate_offsets(const off_t* __restrict__ Ap, uint32_t n_rows, uint64_t nnz,
                                                           unsigned long long* word) {
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i <= n_rows; i += stride) {
        const bool bad = i == 0 ? Ap[0] != 0 : (Ap[i] < Ap[i - 1] || (i == n_rows && uint64_t(Ap[i]) != nnz));
        if (bad) {
            atomicMin(word + 1, (unsigned long long)i);
            atomicMin(word, kBadOffsets);
        }
    }
}

__global__ void __launch_bounds__(kBlock) validate_columns(const int32_t* __restrict__ Aj, uint64_t nnz, uint32_t n_cols,
                                                           unsigned long long* bad) {
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x; k < nnz; k += stride)
        if (uint32_t(Aj[k]) >= n_cols) atomicMin(bad, (unsigned long long)k);
}

// perm[t] = the CSR slot behind transposed slot t (the sorted payload; pay == nullptr: the identity, no pass ran) and
// Ajt[t] = that slot's row: the last r with Ap[r] <= slot (rows without entries are stepped over by the search).
template <typename off_t>
__global__ void __launch_bounds__(kBlock) slot_rows(const uint32_t* __restrict__ pay, uint64_t nnz, const off_t* __restrict__ Ap,
                                                    uint32_t n_rows, int32_t* __restrict__ Ajt, uint32_t* __restrict__ perm,
                                                    const unsigned long long* bad) {
    if (*bad != kNoBad) return;
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    for (uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x; t < nnz; t += stride) {
        const uint64_t p = pay ? pay[t] : t;
        uint32_t lo = 0, hi = n_rows;           // the first r in (0, n_rows] with Ap[r] > p, minus one
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (uint64_t(Ap[mid + 1]) <= p) lo = mid + 1; else hi = mid;
        }
        Ajt[t] = int32_t(lo);
        perm[t] = uint32_t(p);
    }
}

template <typename off_t>
static int run_transpose(const Layout& L, int32_t n_rows, int32_t n_cols, uint64_t nnz, const off_t* Ap, const int32_t* Aj,
                         off_t* Apt, int32_t* Ajt, uint32_t* perm, char* ws, hipStream_t s) {
    auto* bad = reinterpret_cast<unsigned long long*>(ws);   // [0] the validation word, [1] the first offset out of order
    MI355_HIP_TRY(hipMemsetAsync(bad, 0xff, 2 * sizeof(unsigned long long), s));
    if (n_rows > 0) MI355_COO_LAUNCH(validate_offsets<off_t>, grid_for(uint64_t(n_rows) + 1), Ap, uint32_t(n_rows), nnz, bad);
    if (nnz) MI355_COO_LAUNCH(validate_columns, grid_for(nnz), Aj, nnz, uint32_t(n_cols), bad);
    const uint32_t* keys = nullptr;
    const uint32_t* pay = nullptr;
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws + L.o_counts);
    uint32_t* bsum = reinterpret_cast<uint32_t*>(ws + L.o_bsum);
    for (int p = 0; p < L.passes; ++p) {        // the column is the key, the slot its payload
        const int shift = 8 * p;
        const uint32_t* keys_in = p == 0 ? reinterpret_cast<const uint32_t*>(Aj) : keys;
        uint32_t* keys_out = reinterpret_cast<uint32_t*>(ws + L.o_keys[p & 1]);
        uint32_t* pay_out = reinterpret_cast<uint32_t*>(ws + L.o_pay[p & 1]);
        MI355_COO_LAUNCH(count_digits, unsigned(L.n_tiles), keys_in, nnz, shift, L.n_tiles, counts, bad);
        MI355_COO_LAUNCH(scan_reduce, unsigned(L.n_scan_blocks), counts, L.n_counts, bsum, bad);
        MI355_COO_LAUNCH(scan_sums, 1u, bsum, L.n_scan_blocks, bad);
        MI355_COO_LAUNCH(scan_apply, unsigned(L.n_scan_blocks), counts, L.n_counts, bsum, bad);
        MI355_COO_LAUNCH(scatter, unsigned(L.n_tiles), keys_in, pay, nnz, shift, L.n_tiles, counts, keys_out, pay_out, bad);
        keys = keys_out;
        pay = pay_out;
    }
    MI355_COO_LAUNCH(row_offsets<off_t>, grid_for(uint64_t(n_cols) + 1), keys, nnz, uint32_t(n_cols), Apt, bad);
    if (nnz) MI355_COO_LAUNCH(slot_rows<off_t>, grid_for(nnz), pay, nnz, Ap, uint32_t(n_rows), Ajt, perm, bad);
    // the one synchronisation: the validation words
    unsigned long long word[2] = {kNoBad, kNoBad};
    MI355_HIP_TRY(hipMemcpyAsync(word, bad, sizeof(word), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if (word[1] != kNoBad) {
        const uint64_t i = word[1];
        off_t at = 0, before = 0;
        MI355_HIP_TRY(hipMemcpy(&at, Ap + i, sizeof(at), hipMemcpyDeviceToHost));
        if (i > 0) MI355_HIP_TRY(hipMemcpy(&before, Ap + i - 1, sizeof(before), hipMemcpyDeviceToHost));
        if (i == 0) set_error("csr_transpose: Ap[0] is %lld, not 0", (long long)at);
        else if (at < before) set_error("csr_transpose: Ap[%llu] = %lld is below Ap[%llu] = %lld (offsets must ascend)", (unsigned long long)i, (long long)at, (unsigned long long)(i - 1), (long long)before);
        else set_error("csr_transpose: Ap[%llu] = %lld, the last offset, is not nnz = %llu", (unsigned long long)i, (long long)at, (unsigned long long)nnz);
        return MI355_SPMV_EINVAL;
    }
    if (word[0] != kNoBad) {
        int32_t c = 0;
        MI355_HIP_TRY(hipMemcpy(&c, Aj + word[0], sizeof(c), hipMemcpyDeviceToHost));
        set_error("csr_transpose: entry %llu of Aj is column %d, outside the %d x %d matrix", word[0], c, n_rows, n_cols);
        return MI355_SPMV_EINVAL;
    }
    return MI355_SPMV_OK;
}

}  // namespace coo
}  // namespace mi355

extern "C" int mi355_spmv_csr_transpose(int off_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap,
                                        const int32_t* Aj, void* Apt, int32_t* Ajt, uint32_t* perm, void* workspace,
                                        size_t* workspace_bytes, void* stream) {
    using namespace mi355;
    const char* const fn = "csr_transpose";
    set_error("%s", "");
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown offset type %d", fn, off_type); return MI355_SPMV_EINVAL; }
    if (n_rows < 0 || n_cols < 0 || nnz < 0) { set_error("%s: negative size", fn); return MI355_SPMV_EINVAL; }
    if (off_type == MI355_OFF_I32 && nnz > INT32_MAX) { set_error("%s: nnz does not fit 32-bit offsets (use 64-bit offsets)", fn); return MI355_SPMV_EINVAL; }
    if (uint64_t(nnz) >= (1ull << 32)) { set_error("%s: 2^32 or more entries (the sort's payload is 32-bit)", fn); return MI355_SPMV_ENOTSUP; }
    if (nnz > 0 && (n_rows == 0 || n_cols == 0)) { set_error("%s: nnz > 0 but n_rows or n_cols is 0", fn); return MI355_SPMV_EINVAL; }
    if (!workspace_bytes) { set_error("%s: null workspace_bytes", fn); return MI355_SPMV_EINVAL; }
    const coo::Layout L = coo::layout(n_cols, uint64_t(nnz));
    if (!workspace) { *workspace_bytes = L.bytes; return MI355_SPMV_OK; }
    if (*workspace_bytes < L.bytes) { set_error("%s: workspace of %zu bytes, %zu needed", fn, *workspace_bytes, L.bytes); return MI355_SPMV_EINVAL; }
    if (!Apt) { set_error("%s: null Apt", fn); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !Ap) { set_error("%s: null Ap", fn); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && (!Aj || !Ajt || !perm)) { set_error("%s: null Aj, Ajt or perm", fn); return MI355_SPMV_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    return off_type == MI355_OFF_I32
               ? coo::run_transpose<int32_t>(L, n_rows, n_cols, uint64_t(nnz), static_cast<const int32_t*>(Ap), Aj, static_cast<int32_t*>(Apt), Ajt, perm, ws, s)
               : coo::run_transpose<int64_t>(L, n_rows, n_cols, uint64_t(nnz), static_cast<const int64_t*>(Ap), Aj, static_cast<int64_t*>(Apt), Ajt, perm, ws, s);
}

extern "C" int mi355_spmv_coo_symmetric_nnz(int64_t nnz_stored, const int32_t* rows, const int32_t* cols, void* stream,
                                            int64_t* nnz_expanded) {
    using namespace mi355;
    using namespace mi355::coo;   // (MI355_COO_LAUNCH names the kernels unqualified)
    set_error("%s", "");
    if (!nnz_expanded) { set_error("coo_symmetric_nnz: null nnz_expanded"); return MI355_SPMV_EINVAL; }
    if (nnz_stored < 0) { set_error("coo_symmetric_nnz: negative size"); return MI355_SPMV_EINVAL; }
    if (nnz_stored > 0 && (!rows || !cols)) { set_error("coo_symmetric_nnz: null rows or cols"); return MI355_SPMV_EINVAL; }
    *nnz_expanded = 0;
    if (nnz_stored == 0) return MI355_SPMV_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* total = nullptr;
    MI355_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&total), sizeof(*total)));
    unsigned long long off_diag = 0;
    const int st = [&]() -> int {
        MI355_HIP_TRY(hipMemsetAsync(total, 0, sizeof(*total), s));
        MI355_COO_LAUNCH(offdiag_total, grid_for(uint64_t(nnz_stored)), rows, cols, uint64_t(nnz_stored), total);
        MI355_HIP_TRY(hipMemcpyAsync(&off_diag, total, sizeof(off_diag), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        return MI355_SPMV_OK;
    }();
    (void)hipFree(total);
    if (st != MI355_SPMV_OK) return st;
    *nnz_expanded = nnz_stored + int64_t(off_diag);
    return MI355_SPMV_OK;
}

extern "C" int mi355_spmv_coo_to_csr_symmetric(int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                                               int64_t nnz_stored, int64_t nnz_expanded, const int32_t* rows,
                                               const int32_t* cols, const void* vals, void* Ap, int32_t* Aj, void* Ax,
                                               int64_t* perm, void* workspace, size_t* workspace_bytes, void* stream) {
    using namespace mi355;
    const char* const fn = "coo_to_csr_symmetric";
    set_error("%s", "");
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("%s: unknown offset type %d", fn, off_type); return MI355_SPMV_EINVAL; }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64 && val_type != MI355_VAL_I32) { set_error("%s: unknown value type %d", fn, val_type); return MI355_SPMV_EINVAL; }
    if (n_rows < 0 || n_cols < 0 || nnz_stored < 0 || nnz_expanded < 0) { set_error("%s: negative size", fn); return MI355_SPMV_EINVAL; }
    if (nnz_expanded < nnz_stored || uint64_t(nnz_expanded) > 2 * uint64_t(nnz_stored)) { set_error("%s: nnz_expanded %lld is not between nnz_stored %lld and twice that", fn, (long long)nnz_expanded, (long long)nnz_stored); return MI355_SPMV_EINVAL; }
    if (off_type == MI355_OFF_I32 && nnz_expanded > INT32_MAX) { set_error("%s: nnz_expanded does not fit 32-bit offsets (use 64-bit offsets)", fn); return MI355_SPMV_EINVAL; }
    if (uint64_t(nnz_expanded) >= (1ull << 32)) { set_error("%s: 2^32 or more expanded entries (the sort's counters are 32-bit)", fn); return MI355_SPMV_ENOTSUP; }
    if (uint64_t(nnz_stored) >= (1ull << 31)) { set_error("%s: 2^31 or more stored entries (the sort's 32-bit payload holds the stored index and the mirror bit)", fn); return MI355_SPMV_ENOTSUP; }
    if (!workspace_bytes) { set_error("%s: null workspace_bytes", fn); return MI355_SPMV_EINVAL; }
    const coo::SymLayout S = coo::sym_layout(n_rows, uint64_t(nnz_stored), uint64_t(nnz_expanded));
    if (!workspace) { *workspace_bytes = S.bytes; return MI355_SPMV_OK; }
    if (*workspace_bytes < S.bytes) { set_error("%s: workspace of %zu bytes, %zu needed", fn, *workspace_bytes, S.bytes); return MI355_SPMV_EINVAL; }
    if (!Ap) { set_error("%s: null Ap", fn); return MI355_SPMV_EINVAL; }
    if (nnz_stored > 0 && (!rows || !cols || !Aj)) { set_error("%s: null rows, cols or Aj", fn); return MI355_SPMV_EINVAL; }
    if ((vals == nullptr) != (Ax == nullptr)) { set_error("%s: Ax and vals must be both given or both null", fn); return MI355_SPMV_EINVAL; }
    const int val_bytes = val_type == MI355_VAL_F64 ? 8 : 4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    return off_type == MI355_OFF_I32
               ? coo::run_symmetric<int32_t>(S, val_bytes, n_rows, n_cols, uint64_t(nnz_stored), uint64_t(nnz_expanded), rows, cols, vals, Ap, Aj, Ax, perm, ws, s)
               : coo::run_symmetric<int64_t>(S, val_bytes, n_rows, n_cols, uint64_t(nnz_stored), uint64_t(nnz_expanded), rows, cols, vals, Ap, Aj, Ax, perm, ws, s);
}
