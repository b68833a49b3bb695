// slice_cut.inc — from "wave w of the grid" to "rows r0 .. r0 + nr - 1, nonzeros n0 .. n0 + nn - 1, offsets in LDS": the
// prologue of every slice kernel, included inside the kernel's braces by multi_slice_walk.inc (multi_slice_kernel,
// mh::multi_half_slice_kernel) and by sddmm_slice_kernel (sddmm.hip) and sddmm_half_slice_kernel (sddmm_half_kernel.hpp),
// each in front of sddmm_slice_walk.inc.  Text and not a function, for multi_slice_walk.inc's
// reason: the kernels compile to the device code on record only when this is compiled as part of them.
//
// In scope where it is included (kernel arguments and template arguments, or bound by the includer in front):
//   a, Ap            the kernel's arguments: a.n_rows, a.nnz and a.n_slices are read; Ap is const off_t* __restrict__
//   C                the kernel's template argument: lanes per nonzero slot
//   kCutCarriedIn    constexpr bool: carried_in is computed (one more read of Ap[r0]); false leaves it false
//   kCutKeepsR1      constexpr bool: r1 outlives the cut (the multi-vector walk's empty rows end at it); false leaves it 0
//   cut_block        the workgroup's index among those that cut this structure: blockIdx.x everywhere but in the attention
//                    kernels, whose grid holds every head's workgroups (blockIdx.x / n_heads, DESIGN.md §3.15.4)
//   kCutNrInit       constexpr int: what nr holds in a wave without a slice, which returns below and never reads it.
//                    Each family keeps the value it was written with (multi -1, SDDMM 0): the value is an
//                    instruction's immediate, and the kernels compile as on record only with their own
// Leaves in scope: lane; c, s (the lane's column group and slot); w (the slice); r0 (its first row); r1 (the row that is
// open at its end: rows r0 .. r1 - 1 end in the slice); n0, nn (its first nonzero, and how many it has); nr (rows with
// nonzeros or their end here); rel (LDS, this wave's: rel[i] = where row r0 + i begins relative to n0, clamped to
// [0, nn + 1], for i = 0 .. nr; slice_cut_row.inc searches it); carried_in (row r0 began in an earlier slice).
// Leaves by `return`, behind the workgroup's one barrier, in a wave that has no slice.
    __shared__ int32_t rel_all[kSliceWaves][kSliceLen + 2];
    const int lane = threadIdx.x & (kWave - 1);
    const int c = lane % C, s = lane / C;
    int32_t* rel = rel_all[threadIdx.x / kWave];
    const int64_t w = int64_t(cut_block) * kSliceWaves + threadIdx.x / kWave;
    const bool active = w < a.n_slices;
    [[maybe_unused]] int64_t r0 = 0, r1 = 0, n0 = 0;     // (r1 may go unused; one declaration in this order, as on record)
    int nr = kCutNrInit, nn = 0;
    [[maybe_unused]] bool carried_in = false;
    if (active) {
        // merge-path diagonals of the slice: lanes 0..31 search its start, lanes 32..63 its end.  Row end r comes before
        // nonzero n iff Ap[r + 1] <= n; (r, n) = row ends and nonzeros in front of the diagonal.
        const int64_t items = int64_t(a.n_rows) + a.nnz;
        int64_t d = (lane < 32 ? w : w + 1) * kSliceLen;
        if (d > items) d = items;
        int64_t lo = d > a.nnz ? d - a.nnz : 0, hi = d < a.n_rows ? d : a.n_rows;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (int64_t(Ap[mid + 1]) <= d - mid - 1) lo = mid + 1; else hi = mid;
        }
        const int64_t n = d - lo;
        r0 = __shfl(lo, 0);
        const int64_t r_open = __shfl(lo, 32);
        if constexpr (kCutKeepsR1) r1 = r_open;
        n0 = __shfl(n, 0);
        nn = int(__shfl(n, 32) - n0);
        // rows r0 .. r_last have nonzeros or their end here (row r_open, when there is one, does not end in this slice)
        const int64_t r_last = r_open < a.n_rows ? r_open : int64_t(a.n_rows) - 1;
        nr = int(r_last - r0) + 1;
        for (int i = lane; i <= nr; i += kWave) {
            const int64_t v = int64_t(Ap[r0 + i]) - n0;
            rel[i] = v < 0 ? 0 : v > nn ? nn + 1 : int32_t(v);
        }
        if constexpr (kCutCarriedIn) carried_in = int64_t(Ap[r0]) < n0;
    }
    __syncthreads();
    if (!active) return;
