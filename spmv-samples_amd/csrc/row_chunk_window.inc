// row_chunk_window.inc — from "rows [rb, re) are this workgroup's" to the chunk body (xwindow.hpp, chunk_rows_any) and
// back: the per-chunk text of every window kernel of the row kinds, included inside csr_vector_window_kernel
// (csr_vector.hip), h16::csr_vector_window_kernel (csr_vector_h16.hip) and run_chunk of light_rows_window_kernel
// (light_rows.hip).  Text and not a function template: a function is optimised once on its own before it is inlined,
// and the kernels then no longer compile to the device code on record (a function around this text changed register
// assignment and scheduling all through csr_vector_h16.hip); included text is compiled as part of the kernel, as it
// always was.
//
// In scope where it is included (kernel arguments and template arguments, or bound by the includer in front):
//   BLOCK, T, R, NSEG        the kernel's template arguments (NSEG: 0 = no window, 1 = one, kMaxSegments = several bands)
//   ADAPT, PACKED            vector width per chunk (weight-cut chunks); the 16-bit window index Aj16 is streamed
//   val_t, mat_t             the type of x and y, and the type Ax is stored in
//   kBarrierAfterWide        LIGHT: a barrier behind the wide path (its persistent loop dequeues next)
//   rb, re                   the chunk's rows (int64_t), rb < re
//   Ap, Aj, Ax, x, y, Aj16   the operands (LIGHT: its opaque copies; Aj16 is nullptr where PACKED never is true)
//   n_cols, nnz, cmap, window_cap, hint, segs, alpha, beta   as the kernel took them (segs is read where NSEG > 1 only)
//   scr, s_red               the workgroup's ChunkScratch and the two LDS words stage_x_window reduces in
// Leaves by `return` where the chunk does not fit 32-bit offsets: from the kernel, or from LIGHT's run_chunk.
    bool fits;
    const int64_t base = stage_chunk_bounds<val_t>(scr, rb, re, Ap, cmap.rel_limit, fits);
    if (!fits) {            // (uniform) more nonzeros than 32-bit chunk-relative offsets reach
        chunk_rows_wide<BLOCK, val_t>(rb, re, Ap, Aj, Ax, x, y, alpha, beta, cmap.giant_len);
        if constexpr (kBarrierAfterWide) __syncthreads();
        return;
    }
    __syncthreads();        // (LIGHT: also orders the read of s_got before the next dequeue writes it)
    const int32_t* const Aj_c = Aj + base;       // the chunk's view: element 0 = its first 16-byte group (base is a multiple of 4)
    const mat_t* const Ax_c = Ax + base;
    const int32_t nnz_c = chunk_nnz_reach(nnz - base);
    // the window is staged inside chunk_rows, behind the first group's stream loads
    if constexpr (NSEG > 1) {
        auto stage = [&] { return stage_x_segments<val_t>(rb, re, n_cols, x, scr.s_x, window_cap, segs); };
        chunk_rows_any<BLOCK, T, R, true, ADAPT, val_t>(rb, re, nnz_c, Aj_c, Ax_c, x, y, stage, scr);
    } else {
        auto first_last = [&](int64_t r, int& first, int& last) {
            const int32_t s = scr.s_b[r - rb], e = scr.s_b[r - rb + 1];
            if (e <= s) return false;
            first = Aj_c[s];
            last = Aj_c[e - 1];
            return true;
        };
        auto stage = [&] {
            return stage_x_window<val_t>(rb, re, n_cols, first_last, x, scr.s_x, window_cap, s_red, hint);
        };
        // (PACKED: hint.use holds, the window staged is the one the index was encoded against)
        chunk_rows_any<BLOCK, T, R, NSEG == 1, ADAPT, val_t, decltype(stage)&, false, PACKED>(
            rb, re, nnz_c, Aj_c, Ax_c, x, y, stage, scr, PACKED ? Aj16 + base : nullptr);
    }
