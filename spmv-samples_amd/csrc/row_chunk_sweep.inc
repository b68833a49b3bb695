// row_chunk_sweep.inc — row_chunk_window.inc's counterpart for the sweeping kernels (xwindow.hpp, chunk_rows_sweep):
// included inside csr_vector_sweep_kernel (csr_vector.hip) and light_rows_sweep_kernel (light_rows.hip), and text for the
// same reason.  In scope where it is included: T, R, val_t; rb < re (int64_t); Ap, Aj, Ax, x, y, n_cols, nnz, cmap,
// window_cap, hint, alpha, beta as the kernel took them; scr.  Falls through to the includer's text when the chunk is done.
// (The wide path gets no giant-row threshold: a sweep plan's ChunkMap holds none, row_launch.hpp launch_rows_sweep.)
    bool fits;
    const int64_t base = stage_chunk_bounds<val_t>(scr, rb, re, Ap, cmap.rel_limit, fits);
    if (!fits) {            // (uniform) more nonzeros than 32-bit chunk-relative offsets reach
        chunk_rows_wide<kHugeBlock, val_t>(rb, re, Ap, Aj, Ax, x, y, alpha, beta, 0);
    } else {
        __syncthreads();
        const int32_t nnz_c = chunk_nnz_reach(nnz - base);
        // (a persistent workgroup per CU walking its share of the chunks measured WORSE, 194 vs 187 us at two passes,
        // 438 vs 358 at seven: the hardware dispatcher's refill costs less than the registers the loop does)
        chunk_rows_sweep<kHugeBlock, T, R, val_t>(rb, re, nnz_c, Aj + base, Ax + base, x, y, n_cols, window_cap, hint, scr);
    }
