// sddmm_slice_walk.inc — the walk of one slice's nonzeros by one wave: what follows the cut (slice_cut.inc) in the body of
// both SDDMM kernels, sddmm_slice_kernel (sddmm.hip) and sddmm_half_slice_kernel (sddmm_half_kernel.hpp), included inside
// the kernel's braces.  Text and not a function template for multi_slice_walk.inc's reason: a template over the storage
// type would rename the kernels on record (profiles/sddmm_kernel_resources.txt, profiles/sddmm_half_kernel_resources.txt),
// and included text is compiled as part of each kernel, as it always was.  The order of addition that sddmm.hip promises
// is this file's and nobody else's.
//
// In scope where it is included:
//   a, C, VALUED     the kernel's arguments (SddmmArgs<val_t> or SddmmHalfArgs<vec_t>: a.Aj, a.Ax, a.U, a.V, a.out, a.ldu,
//                    a.ldv, a.k, a.u_vec, a.v_vec, a.alpha, a.beta are read) and its template arguments
//   acc_t            the type of Ax, out and the arithmetic: val_t, or float over 16-bit U and V
//   W, S             columns of a lane per tile (16 bytes of a row of U / V), and the wave's slots, 64 / C
//   load_cols        load_cols(acc_t (&)[W], row pointer, nv, vec): the lane's W columns of a row of U / V as acc_t, a
//                    column that does not exist as 0 — slice_cut.hpp's, or half_cols.hpp's by a using-declaration
//   kWalkFmaInPlace  constexpr bool: the fma of a column, one rounding whatever the compiler would otherwise contract, is
//                    __builtin_fmaf written in place (acc_t = float only) instead of the call of sddmm_fma (sddmm.hip),
//                    which is that builtin.  One operation; each kernel keeps the form it was written with, for
//                    kCutNrInit's reason: an inlined call and the builtin in place order two moves differently in every
//                    C > 1 kernel, and the kernels compile as on record only with their own
//   what slice_cut.inc leaves: lane, c, s, r0, n0, nn, nr, rel
    for (int base = 0; base < nn; base += kWave) {
        // 64 nonzeros, one per lane, coalesced; each lane finds its nonzero's row in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        int row_i = 0;
        [[maybe_unused]] acc_t ax = acc_t(1);
        if (m < nn) {
            col = a.Aj[n0 + m];
            if constexpr (VALUED) ax = a.Ax[n0 + m];
#include "slice_cut_row.inc"     // leaves lo: the nonzero's row, relative to r0
            row_i = lo;
        }
        const int left = nn - base;
        const int steps = slice_group_steps<C>(left);
        acc_t dot = acc_t(0);           // of this lane's own nonzero m, handed back by the step that took it
        for (int t = 0; t < steps; ++t) {
            // slot s takes nonzero t * S + s of the 64
            const int src = t * S + s;
            int32_t col_s = col;
            int row_s = row_i;
            if constexpr (C > 1) {
                col_s = __shfl(col, src);
                row_s = __shfl(row_i, src);
            }
            acc_t part = acc_t(0);
            if (src < left) {
                const auto* up = a.U + (r0 + row_s) * a.ldu + c * W;
                const auto* vp = a.V + int64_t(col_s) * a.ldv + c * W;
                for (int32_t cb = 0; cb < a.k; cb += C * W) {       // the tiles of k: the same register all along
                    const int nv = min(max(a.k - cb - c * W, 0), W);
                    if (nv > 0) {
                        acc_t u[W], v[W];
                        load_cols(u, up + cb, nv, a.u_vec != 0);
                        load_cols(v, vp + cb, nv, a.v_vec != 0);
#pragma unroll
                        for (int j = 0; j < W; ++j) {
                            if constexpr (kWalkFmaInPlace) part = __builtin_fmaf(u[j], v[j], part);
                            else part = sddmm_fma(u[j], v[j], part);
                        }
                    }
                }
            }
            // the dot of the slot's nonzero, in every lane of the slot: a fixed tree over its C lanes
#pragma unroll
            for (int d = 1; d < C; d <<= 1) part += __shfl_xor(part, d);
            // back to the lane that loaded the nonzero: lane l holds nonzero l = t' * S + s', taken at step t' by slot s'
            acc_t mine = part;
            if constexpr (C > 1) mine = __shfl(part, (lane % S) * C);
            if (lane / S == t) dot = mine;
        }
        if (m < nn) {
            acc_t o;
            if constexpr (VALUED) o = a.alpha * (ax * dot); else o = a.alpha * dot;
            if (a.beta != acc_t(0)) o += a.beta * a.out[n0 + m];
            a.out[n0 + m] = o;
        }
    }
