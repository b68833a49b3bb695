// attention_bwd_slice_walk.inc — the walk of one slice's entries by one wave in one of the backward's three roles: what
// follows the cut (slice_cut.inc) in the body of both backward kernels, attention_bwd_slice_kernel (attention_bwd.hip) and
// attention_bwd_half_slice_kernel (attention_bwd_half_kernel.hpp), included inside the kernel's braces.  Text and not a
// function template for attention_slice_walk.inc's reason: a template over the storage type would rename the kernels on
// record (profiles/attention_backward_kernel_resources.txt), and included text is compiled as part of each kernel, as it
// always was.  The order of operations that attention_bwd.hip promises is this file's and nobody else's.
//
// In scope where it is included:
//   a, C, ROLE, Ap   the kernel's arguments (AttnBwdArgs<val_t> or AttnBwdHalfArgs<vec_t>: a.Aj, a.perm, a.Q, a.K, a.V, a.dO,
//                    a.bias, a.lse, a.delta, a.out, a.dbias, the ld*, a.d, a.dv, a.col_begin, a.cols, the *_vec, a.scale and
//                    a.sc are read) and its template arguments
//   acc_t            the type of bias, lse, delta, dbias, scale, the scores, p, dp, ds, the coefficients, the per-slot partials
//                    and the scratch pieces: val_t, or float over 16-bit Q, K, V, dO and out
//   W, S, kNegInf    columns of a lane per tile (16 bytes of a row), the wave's slots 64 / C, and -inf in acc_t
//   load_cols        load_cols(acc_t (&)[W], row pointer, nv, vec): the lane's W columns of a row of Q / K / V / dO as acc_t, a
//                    column that does not exist as 0 — slice_cut.hpp's, or half_cols.hpp's by a using-declaration
//   store_cols       store_cols(const acc_t (&)[W], row pointer of out, nv, vec): the store of a finished line's W columns, the
//                    nv that exist — slice_cut.hpp's, or half_cols.hpp's (which narrows each column once, nearest even)
//   what slice_cut.inc leaves: lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
    const bool first_pass = a.col_begin == 0;
    const bool biased = a.bias != nullptr;
    const int nv = min(max(a.cols - c * W, 0), W);
    // the line carried in ends here with entries of its own (a slice inside one line is a tail; a line whose last entry
    // was the slice before's last item has nothing here)
    const bool has_head = carried_in && nr >= 1 && rel[1] >= 1 && rel[1] <= nn;

    acc_t acc[W];           // per-slot partial of the open line (the line whose entries are not all seen yet)
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = acc_t(0);
    int open_i = -1;        // that line, relative to r0; -1 = none (acc is +0)
    int holder = -1;        // >= 0: acc is not +0 in this slot only; -2: spread over the slots

    for (int base = 0; base < nn; base += kWave) {
        // 64 entries, one per lane, coalesced; each lane finds its entry's line in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        acc_t bias = acc_t(0);
        int ie = nr * 2;    // line * 2 + (1 = this entry is the last of its line); nr = no entry
        if (m < nn) {
            col = a.Aj[n0 + m];
            if (biased) {
                if constexpr (ROLE == kBwdDQ) bias = a.bias[n0 + m];
                else bias = a.bias[a.perm[n0 + m]];
            }
#include "slice_cut_row.inc"     // leaves lo: the entry's line, relative to r0
            ie = lo * 2 + (rel[lo + 1] == m + 1 ? 1 : 0);
        }
        const int left = nn - base;
        const int steps = slice_group_steps<C>(left);
        for (int t = 0; t < steps; ++t) {
            // slot s takes entry t * S + s of the 64
            int32_t col_s = col;
            acc_t bias_s = bias;
            int ie_s = ie;
            if constexpr (C > 1) {
                const int src = t * S + s;
                col_s = __shfl(col, src);
                bias_s = __shfl(bias, src);
                ie_s = __shfl(ie, src);
            }
            const int i_s = ie_s >> 1;
            const bool live = i_s < nr;
            // the entry's query and key: the line and the gathered index, or the other way round on A^T
            const int64_t qi = ROLE == kBwdDQ ? r0 + i_s : int64_t(col_s);
            const int64_t ki = ROLE == kBwdDQ ? int64_t(col_s) : r0 + i_s;
            // a masked edge loads nothing and contributes exactly +0
            const bool seen = live && !(biased && bias_s == kNegInf);

            // the two dots, each SDDMM's tile loop and then a fixed tree over the slot's C lanes: the score over d, dp over dv
            acc_t part = acc_t(0), dpart = acc_t(0);
            if (seen) {
                const auto* qp = a.Q + qi * a.ldq + c * W;
                const auto* kp = a.K + ki * a.ldk + c * W;
                for (int32_t cb = 0; cb < a.d; cb += C * W) {       // the tiles of d: the same register all along
                    const int nd = min(max(a.d - cb - c * W, 0), W);
                    if (nd > 0) {
                        acc_t q[W], k[W];
                        load_cols(q, qp + cb, nd, a.q_vec != 0);
                        load_cols(k, kp + cb, nd, a.k_vec != 0);
#pragma unroll
                        for (int j = 0; j < W; ++j) part = attn_fma(q[j], k[j], part);
                    }
                }
                const auto* gp = a.dO + qi * a.lddo + c * W;
                const auto* vp = a.V + ki * a.ldv + c * W;
                for (int32_t cb = 0; cb < a.dv; cb += C * W) {      // the tiles of dv
                    const int nd = min(max(a.dv - cb - c * W, 0), W);
                    if (nd > 0) {
                        acc_t g[W], x[W];
                        load_cols(g, gp + cb, nd, a.do_vec != 0);
                        load_cols(x, vp + cb, nd, a.v_vec != 0);
#pragma unroll
                        for (int j = 0; j < W; ++j) dpart = attn_fma(g[j], x[j], dpart);
                    }
                }
            }
#pragma unroll
            for (int dd = 1; dd < C; dd <<= 1) {
                part += __shfl_xor(part, dd);
                dpart += __shfl_xor(dpart, dd);
            }
            // one exp; the coefficient of this role and the lane's W columns of the row it multiplies
            acc_t coef = acc_t(0), ds = acc_t(0);
            acc_t xv[W];
#pragma unroll
            for (int j = 0; j < W; ++j) xv[j] = acc_t(0);
            if (seen) {
                acc_t v = a.scale * part;
                if (biased) v = v + bias_s;
                if (v != kNegInf) {     // (the test comes before the subtraction)
                    const acc_t p = attn_exp(v - a.lse[qi]);
                    ds = p * (dpart - a.delta[qi]);
                    if constexpr (ROLE == kBwdDQ) {
                        coef = a.scale * ds;
                        load_cols(xv, a.K + ki * a.ldk + a.col_begin + c * W, nv, a.k_vec != 0);
                    } else if constexpr (ROLE == kBwdDK) {
                        coef = a.scale * ds;
                        load_cols(xv, a.Q + qi * a.ldq + a.col_begin + c * W, nv, a.q_vec != 0);
                    } else {
                        coef = p;
                        load_cols(xv, a.dO + qi * a.lddo + a.col_begin + c * W, nv, a.do_vec != 0);
                    }
                }
            }
            if constexpr (ROLE == kBwdDQ) {
                // one writer per element: lane 0 of the slot, on the first pass
                if (live && c == 0 && first_pass && a.dbias) a.dbias[n0 + base + t * S + s] = ds;
            }
            acc_t p[W];
#pragma unroll
            for (int j = 0; j < W; ++j) p[j] = coef * xv[j];

            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one line, and the line goes on: partials stay per slot
#pragma unroll
                for (int j = 0; j < W; ++j) acc[j] = acc[j] + p[j];
                open_i = i_first;
                holder = -2;
                continue;
            }
            // a line ends in this step (or the slice does).  The open line's partial joins slot 0, whose entry is the
            // next of that line; then a segmented inclusive scan over the slots sums each line's run of products.
            if (open_i >= 0) {
                if (holder >= 0) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
                } else {
                    attn_bwd_reduce_slots<acc_t, W, C>(acc);
                }
                if (s == 0) {
#pragma unroll
                    for (int j = 0; j < W; ++j) p[j] = p[j] + acc[j];
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = acc_t(0);
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
#pragma unroll
            for (int dd = C; dd < kWave; dd <<= 1) {
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const acc_t o = __shfl_up(p[j], dd);
                    if (lane - c - dd >= start) p[j] = p[j] + o;
                }
            }
            const bool tail = s == S - 1 || ((heads >> (lane - c + C)) & 1ull);
            if (live && tail && (ie_s & 1)) {
                if (i_s == 0 && carried_in) {
                    // the HEAD piece: as computed, for the fix-up (whole tiles fit carry_ld)
                    acc_t* hv = a.sc.acc + (w * 2 + 0) * a.sc.carry_ld + a.col_begin + c * W;
#pragma unroll
                    for (int j = 0; j < W; ++j) hv[j] = p[j];
                } else if (nv > 0) {
                    store_cols(p, a.out + (r0 + i_s) * a.ldout + a.col_begin + c * W, nv, a.out_vec != 0);
                }
            }
            // the last entry of the step: if its line goes on, its run's sum is the new open partial
            const int lv = min(S - 1, left - t * S - 1);
            const int ie_lv = __shfl(ie_s, lv * C);
            if (!(ie_lv & 1)) {
                open_i = ie_lv >> 1;
                holder = lv;
                if (s == lv) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = p[j];
                }
            } else {
                open_i = -1;
                holder = -1;
            }
        }
    }

    // the TAIL piece: what this slice holds of a line that ends in a later one
    if (open_i >= 0) {
        if (holder >= 0) {
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
        } else {
            attn_bwd_reduce_slots<acc_t, W, C>(acc);
        }
        if (s == 0) {
            acc_t* tv = a.sc.acc + (w * 2 + 1) * a.sc.carry_ld + a.col_begin + c * W;      // (carry_ld covers whole tiles)
#pragma unroll
            for (int j = 0; j < W; ++j) tv[j] = acc[j];
        }
    }
    if (lane == 0 && first_pass) {
        a.sc.row[w * 2 + 0] = has_head ? int32_t(r0) : -1;
        a.sc.row[w * 2 + 1] = open_i >= 0 ? int32_t(r0 + open_i) : -1;
    }

    // lines without entries whose end lies in this slice: +0; a line with entries is stored where its last one is
    if (nv > 0) {
        acc_t none[W];
#pragma unroll
        for (int j = 0; j < W; ++j) none[j] = acc_t(0);
        for (int64_t r = r0 + s; r < r1; r += S)
            if (Ap[r] == Ap[r + 1]) store_cols(none, a.out + r * a.ldout + a.col_begin + c * W, nv, a.out_vec != 0);
    }
