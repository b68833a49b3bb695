// attention_slice_walk.inc — the walk of one slice's nonzeros by one wave: what follows the cut (slice_cut.inc) in the body of
// both attention kernels, attention_slice_kernel (attention.hip) and attention_half_slice_kernel (attention_half_kernel.hpp),
// included inside the kernel's braces.  Text and not a function template for sddmm_slice_walk.inc's reason: a template over
// the storage type would rename the kernels on record (profiles/attention_kernel_resources.txt), and included text is
// compiled as part of each kernel, as it always was.  The order of operations that attention.hip promises is this file's
// and nobody else's.
//
// In scope where it is included:
//   a, C, Ap         the kernel's arguments (AttnArgs<val_t> or AttnHalfArgs<vec_t>: a.Aj, a.Q, a.K, a.V, a.bias, a.O, a.lse, the
//                    ld*, a.d, a.col_begin, a.cols, the *_vec, a.scale and a.sc are read) and its template argument
//   acc_t            the type of bias, lse, scale, the scores, the (m, l, acc) states and the scratch pieces: val_t, or float
//                    over 16-bit Q, K, V and O
//   W, S, kNegInf    columns of a lane per tile (16 bytes of a row), the wave's slots 64 / C, and -inf in acc_t
//   load_cols        load_cols(acc_t (&)[W], row pointer, nv, vec): the lane's W columns of a row of Q / K / V as acc_t, a
//                    column that does not exist as 0 — slice_cut.hpp's, or half_cols.hpp's by a using-declaration
//   store_cols       store_cols(const acc_t (&)[W], row pointer of O, nv, vec): the store of a finished row's W columns, the
//                    nv that exist — slice_cut.hpp's, or half_cols.hpp's (which narrows each column once, nearest even)
//   what slice_cut.inc leaves: lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in
    const bool first_pass = a.col_begin == 0;
    const bool biased = a.bias != nullptr;
    const int nv = min(max(a.cols - c * W, 0), W);
    // the row carried in ends here with nonzeros of its own (a slice inside one row is a tail; a row whose last nonzero
    // was the slice before's last item has nothing here)
    const bool has_head = carried_in && nr >= 1 && rel[1] >= 1 && rel[1] <= nn;

    // per-slot state of the open row (the row whose nonzeros are not all seen yet)
    acc_t m_o = kNegInf, l_o = acc_t(0), acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = acc_t(0);
    int open_i = -1;        // that row, relative to r0; -1 = none (the state is the identity)
    int holder = -1;        // >= 0: the state is not the identity in this slot only; -2: spread over the slots

    for (int base = 0; base < nn; base += kWave) {
        // 64 nonzeros, one per lane, coalesced; each lane finds its nonzero's row in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        acc_t bias = acc_t(0);
        int ie = nr * 2;    // row * 2 + (1 = this nonzero is the last of its row); nr = no nonzero
        if (m < nn) {
            col = a.Aj[n0 + m];
            if (biased) bias = a.bias[n0 + m];
#include "slice_cut_row.inc"     // leaves lo: the nonzero's row, relative to r0
            ie = lo * 2 + (rel[lo + 1] == m + 1 ? 1 : 0);
        }
        const int left = nn - base;
        const int steps = slice_group_steps<C>(left);
        for (int t = 0; t < steps; ++t) {
            // slot s takes nonzero t * S + s of the 64
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

            // the score: SDDMM's tile loop over d, then a fixed tree over the slot's C lanes
            acc_t part = acc_t(0);
            if (live) {
                const auto* qp = a.Q + (r0 + i_s) * a.ldq + c * W;
                const auto* kp = a.K + int64_t(col_s) * a.ldk + c * W;
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
            }
#pragma unroll
            for (int dd = 1; dd < C; dd <<= 1) part += __shfl_xor(part, dd);
            acc_t v = kNegInf;
            acc_t xv[W];
#pragma unroll
            for (int j = 0; j < W; ++j) xv[j] = acc_t(0);
            if (live) {
                v = a.scale * part;
                if (biased) v = v + bias_s;
                // (a masked edge contributes +0 whatever its row of V holds)
                if (v != kNegInf) load_cols(xv, a.V + int64_t(col_s) * a.ldv + a.col_begin + c * W, nv, a.v_vec != 0);
            }

            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one row, and the row goes on: the entry joins its slot's state, one exp
                const bool up = v > m_o;
                const acc_t low = up ? m_o : v;
                const acc_t f = low == kNegInf ? acc_t(0) : attn_exp_diff(up ? m_o - v : v - m_o);
                const acc_t e = up ? f : acc_t(1), ev = v == kNegInf ? acc_t(0) : up ? acc_t(1) : f;
                l_o = l_o * e + ev;
#pragma unroll
                for (int j = 0; j < W; ++j) acc[j] = acc[j] * e + ev * xv[j];
                if (up) m_o = v;
                open_i = i_first;
                holder = -2;
                continue;
            }
            // a row ends in this step (or the slice does).  The open row's state, folded once, joins slot 0, whose
            // nonzero is the next of that row.
            const bool joins = open_i >= 0 && s == 0;
            if (open_i >= 0) {
                if (holder >= 0) {
                    m_o = __shfl(m_o, holder * C + c);
                    l_o = __shfl(l_o, holder * C + c);
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
                } else {
                    attn_reduce_slots<acc_t, W, C>(m_o, l_o, acc);
                }
            }
            // the runs of one row over the slots, and each run's maximum M in every one of its lanes
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
            const int behind = lane - c + C;
            const unsigned long long later = behind >= kWave ? 0ull : heads >> behind;
            const int end = later ? behind + __builtin_ctzll(later) - C : kWave - C;     // lane c == 0 of its last slot
            acc_t mx = joins && m_o > v ? m_o : v;
#pragma unroll
            for (int dd = C; dd < kWave; dd <<= 1) {
                const acc_t o = __shfl_up(mx, dd);
                if (lane - c - dd >= start && o > mx) mx = o;
            }
            const acc_t M = __shfl(mx, end + c);
            // one exp per entry; the open row's state is rescaled into slot 0
            const acc_t e = attn_side(v, M);
            acc_t lp = e, p[W];
#pragma unroll
            for (int j = 0; j < W; ++j) p[j] = e * xv[j];
            if (joins) {
                const acc_t eo = attn_side(m_o, M);
                lp = l_o * eo + lp;
#pragma unroll
                for (int j = 0; j < W; ++j) p[j] = acc[j] * eo + p[j];
            }
            m_o = kNegInf;
            l_o = acc_t(0);
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = acc_t(0);
            // the segmented inclusive sum scan of the multi-vector walk, l beside the W columns
#pragma unroll
            for (int dd = C; dd < kWave; dd <<= 1) {
                const acc_t ol = __shfl_up(lp, dd);
                const bool in_run = lane - c - dd >= start;
                if (in_run) lp = lp + ol;
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const acc_t o = __shfl_up(p[j], dd);
                    if (in_run) p[j] = p[j] + o;
                }
            }
            if (live && lane - c == end && (ie_s & 1)) {
                if (i_s == 0 && carried_in) {
                    // the HEAD piece: the state as computed, for the fix-up (whole tiles fit carry_ld)
                    acc_t* hv = a.sc.acc + (w * 2 + 0) * a.sc.carry_ld + a.col_begin + c * W;
#pragma unroll
                    for (int j = 0; j < W; ++j) hv[j] = p[j];
                    if (c == 0 && first_pass) {
                        a.sc.ml[(w * 2 + 0) * 2 + 0] = M;
                        a.sc.ml[(w * 2 + 0) * 2 + 1] = lp;
                    }
                } else {
                    const int64_t r = r0 + i_s;
                    if (nv > 0) {
                        acc_t o[W];
#pragma unroll
                        for (int j = 0; j < W; ++j) o[j] = attn_out(p[j], lp);
                        store_cols(o, a.O + r * a.ldo + a.col_begin + c * W, nv, a.o_vec != 0);
                    }
                    if (c == 0 && first_pass && a.lse) a.lse[r] = attn_lse(M, lp);
                }
            }
            // the last nonzero of the step: if its row goes on, its run's state is the new open state
            const int lv = min(S - 1, left - t * S - 1);
            const int ie_lv = __shfl(ie_s, lv * C);
            if (!(ie_lv & 1)) {
                open_i = ie_lv >> 1;
                holder = lv;
                if (s == lv) {
                    m_o = M;
                    l_o = lp;
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] = p[j];
                }
            } else {
                open_i = -1;
                holder = -1;
            }
        }
    }

    // the TAIL piece: what this slice holds of a row that ends in a later one
    if (open_i >= 0) {
        if (holder >= 0) {
            m_o = __shfl(m_o, holder * C + c);
            l_o = __shfl(l_o, holder * C + c);
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = __shfl(acc[j], holder * C + c);
        } else {
            attn_reduce_slots<acc_t, W, C>(m_o, l_o, acc);
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
        if (open_i >= 0) {
            a.sc.ml[(w * 2 + 1) * 2 + 0] = m_o;
            a.sc.ml[(w * 2 + 1) * 2 + 1] = l_o;
        }
    }

    // empty rows whose end lies in this slice: O = +0 and lse = -inf; a row with nonzeros is stored where its last one is
    // (and a row carried in has nonzeros: an empty row is never a piece)
    if (nv > 0 || (c == 0 && first_pass && a.lse)) {
        acc_t none[W];
#pragma unroll
        for (int j = 0; j < W; ++j) none[j] = acc_t(0);
        for (int64_t r = r0 + s; r < r1; r += S) {
            if (Ap[r] == Ap[r + 1]) {
                if (nv > 0) store_cols(none, a.O + r * a.ldo + a.col_begin + c * W, nv, a.o_vec != 0);
                if (c == 0 && first_pass && a.lse) a.lse[r] = kNegInf;
            }
        }
    }
