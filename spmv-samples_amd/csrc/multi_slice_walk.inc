// multi_slice_walk.inc — the walk of one slice by one wave: the BODY of every multi-vector slice kernel, typed
// (multi_slice_kernel, multi_kernels.hpp) and 16-bit (mh::multi_half_slice_kernel, multi_half_kernels.hpp), included inside
// the kernel's braces.  Text and not a function template: a function is optimised once on its own before it is inlined,
// and the typed kernels then no longer compile to the registers and occupancy on record (profiles/); included text is
// compiled as part of the kernel, as it always was.
//
// The walk begins with the cut that SDDMM shares (slice_cut.inc, included below; slice_cut.hpp holds the geometry).
//
// In scope where it is included: the kernel's arguments a (the policy's Args) and Ap (const off_t* __restrict__), the
// kernel's template argument C = lanes per nonzero slot (16-byte column groups of the tile; the wave holds S = 64 / C
// slots), and a policy type P that says what differs between the value-type families:
//   acc_t, SR, V, Args         the arithmetic type, its semiring, the columns of a lane, the kernel's argument struct
//   kValued, kAxFill           Ax is loaded, converted by P::ax and shuffled; otherwise every entry is kAxFill (one).  A valued
//                              kernel's kAxFill is what a lane past the slice's last nonzero holds: never used, and kept as
//                              each family wrote it so that its kernels compile as on record
//   kPermuted                  (a valued policy) nonzero n's value is a.Ax[a.perm[n]], not a.Ax[n]: the index is loaded
//                              coalesced next to Aj and the value gathered through it (multi_perm_slice_kernel).  A constant
//                              under `if constexpr`: the other policies' kernels see the line they always had
//   kMaskCombine               combine() must not see a masked column (every semiring except (+, *), whose product with
//                              the 0 that a masked column is loaded as is the identity already)
//   kTails                     the last piece of a row that began in an earlier slice goes to a.tail_val, not to Y
//   load_cols(v, p, nv, vec)   the lane's V columns of a row of X as acc_t
//   kFields, store_row         a complete row's store: store_row(a, r, c, sum), or with kFields the fields of a one by one
//                              (the 16-bit kernels hand no function their argument struct: a struct whose address is taken
//                              is split into registers later, and they would then not compile as on record)
#define MI355_WALK_STORE_ROW(r, sum)                                                                                   \
    do {                                                                                                               \
        if constexpr (P::kFields) P::store_row(a.Y, a.ldy, a.col_begin, a.cols, a.y_vec != 0, a.alpha, a.beta, r, c, sum); \
        else P::store_row(a, r, c, sum);                                                                               \
    } while (0)
    using SR = typename P::SR;
    using acc_t = typename P::acc_t;
    constexpr int V = P::V;
    constexpr int S = kWave / C;
    constexpr bool kCutCarriedIn = P::kTails, kCutKeepsR1 = true;   // what slice_cut.inc asks its includer
    constexpr int kCutNrInit = -1;
    const unsigned cut_block = blockIdx.x;
#include "slice_cut.inc"        // leaves lane, c, s, w, r0, r1, n0, nn, nr, rel, carried_in

    acc_t acc[V];           // per-slot partial of the open row (the row whose nonzeros are not all seen yet)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = SR::identity();
    int open_i = -1;        // that row, relative to r0; -1 = none (acc is the identity)
    int holder = -1;        // >= 0: acc is not the identity in this slot only; -2: spread over the slots
    const int nv = min(max(a.cols - c * V, 0), V);

    for (int base = 0; base < nn; base += kWave) {
        // 64 nonzeros, one per lane, coalesced; each lane finds its nonzero's row in the slice's offsets
        const int m = base + lane;
        int32_t col = 0;
        acc_t ax = P::kAxFill;  // every entry of a matrix without values; a valued one's is loaded below (a lane past nn: unused)
        int ie = nr * 2;    // row * 2 + (1 = this nonzero is the last of its row); nr = no nonzero
        if (m < nn) {
            col = a.Aj[n0 + m];
            if constexpr (P::kPermuted) ax = P::ax(a.Ax[a.perm[n0 + m]]);
            else if constexpr (P::kValued) ax = P::ax(a.Ax[n0 + m]);
#include "slice_cut_row.inc"     // leaves lo: the nonzero's row, relative to r0
            ie = lo * 2 + (rel[lo + 1] == m + 1 ? 1 : 0);
        }
        const int left = nn - base;
        const int steps = slice_group_steps<C>(left);
        for (int t = 0; t < steps; ++t) {
            // slot s takes nonzero t * S + s of the 64
            int32_t col_s = col;
            acc_t ax_s = ax;
            int ie_s = ie;
            if constexpr (C > 1) {
                const int src = t * S + s;
                col_s = __shfl(col, src);
                if constexpr (P::kValued) ax_s = __shfl(ax, src);
                ie_s = __shfl(ie, src);
            }
            const int i_s = ie_s >> 1;
            acc_t p[V];
            if (i_s < nr) {
                acc_t xv[V];
                P::load_cols(xv, a.X + int64_t(col_s) * a.ldx + a.col_begin + c * V, nv, a.x_vec != 0);
                if constexpr (!P::kMaskCombine) {
#pragma unroll
                    for (int j = 0; j < V; ++j) p[j] = SR::combine(ax_s, xv[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) p[j] = j < nv ? SR::combine(ax_s, xv[j]) : SR::identity();
                }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) p[j] = SR::identity();
            }
            const int i_first = __shfl(ie_s, 0) >> 1;
            const int ie_last = __shfl(ie_s, kWave - 1);
            if (i_first == (ie_last >> 1) && !(ie_last & 1)) {
                // every slot is inside one row, and the row goes on: partials stay per slot
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = SR::reduce(acc[j], p[j]);
                open_i = i_first;
                holder = -2;
                continue;
            }
            // a row ends in this step (or the slice does).  The open row's partial joins slot 0, whose nonzero is the
            // next of that row; then a segmented inclusive scan over the slots reduces each row's run of products.
            if (open_i >= 0) {
                if (holder >= 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = __shfl(acc[j], holder * C + c);
                } else {
                    reduce_slots<SR, acc_t, V, C>(acc);
                }
                if (s == 0) {
#pragma unroll
                    for (int j = 0; j < V; ++j) p[j] = SR::reduce(p[j], acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = SR::identity();
            const int i_prev = __shfl_up(i_s, C);
            const bool head = s == 0 || i_prev != i_s;
            const unsigned long long heads = __ballot(head && c == 0);
            const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));   // lane c == 0 of the slot that starts this run
#pragma unroll
            for (int d = C; d < kWave; d <<= 1) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const acc_t o = __shfl_up(p[j], d);
                    if (lane - c - d >= start) p[j] = SR::reduce(p[j], o);
                }
            }
            const bool tail = s == S - 1 || ((heads >> (lane - c + C)) & 1ull);
            if (i_s < nr && tail && (ie_s & 1)) {
                if constexpr (P::kTails) {
                    if (i_s == 0 && carried_in) {
                        // the last piece of a row that crossed slices: as computed, for the fix-up (whole tiles fit carry_ld)
                        acc_t* tv = a.tail_val + w * a.carry_ld + a.col_begin + c * V;
#pragma unroll
                        for (int j = 0; j < V; ++j) tv[j] = p[j];
                    } else {
                        MI355_WALK_STORE_ROW(r0 + i_s, p);
                    }
                } else {
                    MI355_WALK_STORE_ROW(r0 + i_s, p);
                }
            }
            // the last nonzero of the step: if its row goes on, its run's reduction is the new open partial
            const int lv = min(S - 1, left - t * S - 1);
            const int ie_lv = __shfl(ie_s, lv * C);
            if (!(ie_lv & 1)) {
                open_i = ie_lv >> 1;
                holder = lv;
                if (s == lv) {
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = p[j];
                }
            } else {
                open_i = -1;
                holder = -1;
            }
        }
    }

    // the carry: what this slice holds of a row that ends in a later one
    if (open_i >= 0) {
        if (holder >= 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = __shfl(acc[j], holder * C + c);
        } else {
            reduce_slots<SR, acc_t, V, C>(acc);
        }
        if (s == 0) {
            acc_t* cv = a.carry_val + w * a.carry_ld + a.col_begin + c * V;    // (carry_ld covers whole tiles)
#pragma unroll
            for (int j = 0; j < V; ++j) cv[j] = acc[j];
        }
    }
    if (lane == 0) a.carry_row[w] = open_i >= 0 ? int32_t(r0 + open_i) : -1;

    // empty rows whose end lies in this slice: the identity through the row's end ((+, *): Y = beta * Y); a row with
    // nonzeros is stored where its last one is (and a row carried in has nonzeros: an empty row is never a tail piece)
    acc_t none[V];
#pragma unroll
    for (int j = 0; j < V; ++j) none[j] = SR::identity();
    for (int64_t r = r0 + s; r < r1; r += S)
        if (Ap[r] == Ap[r + 1]) MI355_WALK_STORE_ROW(r, none);
#undef MI355_WALK_STORE_ROW
