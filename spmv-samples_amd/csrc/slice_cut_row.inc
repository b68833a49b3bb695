// slice_cut_row.inc — the row that owns nonzero m of the slice, included where a lane has loaded its nonzero of a group
// of 64 (multi_slice_walk.inc, sddmm_slice_walk.inc).  Text for slice_cut.inc's reason: as a __forceinline__ function the
// search reordered instructions in every slice kernel and changed the registers of three SDDMM kernels.
// In scope: rel, nr (slice_cut.inc) and m, 0 <= m < nn.  Leaves lo: row r0 + lo, the last i < nr with rel[i] <= m
// (empty rows repeat an offset: the last is the owner).
            int lo = 0, hi = nr - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (rel[mid] <= m) lo = mid; else hi = mid - 1;
            }
