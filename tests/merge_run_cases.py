"""The table of merge_rows_kernel cases (csrc/merge_path.hip: the row-parallel run kernel of a MERGE plan) that
tests/test_gpu_merge_run_edges.py executes on the device and whose reach tests/test_merge_run_cases_cpu.py proves on the
host.  The tile kernel's table is tests/merge_cases.py; its structures' tools (Rows, coords, TILE) are imported from
there, not copied.

Geometry.  The merge of the row ends with the nonzeros is cut into tiles of TILE items (merge_cases.py); a workgroup of
the run kernel owns a RUN of MI355_MERGE_TPS consecutive tiles, between the merge diagonals (row_lo, y_first) and
(row_last, y_last).  The rows [row_lo, row_last) END in the run and are stored by it (n_store_all of them); row
row_last, if the matrix has one, is open at the run's end and its part in the run becomes the run's carry
(n_all = n_store_all + 1).  The n_all rows are walked in PIECES of PIECE = kMergeRowsCap rows; the bounds of a piece's
rows are Ap clipped to [y_first, y_last), relative to base = y_first & ~3, and handed to the row-chunk body of the
vector kind (xwindow.hpp, chunk_rows_any, its REGULAR form): T = 2 / 4 / 8 / 16 / 32 lanes per row by the piece's mean
clipped length (<= 8, 16, 32, 64, beyond), a row whose CLIPPED length passes LONG = 4 T kLongSteps left to the wave
pass, beyond kHugeRow to the whole workgroup, elements from nnz & ~3 on to scalar code.  merge_fixup_kernel adds the
carries to the rows that close in a later run.  (The lane widths are the kernel's own five, not the three of a
weight-cut VECTOR plan in tests/row_cases.py: the run kernel instantiates the body's REGULAR branch.)

census() restates that DECOMPOSITION only — the runs, their pieces, every row's clipped length and the pass it gets —
and never computes a y.  Expected values come from the serial oracle alone.

Data.  Integer values without zeros ({+-1, +-2, +-3} x {+-1, +-2}): every sum is exact in any order and ONE element
leaking into or missing from a row changes it; "rowid" matrices of the pieces family give row r the sum r + 1 instead
(a row mapping shifted by a piece is seen); real values in (-1, 1) for the parity bound (run_edges, spanning, pieces,
tail).  The columns of a float x that no row references hold NaN.

Not here: the 512- and 1 024-thread run kernels, the sweeping runs (TS > 0) and the segmented runs (NSEG > 1).  Their
plans need MI355_MERGE_TPS unset and at least 2 kCus runs, so no small matrix reaches them; they stay with the at-size
tests of tests/test_gpu_parity.py (test_merge_runs_*), tests/test_gpu_merge_fallbacks.py, tests/test_gpu_block_shapes.py
and tests/test_gpu_kept_plans.py.  (The body the sweeping runs share with the vector and light kinds, chunk_rows_sweep,
has its edge table in tests/sweep_cases.py, on hand-written plan shapes; merge blocks are shaped on their own, so such a
shape does not reach merge_rows_kernel, and the run's clipping of the piece stays with the at-size tests.)"""
import collections
import os
import re

import numpy as np

from merge_cases import FUSED_MAX_DIAGONALS, NP_OFF, TILE, Rows, coords, ragged   # noqa: F401  (NP_OFF: for the device test)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spmv-samples_amd", "csrc")

# the literals the table was written with; source_constants() reads the same from the product's text
BLOCK = 256                          # kBlock: the only run kernel a forced-TPS plan takes
PIECE = 1984                         # kMergeRowsCap
K_LONG_STEPS = 16                    # kLongSteps
K_HUGE_ROW = 1024                    # kHugeRow
ADAPT_MEANS = (8, 16, 32, 64)        # chunk_rows_any, REGULAR: T = 2 / 4 / 8 / 16 / 32 at a piece mean <= 8, 16, 32, 64, beyond
ADAPT_LANES = (2, 4, 8, 16, 32)
ROWS_IN_FLIGHT = {4: 4, 8: 2}        # launch_merge_runs, RR: bytes of a value -> rows a vector keeps in flight
WINDOW_MIN_ITEMS = 8192              # run_window_elems: a shorter run gets no window of x
MAX_TILES = 40
MAX_COLS = 4096

TYPES = {"f32": np.float32, "f64": np.float64}
ALL_TYPES = tuple((off, val) for off in ("i32", "i64") for val in ("f32", "f64"))
ALPHA_BETA = (2.0, -1.0)             # integers: exact on integer data


def source_constants():
    """The same constants from csrc/*, as text: a changed constant fails test_merge_run_cases_cpu instead of moving an edge."""
    read = lambda f: open(os.path.join(CSRC, f)).read()
    path, plan, launch, xw, common = (read(f) for f in ("merge_path.hip", "merge_plan.hip", "merge_launch.hpp", "xwindow.hpp", "common.hpp"))
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    ipt = re.search(r"const int ipt = p\.block_threads == kWideBlock \? (\d+) : (\d+);", plan)
    rr = re.search(r"RR = sizeof\(val_t\) == 4 \? (\d+) : (\d+);", launch)
    regular = xw[xw.index("if constexpr (REGULAR)"):].split("return;", 1)[0]
    adapt = re.findall(r"(?:if \(mean <= (\d+)\)|else) chunk_rows<BLOCK, (\d+), R, WINDOW, val_t>", regular)
    return {
        "kBlock": const(common, "kBlock"), "kMergeRowsCap": const(path, "kMergeRowsCap"),
        "kLongSteps": const(xw, "kLongSteps"), "kHugeRow": const(xw, "kHugeRow"),
        "tile_items": const(common, "kBlock") * int(ipt.group(2)) - 4 if "p.tile_items = int64_t(p.block_threads) * ipt - 4;" in plan else None,
        "adapt_means": tuple(int(m) for m, _ in adapt if m), "adapt_lanes": tuple(int(t) for _, t in adapt),
        "rows_in_flight": {4: int(rr.group(1)), 8: int(rr.group(2))},
        "window_min_items": int(re.search(r"return \(tps \* p\.tile_items >= (\d+)\) \? pick_window_elems", plan).group(1)),
        # merge_rows_wanted: MI355_MERGE_ROWS = 0 | 1 decides before any size or regularity rule
        "rows_knob_first": bool(re.search(r"bool merge_rows_wanted\(const Plan& p\) \{\s+if \(p\.knob\.merge_rows >= 0\) return p\.knob\.merge_rows != 0;", plan)),
        # a forced-TPS plan walks pieces of kMergeRowsCap rows with the 256-thread kernel and its long-row defaults
        "piece_is_cap": "p.mr_piece_rows = segment_piece > 0 ? segment_piece : kMergeRowsCap;" in plan and "p.knob.merge_tps <= 0" in plan,
        "kernel_count": "return (p.n_super > 1 ? 2 : 1) + ((merge_search_in_kernel(p) && p.block_threads == kBlock) ? 0 : 1);" in plan,
        "fused_max_diagonals": int(re.search(r"if \(p\.tiles_per_super \+ 1 > (\d+)\) return false;", plan).group(1)),
        "run_body_is_regular_adapt": path.count("chunk_rows_any<BLOCK, 2, R, WINDOW, true, val_t, decltype(stage)&, true>") == 1,
        "long_steps_default": "int long_steps = kLongSteps;" in xw and "scr.long_steps" not in path,
    }


# cols: "pool" (a random half of the columns) | "band" (column = row // 2 + position; escapes ~3 000 further on)
# data: "signs" | "rowid";  escapes: nonzero numbers whose column lies far outside the band
Matrix = collections.namedtuple("Matrix", "name lens n_cols seed cols escapes data")
# knobs: the environment the plan is created under; edge: the census states the case is there for; window: the plan
# must have a window of x (else it must have none)
Case = collections.namedtuple("Case", "name family matrix knobs tps edge window")


def lanes_of(mean):
    for m, t in zip(ADAPT_MEANS, ADAPT_LANES):
        if mean <= m:
            return t
    return ADAPT_LANES[-1]


def long_of(T):
    return 4 * T * K_LONG_STEPS


def stride_of(T, R):
    """Rows of one group of chunk_rows: BLOCK / T vectors of R rows each (R = ROWS_IN_FLIGHT[bytes of a value])."""
    return (BLOCK // T) * R


# ---- the decomposition -------------------------------------------------------------------------------------------------
Run = collections.namedtuple("Run", "row_lo row_last y_first y_last n_store_all n_all clipped pieces")
# passes: per row of the piece 0 = its T lanes, 1 = the wave pass, 2 = the whole workgroup
Piece = collections.namedtuple("Piece", "pb pe rows store_rows mean T passes")
Census = collections.namedtuple("Census", "runs states n_tiles n_super run_row run_nnz")


def census(lens, tps, escapes=()):
    """The runs of merge_rows_kernel on a matrix of these row lengths at tps tiles per run, their pieces, every row's
    clipped length and pass, and the states all that reaches, as a set of names."""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    nnz = int(Ap[-1])
    xs, ys = coords(lens)
    n_tiles = len(xs) - 1
    n_super = -(-n_tiles // tps)
    cut = np.minimum(np.arange(n_super + 1) * tps, n_tiles)
    rr, ry = xs[cut], ys[cut]
    s = set()
    runs = []
    for u in range(n_super):
        row_lo, row_last, y_first, y_last = int(rr[u]), int(rr[u + 1]), int(ry[u]), int(ry[u + 1])
        n_store_all = row_last - row_lo
        n_all = n_store_all + (1 if row_last < n else 0)
        b = np.clip(Ap[np.minimum(np.arange(row_lo, row_lo + n_all + 1), n)], y_first, y_last)
        clipped = np.diff(b)
        pieces = []
        for pb in range(0, n_all, PIECE):
            pe = min(pb + PIECE, n_all)
            rows = pe - pb
            mean = int(b[pe] - b[pb]) // rows
            T = lanes_of(mean)
            cl = clipped[pb:pe]
            passes = np.where(cl > long_of(T), np.where(cl > K_HUGE_ROW, 2, 1), 0)
            pieces.append(Piece(pb, pe, rows, min(pe, n_store_all) - pb, mean, T, passes))
        runs.append(Run(row_lo, row_last, y_first, y_last, n_store_all, n_all, clipped, tuple(pieces)))
    # ---- runs
    s.add("single_run" if n_super == 1 else "several_runs")
    if n_tiles % tps:
        s.add("last_run_short")
    if n_super > 1:
        assert runs[-1].n_all == runs[-1].n_store_all           # (the last run's row_last is n_rows for EVERY matrix)
        s.add("no_open_row")
    whole = [r.n_store_all == 0 for r in runs]
    for u, r in enumerate(runs):
        opened = r.n_all > r.n_store_all
        if opened and r.clipped[-1] > 0:
            s.add("open_row")
        if opened and r.clipped[-1] == 0:
            s.add("run_ends_on_a_row_end")
        if whole[u]:
            s.add("whole_run_row")
            if r.row_last == 0:
                s.add("whole_run_row_is_first_row")
            if r.row_last == n - 1:
                s.add("whole_run_row_is_last_row")
            if Ap[r.row_last] == r.y_first and Ap[r.row_last + 1] == r.y_last:
                s.add("whole_run_row_exact")
            if u + 1 < n_super and whole[u + 1] and runs[u + 1].row_last == r.row_last:
                s.add("chain_2plus")
                if u + 2 < n_super and whole[u + 2] and runs[u + 2].row_last == r.row_last:
                    s.add("chain_3plus")
            if any(whole[v] and runs[v].row_last == r.row_last + 1 for v in range(u + 1, n_super)):
                s.add("whole_run_rows_back_to_back")
        # the stored rows and the pieces
        for name, v in (("PIECE-1", PIECE - 1), ("PIECE", PIECE), ("PIECE+1", PIECE + 1), ("2PIECE-1", 2 * PIECE - 1), ("2PIECE", 2 * PIECE)):
            if r.n_store_all == v:
                s.add("stored_rows=%s_%s" % (name, "open" if opened else "closed"))
        if len(r.pieces) == 2:
            s.add("pieces_2")
        if len(r.pieces) >= 3:
            s.add("pieces_3plus")
        if len(r.pieces) >= 5:
            s.add("pieces_5")
        if r.n_all % PIECE == 0:
            s.add("piece_exact")
        if len(r.pieces) >= 2:
            if Ap[r.row_lo] < r.y_first:
                s.add("carry_in_into_piece_0")
            if opened and r.clipped[-1] > 0:
                s.add("carry_out_of_a_later_piece")
            last = r.pieces[-1]
            if opened and last.rows == 1 and r.clipped[-1] > 0:
                s.add("open_row_alone_in_piece")            # (store_rows == 0 there: nothing but the carry)
            if not opened and last.rows == 1:
                s.add("stored_row_alone_in_piece")
        if opened and r.pieces[-1].rows == PIECE and r.clipped[-1] > 0:
            s.add("open_row_last_of_full_piece")
        # the rows
        own = lens[r.row_lo:r.row_lo + r.n_store_all]
        if r.n_store_all >= 3:
            if own[0] == 0 and Ap[r.row_lo] == r.y_first:
                s.add("empty_first")
            if own[-1] == 0:
                s.add("empty_last")
            if (own[1:-1] == 0).any():
                s.add("empty_between")
        for p in r.pieces:
            s.add("adaptT%d" % p.T)
            if p.rows >= 8 and p.mean in ADAPT_MEANS + tuple(m + 1 for m in ADAPT_MEANS):
                s.add("mean=%d" % p.mean)
            for R in sorted(set(ROWS_IN_FLIGHT.values())):       # rows of the piece against a group of (BLOCK / T) R rows
                for e in (-1, 0, 1):
                    if p.rows == stride_of(p.T, R) + e:
                        s.add("rows=stride%+d_R%d" % (e, R))
            LONG = long_of(p.T)
            cl = r.clipped[p.pb:p.pe]
            full = lens[np.minimum(np.arange(r.row_lo + p.pb, r.row_lo + p.pe), n - 1)]
            for i in np.nonzero((cl >= LONG) | (full > LONG))[0]:
                row = r.row_lo + p.pb + int(i)
                left = Ap[row] < r.y_first
                right = Ap[row + 1] > r.y_last
                where = "both" if left and right else "left" if left else "right" if right else None
                if cl[i] == LONG and where is None:
                    s.add("len=LONG@T%d" % p.T)
                if cl[i] == LONG + 1 and where is None:
                    s.add("len=LONG+1@T%d" % p.T)
                which = ("ordinary", "long", "huge")[int(p.passes[i])]
                if which == "ordinary":
                    if where and full[i] > LONG:
                        s.add("long_row_ordinary_part")      # (long as a whole, its part in this run is not)
                    continue
                s.add("%s_%s" % (which, "whole" if where is None else "clipped"))
                if where:
                    s.add("%s_clipped_%s" % (which, where))
                if where in ("right", "both") and row == r.row_last:
                    s.add("%s_row_is_the_carry" % which)
    # ---- the inner run boundaries
    for u in range(1, n_super):
        r, y = int(rr[u]), int(ry[u])
        k = y & 3
        if runs[u].y_last > y:
            s.add("phase%d" % k)
        if Ap[r] == y:
            name = "end_is_last_item" if r > 0 else None
            if lens[r] == 0:
                s.add("empty_row_behind_run_end")
        elif Ap[r + 1] == y:
            name = "end_is_first_item"
        else:
            left, right = y - Ap[r], Ap[r + 1] - y
            name = "cut_1_left" if left == 1 else "cut_1_right" if right == 1 else "cut_middle"
            if left == 1 and right == 1:
                s.add("cut_1_right")
        if name:
            s |= {name, "%s@phase%d" % (name, k)}
    if n_super > 1 and runs[-1].y_last == runs[-1].y_first and runs[-1].n_store_all == 1 and lens[n - 1] > 0:
        s.add("last_run_is_one_row_end")
    # ---- the arrays' tail
    if nnz == 4:
        s.add("nnz4")
    if n_super > 1:
        yl = runs[-1].y_first
        s.add("tail%d@phase%d" % (nnz & 3, yl & 3))
        if yl >= (nnz & ~3) and nnz > yl:
            s.add("last_run_starts_in_tail_%d" % (nnz - yl))
    if n > 0 and lens[n - 1] in (1, 2, 3, 5):
        s.add("last_row_len%d" % lens[n - 1])
    # ---- window escapes
    esc = np.asarray(escapes, dtype=np.int64)
    if len(esc):
        s |= {"escape_on_element_%d" % e for e in set((esc & 3).tolist())}
        row_of = np.searchsorted(Ap, esc, "right") - 1
        for u, r in enumerate(runs):
            inside = (esc >= r.y_first) & (esc < r.y_last)
            if (inside & (row_of == r.row_lo) & (Ap[r.row_lo] < r.y_first)).any():
                s.add("escape_in_a_row_cut_on_the_left")
            if r.n_all > r.n_store_all and (inside & (row_of == r.row_last)).any():
                s.add("escape_in_the_open_row")
            if u > 0 and (r.y_first & 3):
                g = r.y_first & ~3
                if ((esc >= g) & (esc < r.y_first)).any():
                    s.add("escape_left_of_a_cut_inside_a_group")
                if ((esc >= r.y_first) & (esc < g + 4)).any():
                    s.add("escape_right_of_a_cut_inside_a_group")
            for p in r.pieces[1:]:
                if (row_of == r.row_lo + p.pb - 1).any():
                    s.add("escape_in_last_row_of_a_piece")
                if (row_of == r.row_lo + p.pb).any():
                    s.add("escape_in_first_row_of_a_piece")
    return Census(tuple(runs), s, n_tiles, n_super, rr, ry)


_census = {}


def census_of(c):
    key = (c.matrix.name, c.tps)
    if key not in _census:
        _census[key] = census(c.matrix.lens, c.tps, c.matrix.escapes)
    return _census[key]


# ---- structures --------------------------------------------------------------------------------------------------------
SCENARIOS = ("end_is_last_item", "end_is_first_item", "cut_middle", "cut_1_left", "cut_1_right")


def fill(r, item, width):
    """Rows of `width` nonzeros (the last one up to twice that), the last of which ends on `item`."""
    assert item >= r.items, (item, r.items)
    while item - r.items >= 2 * (width + 1):
        r.add(width)
    return r.end_at(item)


def fill_phase(r, item, rows_mod4, width):
    """fill(), behind as many empty rows (0..7) as make the number of rows a multiple of 4 plus rows_mod4."""
    for e in range(8):
        t = Rows(r.lens)
        fill(t.add(*[0] * e), item, width)
        if len(t.lens) % 4 == rows_mod4:
            return fill(r.add(*[0] * e), item, width)
    raise AssertionError((item, rows_mod4, width))


def boundary(r, d, phase, scenario, width, left=9, right=13):
    """Rows up to and across the merge diagonal d (a run boundary), so that d - (row ends before d), the run's first
    nonzero, is `phase` modulo 4, and the row at the boundary is in the given scenario."""
    want = (d - phase) % 4                                   # row ends before d
    if scenario == "end_is_last_item":
        return fill_phase(r, d - 1, want, width)
    if scenario == "end_is_first_item":
        return fill_phase(r, d - 1 - left, want, width).end_at(d)
    a, b = {"cut_middle": (left, right), "cut_1_left": (1, right), "cut_1_right": (left, 1)}[scenario]
    return fill_phase(r, d - 1 - a, want, width).end_at(d + b)


def run_edge_matrices(tps, width):
    run = tps * TILE
    out = []
    for sc in SCENARIOS:                                     # boundary u at phase u - 1, then a short last run
        r = Rows()
        for u in range(1, 5):
            boundary(r, u * run, u - 1, sc, width)
        out.append(("%s_tps%d" % (sc, tps), fill(r, 4 * run + 300, width).lens))
    r = Rows()                                               # a run that ends exactly on a row end, an empty row behind it
    for u in range(1, 5):
        boundary(r, u * run, u - 1, "end_is_last_item", width).add(0)
    out.append(("empty_row_behind_run_end_tps%d" % tps, fill(r, 5 * run - 1, width).lens))   # ... and a full last run
    return out


def spanning_matrices(tps, width):
    run = tps * TILE
    h = run // 2
    out = []
    r = fill(Rows(), h, width).end_at(2 * run + h)           # one whole run, parts on both sides
    fill(r, 3 * run + h, width).end_at(6 * run + h)          # two
    fill(r, 7 * run + h, width).end_at(11 * run + h)         # three
    out.append(("whole_runs_1_2_3_tps%d" % tps, fill(r, 12 * run + 300, width).lens))
    r = fill(Rows(), h, width).end_at(2 * run + h).end_at(4 * run + h)
    out.append(("back_to_back_tps%d" % tps, fill(r, 5 * run + 300, width).lens))
    # a row that IS run 1, nothing more: its end is the first item of run 2, which row r + 1 then fills but for that item
    r = fill(Rows(), run - 1, width).end_at(2 * run).end_at(3 * run)
    out.append(("exact_tps%d" % tps, fill(r, 3 * run + 300, width).lens))
    r = Rows().end_at(2 * run + h)
    out.append(("first_row_tps%d" % tps, fill(r, 3 * run + 300, width).lens))
    r = fill(Rows(), h, width).end_at(3 * run + 40)
    out.append(("last_row_tps%d" % tps, r.lens))
    r = fill(Rows(), h, width).end_at(3 * run)                # ... and the last run is that row's end alone
    out.append(("last_row_end_alone_tps%d" % tps, r.lens))
    return out


def piece_matrix(tps, stored, pattern, opened, carry_in=10, width=37):
    """Run 1 stores exactly `stored` rows: the row that run 0 left open (carry_in nonzeros of it in run 1; 0: run 0 ends
    on a row end), then rows of the lengths of `pattern` in turn; behind them a row that stays open (opened) or nothing
    at all (run 1 is the last run and has no open row)."""
    run = tps * TILE
    r = Rows()
    if carry_in:
        fill(r, run - 20, width).end_at(run + carry_in)
    else:
        fill(r, run - 1, width)
    own = stored - (1 if carry_in else 0)
    r.add(*[pattern[i % len(pattern)] for i in range(own)])
    assert r.items <= 2 * run - 2, (r.items, run)
    if opened:
        r.end_at(2 * run + 25)
        fill(r, 2 * run + 400, width)
    return r.lens


def piece_matrices():
    out = []
    one, four = TILE, 4 * TILE
    for name, tps, stored, pattern, opened in (
            ("empty_rows_two_pieces", 1, 2001, (0,), True),
            ("stored_PIECE-1_open", 1, PIECE - 1, (0,), True),
            ("stored_PIECE_open", 1, PIECE, (0,), True),
            ("stored_PIECE_closed", 1, PIECE, (0,), False),
            ("stored_PIECE+1_open", 1, PIECE + 1, (0,), True),
            ("stored_PIECE+1_closed", 1, PIECE + 1, (0,), False),
            ("stored_2PIECE-1_open", 4, 2 * PIECE - 1, (1,), True),
            ("stored_2PIECE_open", 4, 2 * PIECE, (1,), True),
            ("stored_2PIECE_closed", 4, 2 * PIECE, (1,), False),
            ("ones_three_pieces", 4, (four - 40) // 2, (1,), True),
            ("mixed_012", 4, (four - 60) // 2, (0, 1, 2), True),
            ("empty_rows_five_pieces", 4, four - 40, (0,), True)):
        out.append((name, tps, piece_matrix(tps, stored, pattern, opened)))
    # no carry into the pieces: run 0 ends on a row end
    out.append(("mixed_012_no_carry_in", 4, piece_matrix(4, (four - 60) // 2, (0, 1, 2), True, carry_in=0)))
    assert one - 11 > 2001
    return out


def exact_run(r, d_end, head, width):
    """The rows of `head`, then rows of `width`, the last of which ends on the last item before diagonal d_end: the run
    that starts where r stands (on a row start) ends on a row end."""
    r.add(*head)
    return fill(r, d_end - 1, width)


def stride_matrix(tps=1):
    """(row lengths, the states reached).  One run per (R, e), R the rows a vector keeps in flight for 4- and 8-byte
    values and e in -1, 0, +1: the run starts on a row start, ends on a row end and holds k equal-as-can-be stored rows,
    with k such that the piece's k + 1 rows (the empty open part included) are one group of the lane width that their
    mean picks, plus e — the last group of the piece's walk is one row short, full, or one row alone."""
    run = tps * TILE
    r = Rows()
    reached = []
    for R in sorted(set(ROWS_IN_FLIGHT.values())):
        for e in (-1, 0, 1):
            for k in range(2, run // 2):
                if k + 1 == stride_of(lanes_of((run - k) // (k + 1)), R) + e:
                    base, extra = divmod(run - k, k)
                    r.add(*[base + (1 if i < extra else 0) for i in range(k)])
                    reached.append("rows=stride%+d_R%d" % (e, R))
                    assert r.items == len(reached) * run
                    break
    return r.add(7, 0, 3).lens, reached


def means_matrix(tps):
    """(row lengths, the means reached).  One run per mean of 8, 9, 16, 17, 32, 33, 64, 65 that a run of this length can
    have: each starts on a row start, stores k equal-as-can-be rows and ends on a row end, with k such that
    (clipped nonzeros) // (k + 1 rows, the empty open part included) is that mean; a short run behind them all."""
    run = tps * TILE
    r = Rows()
    reached = []
    for m in [m + e for m in ADAPT_MEANS for e in (0, 1)]:
        k = (run - m) // (m + 1)
        nz = run - k
        if nz // (k + 1) != m:                               # (no number of row ends gives a run of this length that mean)
            continue
        base, extra = divmod(nz, k)
        r.add(*[base + (1 if i < extra else 0) for i in range(k)])
        reached.append(m)
        assert r.items == len(reached) * run
    return r.add(7, 0, 3).lens, reached


def long_matrix(tps=4):
    """One run per lane width: rows of LONG and LONG + 1 nonzeros whole inside a run of short rows of that width's mean
    (LONG + 1 is the wave pass at T = 2, 4, 8, and already the whole workgroup's at T = 16, 32), a row beyond kHugeRow
    among rows of 3, and empty rows first, in between and last."""
    run = tps * TILE
    r = Rows()
    for u, (T, width) in enumerate(zip(ADAPT_LANES, (3, 12, 24, 40, 100))):
        L = long_of(T)
        assert L + L + 1 + 2 + 30 * (width + 1) < run, T
        head = [0, 0] + [width] * 6 + [L, width, 0, width, L + 1] + ([K_HUGE_ROW + 476] if T == 2 else [])
        exact_run(r, (u + 1) * run - 2, head, width).add(0, 0)
        assert r.items == (u + 1) * run
    return fill(r, 5 * run + 200, 37).lens


def clipped_matrix(phase, tps=4):
    """Long and huge rows cut by a run boundary, among rows of 3 (T = 2, LONG = 128): 200 | 300 (the wave pass on both
    sides), 1 100 | 1 200 (the whole workgroup on both sides), 100 | 300 and 300 | 100 (long as a whole, ordinary on one
    side), then a row over two whole runs (the whole workgroup, clipped on both sides).  Every boundary at `phase`."""
    run = tps * TILE
    r = Rows()
    for u, (a, b) in enumerate(((200, 300), (1100, 1200), (100, 300), (300, 100))):
        boundary(r, (u + 1) * run, phase, "cut_middle", 3, left=a, right=b)
    boundary(r, 5 * run, phase, "cut_middle", 3, left=150, right=2 * run + 700)
    return fill(r, 8 * run + 100, 3).lens


def tail_matrices(tps=2):
    run = tps * TILE
    out = []
    for k4 in range(4):
        for phase in range(4):
            last_len = (1, 2, 3, 5)[(k4 + phase) % 4]
            r = boundary(Rows(), run, phase, "cut_middle", 37)
            r.add(*ragged(300 + 4 * k4 + phase, 12, hi=9))
            nz = sum(r.lens)
            r.add(5 + (k4 - nz - 5 - last_len) % 4).add(last_len)
            assert sum(r.lens) % 4 == k4
            out.append(("tail%d_phase%d" % (k4, phase), tps, r.lens))
    for c, phase in ((1, 2), (2, 1), (3, 0)):                # the last run STARTS inside the arrays' tail: c nonzeros in it
        r = boundary(Rows(), run, phase, "cut_middle", 37, left=9, right=c)
        assert sum(r.lens) % 4 == phase + c
        out.append(("last_run_starts_in_tail_%d" % c, tps, r.add(0, 0).lens))
    out.append(("nnz_4", 2, [1, 0, 3]))
    for nnz in (5, 7, 8):
        out.append(("nnz_%d" % nnz, 2, [1, 0, nnz - 1]))
    out.append(("one_run_of_one_tile", 1, fill(Rows(ragged(71, 60)), TILE - 200, 9).lens))
    out.append(("one_run_of_three_tiles_of_four", 4, fill(Rows(ragged(72, 150)), 2 * TILE + 700, 21).lens))
    out.append(("one_run_of_exactly_its_tiles", 2, fill(Rows(ragged(73, 100)), 2 * TILE - 1, 13).lens))
    return out


def window_matrix(tps):
    """Rows of 40 in a band (column = row // 2 + position), a stretch of 2 100 rows of 3 in run 1 (two pieces), and
    single columns ~3 000 away (escapes): inside the rows that the run boundaries cut, inside the 16-byte groups that
    hold a boundary, and in the last row of piece 0 and the first of piece 1.  No escape is the first or last nonzero of
    its row or of a row's part in a run, so no sampled row widens the window towards it."""
    run = tps * TILE
    r = fill(Rows(), run + 500, 40)
    r.add(*[3] * 2100)
    assert r.items < 2 * run - 100
    lens = fill(r, 3 * run + 900, 40).lens
    cs = census(lens, tps)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    esc = set()
    for u, rn in enumerate(cs.runs):
        if u > 0:
            g = rn.y_first & ~3
            esc |= set(range(g, g + 4)) - {rn.y_first - 1, rn.y_first}
            esc |= {rn.y_first + 5, rn.y_first - 6}
        for p in rn.pieces[1:]:
            for row in (rn.row_lo + p.pb - 1, rn.row_lo + p.pb):
                esc.add(int(Ap[row]) + 1)
    edges = set(Ap.tolist()) | set((Ap - 1).tolist())
    for rn in cs.runs:
        edges |= {rn.y_first, rn.y_first - 1}
    return lens, tuple(sorted(e for e in esc - edges if 0 <= e < Ap[-1]))


# ---- the table ---------------------------------------------------------------------------------------------------------
FAMILIES = ("run_edges", "spanning", "pieces", "ragged", "tail", "search", "window")
REAL_FAMILIES = ("run_edges", "spanning", "pieces", "tail")
ALPHA_BETA_FAMILIES = ("run_edges", "spanning", "pieces")
FALLBACK_FAMILIES = ("pieces", "spanning")      # the executes the run kernel does not serve (test_gpu_merge_run_edges)
BASE = {"MI355_MERGE_ROWS": "1", "MI355_MERGE_FUSED": "1", "MI355_SPMV_WINDOW": "0"}
KNOB_NAMES = ("MI355_MERGE_TPS", "MI355_MERGE_FUSED", "MI355_MERGE_SEARCH_LANES", "MI355_MERGE_BLOCK", "MI355_MERGE_ROWS",
              "MI355_SPMV_WINDOW", "MI355_MERGE_SEGMENTS", "MI355_MERGE_WIDE_WINDOW", "MI355_SPMV_SWEEP", "MI355_SPMV_WINDOW_FROM_BAND", "MI355_SPMV_SEGMENTS")

PHASES = ["phase%d" % k for k in range(4)]
STATES = {
    "run_edges": ["%s@phase%d" % (sc, k) for sc in SCENARIOS for k in range(4)] + list(SCENARIOS) + PHASES + [
        "empty_row_behind_run_end", "run_ends_on_a_row_end", "no_open_row", "open_row", "several_runs", "empty_first"],
    "spanning": ["whole_run_row", "chain_2plus", "chain_3plus", "whole_run_row_is_first_row", "whole_run_row_is_last_row",
                 "whole_run_row_exact", "whole_run_rows_back_to_back", "last_run_is_one_row_end", "huge_clipped_both",
                 "huge_row_is_the_carry"],
    "pieces": ["pieces_2", "pieces_3plus", "pieces_5", "open_row_alone_in_piece", "open_row_last_of_full_piece", "piece_exact",
               "carry_in_into_piece_0", "carry_out_of_a_later_piece", "stored_row_alone_in_piece"] + [
        "stored_rows=%s" % v for v in ("PIECE-1_open", "PIECE_open", "PIECE_closed", "PIECE+1_open", "PIECE+1_closed",
                                       "2PIECE-1_open", "2PIECE_open", "2PIECE_closed")],
    "ragged": ["adaptT%d" % t for t in ADAPT_LANES] + ["mean=%d" % (m + e) for m in ADAPT_MEANS for e in (0, 1)] + [
        "len=LONG@T%d" % t for t in ADAPT_LANES] + ["len=LONG+1@T%d" % t for t in ADAPT_LANES] + [
        "long_whole", "huge_whole", "long_clipped", "long_clipped_left", "long_clipped_right", "huge_clipped", "huge_clipped_left",
        "huge_clipped_right", "huge_clipped_both", "long_row_is_the_carry", "huge_row_is_the_carry", "long_row_ordinary_part",
        "empty_first", "empty_between", "empty_last"] + [
        "rows=stride%+d_R%d" % (e, R) for R in sorted(set(ROWS_IN_FLIGHT.values())) for e in (-1, 0, 1)],
    "tail": ["tail%d@phase%d" % (k, p) for k in range(4) for p in range(4)] + ["last_row_len%d" % v for v in (1, 2, 3, 5)] + [
        "last_run_starts_in_tail_%d" % c for c in (1, 2, 3)] + ["nnz4", "single_run", "last_run_short"],
    "window": ["escape_on_element_%d" % e for e in range(4)] + [
        "escape_in_a_row_cut_on_the_left", "escape_in_the_open_row", "escape_left_of_a_cut_inside_a_group",
        "escape_right_of_a_cut_inside_a_group", "escape_in_last_row_of_a_piece", "escape_in_first_row_of_a_piece", "pieces_2"],
}


def states():
    """Every state the table must reach."""
    return set().union(*[set(v) for v in STATES.values()])


def _knobs(tps, **kw):
    k = dict(BASE, MI355_MERGE_TPS=str(tps))
    k.update({"MI355_" + name: str(v) for name, v in kw.items()})
    return k


_seed = [7000]


def _case(family, name, lens, tps, edge, n_cols=1500, cols="pool", escapes=(), data="signs", window=False, tag="", **kw):
    _seed[0] += 1
    m = Matrix(name, tuple(int(v) for v in lens), n_cols, _seed[0], cols, tuple(escapes), data)
    return Case(name + tag, family, m, _knobs(tps, **kw), tps, tuple(edge), window)


def _run_edge_cases(family, tag="", **kw):
    out = []
    for tps, width in ((1, 37), (2, 11)):
        for name, lens in run_edge_matrices(tps, width):
            sc = name.rsplit("_tps", 1)[0]
            if sc in SCENARIOS:
                edge = [sc] + ["%s@phase%d" % (sc, k) for k in range(4)] + PHASES + ["several_runs", "no_open_row"]
                edge += [] if sc in ("end_is_last_item", "end_is_first_item") else ["open_row"]
                edge += ["run_ends_on_a_row_end"] if sc == "end_is_last_item" else []
            else:
                edge = ["empty_row_behind_run_end", "run_ends_on_a_row_end", "empty_first"] + PHASES
            out.append(_case(family, name, lens, tps, edge, tag=tag, **kw))
    return out


def _spanning_cases(family, tag="", **kw):
    edges = {"whole_runs_1_2_3": ["whole_run_row", "chain_2plus", "chain_3plus"],
             "back_to_back": ["whole_run_row", "whole_run_rows_back_to_back"],
             "exact": ["whole_run_row", "whole_run_row_exact", "end_is_first_item", "end_is_last_item"],
             "first_row": ["whole_run_row", "whole_run_row_is_first_row", "chain_2plus"],
             "last_row": ["whole_run_row", "whole_run_row_is_last_row", "chain_2plus"],
             "last_row_end_alone": ["whole_run_row", "whole_run_row_is_last_row", "last_run_is_one_row_end", "end_is_first_item"]}
    out = []
    for tps, width in ((1, 37), (2, 5)):
        for name, lens in spanning_matrices(tps, width):
            edge = list(edges[name.rsplit("_tps", 1)[0]])
            if tps > 1:                                      # (a row of a whole run of 2 044 nonzeros is an ORDINARY row of T = 32)
                edge += ["huge_whole"] if name.startswith("exact") else ["huge_clipped_both", "huge_row_is_the_carry"]
            out.append(_case(family, name, lens, tps, edge, tag=tag, **kw))
    return out


def _table():
    _seed[0] = 7000
    out = _run_edge_cases("run_edges") + _spanning_cases("spanning")
    # pieces
    piece_edges = {
        "empty_rows_two_pieces": ["pieces_2", "carry_in_into_piece_0", "carry_out_of_a_later_piece"],
        "stored_PIECE-1_open": ["stored_rows=PIECE-1_open", "piece_exact", "open_row_last_of_full_piece"],
        "stored_PIECE_open": ["stored_rows=PIECE_open", "pieces_2", "open_row_alone_in_piece", "carry_in_into_piece_0"],
        "stored_PIECE_closed": ["stored_rows=PIECE_closed", "piece_exact"],
        "stored_PIECE+1_open": ["stored_rows=PIECE+1_open", "pieces_2", "carry_out_of_a_later_piece"],
        "stored_PIECE+1_closed": ["stored_rows=PIECE+1_closed", "pieces_2", "stored_row_alone_in_piece"],
        "stored_2PIECE-1_open": ["stored_rows=2PIECE-1_open", "pieces_2", "piece_exact", "open_row_last_of_full_piece"],
        "stored_2PIECE_open": ["stored_rows=2PIECE_open", "pieces_3plus", "open_row_alone_in_piece", "carry_in_into_piece_0"],
        "stored_2PIECE_closed": ["stored_rows=2PIECE_closed", "pieces_2", "piece_exact"],
        "ones_three_pieces": ["pieces_3plus", "carry_in_into_piece_0", "carry_out_of_a_later_piece"],
        "mixed_012": ["pieces_3plus", "carry_in_into_piece_0", "carry_out_of_a_later_piece"],
        "empty_rows_five_pieces": ["pieces_3plus", "pieces_5", "carry_in_into_piece_0"],
        "mixed_012_no_carry_in": ["pieces_3plus", "run_ends_on_a_row_end"]}
    pieces = piece_matrices()
    for name, tps, lens in pieces:
        out.append(_case("pieces", name, lens, tps, piece_edges[name]))
    for name, tps, lens in pieces:                           # row r sums to r + 1: a row mapping shifted by a piece is seen
        if name in ("stored_PIECE+1_open", "stored_2PIECE_open", "ones_three_pieces", "mixed_012"):
            out.append(_case("pieces", name + "_rowid", lens, tps, piece_edges[name], data="rowid"))
    # ragged
    for tps in (2, 3):
        lens, means = means_matrix(tps)
        out.append(_case("ragged", "means_tps%d" % tps, lens, tps,
                         ["mean=%d" % m for m in means] + sorted({"adaptT%d" % lanes_of(m) for m in means})))
    edge = ["len=LONG@T%d" % t for t in ADAPT_LANES] + ["len=LONG+1@T%d" % t for t in ADAPT_LANES]
    edge += ["adaptT%d" % t for t in ADAPT_LANES] + ["long_whole", "huge_whole", "empty_first", "empty_between", "empty_last"]
    out.append(_case("ragged", "long_rows_whole", long_matrix(), 4, edge))
    edge = ["long_clipped", "long_clipped_left", "long_clipped_right", "huge_clipped", "huge_clipped_left", "huge_clipped_right",
            "huge_clipped_both", "long_row_is_the_carry", "huge_row_is_the_carry", "long_row_ordinary_part", "whole_run_row",
            "chain_2plus", "adaptT2", "adaptT32"]
    for phase in range(4):
        out.append(_case("ragged", "long_rows_clipped_phase%d" % phase, clipped_matrix(phase), 4,
                         edge + ["cut_middle@phase%d" % phase], MERGE_FUSED=phase & 1))
    # tail
    for name, tps, lens in tail_matrices():
        if name.startswith("tail"):
            k4, phase = int(name[4]), int(name[-1])
            edge = ["tail%d@phase%d" % (k4, phase), "last_row_len%d" % (1, 2, 3, 5)[(k4 + phase) % 4], "last_run_short"]
        elif name.startswith("last_run_starts"):
            edge = [name, "last_run_short"]
        elif name == "nnz_4":
            edge = ["nnz4", "single_run"]
        else:
            edge = ["single_run"] + (["last_run_short"] if name in ("nnz_5", "nnz_7", "nnz_8", "one_run_of_three_tiles_of_four") else [])
        out.append(_case("tail", name, lens, tps, edge))
    # search: the search kernel in front (run_row / run_nnz) and the 16 lanes per diagonal in the kernel, on the same matrices
    for fused in (0, 1):
        tag = "-fused%d" % fused
        out += _run_edge_cases("search", tag=tag, MERGE_FUSED=fused) + _spanning_cases("search", tag=tag, MERGE_FUSED=fused)
    # window
    esc_edge = STATES["window"]
    for tps in (5, 8):
        lens, esc = window_matrix(tps)
        for win in (1, 0):
            out.append(_case("window", "band_with_escapes_tps%d" % tps, lens, tps, esc_edge, n_cols=MAX_COLS, cols="band",
                             escapes=esc, window=bool(win), tag="-window%d" % win, SPMV_WINDOW=win, MERGE_FUSED=win))
    # ragged again (behind the others, so that their seeds stay what profiles/merge_run_edges_mutations.txt ran): pieces of one group of rows
    lens, reached = stride_matrix()
    out.append(_case("ragged", "group_strides", lens, 1, reached))
    return out


_tables = []


def table():
    if not _tables:
        _tables.append(_table())
    return _tables[0]


def family(name):
    return [c for c in table() if c.family == name]


def fused_of(case):
    """Whether the run kernel searches its own two diagonals (merge_plan.hip, merge_search_in_kernel, under an explicit
    MI355_MERGE_FUSED)."""
    return case.knobs["MI355_MERGE_FUSED"] == "1" and case.tps + 1 <= FUSED_MAX_DIAGONALS


def n_kernels_of(case):
    """The search kernel in front unless the run kernel searches, the run kernel, the fix-up behind more than one run."""
    return (2 if census_of(case).n_super > 1 else 1) + (0 if fused_of(case) else 1)


# ---- operands ------------------------------------------------------------------------------------------------------------
_arrays = {}


def arrays(m, integer):
    """(Ap int64, Aj int32, Ax float64, x float64, y0 float64, used columns) of a matrix; made once and left unchanged.
    The caller casts, and puts NaN into the columns of x that are not used."""
    key = (m.name, m.seed, integer)
    if key not in _arrays:
        rng = np.random.RandomState(m.seed)
        lens = np.asarray(m.lens, dtype=np.int64)
        n = len(lens)
        Ap = np.concatenate(([0], np.cumsum(lens)))
        nnz = int(Ap[-1])
        if m.cols == "band":
            rows = np.repeat(np.arange(n), lens)
            Aj = rows // 2 + (np.arange(nnz) - Ap[rows])
            esc = np.asarray(m.escapes, dtype=np.int64)
            Aj[esc] = 3000 + (Aj[esc] + esc) % 1000
        else:
            pool = np.sort(rng.choice(m.n_cols, size=m.n_cols // 2, replace=False))
            Aj = pool[rng.randint(0, len(pool), size=nnz)]
        assert nnz == 0 or (Aj.min() >= 0 and Aj.max() < m.n_cols), m.name
        y0 = rng.randint(-5, 6, size=n).astype(np.float64)
        if m.data == "rowid":            # x = 1, values 1 except a row's last: row r sums to r + 1, and no value is 0
            assert integer
            Ax, x = np.ones(nnz), np.ones(m.n_cols)
            r = np.nonzero(lens)[0]
            last = (r + 1) - (lens[r] - 1)
            Ax[Ap[r + 1] - 1] = last
            z = r[last == 0]             # (r + 1 == len - 1, so len >= 2: first 2, last -1, the same sum)
            Ax[Ap[z]], Ax[Ap[z + 1] - 1] = 2, -1
        elif integer:
            Ax = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=nnz)
            x = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=m.n_cols)
        else:
            Ax, x = rng.rand(nnz) * 2 - 1, rng.rand(m.n_cols) * 2 - 1
            y0 = rng.rand(n) * 2 - 1
        used = np.zeros(m.n_cols, dtype=bool)
        used[Aj] = True
        _arrays[key] = (Ap, Aj.astype(np.int32), Ax, x, y0, used)
    return _arrays[key]


def operands(m, val, integer):
    """(Aj, Ax, x, y0) in value type `val`; x holds NaN where no row references it."""
    t = TYPES[val]
    Ap, Aj, Ax, x, y0, used = arrays(m, integer)
    xv = x.astype(t)
    xv[~used] = np.nan
    return Aj, Ax.astype(t), xv, y0.astype(t)
