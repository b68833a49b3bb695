"""The census of tests/merge_run_cases.py: the table of merge_rows_kernel cases reaches what it claims (no GPU).

census() is a plain restatement of the run kernel's DECOMPOSITION — runs, pieces, clipped row bounds, the lane width and
the pass every row gets — on run boundaries that must equal oracle.merge_tile_coords taken every MI355_MERGE_TPS tiles.
It is never used for an expected y.  Asserted: the constants the table was written with are the sources'; every case
reaches the states it names; every listed state is reached by a case that names it; every case forces the run kernel
and its tiles per run; the table keeps within its size limits; the oracle's y is NaN-free on every matrix."""
import numpy as np
import pytest

import merge_cases as mc
import merge_run_cases as rc


def test_geometry_constants_match_the_sources():
    src = rc.source_constants()
    assert src["kBlock"] == rc.BLOCK
    assert src["kMergeRowsCap"] == rc.PIECE
    assert src["tile_items"] == rc.TILE == mc.TILE
    assert (src["kLongSteps"], src["kHugeRow"]) == (rc.K_LONG_STEPS, rc.K_HUGE_ROW)
    assert src["adapt_means"] == rc.ADAPT_MEANS and src["adapt_lanes"] == rc.ADAPT_LANES
    assert src["rows_in_flight"] == rc.ROWS_IN_FLIGHT
    assert src["window_min_items"] == rc.WINDOW_MIN_ITEMS
    assert src["fused_max_diagonals"] == rc.FUSED_MAX_DIAGONALS
    for name in ("rows_knob_first", "piece_is_cap", "kernel_count", "run_body_is_regular_adapt", "long_steps_default"):
        assert src[name], name


def test_case_names_are_unique_matrices_small_and_knobs_explicit():
    table = rc.table()
    assert len({c.name for c in table}) == len(table) >= 60
    assert {c.family for c in table} == set(rc.FAMILIES)
    by_name = {}
    for c in table:
        items = len(c.matrix.lens) + sum(c.matrix.lens)
        assert items <= rc.MAX_TILES * rc.TILE and c.matrix.n_cols <= rc.MAX_COLS, c.name
        assert sum(c.matrix.lens) >= 4, c.name                     # (vec = aligned && nnz >= 4: fewer never reach the run kernel)
        assert c.knobs["MI355_MERGE_ROWS"] == "1", c.name
        assert int(c.knobs["MI355_MERGE_TPS"]) == c.tps >= 1, c.name
        assert c.knobs["MI355_MERGE_FUSED"] in ("0", "1") and c.knobs["MI355_SPMV_WINDOW"] in ("0", "1"), c.name
        assert set(c.knobs) <= set(rc.KNOB_NAMES), c.name
        assert c.window == (c.knobs["MI355_SPMV_WINDOW"] == "1"), c.name
        if c.window:
            assert c.tps * rc.TILE >= rc.WINDOW_MIN_ITEMS, c.name
        assert by_name.setdefault(c.matrix.name, c.matrix.lens) == c.matrix.lens, c.name   # one structure per matrix name
    assert {c.knobs["MI355_MERGE_FUSED"] for c in rc.family("search")} == {"0", "1"}
    assert {c.tps for c in rc.family("window")} == {5, 8} and {c.window for c in rc.family("window")} == {True, False}
    assert {c.matrix.data for c in rc.family("pieces")} == {"signs", "rowid"}


def test_run_boundaries_equal_the_oracles_tile_coordinates(oracle):
    seen = set()
    for c in rc.table():
        if (c.matrix.name, c.tps) in seen:
            continue
        seen.add((c.matrix.name, c.tps))
        Ap = np.concatenate(([0], np.cumsum(np.asarray(c.matrix.lens, dtype=np.int64))))
        xs, ys = oracle.merge_tile_coords(Ap, rc.TILE)
        cs = rc.census_of(c)
        assert cs.n_tiles == len(xs) - 1 and cs.n_super == -(-cs.n_tiles // c.tps), c.name
        cut = np.minimum(np.arange(cs.n_super + 1) * c.tps, cs.n_tiles)
        assert np.array_equal(cs.run_row, xs[cut]) and np.array_equal(cs.run_nnz, ys[cut]), c.name
        n = len(c.matrix.lens)
        stored = 0
        for u, r in enumerate(cs.runs):
            assert (r.row_lo, r.y_first, r.row_last, r.y_last) == (xs[cut[u]], ys[cut[u]], xs[cut[u + 1]], ys[cut[u + 1]]), c.name
            assert r.n_all == r.n_store_all + (r.row_last < n) and r.n_all >= 1, c.name
            assert int(r.clipped.sum()) == r.y_last - r.y_first, c.name              # the clipped rows are the run's nonzeros
            assert [p.pb for p in r.pieces] == list(range(0, r.n_all, rc.PIECE)), c.name
            assert sum(p.store_rows for p in r.pieces) == r.n_store_all and all(p.store_rows >= 0 for p in r.pieces), c.name
            stored += r.n_store_all
        assert stored == n, c.name                                                   # every row is stored by exactly one run


def test_every_case_reaches_the_states_it_is_named_for():
    for c in rc.table():
        missing = set(c.edge) - rc.census_of(c).states
        assert not missing, (c.name, sorted(missing))


def test_every_state_is_reached_by_a_case_that_names_it():
    for fam in rc.FAMILIES:
        if fam == "search":                      # (its states are run_edges' and spanning's: the same matrices, the other search)
            continue
        named = set().union(*[set(c.edge) for c in rc.family(fam)])
        missing = set(rc.STATES[fam]) - named
        assert not missing, (fam, sorted(missing))
    named = set().union(*[set(c.edge) for c in rc.table()])
    assert not rc.states() - named, sorted(rc.states() - named)
    # the states the issue of this table asked for by name
    for s in ("pieces_2", "pieces_3plus", "whole_run_row", "chain_2plus", "end_is_first_item", "cut_1_left", "cut_1_right", "phase0",
              "phase1", "phase2", "phase3", "no_open_row", "open_row", "open_row_alone_in_piece", "piece_exact",
              "carry_in_into_piece_0", "adaptT2", "adaptT8", "adaptT32", "long_clipped", "huge_clipped", "long_whole", "single_run"):
        assert s in named, s
    # ... each search on every run_edges and spanning matrix
    base = {c.matrix.name for c in rc.family("run_edges") + rc.family("spanning")}
    for fused in ("0", "1"):
        assert {c.matrix.name for c in rc.family("search") if c.knobs["MI355_MERGE_FUSED"] == fused} == base


def test_the_passes_of_a_whole_run_row():
    """A row over a whole run of ONE tile is an ordinary row of 32 lanes (2 044 <= 4 * 32 * kLongSteps); over a run of two
    tiles and more it is the whole workgroup's: there is no wave-pass row clipped on both sides."""
    assert rc.TILE <= rc.long_of(32) < 2 * rc.TILE - 2 and rc.K_HUGE_ROW < rc.long_of(32)
    for c in rc.family("spanning"):
        for r in rc.census_of(c).runs:
            if r.n_store_all == 0:
                assert r.n_all == 1 and len(r.pieces) == 1 and r.pieces[0].T == 32, c.name
                assert int(r.pieces[0].passes[0]) == (0 if c.tps == 1 else 2), c.name
    assert "long_clipped_both" not in set().union(*[rc.census_of(c).states for c in rc.table()])


def test_escapes_lie_outside_the_band_and_inside_their_rows():
    for c in rc.family("window"):
        m = c.matrix
        Ap, Aj = rc.arrays(m, True)[:2]
        esc = np.asarray(m.escapes)
        assert len(esc) >= 8 and (Aj[esc] >= 3000).all(), c.name
        band = np.delete(Aj, esc)
        assert band.max() < 3000 - 500, c.name
        assert not np.isin(esc, Ap).any() and not np.isin(esc + 1, Ap).any(), c.name     # never a row's first or last nonzero


def test_operands_leave_unreferenced_columns_and_a_nan_free_reference(oracle):
    """Float x holds NaN in the columns no row references; the oracle's y of every matrix is NaN-free all the same, on
    integer and on real data; no integer value is zero, and a rowid matrix sums row r to r + 1."""
    seen = set()
    for c in rc.table():
        m = c.matrix
        if m.name in seen:
            continue
        seen.add(m.name)
        for integer in (True, False) if m.data == "signs" else (True,):
            Ap = rc.arrays(m, integer)[0]
            for val in ("f32", "f64"):
                Aj, Ax, x, y0 = rc.operands(m, val, integer)
                assert (Ax != 0).all() and not np.isnan(y0).any(), m.name
                if len(Aj) >= 8:
                    assert np.isnan(x).any(), m.name
                assert (x[Aj] != 0).all(), m.name
                y = oracle.spmv_genl_serial(0, Ap, Aj, Ax, x)
                assert not np.isnan(y).any(), (m.name, val, integer)
                if m.data == "rowid":
                    lens = np.asarray(m.lens)
                    assert np.array_equal(y, np.where(lens > 0, np.arange(len(lens)) + 1, 0).astype(y.dtype)), m.name
