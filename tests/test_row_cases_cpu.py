"""The census of tests/row_cases.py: the table of chunk_rows cases reaches what it claims (no GPU).

row_cases.census() is a plain restatement of the kernel's DECOMPOSITION — the chunk a row falls in, its group and slot
under the row_of mapping, its phase, its step count, whether it is deferred, which pass sums it and whether it meets the
arrays' partial last group — from Ap and the plan's geometry alone.  It is never used for an expected y.  Asserted:
the constants the table was written with are the product's, every case reaches the edges it is named for, every
(T, R, block) the window kernels can be launched with occurs, and every listed state is reached at every T it is
listed for."""
import os

import numpy as np
import pytest

import row_cases as rc
from conftest import ROOT

CSRC = os.path.join(ROOT, "spmv-samples_amd", "csrc")


def test_constants_match_the_sources():
    k = rc.source_constants()
    assert k["kWave"] == rc.WAVE and (k["kBlock"], k["kWideBlock"]) == (rc.K_BLOCK, rc.K_WIDE_BLOCK)
    assert (k["kLongSteps"], k["kHugeRow"], k["kMaxChunkRows"]) == (rc.K_LONG_STEPS, rc.K_HUGE_ROW, rc.K_MAX_CHUNK_ROWS)
    assert k["kWindowBytes"] == rc.K_WINDOW_BYTES
    # rows_in_flight: (val_bytes == 4 && lanes < 16) ? 4 : 2
    assert k["rows_in_flight"] == (16, 4, 2)
    assert [rc.rows_in_flight(4, t) for t in rc.LANES] == [4, 4, 4, 2, 2, 2] and {rc.rows_in_flight(8, t) for t in rc.LANES} == {2}
    # chunk_rows_any, ADAPT: (mean <= 16: T = 2), (mean <= 64: T = 8), else T = 32
    assert k["adapt"] == (rc.ADAPT_MEANS[0], rc.ADAPT_LANES[0], rc.ADAPT_MEANS[1], rc.ADAPT_LANES[1], rc.ADAPT_LANES[2])
    assert k["balanced_long_steps"] == rc.BALANCED_LONG_STEPS and k["giant_row_min"] == rc.GIANT_ROW
    xw = open(os.path.join(CSRC, "xwindow.hpp")).read()
    plan = open(os.path.join(CSRC, "rows_plan.hip")).read()
    launch = open(os.path.join(CSRC, "row_launch.hpp")).read()
    # the predicates census() restates
    assert "deferred[r] = len_r > LONG || (scr.giant_len > 0 && int64_t(len_r) > scr.giant_len);" in xw
    assert "const off_t LONG = off_t(T) * 4 * scr.long_steps;" in xw
    assert "if (end - start > off_t(kHugeRow)) {" in xw and "if (end - start <= off_t(kHugeRow)) continue;" in xw
    assert "return g * STRIDE + wave_rows0 + r * VW + row_in_wave;" in xw
    assert "for (int64_t it = first; it < int64_t(hi_v); it += 2 * R * SLAB)" in xw
    assert "const off_t nnz_vec = nnz & ~off_t(3);" in xw
    # the planner rules plan_of() and chunk_bounds() restate
    assert "r = (r + pass - 1) / pass * pass;" in plan and "if (r >= pass && r <= kMaxChunkRows) rows = r;" in plan
    assert "p.bal_q = 2 * p.bal_k * r0;" in plan and "p.rows_cap = int(2 * r0 + 4);" in plan
    assert "chunk_row[c] = int32_t(lo & ~int64_t(3));" in plan
    assert [("case %d:" % t) in launch for t in rc.LANES] == [True] * 6


def test_case_names_are_unique_and_matrices_small():
    for vb in (4, 8):
        table = rc.table(vb)
        assert len({c.name for c in table}) == len(table) > 100
        assert {c.family for c in table} == set(rc.FAMILIES)
        for c in table:
            assert sum(c.matrix.lens) < 200_000 and len(c.matrix.lens) <= 8192 and c.matrix.n_cols < 20_000, c.name
            assert c.knobs["MI355_SPMV_SMALL"] == "0" and set(c.knobs) <= set(rc.KNOB_NAMES), c.name
            assert c.T in rc.FAMILY_LANES[c.family]
    for fam, name in rc.ALPHA_BETA_CASES.items():
        assert [c.family for c in rc.table(4) if c.name == name] == [fam], name


@pytest.fixture(scope="module")
def reached():
    return {(c.name, c.vb): rc.census(c) for c in rc.table()}


def test_every_case_reaches_the_edge_it_is_named_for(reached):
    for c in rc.table():
        missing = set(c.edge) - reached[(c.name, c.vb)]
        assert c.edge and not missing, (c.name, c.vb, sorted(missing))


def test_every_launchable_shape_occurs(reached):
    """row_launch.hpp, launch_rows_window: T of with_lanes, R = rows_in_flight(sizeof(val_t), T), 256 or 512 threads."""
    want = {"T%d_R%d_b%d" % (t, rc.rows_in_flight(vb, t), b) for t in rc.LANES for vb in (4, 8) for b in (rc.K_BLOCK, rc.K_WIDE_BLOCK)}
    have = {s for v in reached.values() for s in v if s.startswith("T")}
    assert have == want and len(want) == 18


def test_every_state_is_reached_at_every_lane_width_it_is_listed_for(reached):
    want = rc.states()
    # the lane widths each family runs at, as the issue sets them and NOT as the table declares them: all six unless the
    # family says otherwise (huge: 2, 16, 64; tail: 2, 8, 64).  adapt: the weight-cut kernel takes its width per chunk
    # (2 / 8 / 32, all three reached in one plan) and ignores the plan's own T, so one plan T is every T there is:
    launch = open(os.path.join(CSRC, "row_launch.hpp")).read()
    assert "vector width per chunk (chunk_rows_any); the T of the template is not used" in launch
    lanes = {"steps": rc.LANES, "long": rc.LANES, "huge": (2, 16, 64), "tail": (2, 8, 64), "groups": rc.LANES,
             "window": rc.LANES, "adapt": (8,)}
    assert rc.LANES == (2, 4, 8, 16, 32, 64) and lanes == rc.FAMILY_LANES
    at = ("step0", "later_step", "wave")
    # the states the issue lists, each for the lane widths of its family
    listed = {"steps": ("step1", "step2", "step3", "empty", "empty_group", "empty_vector", "second_step_by_phase", "len1@phase3",
                        "len4@phase0", "k1d-1@phase2", "k1d+0@phase1", "k2d+1@phase3"),
              "long": ("long-1", "long", "long+1", "marked=1", "marked=W", "marked=W+1", "marked=2W+1", "word0", "word1", "bit0",
                       "bit31", "bit32", "wave_phase0", "wave_phase3", "wave256k2-1", "wave256k2+0", "wave256k2+1", "wave256k3+1"),
              "huge": ("huge", "len=kHuge", "len=kHuge+1", "slabs1", "slabs2", "slabs3+", "two_huge_in_chunk", "huge_and_wave_in_chunk"),
              "tail": tuple("tail%d_%s" % (r, w) for r in (1, 2, 3) for w in ("ordinary", "wave", "huge")) +
                      ("starts_at_nnz_vec+0", "starts_at_nnz_vec+1", "starts_at_nnz_vec+2", "trailing_empty", "nnz4", "nnz5", "nnz7", "nnz8"),
              "groups": ("groups1", "groups2", "groups3", "groups4", "last_chunk=1", "last_chunk=S-1", "last_chunk=S", "last_chunk=S+1",
                         "single_chunk", "below_one_group"),
              "window": ("window_band", "window_sampled", "window_none", "window_segments", "escape_step0", "escape_later_step",
                         "escape_wave", "escape_low", "escape_high", "col0", "col_last") +
                        tuple("%s@%s" % (b, w) for b in rc.BOUNDARY for w in at),
              "adapt": ("adaptT2", "adaptT8", "adaptT32", "mean16", "mean17", "mean64", "mean65", "giant", "below_giant")}
    for fam, names in listed.items():
        for s in names:
            for t in lanes[fam]:
                hit = [k for k, v in reached.items() if s in v and any(c.T == t and c.name == k[0] and c.family == fam and s in c.edge
                                                                       for c in rc.family(fam, t, k[1]))]
                assert hit, (fam, s, t)
                assert t in want[s]
    # ... for both value sizes (R = 4 and R = 2 bodies)
    for vb in (4, 8):
        union = set().union(*[v for k, v in reached.items() if k[1] == vb])
        assert not set(want) - union, (vb, sorted(set(want) - union))


def test_default_long_steps_run_where_they_are_small():
    names = {c.name for c in rc.table(4)}
    assert all("long_T%d_R4_b256_ls16_default" % t in names for t in (2, 4, 8))


def test_weight_cut_chunks_have_the_means_they_are_named_for():
    for vb in (4, 8):
        c = [c for c in rc.family("adapt", 8, vb) if c.name == "adapt_means"][0]
        Ap = rc.structure(c.matrix)[0]
        b = rc.chunk_bounds(c)
        p = rc.plan_of(c)
        assert len(b) == p["n_chunks"] + 1 and b[0] == 0 and b[-1] == len(c.matrix.lens) and all(v % 4 == 0 for v in b[:-1])
        assert max(np.diff(b)) <= p["rows_cap"]
        means = {int(Ap[e] - Ap[s]) // (e - s) for s, e in zip(b[:-1], b[1:]) if e > s}
        assert {16, 17, 64, 65} <= means and min(means) <= 3 and max(means) >= 100


def test_operands_are_exact_and_leave_unreferenced_columns(oracle):
    """Integer data: no zero anywhere (one leaked or lost element changes a row's sum) and every partial sum far below
    2^24; x holds NaN in the columns no row references and the oracle's y is NaN-free all the same."""
    seen = set()
    for c in rc.table():
        if (c.matrix.name, c.vb) in seen:
            continue
        seen.add((c.matrix.name, c.vb))
        Ap, Aj = rc.structure(c.matrix)
        for integer in (True, False) if c.family in rc.REAL_FAMILIES else (True,):
            Ax, x, y0 = rc.operands(c.matrix, c.vb, integer)
            assert np.isnan(x).any() and not np.isnan(x[Aj]).any(), c.name
            if integer and c.matrix.data == "signs":
                assert (Ax != 0).all() and (x[Aj] != 0).all() and np.diff(Ap).max() * 6 < 2 ** 24
        if c.matrix.data == "rowid":
            Ax, x, _ = rc.operands(c.matrix, c.vb, True)
            assert (Ax != 0).all() and (x[Aj] == 1).all(), c.name
            y = oracle.spmv_serial(Ap.astype(np.int32), Aj, Ax, x)
            assert np.array_equal(y, np.arange(1, len(c.matrix.lens) + 1))


def test_window_cases_plant_the_edges_of_the_band_and_of_the_staged_window():
    """In both middle chunks of every band-window matrix: the band's extremes +- 1 as the issue names them, and — the
    window starts on a 16-byte boundary and is padded, so its edges are not the band's — the window's own first and last
    column (inside) and the column just outside each, all of them in a step-0 group, in a later step and in a long row."""
    for vb in (4, 8):
        for T in rc.LANES:
            for c in rc.family("window", T, vb):
                if rc.window_kind(c) != "band":
                    continue
                p = rc.plan_of(c)
                Ap, Aj = rc.structure(c.matrix)
                rpc = p["rows_per_chunk"]
                probed = set(int(v) for v in rc.probed_rows(len(c.matrix.lens)))
                assert not probed & {r for r, _, _ in c.matrix.planted}, c.name
                for rb in (rpc, 2 * rpc):
                    b = rc.boundary_columns(rb, rb + rpc, c.matrix.n_cols, p["band_window_elems"], vb)
                    w_lo, w_len = rc.band_window(rb, rb + rpc, c.matrix.n_cols, p["band_window_elems"], vb)
                    assert (b["band_lo"], b["band_hi"]) == (rb - rc.HW, rb + rpc - 1 + rc.HW)
                    assert w_lo % (16 // vb) == 0 and w_lo <= b["band_lo"] and (b["window_first"], b["window_last"]) == (w_lo, w_lo + w_len - 1)
                    held = set(int(v) for v in Aj[Ap[rb]:Ap[rb + rpc]])
                    assert set(b.values()) <= held, (c.name, rb)
