"""The census of tests/sweep_cases.py: the table of chunk_rows_sweep cases reaches what it claims (no GPU).

sweep_cases.census() is a plain restatement of the body's DECOMPOSITION — the chunk, wave, slot and lane of every stored
element, its step, whether it is a register slot, a later-step gather or the scalar tail, and for a register slot the
pass whose window holds its column (or below c_lo / above c_hi / beyond the whole groups of x) — from Ap, Aj and the
hand-written shape alone.  It is never used for an expected y.  Asserted: the constants the table was written with are
the product's, every case reaches the states it names, every state the table is there for is reached for each value size
and each number of rows a vector holds, and check_shape() refuses malformed field sets on the host."""
import ctypes
import os

import numpy as np
import pytest

import sweep_cases as sc
from conftest import ROOT

CSRC = os.path.join(ROOT, "spmv-samples_amd", "csrc")


def test_constants_match_the_sources(sp):
    k = sc.source_constants()
    assert (k["kWave"], k["kHugeBlock"], k["kSweepRows"]) == (sc.WAVE, sc.K_HUGE_BLOCK, sc.K_SWEEP_ROWS)
    assert k["sweep_rows_for"] == (sc.SWEEP_ROWS_WIDE, sc.SWEEP_ROWS_WIDE_MAX, sc.SWEEP_ROWS_WIDE)
    assert k["lds_bytes"] == sc.SWEEP_LDS_BYTES == 155 * 1024
    assert k["round_bytes_per_thread"] * k["kHugeBlock"] == sc.ROUND_BYTES == 16 * 1024
    assert k["one_round_bytes_per_thread"] * k["kHugeBlock"] == sc.ROUND_BYTES          # launch_rows_sweep: >= one round
    assert k["light_resident_is_kCus"] and 2 * k["kCus"] == sc.LIGHT_STATIC_CHUNKS
    # one round is 4 096 columns in fp32 and 2 048 in fp64; the planner's rows per vector
    assert [sc.ROUND_BYTES // vb for vb in (4, 8)] == [4096, 2048]
    assert [sc.sweep_rows_for(4, t) for t in sc.LANES] == [4, 8, 8, 8, 8, 8] and {sc.sweep_rows_for(8, t) for t in sc.LANES} == {4}
    assert [sc.helds(4, t) for t in sc.LANES] == [(4,)] + [(4, 8)] * 5 and {sc.helds(8, t) for t in sc.LANES} == {(4,)}
    xw = open(os.path.join(CSRC, "xwindow.hpp")).read()
    launch = open(os.path.join(CSRC, "row_launch.hpp")).read()
    plan = open(os.path.join(CSRC, "rows_plan.hip")).read()
    # what check_shape() restates of launch_rows_sweep and chunk_lds_bytes
    assert ("if (p.rows_per_chunk != vectors * held || !(held == kSweepRows || (kHasEight && held == 8 && p.lanes_per_row >= 4)) ||\n"
            "        p.rows_cap < p.rows_per_chunk || p.window_elems < int(kHugeBlock * 16 / sizeof(val_t))) {") in launch
    assert "const int64_t vectors = kHugeBlock / p.lanes_per_row;" in launch and "constexpr bool kHasEight = sizeof(val_t) == 4;" in launch
    assert ("return lds_align16(size_t(window_elems) * val_bytes) + lds_align16(size_t(rows + 1) * 4) +\n"
            "           lds_align16(size_t(rows) * val_bytes) + lds_align16(size_t(rows / 32 + 1) * 4);") in xw
    # what census() restates of chunk_rows_sweep
    body = xw[xw.index("__device__ __forceinline__ void chunk_rows_sweep("):xw.index("// A chunk whose nonzeros span more than the 32-bit path")]
    for text in ("auto row_of = [&](int r) { return wave_rows0 + r * VW + row_in_wave; };",
                 "const int wave_rows0 = (tid / kWave) * (VW * R);",
                 "j = (lo & ~off_t(3)) + off_t(lane) * 4;",
                 "const bool mine = j + e >= lo && j + e < top;",
                 "int64_t l = chunk_begin + hint.lo, h = chunk_end - 1 + hint.hi;",
                 "l = l < 0 ? 0 : l;", "h = h >= n_cols ? int64_t(n_cols) - 1 : h;",
                 "const int whole_end = (n_cols & ~(PER16 - 1)) - 1;",
                 "const int c_lo = int(l) & ~(PER16 - 1), c_hi = int(h) < whole_end ? int(h) : whole_end;",
                 "cap = (cap / (BLOCK * PER16)) * (BLOCK * PER16);",
                 "for (int w0 = c_lo; w0 <= c_hi; w0 += cap) {",
                 "const int len = min(cap, c_hi + 1 - w0);",
                 "int full = (min((w0 + len + PER16 - 1) & ~(PER16 - 1), n_cols & ~(PER16 - 1)) - w0) / PER16;",
                 "const bool in = unsigned(c[r][e] - w0) < unsigned(len);",
                 "if (c[r][e] != INT32_MAX && (c[r][e] < c_lo || c[r][e] > c_hi))",
                 "for (off_t jj = j + off_t(T) * 4; jj < top; jj += off_t(T) * 4) {",
                 "for (off_t k = (lo > nnz_vec ? lo : nnz_vec); k < hi; ++k) sum[r] += Ax[k] * x[Aj[k]];"):
        assert text in body, text
    # a block copies the shape (no shaping), and light's single dequeue starts beyond two chunks per resident workgroup
    assert "p.sweep = w.window_sweep != 0;" in plan and "p.light_dequeue_once = !p.balanced && p.n_chunks > 2 * resident;" in plan
    assert ctypes.sizeof(sp.capi.PlanShape) == sc.SHAPE_BYTES
    assert [n for n, _ in sp.capi.PlanShape._fields_ if n not in ("seg_lo", "seg_hi")] == list(sc.sweep_shape("vector", "f32-i32", 8, 4, 1, (0, 9), 9, 9, 9))
    assert sp.capi.KINDS["vector"] == sc.KINDS["vector"] and sp.capi.KINDS["light"] == sc.KINDS["light"]


def test_case_names_are_unique_and_matrices_small():
    for vb in (4, 8):
        table = sc.table(vb)
        assert len({c.name for c in table}) == len(table) > 80
        assert {c.family for c in table} == set(sc.FAMILIES) - ({"light"} if vb == 4 else set())
        for c in table:
            big = c.family == "light"            # the dequeue-once matrix: the only one above a few thousand rows
            assert len(c.matrix.lens) <= (40_000 if big else 6200) and sum(c.matrix.lens) < 70_000 and c.matrix.n_cols < 80_000, c.name
            assert c.T in sc.FAMILY_LANES[c.family] and c.held in sc.helds(c.vb, c.T) and c.matrix.rpc == (1024 // c.T) * c.held
    for fam, name in sc.ALPHA_BETA_CASES.items():
        assert [c.family for c in sc.table(4) if c.name == name] == [fam], name
    assert set(sc.ALPHA_BETA_CASES) == set(sc.FAMILIES) - {"light"}


def test_every_case_has_a_shape_the_launcher_accepts():
    for c in sc.table():
        m = c.matrix
        for types in [t for t in sc.TYPES if np.dtype(sc.TYPES[t][0]).itemsize == c.vb]:
            for kind in sc.KINDS:
                f = sc.sweep_shape(kind, types, c.T, c.held, c.rounds, m.band, len(m.lens), m.n_cols, sum(m.lens))
                assert f["rows_per_chunk"] == m.rpc and f["window_elems"] == sc.cap_of(c)


@pytest.fixture(scope="module")
def reached():
    return {(c.name, c.vb): sc.census(c) for c in sc.table()}


def test_every_case_reaches_the_states_it_is_named_for(reached):
    for c in sc.table():
        missing = set(c.edge) - reached[(c.name, c.vb)]
        assert c.edge and not missing, (c.name, c.vb, sorted(missing))


def listed(vb, held):
    """The states of the issue's list, for one value size and one number of rows per vector."""
    P = 16 // vb
    out = {
        "window": ["l%%P=%d" % i for i in range(P)] + ["h%%P=%d" % i for i in range(P)] + ["ncols%%P=%d" % i for i in range(P)] +
                  ["staged_below_band", "col=c_lo-1", "partial_last_window", "partial_last_group", "full_last_window", "h_past_whole_end",
                   "beyond_whole_groups", "col=col_last", "clip0", "col=col0", "passes1", "passes2", "passes5", "passes16", "pass15",
                   "rounds1", "rounds2", "rounds9", "dma_reload_last_group", "dma_full_window"] +
                  ["col=%s@p%d" % (e, p) for e in sc.EDGES for p in range(3)] +
                  ["col=%s@p%d" % (e, p) for e in sc.EDGES[1:] for p in range(16)],
        "outside": ["%s@r%de%d" % (w, r, e) for w in ("below", "above") for r in range(held) for e in range(4)] +
                   ["row_all_outside", "lane_all_outside_neighbour_inside", "empty_sweep", "unsorted_row", "duplicate_in_row"],
        "rows": ["len0", "steps1", "steps2", "steps3", "steps4+", "second_step_by_phase", "long_row", "rowid_full_chunk",
                 "last_chunk=1", "last_chunk=VW-1", "last_chunk=VW", "last_chunk=rpc-1", "empty_at_chunk_end", "empty_at_chunk_start"] +
                ["len1@phase%d" % p for p in range(4)] +
                ["k%dd%+d@phase%d" % (k, d, p) for k, d in ((1, -1), (1, 0), (1, 1), (2, 0), (2, 1)) for p in range(4)] +
                ["corner_wave_%s_vector_%s_slot_%s" % (a, b, c) for a in ("first", "last") for b in ("first", "last") for c in ("first", "last")],
        "tail": ["tail%d_row_crosses" % r for r in (1, 2, 3)] + ["tail%d_empty_behind" % r for r in (1, 2, 3)] +
                ["tail%d_row_starts_at+0" % r for r in (1, 2, 3)] + ["tail2_row_starts_at+1", "tail3_row_starts_at+1", "tail3_row_starts_at+2",
                 "tail_row_starts_inside", "j_max_clamp", "tail_in_last_of_several_chunks", "nnz4", "nnz5", "nnz6", "nnz7", "scalar_tail"],
        "blocks": ["nnz%4=1", "tail1_row_starts_at+0"],
    }
    if vb == 8:
        out["light"] = ["light_dequeue_once"]
    return out


def test_every_state_is_reached_per_type_and_per_held(reached):
    table = sc.table()
    for vb in (4, 8):            # (f32-i64 runs the f32 structures: the offset width changes no decomposition)
        for held in (4, 8) if vb == 4 else (4,):
            for fam, names in listed(vb, held).items():
                lanes_hit = {}
                for c in table:
                    if (c.family, c.vb, c.held) == (fam, vb, held):
                        for s_ in set(names) & reached[(c.name, c.vb)] & set(c.edge):
                            lanes_hit.setdefault(s_, set()).add(c.T)
                for s_ in names:
                    assert s_ in lanes_hit, (fam, vb, held, s_)
                # rows and outside: at every T the kernels have for this `held`
                if fam in ("rows", "outside"):
                    want = {t for t in sc.LANES if held in sc.helds(vb, t)}
                    for s_ in names:
                        skip = {64} if s_ in ("last_chunk=VW-1", "last_chunk=VW") else set()      # (T = 64: one row per vector)
                        assert lanes_hit[s_] >= want - skip, (fam, vb, held, s_, sorted(want - lanes_hit[s_]))
    assert any("light_static" in v for v in reached.values())


def test_every_launchable_body_occurs(reached):
    """row_launch.hpp, launch_rows_sweep: T of with_lanes, four rows per vector, or eight in fp32 from T = 4 on."""
    for vb in (4, 8):
        have = {s_ for k, v in reached.items() if k[1] == vb for s_ in v if s_.startswith("T")}
        assert have == {"T%d_held%d" % (t, h) for t in sc.LANES for h in sc.helds(vb, t)}


def test_decomposition_is_a_partition():
    """Every stored element is exactly one of register slot / later step / scalar tail, a register slot sits in a lane
    below T at e = k % 4, and a slot that a pass holds lies inside that pass's window."""
    for c in sc.table():
        d = sc.decompose(c)
        Ap, Aj = sc.structure(c.matrix)
        reg = d["kind"] == sc.REG
        assert (d["lane"][reg] < c.T).all() and (d["step"][d["kind"] == sc.LATER] >= 1).all(), c.name
        assert (d["e"] == np.arange(int(Ap[-1])) % 4).all() and (d["r"] < c.held).all() and (d["wave"] < 16).all(), c.name
        cap = sc.cap_of(c)
        for ci, (rb, re_) in enumerate(sc.chunks_of(c)):
            sl = slice(int(Ap[rb]), int(Ap[re_]))
            w, col, sp_ = d["where"][sl], d["col"][sl], d["spans"][ci]
            held_ = w >= 0
            assert (w[held_] < len(sp_["passes"])).all(), c.name
            for p, (w0, ln) in enumerate(sp_["passes"]):
                at = w == p
                assert ((col[at] >= w0) & (col[at] < w0 + ln)).all() and ln <= cap, c.name


def test_operands_are_exact_and_leave_unreferenced_columns(oracle):
    seen = set()
    for c in sc.table():
        if (c.matrix.name, c.vb) in seen:
            continue
        seen.add((c.matrix.name, c.vb))
        Ap, Aj = sc.structure(c.matrix)
        for integer in (True, False) if c.family in sc.REAL_FAMILIES and c.matrix.data == "signs" else (True,):
            Ax, x, _ = sc.operands(c.matrix, c.vb, integer)
            assert np.isnan(x).any() and not np.isnan(x[Aj]).any(), c.name
            if integer and c.matrix.data == "signs":
                assert (Ax != 0).all() and (x[Aj] != 0).all() and np.diff(Ap).max() * 6 < 2 ** 24
        if c.matrix.data == "rowid":
            Ax, x, _ = sc.operands(c.matrix, c.vb, True)
            y = oracle.spmv_serial(Ap.astype(np.int32), Aj, Ax, x)
            assert (Ax != 0).all() and np.array_equal(y, np.arange(1, len(c.matrix.lens) + 1))


def test_block_cuts_start_at_every_phase_and_end_in_the_tail():
    for T in sc.FAMILY_LANES["blocks"]:
        for vb in (4, 8):
            for c in sc.family("blocks", T, vb):
                Ap = sc.structure(c.matrix)[0]
                nnz = int(Ap[-1])
                phases = set()
                for cuts in sc.block_cuts(c):
                    assert cuts[0][0] == 0 and cuts[-1][1] == len(c.matrix.lens) and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
                    for r0, r1 in cuts:
                        assert r0 % c.matrix.rpc == 0
                        phases.add(int(Ap[r0]) % 4)
                assert phases == {0, 1, 2, 3}
                r0 = sc.block_cuts(c)[1][-1][0]          # the last block of the second cutting: ends in the arrays' partial group
                assert int(Ap[r0]) % 4 == 3 and int(Ap[r0]) < (nnz & ~3) < nnz and nnz - (int(Ap[r0]) & ~3) >= 4


def test_check_shape_refuses_malformed_field_sets():
    good = sc.sweep_shape("vector", "f32-i32", 8, 4, 1, (-40, 5000), 700, 6000, 2100)
    sc.check_shape(dict(good))
    for types in ("f32-i32", "f64-i64"):
        for name, f in sc.refused_shapes(types):
            with pytest.raises(AssertionError):
                sc.check_shape(f)
    for bad in (dict(good, window_elems=good["window_elems"] + 4, window_bytes=good["window_bytes"] + 16),     # not whole rounds
                dict(good, window_elems=10 * 4096, window_bytes=10 * 16384),                                   # ten rounds: beyond 155 KB
                dict(good, lanes_per_row=3), dict(good, block_threads=512), dict(good, window_sweep=0),
                dict(good, nnz=3), dict(good, n_chunks=good["n_chunks"] + 1), dict(good, struct_bytes=200)):
        with pytest.raises(AssertionError):
            sc.check_shape(bad)
    with pytest.raises(AssertionError):
        sc.sweep_shape("vector", "f64-i64", 8, 8, 1, (-40, 5000), 700, 6000, 2100)          # eight rows of doubles
    with pytest.raises(AssertionError):
        sc.sweep_shape("vector", "f32-i32", 2, 8, 1, (-40, 5000), 700, 6000, 2100)          # eight rows at T = 2
    with pytest.raises(AssertionError):
        sc.sweep_shape("vector", "f32-i32", 2, 4, 9, (-40, 5000), 700, 6000, 2100)          # 2 048 rows leave eight rounds


def test_tie_matrix_is_what_the_planner_is_meant_to_sweep():
    """512 chunks at T = 64; the probed rows 129-256 long and showing both ends of the band; every other row short."""
    for vb in (4, 8):
        Ap, Aj, n_cols, band = sc.tie_matrix(vb)
        n = len(Ap) - 1
        held = sc.sweep_rows_for(vb, 64)
        assert n == 512 * 16 * held == {4: 65536, 8: 32768}[vb]
        lens = np.diff(Ap)
        probed = sc.rc.probed_rows(n)
        assert probed.size == 256 and lens[probed].min() == 129 and lens[probed].max() == 256
        rest = np.ones(n, dtype=bool)
        rest[probed] = False
        assert (lens[rest] == 3).all()
        off = Aj.astype(np.int64) - np.repeat(np.arange(n), lens)
        assert off.min() == 0 == band[0] and off.max() == band[1] == 2 * sc.TIE_HALF_BAND[vb] and Aj.max() < n_cols
        first, last = off[Ap[probed]], off[Ap[probed + 1] - 1]
        assert first.min() == 0 and last.max() == band[1]
        gaps = np.diff(np.sort(np.concatenate([first, last])))
        # one cluster, no window segment per band: cluster_bands splits at a gap wider than a workgroup's rows, and the
        # shortest chunk there is is one pass of 256 threads at two lanes per row, two rows per vector: 256 rows
        assert gaps.max() < 256
        # no window of any workgroup size holds the band (155 KB), and the sweep takes two passes of nine rounds
        assert vb * (band[1] - band[0] + 1 + 8) > 155 * 1024
        cap = sc.sweep_window_cap(vb, sc.chunk_lds_bytes(0, 16 * held, vb))
        assert cap == 9 * sc.ROUND_BYTES // vb and -(-(band[1] - band[0] + 1 + 16 * held + 8) // cap) == 2
