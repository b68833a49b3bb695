"""The census of tests/functor_cases.py: the table of run-time functor cases reaches what it claims (no GPU).

census() is a plain restatement of the DECOMPOSITION of csrc/functor_kernel.inc under the launch shape of
csrc/functor_shape.hpp - T, the kernel that takes each row, the rounds of the two grid loops, the ballot's groups and
lanes, the walks' iterations, where a planted element lands.  It is never used for an expected y.  Asserted: the
constants the table was written with are the sources'; the kernel text is one raw string literal; every case reaches the
states it names; every state of every family is reached by a case that names it; the data are what the table's
docstring says; every functor of the table compiles (hiprtc needs no device).  The launch shape of the census is held
against the product's functor_shape in tests/test_functor_sim_cpu.py (read through the simulation program)."""
import os

import numpy as np
import torch

import functor_cases as fc


def test_geometry_constants_match_the_sources():
    src = fc.source_constants()
    assert src["kBlock"] == src["shape_block"] == fc.BLOCK and src["kWave"] == src["shape_wave"] == fc.WAVE
    assert src["kCus"] == fc.CUS
    assert src["step"] == (fc.STEP, fc.STEP, fc.STEP - 1) and src["running_values"] == [fc.STEP, fc.STEP]
    assert src["walk"] == (3, 4) and src["walk_tail_step_is_a_wave"]
    assert src["rows_kernels"] == src["lanes"] == fc.LANES and src["t_means"] == fc.T_MEANS
    assert src["long_per_lane"] == fc.LONG_PER_LANE and src["long_min"] == (fc.LONG_MIN, fc.LONG_MIN)
    assert src["rows_cap"] == (fc.ROWS_CAP // fc.CUS,) * 2 and src["long_cap"] == (fc.LONG_CAP // fc.CUS,) * 2
    assert src["mean_is_floor"] and src["long_launch_rule"] and src["long_row_rule"]
    assert {fc.long_len_of(T) for T in fc.LANES} == set(fc.LONG_LENS)


def test_the_kernel_text_is_one_raw_string_literal():
    with open(os.path.join(fc.CSRC, "functor_kernel.inc")) as f:
        lines = f.read().split("\n")
    assert lines[0] == 'R"MI355SRC(' and lines[-2:] == [')MI355SRC"', ""]
    assert not any("MI355SRC" in l for l in lines[1:-2])


def test_functor_rtc_keeps_no_shape_arithmetic():
    with open(os.path.join(fc.CSRC, "functor_rtc.hip")) as f:
        rtc = f.read()
    assert "functor_shape(n_rows, nnz)" in rtc
    for word in ("mean", "kCus *", "2048", "128ll", "rows_per_wg", "nnz > long", "kWave", "<<"):
        assert word not in rtc.split("mi355_spmv_functor_spmv(")[1], word


def test_case_names_are_unique_and_families_complete():
    table = fc.table()
    assert len({c.name for c in table}) == len(table) >= 80
    assert {c.family for c in table} == set(fc.FAMILIES)
    assert {c.typeset for c in table} == set(fc.TYPE_SETS)
    by_name = {}
    for c in table:
        assert by_name.setdefault(c.matrix.name, c.matrix.lens) == c.matrix.lens, c.name
        assert len(c.matrix.lens) >= 1 and c.shift in (0, 1, 3), c.name
    assert sorted({fc.TYPE_SETS[c.typeset].np_y.itemsize for c in table}) == list(fc.Y_BYTES)
    # ONE functor text for every handle (its issue allowed six); what it does not keep is one compile per text: a handle
    # is a (functor, five types) instantiation, and y of 1, 2, 4, 6, 8, 12 and 16 bytes, both offset widths, the five
    # semirings and the five-types mix need eleven of them: 0.2 s each on hiprtc (profiles/functor_edges_mutations.txt)
    assert os.path.basename(fc.TEXT_FILE) == "functor_texts.inc" and len(fc.TYPE_SETS) == 11
    assert len({ts.functor.split("<")[0] for ts in fc.TYPE_SETS.values()}) == 10
    big = [c for c in table if len(c.matrix.lens) > 100000]
    assert [c.name for c in big] == ["stride_true_caps-pt_f32"]
    n = len(big[0].matrix.lens)
    assert n == fc.CUS * 32 * 128 + 300 and 1.0e6 < sum(big[0].matrix.lens) < 1.2e6
    assert sum(big[0].matrix.lens) // n <= fc.T_MEANS[0]


def test_every_case_reaches_the_states_it_is_named_for():
    for c in fc.table():
        missing = set(c.edge) - fc.states_of(c)
        assert not missing, (c.name, sorted(missing))


def test_every_state_is_reached_by_a_case_that_names_it():
    unreached = {}
    for fam in fc.FAMILIES:
        named = set().union(*[set(c.edge) for c in fc.family(fam)])
        if set(fc.STATES[fam]) - named:
            unreached[fam] = sorted(set(fc.STATES[fam]) - named)
    assert not unreached, unreached
    # the planted maxima reach every position class under a functor that needs them
    extremum = [c for c in fc.table() if fc.TYPE_SETS[c.typeset].op not in ("plus_times", "count")]
    reached = set().union(*[fc.states_of(c) for c in extremum])
    assert set(fc.PLANT_STATES) <= reached, sorted(set(fc.PLANT_STATES) - reached)


def test_the_lanes_family_sits_on_both_sides_of_every_threshold():
    means = {}
    for c in fc.family("lanes"):
        n, nnz = len(c.matrix.lens), sum(c.matrix.lens)
        means.setdefault(nnz // n, []).append((nnz, n, fc.census_of(c).shape.T))
    for i, m in enumerate(fc.T_MEANS):
        assert {t for _, _, t in means[m]} == {fc.LANES[i]} and {t for _, _, t in means[m + 1]} == {fc.LANES[i + 1]}
        assert any(nnz == (m + 1) * n - 1 for nnz, n, _ in means[m]), m          # the floor decides


def test_long_rows_go_to_the_long_kernel_only_where_it_launches():
    for c in fc.table():
        cs = fc.census_of(c)
        lens = np.asarray(c.matrix.lens)
        assert np.array_equal(cs.long_rows, np.nonzero(lens > cs.shape.long_len)[0]), c.name
        assert cs.shape.long_launch or len(cs.long_rows) == 0, c.name
    assert any(len(fc.census_of(c).long_rows) == 0 and fc.census_of(c).shape.long_launch for c in fc.table())


def test_the_data_are_exact_poisoned_and_planted():
    seen = set()
    for c in fc.table():
        ts = fc.TYPE_SETS[c.typeset]
        if (c.matrix.name, ts.name) in seen or len(c.matrix.lens) > 100000:
            continue
        seen.add((c.matrix.name, ts.name))
        Ap, Aj, Ax, x = fc.operands(c)
        assert Ap.dtype == ts.np_off and Aj.dtype == np.int32 and Ax.dtype == ts.np_mat and x.dtype == ts.np_x, c.name
        assert (Ax != 0).all() and Aj.min(initial=0) >= 0 and Aj.max(initial=0) < fc.N_COLS, c.name
        used = np.zeros(fc.N_COLS, dtype=bool)
        used[Aj] = True
        if np.issubdtype(ts.np_x, np.floating):
            assert np.isnan(x[~used]).all() and not np.isnan(x[used]).any(), c.name
        else:
            assert (x[~used].view(np.uint8) == fc.FILL).all(), c.name
        if ts.plant != "or":
            assert (x[used] != 0).all(), c.name
        want = fc.expected(c)
        assert want.dtype == ts.np_y and len(want) == len(c.matrix.lens), c.name
        fill = np.full(1, fc.FILL, dtype=np.uint8).repeat(ts.np_y.itemsize).view(ts.np_y)[0]
        assert not (want == fill).any(), c.name                                  # no result equals the prefill of y
        # a planted maximum is the unique maximum of its row's terms (and the minimum the unique minimum)
        if c.matrix.plant and ts.op in ("min_plus", "max_plus", "max_times", "min_plus_i16", "stat12"):
            a, b = Ax.astype(np.float64), x.astype(np.float64)[Aj]
            terms = a + b if ts.plant == "plus" else a * b
            lens = np.asarray(c.matrix.lens)
            hi, lo = fc.plant_positions(lens, fc.census_of(c).shape.T)
            for r in np.nonzero(hi >= 0)[0][:200]:
                row = terms[Ap[r]:Ap[r + 1]]
                assert row.argmax() == hi[r] and (row == row.max()).sum() == 1, (c.name, r)
                assert row.argmin() == lo[r] and (row == row.min()).sum() == 1, (c.name, r)


def test_every_functor_of_the_table_compiles(sp):
    dt = {"int": torch.int32, "long long": torch.int64}
    for ts in fc.TYPE_SETS.values():
        f = sp.Functor(fc.text(), ts.functor, dt[ts.off], ts.mat, ts.x, ts.y)
        assert f.log == "", (ts.name, f.log)
        f.destroy()
