"""csrc/coo_csr.hip executed on the host, lane by lane (tests/cpp/coo_sim.cpp over tests/cpp/simt): the unit and its launch
paths, unchanged, built with the address and undefined-behaviour sanitizers as a stand-alone program and run over the WHOLE
table of tests/coo_cases.py through mi355_spmv_coo_to_csr, mi355_spmv_coo_to_csr_symmetric and mi355_spmv_csr_transpose, size
query included.  Every operand and the workspace is an allocation exactly as long as the call may touch, absent where the
case has none; outputs hold a canary first.

The bar is equality with numpy's stable sort (coo_cases.expected), for Ap, Aj, the bits of Ax and perm.  The children must
end with status 0 and must have written nothing to stderr (where the sanitizers and the stand-in's out-of-step check
report).  Nothing is loaded into this process, and the children's environment is this process's own (the sanitizer runtimes
are linked statically).

What the host execution cannot show is stated in the header of tests/cpp/coo_sim.cpp: orderings that only the lock step of a
wave provides.  tests/test_gpu_coo_edges.py runs the same table on the device.  profiles/coo_edges_mutations.txt records the
one-token errors this file catches.

sim_runner.build makes the program by the rule of tests/cpp/Makefile, behind that Makefile's sanitizer_probe."""
import re
import subprocess

import numpy as np
import pytest

import coo_cases as cc
import sim_runner as sr

# the table's geometry is the unit's
_unit, _common = sr.source("coo_csr.hip"), sr.source("common.hpp")
assert sr.kernel_constant(_common, "kWave") == cc.STEP
assert sr.kernel_constant(_unit, "kSteps") * cc.STEP == cc.QUARTER
assert sr.kernel_constant(_unit, "kSteps") * sr.kernel_constant(_common, "kBlock") == cc.TILE
assert sr.kernel_constant(_unit, "kScanItems") * sr.kernel_constant(_common, "kBlock") == cc.SCAN_CHUNK
assert re.search(r"constexpr int kTile = kBlock \* kSteps;", _unit) and re.search(r"constexpr int kScanChunk = kBlock \* kScanItems;", _unit)


@pytest.fixture(scope="module")
def exe():
    return sr.build("coo_sim")


@pytest.fixture(scope="module")
def run(exe, tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: what coo_cases.check takes}, and the children's
    reports."""
    return sr.run_table(exe, tmp_path_factory.mktemp("coo_sim"), [[c] for c in cc.table()], cc.weight, cc.write_batch, cc.read_results)


def cases_of(results, op, family):
    cases = [c for c in cc.table() if c.op == op and c.family == family]
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
    return cases


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_the_table_holds_every_family_it_promises():
    table = cc.table()
    good = [c for c in table if not c.bad]
    assert len({c.name for c in table}) == len(table)
    for op in cc.OPS:
        mine = [c for c in good if c.op == op]
        n_in = lambda c: len(cc.inputs(c)["Aj" if op == "transpose" else "rows"])
        # every count, at one pass and at two
        for d in (256, 257):
            assert {n_in(c) for c in mine if c.family == "counts" and cc.domain(c) == d} == set(cc.COUNTS)
        # every domain, every pass count 0 .. 4 (four: with a key whose top digit is 1), the five counts at passes 0 .. 3
        assert {cc.domain(c) for c in mine if c.family == "domains"} == set(cc.DOMAINS)
        for p in range(5):
            counts = {n_in(c) for c in mine if c.family == "domains" and cc.passes(cc.domain(c)) == p}
            assert counts >= (set(cc.CROSS) if p < 4 else {4097, 65537}), (op, p)
        for c in mine:
            if cc.passes(cc.domain(c)) == 4:
                x = cc.inputs(c)
                key = x["Aj"] if op == "transpose" else cc.expand(x["rows"], x["cols"])[0] if op == "sym" else x["rows"]
                assert (np.asarray(key) >> 24).max() == 1 and (np.asarray(key) >> 24).min() == 0, c.name
        assert 1 <= len([c for c in mine if c.family == "domains" and cc.domain(c) >= 1 << 24]) <= 4
        # every pattern at both counts and both domains
        assert {(c.args[2], c.args[0], c.args[1]) for c in mine if c.family == "patterns"} == \
            {(p, n, d) for p in cc.PATTERNS for n in cc.PATTERN_COUNTS for d in cc.PATTERN_DOMAINS}
        # every type triple, on three structures and over the rest of the table
        triples = {(c.off, c.val, c.perm) for c in mine}
        want = {(o, "none", True) for o in cc.OFFS} if op == "transpose" else set(cc.TYPE_PAIRS)
        assert triples == want
        by_structure = sr.groups_by([c for c in mine if c.family == "types"], lambda c: c.args)
        assert len(by_structure) == 3 and all({(c.off, c.val, c.perm) for c in g} == want for g in by_structure)
        assert {(c.off, c.val, c.perm) for c in mine if c.family != "types"} == want
        # workspace: every pass count under every prefill
        assert {(cc.passes(cc.domain(c)), c.prefill) for c in mine if c.family == "workspace"} == {(p, f) for p in range(5) for f in cc.PREFILLS}
    # what the patterns promise, on the keys themselves
    for d in cc.PATTERN_DOMAINS:
        for n in cc.PATTERN_COUNTS:
            k = {p: cc.keys(n, d, p, 0).astype(np.int64) for p in cc.PATTERNS}
            steps = lambda a: [a[s:s + 64] for s in range(0, n - 63, 64)]
            assert not k["zeros"].any() and (k["max"] == d - 1).all()
            assert set(k["alternate"][0::2]) == {0} and set(k["alternate"][1::2]) == {d - 1}
            assert (np.diff(k["ascending"]) >= 0).all() and (np.diff(k["descending"]) <= 0).all()
            if d >= n:
                assert (np.diff(k["ascending"]) == 1).all() and (np.diff(k["descending"]) == -1).all()
            assert all(len(set(s & 255)) == 64 for s in steps(k["distinct64"]))
            assert all(len(set(s[1:])) == 1 and s[0] != s[1] for s in steps(k["lane0"]))
            assert all(len(set(s[:63])) == 1 and s[63] != s[0] for s in steps(k["lane63"]))
            assert len(set(k["low_const"] & 255)) == 1 and len(set(k["high_const"] & 255)) > 200
            if d > 65535:
                assert len(set(k["low_const"] >> 8)) > 200 and len(set(k["high_const"] >> 8)) == 1
                assert set(k["d255_d0"] >> 8) == {0, 255}
            assert set(k["d255_d0"] & 255) == {0, 255}
        assert np.bincount(cc.keys(8193, d, "hub", 0)).max() > cc.TILE
    # sym: the expansion edges and the places of the off-diagonal entry
    sym = {c.name: cc.inputs(c) for c in good if c.op == "sym"}
    expanded = sorted((len(x["rows"]), x["nnz_expanded"]) for name, x in sym.items() if "-expanded-" in name)
    assert expanded == [(2047, 4094), (2048, 4096), (2049, 4098), (3000, 4095), (3000, 4096), (3000, 4097)]
    off_at = lambda tag: np.flatnonzero((lambda x: x["rows"] != x["cols"])(next(x for name, x in sym.items() if "-%s-" % tag in name)))
    assert off_at("offdiag_lane63").tolist() == [63] and off_at("offdiag_quarter_last")[0] == cc.QUARTER - 1
    assert off_at("offdiag_tile_last")[0] == cc.TILE - 1 and len(off_at("offdiag_tile_last")) > 1
    assert off_at("offdiag_tile_last_exact").tolist() == [cc.TILE - 1]
    assert off_at("offdiag_list_last").tolist() == [4999] and off_at("offdiag_list_last_tile_edge").tolist() == [2 * cc.TILE - 1]
    assert len(off_at("kind_diag")) == 0 and len(off_at("kind_offdiag")) == 5000 and 0 < len(off_at("kind_mixed")) < 5000
    assert {(x["n_rows"], x["n_cols"]) for x in sym.values()} >= {(300, 1000), (1000, 300), (1, 1), (3, 3)}
    # transpose: the empty runs, and the shapes
    tr = {c.name: cc.inputs(c) for c in good if c.op == "transpose" and c.family == "transpose"}
    lens = {name.split("-")[2]: np.diff(x["Ap"]) for name, x in tr.items()}
    for run_len in (1, 2, 300):
        assert not lens["%d_start" % run_len][:run_len].any() and lens["%d_start" % run_len][run_len] > 0
        assert not lens["%d_end" % run_len][-run_len:].any() and lens["%d_end" % run_len][-run_len - 1] > 0
        assert not lens["%d_middle" % run_len][20:20 + run_len].any() and lens["%d_middle" % run_len][19] > 0 < lens["%d_middle" % run_len][20 + run_len]
    assert lens["last_row_empty"][-1] == 0 and not lens["first_70_rows_empty"][:70].any() and lens["first_70_rows_empty"][70:].any()
    assert sorted(lens["one_row_holds_all"])[-2:] == [0, 5000] and lens["n_rows_1"].tolist() == [5000]
    assert tr[next(n for n in tr if "n_cols_1" in n)]["n_cols"] == 1
    assert np.bincount(tr[next(n for n in tr if "hub_column" in n)]["Aj"]).max() > cc.TILE
    assert {(x["n_rows"], x["n_cols"]) for x in tr.values()} >= {(2, 6), (6, 2)}
    # refusals: every offence first at entry 0, at the last entry, at 4 095 and at 4 096; the offsets' four
    bad = [c for c in table if c.bad]
    n = 2 * cc.TILE + 1
    for op, kinds in (("coo", ("row_minus_1", "row_n_rows", "col_n_cols")), ("sym", ("row_minus_1", "row_n_rows", "col_n_cols", "mirror_outside")),
                      ("transpose", ("col_minus_1", "col_n_cols"))):
        for kind in kinds:
            mine = [c for c in bad if c.op == op and "-%s_at" % kind in c.name]
            assert sorted(c.bad[0][0][1] for c in mine) == [0, cc.TILE - 1, cc.TILE, n - 1], (op, kind)
            assert all(len(c.bad[0]) == 2 and c.bad[0][1][1] > c.bad[0][0][1] for c in mine if c.bad[0][0][1] != n - 1)
    assert sorted(c.bad[0][0][2] for c in bad if c.bad[0][0][0] == "nnz_expanded") == [-1, 1]
    assert {c.name.split("-")[2] for c in bad if c.op == "transpose" and c.bad[0][0][0] == "Ap"} == \
        {"first_not_0", "descent", "last_not_nnz", "last_descends"}


@pytest.mark.parametrize("family", [f for f in cc.FAMILIES if f not in ("bad", "workspace", "sym", "transpose", "expanded")])
@pytest.mark.parametrize("op", cc.OPS)
def test_equals_the_stable_sort(run, op, family):
    for c in cases_of(run[0], op, family):
        cc.check(c, run[0][c.name])


@pytest.mark.parametrize("op,family", [("sym", "expanded"), ("sym", "sym"), ("transpose", "transpose")])
def test_own_structures_equal_the_stable_sort(run, op, family):
    for c in cases_of(run[0], op, family):
        cc.check(c, run[0][c.name])


@pytest.mark.parametrize("op", cc.OPS)
def test_refusals_name_the_first_offender_and_write_nothing(run, op):
    for c in cases_of(run[0], op, "bad"):
        cc.check(c, run[0][c.name])


@pytest.mark.parametrize("op", cc.OPS)
def test_the_result_does_not_depend_on_what_the_workspace_held(run, op):
    cases = cases_of(run[0], op, "workspace")
    for g in sr.groups_by(cases, lambda c: c.args):
        assert {c.prefill for c in g} == set(cc.PREFILLS)
        for c in g:
            cc.check(c, run[0][c.name])
            for k in ("Ap", "Aj", "Ax", "perm"):
                a, b = run[0][g[0].name][k], run[0][c.name][k]
                assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), (c.name, k)


@pytest.mark.parametrize("op", cc.KERNEL_OPS)
def test_kernels_alone_equal_a_host_prefix_sum(exe, tmp_path, op):
    kernels = [k for k in cc.kernel_cases() if k.op == op]
    assert kernels
    if op == "scan_sums":       # the carry between chunks of SCAN_CHUNK, and totals just below 2^32
        assert {k.n for k in kernels} == {1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193, 12293}
        assert any(int(k.data.astype(np.uint64).sum()) == 2 ** 32 - 1 and k.n > 2 * cc.SCAN_CHUNK for k in kernels)
    src, dst = str(tmp_path / "kernels.bin"), str(tmp_path / "kernels.out")
    cc.write_batch(src, [], kernels)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=sr.TIME_LIMIT, env=sr.child_env())
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    for k, got in zip(kernels, cc.read_results(dst, [], kernels)[1]):
        want = cc.kernel_expected(k)
        assert np.array_equal(got, want), "%s%s" % (k.name, cc.first_difference(got, want))
