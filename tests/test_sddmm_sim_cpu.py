"""csrc/sddmm.hip executed on the host, lane by lane (tests/cpp/sddmm_sim.cpp over tests/cpp/simt): the kernel source
and its launch path, unchanged, built with the address and undefined-behaviour sanitizers and run over the WHOLE table
of tests/sddmm_cases.py — every structure, every k, both offset widths, both value types, valued and pattern.  Every
operand is an allocation exactly as long as the call may touch.  Each out is checked exactly as the device run of the
same table is (tests/test_gpu_sddmm.py), the children must end with status 0 and must have written nothing to stderr
(where the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is
loaded into this process, and the children's environment is this process's own (the sanitizer runtimes are linked
statically).

Cost: the table's ~1 300 executes take a few minutes of one core under the sanitizers; the batches run as concurrent
child processes (at most 8), plus ~15 s to compile the program once."""
import numpy as np
import pytest

import sddmm_cases as sc
import sim_runner as sr


def weight(g):
    """Of a plan group: merge items x lanes per slot."""
    return sum((len(c.matrix.lens) + sum(c.matrix.lens) + 2000) * (sc.lanes_per_slot(c.k, c.val) + 2) for c in g)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, out)}, and the children's reports."""
    exe = sr.build("sddmm_sim")
    sddmm, common = sr.source("sddmm.hip"), sr.source("common.hpp")
    assert sr.kernel_constant(sddmm, "kSddmmSlice") == sc.SLICE_LEN
    assert sr.kernel_constant(common, "kWave") == sc.STEP
    assert sr.kernel_constant(sddmm, "kSddmmGroupsMax") == max(sc.LANES_PER_SLOT)
    assert sr.kernel_constant(common, "kBlock") % sc.STEP == 0
    return sr.run_table(exe, tmp_path_factory.mktemp("sddmm_sim"), sr.groups_by(sc.table(), sc.plan_key), weight, sc.write_batch,
                        sc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_every_case_of_the_table_has_a_name_of_its_own_and_the_table_covers_what_it_says():
    table = sc.table()
    assert len({c.name for c in table}) == len(table) > 1000
    assert max(sum(c.matrix.lens) for c in table) < 60000
    ragged = [c for c in table if c.name.endswith("-cross")]
    for val in ("f32", "f64"):
        for k in sc.K_ALL[val]:
            assert {(c.off, c.valued) for c in ragged if c.val == val and c.k == k} == {(o, v) for o in ("i32", "i64") for v in (True, False)}
        assert {sc.lanes_per_slot(k, val) for k in sc.K_REDUCED[val]} == set(sc.LANES_PER_SLOT)
    assert {(c.alpha, c.beta) for c in table} >= set(sc.AB_REDUCED)
    assert any(c.ldu > c.k for c in table) and any(c.ldv > c.k for c in table)


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_family(run, family):
    results = run[0]
    cases = sc.family(family)
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, out = results[c.name]
        assert status == 0, c.name
        sc.check(c, out)


def test_alignment_changes_no_bit(run):
    results = run[0]
    for a, b in sc.alignment_pairs():
        assert np.array_equal(results[a.name][1].view(np.uint8), results[b.name][1].view(np.uint8)), a.name


def test_equal_rows_of_u_and_v_give_equal_bits_wherever_the_entry_lies(run):
    results = run[0]
    for a, b, ia, ib in sc.position_checks():
        oa, ob = results[a.name][1], results[b.name][1]
        assert ia.size > 100
        bad = np.nonzero(oa[ia].view(np.uint8).reshape(ia.size, -1) != ob[ib].view(np.uint8).reshape(ib.size, -1))[0]
        assert bad.size == 0, "%s vs %s: entries %s / %s differ" % (a.name, b.name, ia[bad[:8]], ib[bad[:8]])
