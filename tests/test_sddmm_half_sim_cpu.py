"""csrc/sddmm_half_kernel.hpp — SDDMM with 16-bit U and V, fp32 values and arithmetic — executed on the host, lane by
lane (tests/cpp/sddmm_sim.cpp over tests/cpp/simt, the one program of tests/test_sddmm_sim_cpu.py and this file): the
kernel source and its launch path, unchanged, built as a stand-alone program with the address and undefined-behaviour sanitizers and run over the WHOLE table of
tests/sddmm_half_cases.py — every structure, every k, both offset widths, both 16-bit types, valued and pattern.  Every
operand is an allocation exactly as long as the call may touch.  Each out is checked exactly as the device run of the
same table is (tests/test_gpu_sddmm_half.py), the children must end with status 0 and must have written nothing to
stderr (where the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is
loaded into this process, and the children's environment is this process's own (the sanitizer runtimes are linked
statically).

Cost: the table's ~1 500 executes take a few minutes of one core under the sanitizers; the batches run as concurrent
child processes (at most 8), plus ~15 s to compile the program once."""
import numpy as np
import pytest

import sddmm_half_cases as sc
import sim_runner as sr


def weight(g):
    """Of a plan group: merge items x lanes per slot."""
    return sum((len(c.matrix.lens) + sum(c.matrix.lens) + 2000) * (sc.lanes_per_slot(c.k) + 2) for c in g)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, out)}, and the children's reports."""
    exe = sr.build("sddmm_sim")
    cut, common, cols, kernel = sr.source("slice_cut.hpp"), sr.source("common.hpp"), sr.source("half_cols.hpp"), sr.source("sddmm_half_kernel.hpp")
    assert sr.kernel_constant(cut, "kSliceLen") == sc.SLICE_LEN
    assert sr.kernel_constant(common, "kWave") == sc.STEP
    assert sr.kernel_constant(cut, "kSliceGroupsMax") == max(sc.LANES_PER_SLOT)
    assert sr.kernel_constant(common, "kBlock") % sc.STEP == 0
    assert sr.kernel_constant(cols, "kHalfV") == sc.VEC and sc.TILE == sc.VEC * max(sc.LANES_PER_SLOT)
    assert "constexpr int W = mh::kHalfV;" in kernel and "with_slot_lanes((k + mh::kHalfV - 1) / mh::kHalfV" in kernel
    return sr.run_table(exe, tmp_path_factory.mktemp("sddmm_half_sim"), sr.groups_by(sc.table(), sc.plan_key), weight, sc.write_batch,
                        sc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_the_table_covers_what_it_says():
    sc.self_test()


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
