"""csrc/row_softmax.hip executed on the host, lane by lane (tests/cpp/row_softmax_sim.cpp over tests/cpp/simt): the kernel
source and its launch path, unchanged, built with the address and undefined-behaviour sanitizers and run over the WHOLE
table of tests/row_softmax_cases.py — every structure, forward and backward, both offset widths, both value types.  Every
operand is an allocation exactly as long as the call may touch.  Each result is checked exactly as the device run of the
same table is (tests/test_gpu_row_softmax.py), the children must end with status 0 and must have written nothing to
stderr (where the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is
loaded into this process, and the children's environment is this process's own (the sanitizer runtimes are linked
statically).

sim_runner.build makes the program by the rule of tests/cpp/Makefile, behind that Makefile's sanitizer_probe."""

import numpy as np
import pytest

import row_softmax_cases as rc
import sim_runner as sr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, out)}, and the children's reports."""
    exe = sr.build("row_softmax_sim")
    unit, common = sr.source("row_softmax.hip"), sr.source("common.hpp")
    assert sr.kernel_constant(unit, "kRowSoftmaxSlice") == rc.SLICE_LEN
    assert sr.kernel_constant(unit, "kRowSoftmaxGroups") == rc.GROUPS
    assert sr.kernel_constant(common, "kWave") == rc.STEP
    assert sr.kernel_constant(common, "kBlock") % rc.STEP == 0
    return sr.run_table(exe, tmp_path_factory.mktemp("row_softmax_sim"), sr.groups_by(rc.table(), rc.plan_key), rc.weight, rc.write_batch,
                        rc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_family(run, family):
    results = run[0]
    cases = rc.family(family)
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, out = results[c.name]
        assert status == 0, c.name
        rc.check(c, out)


def test_in_place_equals_out_of_place_bit_for_bit(run):
    results = run[0]
    pairs = rc.in_place_pairs()
    assert {(a.mode, b.in_place) for a, b in pairs} == {("fwd", 1), ("bwd", 1), ("bwd", 2)}
    for a, b in pairs:
        assert np.array_equal(results[a.name][1].view(np.uint8), results[b.name][1].view(np.uint8)), b.name


def test_two_executes_give_equal_bits(run):
    results = run[0]
    for a, b in rc.repeat_pairs():
        assert np.array_equal(results[a.name][1].view(np.uint8), results[b.name][1].view(np.uint8)), a.name
