"""csrc/attention.hip executed on the host, lane by lane (tests/cpp/attention_sim.cpp over tests/cpp/simt): the kernel source
and its launch path, unchanged, built with the address and undefined-behaviour sanitizers and run over the WHOLE table of
tests/attention_cases.py — every structure, every width, both offset widths, both value types — through the real create /
set_scale / execute / destroy.  Every operand is an allocation exactly as long as the call may touch.  Each result is
checked exactly as the device run of the same table is (tests/test_gpu_attention.py), the children must end with status 0
and must have written nothing to stderr (where the sanitizers and the stand-in's out-of-step check report), and each runs
under a time limit.  Nothing is loaded into this process, and the children's environment is this process's own (the
sanitizer runtimes are linked statically).

The program is the 16-bit table's too (tests/test_attention_half_sim_cpu.py); sim_runner.build makes it by the rule of
tests/cpp/Makefile, behind that Makefile's sanitizer_probe."""
import pytest

import attention_cases as ac
import sim_runner as sr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, bad canaries, O, lse)}, and the
    children's reports."""
    exe = sr.build("attention_sim")
    unit, cut, common = sr.source("attention.hip"), sr.source("slice_cut.hpp"), sr.source("common.hpp")
    assert sr.kernel_constant(unit, "kAttentionSlice") == sr.kernel_constant(cut, "kSliceLen") == ac.SLICE_LEN
    assert sr.kernel_constant(unit, "kAttentionGroupsMax") == sr.kernel_constant(cut, "kSliceGroupsMax") == max(ac.LANES_PER_SLOT)
    assert sr.kernel_constant(common, "kWave") == ac.STEP
    assert sr.kernel_constant(common, "kBlock") % ac.STEP == 0
    return sr.run_table(exe, tmp_path_factory.mktemp("attention_sim"), sr.groups_by(ac.table(), ac.plan_key), ac.weight, ac.write_batch,
                        ac.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_family(run, family):
    results = run[0]
    cases = ac.family(family)
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, bad, O, lse = results[c.name]
        assert status == 0, c.name
        assert bad == 0, "%s: %d padding elements of O were written" % (c.name, bad)
        ac.check(c, O, lse)


def test_unaligned_operands_equal_aligned_ones_bit_for_bit(run):
    results = run[0]
    pairs = ac.alignment_pairs()
    assert pairs
    for a, b in pairs:
        assert sr.same_bits(results[a.name][2], results[b.name][2]) and sr.same_bits(results[a.name][3], results[b.name][3]), b.name


def test_two_executes_give_equal_bits(run):
    results = run[0]
    for a, b in ac.repeat_pairs():
        assert sr.same_bits(results[a.name][2], results[b.name][2]) and sr.same_bits(results[a.name][3], results[b.name][3]), a.name
