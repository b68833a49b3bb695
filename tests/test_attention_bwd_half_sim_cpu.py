"""csrc/attention_bwd.hip with its 16-bit kernels (attention_bwd_half_kernel.hpp, attention_bwd_slice_walk.inc) executed on the
host, lane by lane (tests/cpp/attention_bwd_sim.cpp, the fp32 / fp64 table's program, over tests/cpp/simt): the kernel source
and its launch path, unchanged, built with the address and undefined-behaviour sanitizers as a stand-alone program and run over the WHOLE table of
tests/attention_bwd_half_cases.py — every structure as A and as A^T, every width pair, both offset widths, both 16-bit types
— through the real create_half (whose transpose is csrc/coo_csr.hip compiled the same way) / set_scale / execute / destroy.
Every operand is an allocation exactly as long as the call may touch.  Each result is checked exactly as the device run of
the same table is (tests/test_gpu_attention_bwd_half.py), the children must end with status 0 and must have written nothing
to stderr (where the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is
loaded into this process, and the children's environment is this process's own (the sanitizer runtimes are linked
statically)."""
import pytest

import attention_bwd_half_cases as bh
import sim_runner as sr

RATIOS = []


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, bad canaries, dQ, dK, dV, dbias)}, and the
    children's reports."""
    exe = sr.build("attention_bwd_sim")
    return sr.run_table(exe, tmp_path_factory.mktemp("attention_bwd_half_sim"), sr.groups_by(bh.table(), bh.plan_key), bh.weight, bh.write_batch,
                        bh.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


@pytest.mark.parametrize("family", bh.FAMILIES)
def test_family(run, family):
    results = run[0]
    cases = bh.family(family)
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, bad, dQ, dK, dV, dbias = results[c.name]
        assert status == 0, c.name
        assert bad == 0, "%s: %d padding elements of the outputs were written" % (c.name, bad)
        bh.check(c, dQ, dK, dV, dbias, ratios=RATIOS)


def test_the_largest_error_over_bound_of_the_real_cases(run):
    """Printed for DESIGN.md 3.15.3 (the host's figure); not asserted beyond <= 1, which every case has asserted already."""
    if not RATIOS:
        for c in bh.family("widths"):
            bh.check(c, *run[0][c.name][2:], ratios=RATIOS)
    print("16-bit attention backward on the host: largest error / bound over %d outputs of real cases: %.3f" % (len(RATIOS), max(RATIOS)))
    assert max(RATIOS) <= 1.0


def test_unaligned_operands_equal_aligned_ones_bit_for_bit(run):
    results = run[0]
    pairs = bh.alignment_pairs()
    assert pairs
    for a, b in pairs:
        for i in range(2, 6):
            assert sr.same_bits(results[a.name][i], results[b.name][i]), b.name


def test_two_executes_give_equal_bits(run):
    results = run[0]
    for a, b in bh.repeat_pairs():
        for i in range(2, 6):
            assert sr.same_bits(results[a.name][i], results[b.name][i]), a.name


def test_each_output_alone_equals_the_all_three_execute_and_dbias_leaves_dq_unchanged(run):
    results = run[0]
    groups = bh.need_groups()
    assert groups
    for both, dq, dk, dv in groups:
        assert results[dq.name][5] is None and results[both.name][5] is not None
        for alone, i in ((dq, 2), (dk, 3), (dv, 4)):
            assert sr.same_bits(results[both.name][i], results[alone.name][i]), alone.name
