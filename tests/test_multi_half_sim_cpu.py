"""The multi-vector kernels with 16-bit vectors executed on the host, lane by lane (tests/cpp/multi_sim.cpp over
tests/cpp/simt, the one program of tests/test_multi_sim_cpu.py, tests/test_multi_semiring_sim_cpu.py and this file):
csrc/multi.hip with the headers it includes, unchanged, built with the address and undefined-behaviour
sanitizers and run over the WHOLE table of tests/multi_half_cases.py through the real mi355_spmv_multi_create_half /
set_alpha_beta / execute / destroy.  Each Y is held to the table's check exactly as the device run of the same table is
(tests/test_gpu_multi_half.py); the children must end with status 0 and must have written nothing to stderr (where
the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is loaded into
this process, and the children's environment is this process's own (the sanitizer runtimes are linked statically).
The program runs on the host only.

Cost (profiles/multi_sim_merge.txt): the table's 1 476 executes run as concurrent child processes (at most 8): about
half a minute on 8 cores, plus the compilation of the program where no other multi sim file has built it yet (287 s as
measured)."""
import pytest

import multi_cases as mc
import multi_half_cases as hc
import sim_runner as sr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, Y)}, and the children's reports."""
    return sr.run_table(sr.build("multi_sim"), tmp_path_factory.mktemp("multi_half_sim"),
                        sr.consecutive_runs(hc.table(), hc.plan_key), mc.weight, hc.write_batch, hc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_the_program_ran_the_whole_table(run):
    table = hc.self_test()
    assert {c.name for c in table} == set(run[0])


def test_every_case_is_held_to_the_contract(run):
    results = run[0]
    for c in hc.table():
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, y = results[c.name]
        assert status == 0, c.name
        hc.check(c, y)
