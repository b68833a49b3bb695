"""csrc/multi.hip executed on the host, lane by lane (tests/cpp/multi_sim.cpp over tests/cpp/simt, the one program of
this file, tests/test_multi_semiring_sim_cpu.py and tests/test_multi_half_sim_cpu.py): the kernel source
and its launch path, unchanged, built with the address and undefined-behaviour sanitizers and run over the WHOLE table
of tests/multi_cases.py — every structure, every k of the crosses, both offset widths, both value types.  Each Y is
held to the oracle exactly as the device run of the same table is (tests/test_gpu_multi.py), the children must end
with status 0 and must have written nothing to stderr (where the sanitizers and the stand-in's out-of-step check
report), and each runs under a time limit.  Nothing is loaded into this process, and the children's environment is this
process's own (the sanitizer runtimes are linked statically).

Cost (profiles/multi_sim_merge.txt): the table's 5 180 executes take ~4 minutes of one core under the sanitizers; the
batches run as concurrent child processes (at most 8), so the file costs about a minute on 8 cores — the three multi sim
files together 86 s — plus the compilation of the program, once for the three files: 287 s as measured (every
instantiation of the kernels that multi.hip can launch; the three programs it replaced took 866 s together)."""
import subprocess

import pytest

import multi_cases as mc
import sim_runner as sr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, Y)}, and the children's reports."""
    exe = sr.build("multi_sim")
    multi, common = sr.source("multi.hip"), sr.source("common.hpp")
    assert sr.kernel_constant(multi, "kMultiSlice") == mc.SLICE_LEN
    assert sr.kernel_constant(common, "kWave") == mc.STEP
    assert sr.kernel_constant(multi, "kMultiGroupsMax") == max(mc.LANES_PER_SLOT)
    assert sr.kernel_constant(common, "kBlock") % mc.STEP == 0
    return sr.run_table(exe, tmp_path_factory.mktemp("multi_sim"), sr.groups_by(mc.table(), mc.plan_key), mc.weight, mc.write_batch,
                        mc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_every_case_of_the_table_has_a_name_of_its_own():
    table = mc.table()
    assert len({c.name for c in table}) == len(table) > 5000


def test_the_stand_in_keeps_its_own_promises():
    """tests/cpp/simt_selftest.cpp: shuffle, ballot and barrier semantics, block order and the hipMalloc fill; lanes out
    of step end the program with status 3 and a message naming the wave, not with a deadlock."""
    exe = sr.build("simt_selftest")
    r = subprocess.run([exe, "semantics"], capture_output=True, text=True, timeout=60, env=sr.child_env())
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    for mode, message in (("returned", "lanes have returned while others of the wave wait"),
                          ("kind", "out of step"), ("size", "out of step"), ("down", "out of step")):
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60, env=sr.child_env())
        assert r.returncode == 3, (mode, r.returncode, r.stderr[-2000:])
        assert "wave 0, collective 0: " in r.stderr and message in r.stderr and "lane  7" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_family(run, oracle, family):
    results = run[0]
    cases = mc.family(family)
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, y = results[c.name]
        assert status == 0, c.name
        mc.check(oracle, c, y)
