"""The multi-vector kernels with 16-bit vectors executed on the host, lane by lane (tests/cpp/multi_half_sim.cpp over
tests/cpp/simt): csrc/multi.hip with the headers it includes, unchanged, built with the address and undefined-behaviour
sanitizers and run over the WHOLE table of tests/multi_half_cases.py through the real mi355_spmv_multi_create_half /
set_alpha_beta / execute / destroy.  Each Y is held to the table's check exactly as the device run of the same table is
(tests/test_gpu_multi_half.py); the children must end with status 0 and must have written nothing to stderr (where
the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is loaded into
this process, and the children's environment is this process's own (the sanitizer runtimes are linked statically).
The program runs on the host only."""
import os
import subprocess

import pytest

import multi_half_cases as hc
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
TIME_LIMIT = 900        # seconds per child


def build():
    """The program, by the rule of tests/cpp/Makefile (its SIM_SAN flags).  Skips only where the host compiler cannot
    link with those flags at all; any other failure to build is a failure."""
    probe = subprocess.run(["make", "-s", "-C", CPP, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the host compiler cannot link with the sanitizer runtimes: " + probe.stderr.strip()[-300:])
    subprocess.run(["make", "-s", "-C", CPP, "multi_half_sim"], check=True)
    return os.path.join(CPP, "multi_half_sim")


def batches(cases, n):
    """Whole plan groups dealt to n batches, heaviest first onto the lightest batch (weight: merge items x columns)."""
    weight = lambda g: sum((len(c.matrix.lens) + sum(c.matrix.lens) + 2000) * (c.k + 8) for c in g)
    out = [[0, []] for _ in range(n)]
    for g in sorted(hc.groups(cases), key=weight, reverse=True):
        b = min(out, key=lambda b: b[0])
        b[0] += weight(g)
        b[1] += g
    return [b[1] for b in out if b[1]]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, Y)}, and the children's reports."""
    exe = build()
    tmp = tmp_path_factory.mktemp("multi_half_sim")
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    children = []
    for i, cases in enumerate(batches(hc.table(), max(1, min(8, cpus)))):
        src, dst = str(tmp / ("batch%d.bin" % i)), str(tmp / ("y%d.bin" % i))
        order = hc.write_batch(src, cases)
        children.append((subprocess.Popen([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env),
                         order, dst))
    results, reports = {}, []
    for child, order, dst in children:
        try:
            out, err = child.communicate(timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            child.kill()
            out, err = child.communicate()
            err += "\n(killed after %d s)" % TIME_LIMIT
        reports.append((child.returncode, out + err))
        if child.returncode == 0:
            for c, res in zip(order, hc.read_results(dst, order)):
                results[c.name] = res
    return results, reports


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
