"""csrc/sddmm_half_kernel.hpp — SDDMM with 16-bit U and V, fp32 values and arithmetic — executed on the host, lane by
lane (tests/cpp/sddmm_half_sim.cpp over tests/cpp/simt): the kernel source and its launch path, unchanged, built as a
stand-alone program with the address and undefined-behaviour sanitizers and run over the WHOLE table of
tests/sddmm_half_cases.py — every structure, every k, both offset widths, both 16-bit types, valued and pattern.  Every
operand is an allocation exactly as long as the call may touch.  Each out is checked exactly as the device run of the
same table is (tests/test_gpu_sddmm_half.py), the children must end with status 0 and must have written nothing to
stderr (where the sanitizers and the stand-in's out-of-step check report), and each runs under a time limit.  Nothing is
loaded into this process, and the children's environment is this process's own (the sanitizer runtimes are linked
statically).

Cost: the table's ~1 500 executes take a few minutes of one core under the sanitizers; the batches run as concurrent
child processes (at most 8), plus ~15 s to compile the program once."""
import os
import re
import subprocess

import numpy as np
import pytest

import sddmm_half_cases as sc
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
TIME_LIMIT = 900        # seconds per child


def build():
    """The program, built on demand with the sanitizer flags of the other host simulations.  Skips only where the host
    compiler cannot link with those flags at all (a trivial program, the same flags); any other failure to build is a
    failure."""
    probe = subprocess.run(["make", "-s", "-C", CPP, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the host compiler cannot link with the sanitizer runtimes: " + probe.stderr.strip()[-300:])
    subprocess.run(["make", "-s", "-C", CPP, "-f", "sddmm_half_sim.mk", "sddmm_half_sim"], check=True)
    return os.path.join(CPP, "sddmm_half_sim")


def kernel_constant(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def batches(cases, n):
    """Whole plan groups dealt to n batches, heaviest first onto the lightest batch (weight: merge items x lanes per slot)."""
    groups = {}
    for c in cases:
        groups.setdefault(sc.plan_key(c), []).append(c)
    weight = lambda g: sum((len(c.matrix.lens) + sum(c.matrix.lens) + 2000) * (sc.lanes_per_slot(c.k) + 2) for c in g)
    out = [[0, []] for _ in range(n)]
    for g in sorted(groups.values(), key=weight, reverse=True):
        b = min(out, key=lambda b: b[0])
        b[0] += weight(g)
        b[1] += g
    return [b[1] for b in out if b[1]]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, out)}, and the children's reports."""
    exe = build()
    csrc = os.path.join(ROOT, "spmv-samples_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    cut, common, cols, kernel = read("slice_cut.hpp"), read("common.hpp"), read("half_cols.hpp"), read("sddmm_half_kernel.hpp")
    assert kernel_constant(cut, "kSliceLen") == sc.SLICE_LEN
    assert kernel_constant(common, "kWave") == sc.STEP
    assert kernel_constant(cut, "kSliceGroupsMax") == max(sc.LANES_PER_SLOT)
    assert kernel_constant(common, "kBlock") % sc.STEP == 0
    assert kernel_constant(cols, "kHalfV") == sc.VEC and sc.TILE == sc.VEC * max(sc.LANES_PER_SLOT)
    assert "constexpr int W = mh::kHalfV;" in kernel and "with_slot_lanes((k + mh::kHalfV - 1) / mh::kHalfV" in kernel
    tmp = tmp_path_factory.mktemp("sddmm_half_sim")
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    children = []
    for i, cases in enumerate(batches(sc.table(), max(1, min(8, cpus)))):
        src, dst = str(tmp / ("batch%d.bin" % i)), str(tmp / ("out%d.bin" % i))
        order = sc.write_batch(src, cases)
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
            for c, res in zip(order, sc.read_results(dst, order)):
                results[c.name] = res
    return results, reports


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
