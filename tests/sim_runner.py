"""What the host simulations' test files (tests/test_*_sim_cpu.py) share: building a program of tests/cpp with the
sanitizers, dealing a table's plan groups to batches, running the batches as concurrent child processes under a time
limit, and comparing two results bit for bit.  Nothing is loaded into this process, and the children's environment is this
process's own (the sanitizer runtimes are linked statically).  Each test file keeps its table, its geometry asserts, its
tests and its weight function (the three multi-vector files: the one multi_cases.weight)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
TIME_LIMIT = 900        # seconds per child: ~30 x what the slowest batch of any table takes


def build(target, *variables):
    """The program, built on demand by the one rule of tests/cpp/Makefile for every host simulation (its SIM_SAN flags);
    variables: NAME=value words for make's command line (the functor simulation's type names).
    Skips only where the host compiler cannot link with those flags at all (a trivial program, the same flags); any other
    failure to build is a failure."""
    probe = subprocess.run(["make", "-s", "-C", CPP, "sanitizer_probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the host compiler cannot link with the sanitizer runtimes: " + probe.stderr.strip()[-300:])
    subprocess.run(["make", "-s", "-C", CPP, target] + list(variables), check=True)
    return os.path.join(CPP, target)


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def child_env():
    return dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")


def source(name):
    """The text of a file of csrc/."""
    with open(os.path.join(ROOT, "spmv-samples_amd", "csrc", name)) as f:
        return f.read()


def kernel_constant(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def groups_by(cases, key):
    """The cases of each key together, in the order the keys first occur."""
    groups = {}
    for c in cases:
        groups.setdefault(key(c), []).append(c)
    return list(groups.values())


def consecutive_runs(cases, key):
    """Runs of consecutive cases of one key, in table order: for a table that ends in ordered sequences on one object,
    whose cases must stay behind one another (the device files cut their tables the same way)."""
    out = []
    for c in cases:
        if out and key(out[-1][0]) == key(c):
            out[-1].append(c)
        else:
            out.append([c])
    return out


def batches(groups, weight, n):
    """Whole plan groups dealt to at most n batches, heaviest first onto the lightest batch."""
    out = [[0, []] for _ in range(n)]
    for g in sorted(groups, key=weight, reverse=True):
        b = min(out, key=lambda b: b[0])
        b[0] += weight(g)
        b[1] += g
    return [b[1] for b in out if b[1]]


def run_table(exe, tmp, groups, weight, write_batch, read_results, time_limit=TIME_LIMIT):
    """Every case of the groups through the sanitized program, in at most min(8, CPUs) concurrent children, each under
    time_limit seconds (a table whose batches take seconds passes a shorter one: a wrong loop bound is an endless loop here):
    ({case name: what read_results gives for it}, [(exit status, stdout + stderr) per child])."""
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    env = child_env()
    children = []
    for i, cases in enumerate(batches(groups, weight, max(1, min(8, cpus)))):
        src, dst = str(tmp / ("batch%d.bin" % i)), str(tmp / ("out%d.bin" % i))
        order = write_batch(src, cases)
        children.append((subprocess.Popen([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env),
                         order, dst))
    results, reports = {}, []
    for child, order, dst in children:
        try:
            out, err = child.communicate(timeout=time_limit)
        except subprocess.TimeoutExpired:
            child.kill()
            out, err = child.communicate()
            err += "\n(killed after %d s)" % time_limit
        reports.append((child.returncode, out + err))
        if child.returncode == 0:
            for c, res in zip(order, read_results(dst, order)):
                results[c.name] = res
    return results, reports
