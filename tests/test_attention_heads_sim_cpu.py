"""csrc/attention.hip executed on the host, lane by lane, through the heads entry points (tests/cpp/attention_heads_sim.cpp
over tests/cpp/simt, built by tests/cpp/heads.mk with the address and undefined-behaviour sanitizers): every forward case of
tests/attention_heads_cases.py through the real create / create_half, reserve_heads, execute_heads and execute.  Every
operand of all heads is one allocation exactly as long as the heads call may touch, so a read or write one element outside is
a sanitizer report.  Head h of the heads execute must equal the single-head execute on head h's operands bit for bit; no
canary may be lost; an execute of fewer heads than reserved must leave the other heads' scratch alone.  The children must
end with status 0 and an empty stderr.  Nothing is loaded into this process (the sanitizer runtimes are linked statically).

The proof that n_heads = 1 through the old entry point is the old path is tests/test_attention_sim_cpu.py and
tests/test_attention_half_sim_cpu.py, which run the single-head tables, unchanged, on the same kernels; this file asserts
that their program still builds from the same sources."""
import subprocess

import pytest

import attention_heads_cases as hd
import sim_runner as sr

ENOTSUP = 2
# (n_heads, n_slices, width): the slice grid reaches 2^31; the fix-up's does; both stay below
GRID_PROBES = ((2 ** 11, 2 ** 22, 8), (2 ** 10, 2 ** 21, 256), (2 ** 10, 2 ** 21, 128), (5, 8, 72))
GRID_WANT = (ENOTSUP, ENOTSUP, 0, 0)


def build(target):
    sr.build("attention_sim")       # (the sanitizer probe, and the single-head program from the same sources)
    subprocess.run(["make", "-s", "-C", sr.CPP, "-f", "heads.mk", target], check=True)
    return sr.CPP + "/" + target


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = build("attention_heads_sim")
    assert sr.kernel_constant(sr.source("slice_cut.hpp"), "kSliceLen") == hd.SLICE_LEN
    common = sr.source("common.hpp")
    assert sr.kernel_constant(common, "kBlock") // sr.kernel_constant(common, "kWave") == hd.WAVES
    probes = {}

    def write(path, cases):
        first = not probes
        probes[path] = first
        return hd.write_batch(path, cases, GRID_PROBES if first else None)

    def read(path, cases):
        res, got = hd.read_results(path, cases, len(GRID_PROBES) if probes[path.replace("out", "batch")] else 0)
        if got:
            probes["got"] = got
        return res

    results, reports = sr.run_table(exe, tmp_path_factory.mktemp("attention_heads_sim"), sr.groups_by(hd.forward_cases(), hd.plan_key), hd.weight, write, read)
    return results, reports, probes.get("got")


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


@pytest.mark.parametrize("structure", ("one", "two", "five", "eight"))
def test_every_head_equals_the_single_head_execute_bit_for_bit(run, structure):
    cases = [c for c in hd.forward_cases() if c.matrix is hd.structures()[structure]]
    assert cases
    for c in cases:
        assert c.name in run[0], "%s: no result (its child did not end clean)" % c.name
        hd.check_result(c, run[0][c.name], sr.same_bits)


def test_reserve_heads_reports_the_scratch_of_every_head(run):
    """scratch_bytes after every reserve, upward and downward between the executes of one object, is
    (n_heads_max - 1) x round16(one head's bytes) + one head's bytes, one head's bytes being what create allocates."""
    seen = {}
    for c in hd.forward_cases():
        assert run[0][c.name].scratch_bytes == hd.reserved_scratch_bytes(c), c.name
        seen.setdefault(hd.plan_key(c), []).append(c.H_max)
    assert any(len(set(v)) > 1 and v != sorted(v) for v in seen.values())       # some object's reserve went down again
    assert any(len(v) > len(set(v)) for v in seen.values())                      # and some maximum was reserved twice


def test_a_grid_of_2_to_the_31_workgroups_is_refused(run):
    assert tuple(run[2]) == GRID_WANT


def test_overlapping_outputs_and_short_vector_strides_are_refused_before_any_launch(tmp_path):
    """On a real object with rows (one cannot be made without a device outside this program), on dummy pointers that a
    refusal never reads: each overlapping-output case, an lse / dbias stride below its length and a negative stride are
    MI355_SPMV_EINVAL, and the text names the stride."""
    exe = build("attention_heads_sim")
    c = next(c for c in hd.forward_cases() if c.H_max >= 3 and hd.n_slices(c.matrix) == 2)
    refusals = [r for r in hd.forward_refusals(c) if r[1] is not None]
    src, dst = str(tmp_path / "refusals.bin"), str(tmp_path / "refusals.out")
    hd.write_refusals(src, c, refusals)
    child = subprocess.run([exe, src, dst], capture_output=True, text=True, env=sr.child_env(), timeout=sr.TIME_LIMIT)
    assert child.returncode == 0 and child.stderr == "", child.stderr[-3000:]
    got = hd.read_refusals(dst, c, len(refusals))
    for (word, _), (status, text) in zip(refusals, got):
        assert status == 1 and word in text, (word, status, text)
