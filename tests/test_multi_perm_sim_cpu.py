"""csrc/multi.hip and csrc/multi_perm.hip executed on the host, lane by lane (tests/cpp/multi_perm_sim.cpp over
tests/cpp/simt): the sources and their launch path, unchanged, built with the address and undefined-behaviour sanitizers as
a stand-alone program and run over the WHOLE table of tests/multi_perm_cases.py through mi355_spmv_multi_create_permuted /
_execute / _destroy.  Every operand is an allocation exactly as long as the call may touch: Ax of n_values, perm of nnz.

The bar: bit for bit the result of the ordinary multi object on the same structure with Ax[perm] materialised, computed in
the same program — the same walk on the same values, so any difference is a bug.  The children must end with status 0 and
must have written nothing to stderr (where the sanitizers and the stand-in's out-of-step check report).  Nothing is loaded
into this process, and the children's environment is this process's own (the sanitizer runtimes are linked statically).

sim_runner.build makes the program by the rule of tests/cpp/Makefile, behind that Makefile's sanitizer_probe."""
import subprocess

import pytest

import multi_cases as mc
import multi_perm_cases as pc
import sim_runner as sr


@pytest.fixture(scope="module")
def exe():
    path = sr.build("multi_perm_sim")
    multi, common = sr.source("multi.hip"), sr.source("common.hpp")
    assert sr.kernel_constant(multi, "kMultiSlice") == mc.SLICE_LEN
    assert sr.kernel_constant(common, "kWave") == mc.STEP
    assert sr.kernel_constant(multi, "kMultiGroupsMax") == max(mc.LANES_PER_SLOT)
    return path


@pytest.fixture(scope="module")
def run(exe, tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, Y permuted, Y plain)}, and the
    children's reports."""
    return sr.run_table(exe, tmp_path_factory.mktemp("multi_perm_sim"), sr.groups_by(pc.table(), pc.plan_key), pc.weight,
                        pc.write_batch, pc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_the_table_covers_every_family_type_and_k():
    table = pc.table()
    assert len({c.name for c in table}) == len(table)
    by_structure = sr.groups_by(table, lambda c: c.matrix.name)
    assert len(by_structure) == len(pc.structures()) >= 30
    for g in by_structure:
        assert {c.perm for c in g} == set(pc.PERMS)
        assert {(c.val, c.k) for c in g} == {(v, k) for v in pc.K for k in pc.K[v]}
    assert {(c.off, c.poff) for c in table} == {(o, p) for o in ("i32", "i64") for p in ("i32", "i64")}
    assert any(max(c.matrix.lens, default=0) >= 30000 for c in table) and any(c.matrix.n_cols == 1 for c in table)
    assert any(len(c.matrix.lens) == 0 for c in table) and any(c.matrix.lens and sum(c.matrix.lens) == 0 for c in table)
    for c in table:     # what the permutation families promise
        perm, nv = pc.permutation(c.matrix, c.perm)
        nnz = len(perm)
        if c.perm == "shared" and nnz >= 4:
            assert nv < nnz and pc.np.bincount(perm, minlength=nv).min() >= 2
        if c.perm == "sparse":
            assert nv == 2 * nnz + 3 and len(set(perm.tolist())) == nnz


@pytest.mark.parametrize("perm", pc.PERMS)
def test_permuted_equals_plain_on_materialised_values_bit_for_bit(run, perm):
    results = run[0]
    cases = [c for c in pc.table() if c.perm == perm]
    assert cases
    for c in cases:
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, y, y_plain = results[c.name]
        assert status == 0, c.name
        pc.check(c, y, y_plain)


@pytest.mark.parametrize("poff", ("i32", "i64"))
def test_an_index_outside_the_values_is_refused_and_no_object_is_made(exe, tmp_path, poff):
    c = next(c for c in pc.table() if c.matrix.name == "ragged" and c.perm == "random" and c.poff == poff and c.k == 3)
    bad = [b for b in pc.bad_cases() if b[3] == poff]
    assert {b[2] for b in bad} == {pc.permutation(c.matrix, c.perm)[1], -1}     # n_values itself, and -1
    src, dst = str(tmp_path / "bad.bin"), str(tmp_path / "bad.out")
    pc.write_batch(src, [c], bad)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=sr.TIME_LIMIT, env=sr.child_env())
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    results, refused = pc.read_results(dst, [c], len(bad))
    assert results[0][0] == 0
    pc.check(c, results[0][1], results[0][2])
    for (name, _, _, _), (status, made) in zip(bad, refused):
        assert status == 1 and made == 0, (name, status, made)     # MI355_SPMV_EINVAL, *out cleared
