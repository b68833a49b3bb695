"""The multi-vector kernels over semirings, int32 values and pattern matrices executed on the host, lane by lane
(tests/cpp/multi_sim.cpp over tests/cpp/simt, the one program of tests/test_multi_sim_cpu.py,
tests/test_multi_half_sim_cpu.py and this file): csrc/multi.hip with the headers it includes, unchanged, built
with the address and undefined-behaviour sanitizers and run over the WHOLE table of tests/multi_semiring_cases.py
through the real mi355_spmv_multi_create_typed / set_semiring / set_alpha_beta / execute / destroy.  Each Y is held to
the serial oracle exactly as the device run of the same table is (tests/test_gpu_multi_semiring.py); the children must
end with status 0 and must have written nothing to stderr (where the sanitizers — a signed overflow of an identity
that met combine() among them — and the stand-in's out-of-step check report), and each runs under a time limit.
Nothing is loaded into this process, and the children's environment is this process's own (the sanitizer runtimes are
linked statically).

Cost (profiles/multi_sim_merge.txt): the table's ~3 000 executes run as concurrent child processes (at most 8): about
ten seconds on 8 cores, plus the compilation of the program where no other multi sim file has built it yet (every
instantiation of the kernels: 287 s as measured)."""
import pytest

import multi_cases as mc
import multi_semiring_cases as sc
import sim_runner as sr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Every case of the table through the sanitized program: {case name: (status, Y)}, and the children's reports."""
    return sr.run_table(sr.build("multi_sim"), tmp_path_factory.mktemp("multi_semiring_sim"),
                        sr.consecutive_runs(sc.table(), sc.plan_key), mc.weight, sc.write_batch, sc.read_results)


def test_the_children_end_clean_with_an_empty_sanitizer_log(run):
    for status, text in run[1]:
        assert status == 0 and text == "", "status %s\n%s" % (status, text[-4000:])


def test_every_combination_occurs_and_every_case_has_a_name_of_its_own(run):
    """The table that the program just ran (every case has a result) covers every combination."""
    table = sc.table()
    assert {c.name for c in table} == set(run[0])
    assert len({c.name for c in table}) == len(table)
    assert 2500 <= len(table) <= 3300
    seen = {(c.semiring, c.val, c.pattern, sc.tile_lanes(c.val, c.k)) for c in table}
    want = {(s, v, p, lanes) for s in sc.SEMIRINGS for v in sc.VALS for p in (False, True) for lanes in mc.LANES_PER_SLOT}
    assert seen == want, sorted(want - seen)
    # two passes, both offset widths, both kinds of data and every structure under every semiring
    assert {(c.semiring, c.val) for c in table if c.k > sc.TILE[c.val]} == {(s, v) for s in sc.SEMIRINGS for v in sc.VALS}
    assert {(c.semiring, c.off) for c in table} == {(s, o) for s in sc.SEMIRINGS for o in sc.OFFS}
    assert {(c.semiring, c.val, c.integer) for c in table if c.val != "i32"} == {
        (s, v, i) for s in sc.SEMIRINGS for v in ("f32", "f64") for i in (False, True)}
    assert {(c.matrix.name, c.semiring) for c in table} >= {(m.name, s) for m in sc.structures() for s in sc.SEMIRINGS}
    assert {(c.alpha, c.beta) for c in table if c.semiring == "plus_times" and c.val != "i32"} == set(mc.AB_REDUCED)
    assert all((c.alpha, c.beta) == (1.0, 0.0) for c in table if c.semiring != "plus_times" or c.val == "i32")
    assert all(c.integer for c in table if c.val == "i32")


def test_every_case_is_held_to_the_oracle(run, oracle):
    results = run[0]
    for c in sc.table():
        assert c.name in results, "%s: no result (its child did not end clean)" % c.name
        status, y = results[c.name]
        assert status == 0, c.name
        sc.check(oracle, c, y)
