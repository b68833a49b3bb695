"""The run-time functor kernels executed on the HOST, lane by lane, under the address and undefined-behaviour sanitizers
(no GPU): tests/cpp/functor_sim.cpp compiles the kernel text of csrc/functor_kernel.inc unchanged over tests/cpp/simt,
behind the prologue that mi355_spmv_functor_compile writes and the functors of tests/cpp/functor_texts.inc, one program
per type set of tests/functor_cases.py, and launches it in the shape of the product's functor_shape
(csrc/functor_shape.hpp).  Every operand is an allocation of exactly the elements the call may touch, Aj / Ax / x of the
unaligned cases 1 and 3 elements behind a 64-byte boundary, so a read one element outside is a report.

Asserted: every case of the table but the one at the true grid caps runs; the launch shape that the program reports (the
product's) equals the census's; y equals the serial fold bit for bit; the guard elements on both sides of y keep their
bytes; the children end clean.  The true-cap stride case's edge states are all carried by a simulated case whose two
grids are overridden (the only thing a case may override)."""
import concurrent.futures
import os
import struct
import subprocess

import numpy as np
import pytest

import functor_cases as fc
import sim_runner

# seconds per child: the slowest batch of this table takes under 5 s, and a wrong stride or loop bound in these kernels
# is an endless loop in the simulation (profiles/functor_edges_mutations.txt, 11 and 13), seen only at the limit
TIME_LIMIT = 150

SHAPE_PROBES = [(n, nnz) for n in (1, 7, 300, 1000) for m in fc.T_MEANS for nnz in (m * n, (m + 1) * n - 1, (m + 1) * n)] + [
    (1, 0), (5, 0), (64, fc.LONG_MIN), (64, fc.LONG_MIN + 1), (48, 4096), (40, 4097), (1, 8192), (1, 8193),
    (fc.ROWS_CAP * 128 - 1, 10), (fc.ROWS_CAP * 128, 10), (fc.ROWS_CAP * 128 + 1, 10), (fc.ROWS_CAP * 128 + 300, 1063212),
    (fc.LONG_CAP * 256, 1 << 20), (fc.LONG_CAP * 256 + 1, 1 << 20), (fc.ROWS_CAP * 4, 1 << 31), (2147483647, 1 << 40)]


def make_variables(ts):
    return ["FS_FUNCTOR=" + ts.functor, "FS_OFF=" + ts.off, "FS_MAT=" + ts.mat, "FS_X=" + ts.x, "FS_Y=" + ts.y]


def write_batch(path, cases):
    with open(path, "wb") as f:
        for c in cases:
            ts = fc.TYPE_SETS[c.typeset]
            Ap, Aj, Ax, x = fc.operands(c)
            n = len(c.matrix.lens)
            head = [1, Ap.itemsize, Ax.itemsize, x.itemsize, ts.np_y.itemsize, n, len(x), len(Aj), c.shift, c.shift, c.shift,
                    c.grids[0], c.grids[1], fc.GUARD]
            f.write(struct.pack("<%dq" % len(head), *head))
            for a in (Ap, Aj, Ax, x, fc.y_buffer(c)):
                f.write(np.ascontiguousarray(a).tobytes())
        f.write(struct.pack("<q", 0))
    return cases


def read_results(path, order):
    out = []
    with open(path, "rb") as f:
        for c in order:
            shape = struct.unpack("<5q", f.read(40))
            ts = fc.TYPE_SETS[c.typeset]
            y = np.frombuffer(f.read((len(c.matrix.lens) + 2 * fc.GUARD) * ts.np_y.itemsize), dtype=np.uint8)
            out.append((shape, y))
        assert struct.unpack("<q", f.read(8)) == (-1,) and f.read() == b""
    return out


def run_all(exes, tmp, cases):
    """({case name: (shape, y bytes)}, [(exit status, output) per child]) of the cases through their type sets' programs."""
    results, reports = {}, []
    for name, exe in exes.items():
        mine = [[c] for c in cases if c.typeset == name]
        if not mine:
            continue
        d = tmp / name
        d.mkdir()
        res, rep = sim_runner.run_table(exe, d, mine, lambda g: sum(fc.weight(c) for c in g), write_batch, read_results, TIME_LIMIT)
        results.update(res)
        reports += rep
    return results, reports


def verdict(c, res):
    """None, or what is wrong with the result of a case."""
    if res is None:
        return "no result"
    shape, y = res
    cs = fc.census_of(c)
    if tuple(shape) != (cs.shape.T, cs.shape.long_len, cs.shape.rows_grid, int(cs.shape.long_launch), cs.shape.long_grid):
        return "launch shape %s, census %s" % (shape, tuple(cs.shape))
    ts = fc.TYPE_SETS[c.typeset]
    g = fc.GUARD * ts.np_y.itemsize
    if not ((y[:g] == fc.FILL).all() and (y[len(y) - g:] == fc.FILL).all()):
        return "guard elements of y written"
    want = fc.expected(c)
    got = y[g:len(y) - g].view(ts.np_y)
    if not sim_runner.same_bits(got, want):
        bad = np.nonzero(got != want)[0]
        return "rows %s: got %s, want %s" % (bad[:4], got[bad[:4]], want[bad[:4]])
    return None


@pytest.fixture(scope="module")
def exes():
    sim_runner.build("functor_kernel.gen.inc")               # (and the probe: skips where the sanitizers do not link)

    def make(ts):                                            # the same rule, without a probe per program
        subprocess.run(["make", "-s", "-C", sim_runner.CPP, "functor_sim_" + ts.name] + make_variables(ts), check=True)
        return os.path.join(sim_runner.CPP, "functor_sim_" + ts.name)
    with concurrent.futures.ThreadPoolExecutor(4) as pool:
        built = list(pool.map(make, fc.TYPE_SETS.values()))
    return dict(zip(fc.TYPE_SETS, built))


@pytest.fixture(scope="module")
def ran(exes, tmp_path_factory):
    return run_all(exes, tmp_path_factory.mktemp("functor_sim"), [c for c in fc.table() if c.sim])


def test_the_children_end_clean(ran):
    for status, text in ran[1]:
        assert status == 0 and "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]


def test_every_simulated_case_is_the_serial_fold_bit_for_bit(ran):
    results = ran[0]
    wrong = {c.name: v for c in fc.table() if c.sim for v in [verdict(c, results.get(c.name))] if v}
    assert not wrong, wrong


def test_only_the_true_cap_case_is_left_out_and_its_states_are_simulated():
    out = [c for c in fc.table() if not c.sim]
    assert [c.name for c in out] == ["stride_true_caps-pt_f32"]
    assert fc.census_of(out[0]).shape.rows_grid == fc.ROWS_CAP and fc.census_of(out[0]).shape.long_grid == fc.LONG_CAP
    carried = set().union(*[fc.states_of(c) for c in fc.table() if c.sim and c.grids != (0, 0)])
    assert set(out[0].edge) <= carried, sorted(set(out[0].edge) - carried)
    assert all(c.family == "stride" for c in fc.table() if c.grids != (0, 0))


def test_functor_shape_equals_the_census_rule(exes, tmp_path):
    """The product's functor_shape, read through the simulation program, on the table's matrices (the true caps
    included), on both sides of every threshold of the T rule, of nnz against long_len and of the two grid caps."""
    probes = SHAPE_PROBES + [(len(c.matrix.lens), sum(c.matrix.lens)) for c in fc.table()]
    src, dst = tmp_path / "shapes.bin", tmp_path / "shapes.out"
    with open(src, "wb") as f:
        for n, nnz in probes:
            f.write(struct.pack("<3q", 2, n, nnz))
        f.write(struct.pack("<q", 0))
    r = subprocess.run([exes["pt_f32"], str(src), str(dst)], capture_output=True, text=True, env=sim_runner.child_env(), timeout=TIME_LIMIT)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(str(dst), dtype=np.int64)
    assert len(got) == 5 * len(probes) + 1 and got[-1] == -1
    for (n, nnz), g in zip(probes, got[:-1].reshape(-1, 5)):
        s = fc.shape_of(n, nnz)
        assert tuple(g) == (s.T, s.long_len, s.rows_grid, int(s.long_launch), s.long_grid), (n, nnz)
    seen = {tuple(g)[0] for g in got[:-1].reshape(-1, 5)}
    assert seen == set(fc.LANES)
