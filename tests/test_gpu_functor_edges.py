"""The run-time functor kernels (csrc/functor_kernel.inc in the launch shape of csrc/functor_shape.hpp) on the device, at
every lane, step, long-row, ballot, stride and type edge: the whole table of tests/functor_cases.py through
sp.Functor(...).spmv.  tests/test_functor_cases_cpu.py proves on the host that the table reaches the states it names;
tests/test_functor_sim_cpu.py runs the same table lane by lane under sanitizers.

Integer data are compared BIT FOR BIT with the serial fold: the table's own (functor_cases.expected, float64 / int64)
for every functor, and the oracle's spmv_genl_serial besides for the five semirings.  One real-valued (+, x) case per T
is held to the parity bound of tests/test_gpu_parity.py (assert_parity).  Every case also checks: two executes give the
same bytes; the guard elements on both sides of y keep their prefill; Aj / Ax / x of the unaligned cases are views 1 and
3 elements into larger buffers.  Functor handles are compiled once per module."""
import time

import numpy as np
import pytest
import torch

import functor_cases as fc

DEV = "cuda:0"
TORCH_OFF = {"int": torch.int32, "long long": torch.int64}
TIMES = {}                      # what profiles/functor_edges_mutations.txt reports: seconds per hiprtc compile


@pytest.fixture(scope="module")
def handles(sp):
    made = {}

    def get(name):
        if name not in made:
            ts = fc.TYPE_SETS[name]
            t0 = time.perf_counter()
            made[name] = sp.Functor(fc.text(), ts.functor, TORCH_OFF[ts.off], ts.mat, ts.x, ts.y)
            TIMES[name] = time.perf_counter() - t0
            print("hiprtc compile of %s: %.2f s" % (name, TIMES[name]))
        return made[name]
    yield get
    for f in made.values():
        f.destroy()


def shifted(a, shift):
    """The array on the device; under a shift as a view `shift` elements into a larger buffer whose base is 256-byte
    aligned (the allocator's), so the view is that many elements off 16-byte alignment."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    eb = a.itemsize
    buf = torch.full((shift * eb + raw.size + 64,), fc.FILL, dtype=torch.uint8, device=DEV)
    view = buf[shift * eb:shift * eb + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    assert view.data_ptr() % 16 == (shift * eb) % 16
    return view


def execute(f, c, real=False, stream=None):
    """(y bytes with its guards, after the first execute; the same after a second one)."""
    ts = fc.TYPE_SETS[c.typeset]
    Ap, Aj, Ax, x = fc.operands(c, real)
    n, yb = len(c.matrix.lens), ts.np_y.itemsize
    dAp = torch.from_numpy(Ap).to(DEV)
    dAj, dAx, dx = shifted(Aj, c.shift).view(torch.int32), shifted(Ax, c.shift), shifted(x, c.shift)
    y = torch.from_numpy(fc.y_buffer(c)).to(DEV)
    rows = y[fc.GUARD * yb:(fc.GUARD + n) * yb]
    torch.cuda.synchronize()
    out = []
    for _ in range(2):
        f.spmv(n, fc.N_COLS, int(Ap[-1]), dAp, dAj, dAx, dx, rows, stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        out.append(y.cpu().numpy().copy())
    return out


def check(c, got, want):
    ts = fc.TYPE_SETS[c.typeset]
    g = fc.GUARD * ts.np_y.itemsize
    assert (got[:g] == fc.FILL).all() and (got[len(got) - g:] == fc.FILL).all(), "y outside the rows was written"
    rows = got[g:len(got) - g].view(ts.np_y)
    if not np.array_equal(rows.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)):
        bad = np.nonzero(rows != want)[0]
        raise AssertionError("%s: rows %s: got %s, want %s" % (c.name, bad[:5], rows[bad[:5]], want[bad[:5]]))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", fc.table(), ids=lambda c: c.name)
def test_the_table_is_the_serial_fold_bit_for_bit(sp, oracle, handles, case):
    ts = fc.TYPE_SETS[case.typeset]
    t0 = time.perf_counter()
    first, second = execute(handles(case.typeset), case)
    assert np.array_equal(first, second), "two executes differ"
    rows = check(case, first, fc.expected(case))
    if ts.semiring is not None and len(case.matrix.lens) < 100000:
        # the five semirings: the oracle's generalized serial loop (cpu_navie.hpp:20-34) on the same operands
        Ap, Aj, Ax, x = fc.operands(case)
        t = np.float32 if ts.np_mat == np.float32 else np.float64
        ref = oracle.spmv_genl_serial(ts.semiring, Ap, Aj, Ax.astype(t), x.astype(t))
        assert np.array_equal(rows.astype(t), ref)
    print("%s: %.3f s" % (case.name, time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("case", fc.real_cases(), ids=lambda c: c.name)
def test_real_values_keep_the_parity_bound_at_every_T(sp, oracle, handles, case):
    from test_gpu_parity import assert_parity
    first, second = execute(handles(case.typeset), case, real=True)
    assert np.array_equal(first, second)
    g = fc.GUARD * 4
    assert (first[:g] == fc.FILL).all() and (first[len(first) - g:] == fc.FILL).all()
    Ap, Aj, Ax, x = fc.operands(case, real=True)
    assert_parity(oracle, Ap, Aj, Ax, x, first[g:len(first) - g].view(np.float32))


@pytest.mark.gpu
def test_a_side_stream(sp, handles):
    """The two launches of a call are ordered by the caller's stream: a long-row case and a stride case on a side stream."""
    s = torch.cuda.Stream()
    for name in ("ballot_lanes-pt_f32", "stride_small-pt_f32-grids2x1", "types_mix-stat16_i64"):
        c = [c for c in fc.table() if c.name == name][0]
        with torch.cuda.stream(s):
            first, second = execute(handles(c.typeset), c, stream=s)
        assert np.array_equal(first, second)
        check(c, first, fc.expected(c))
