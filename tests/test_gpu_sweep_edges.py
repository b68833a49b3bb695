"""GPU suite: chunk_rows_sweep (csrc/xwindow.hpp), the chunk body of csr_vector_sweep_kernel and light_rows_sweep_kernel,
at every pass, group, step and tail edge — the table of tests/sweep_cases.py, whose reach tests/test_sweep_cases_cpu.py
proves on the host.  No planner: every case creates a row-block plan from a HAND-WRITTEN mi355_spmv_plan_shape
(sweep_cases.sweep_shape, checked on the host) that starts at row 0 and element 0, i.e. is the whole of a small matrix,
and FAILS unless info() reports the sweep kernel of its kind, 1 024 threads, the case's T, rows per chunk, chunk count
and window.  The planner-made tie at the end shows that this route runs the planner's own kernel: identical bytes.

Bars, none of them new: integer-valued data is exact in any order, so y equals the serial loop (oracle.spmv_serial) bit
for bit; real data (window, rows, tail) lies within conftest.parity_bound of the fp64 sum.  Identities: two executes of
one plan give the same bytes; light gives vector's bytes; row blocks of one shape give the whole plan's bytes; and on
one case per family alpha = 2, beta = -1 over a known y0 equals 2 * serial - y0 exactly.  y is poisoned with NaN before
every execute, and the columns of x that no row references hold NaN.  The malformed shapes below are the ones
launch_rows_sweep refuses on the host, before any launch; no case is built to reach the device malformed."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import row_cases as rc
import sweep_cases as sc
from conftest import parity_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = 1


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@contextlib.contextmanager
def knobs(sp, wanted):
    """Exactly `wanted` of the row kinds' knobs while a plan is created (a plan keeps the knobs it was created under)."""
    old = {k: os.environ.get(k) for k in rc.KNOB_NAMES}
    try:
        for k in rc.KNOB_NAMES:
            os.environ.pop(k, None)
        os.environ.update(wanted)
        sp.capi.lib().mi355_spmv_knobs_reload()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        sp.capi.lib().mi355_spmv_knobs_reload()


def shape_struct(sp, fields):
    sh = sp.capi.PlanShape()
    for k, v in fields.items():
        setattr(sh, k, v)
    return sh


def block_plan(sp, kind, fields, r0, r1, Ap64, dAp, dAj, dAx, n_cols):
    """The plan of rows [r0, r1) under the hand-written shape `fields` (of the whole matrix), with its operands."""
    rpc = fields["rows_per_chunk"]
    assert r0 % rpc == 0
    a, j, v, lo = sp.dist.block_view(dAp, dAj, dAx, r0, r1)
    assert j.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 and int(a[0]) == int(Ap64[r0]) % 4
    p = sp.Plan.block(kind, shape_struct(sp, fields), r0, r0 // rpc, -(-(r1 - r0) // rpc), int(Ap64[r0]), r1 - r0, n_cols,
                      int(Ap64[r1]) - lo, a, j, dAx.dtype)
    return p, v


def check_plan(p, kind, fields, n_rows, what):
    """The plan is the hand-written one: the sweep kernel of its kind on the case's geometry."""
    info, sh = p.info(), p.shape()
    what = what + (kind, info)
    assert info["main_kernel"] == sc.KERNEL[kind], what
    assert info["block_threads"] == 1024 == sh.block_threads, what
    assert info["lanes_per_row"] == fields["lanes_per_row"] == sh.lanes_per_row, what
    assert info["rows_per_chunk"] == fields["rows_per_chunk"] == sh.rows_per_chunk, what
    assert info["n_chunks"] == -(-n_rows // fields["rows_per_chunk"]) == sh.n_chunks, what
    assert info["window_elems"] == fields["window_elems"] == sh.window_elems, what
    assert info["rows_cap"] == fields["rows_cap"] and info["balanced_chunks"] == 0 and info["n_kernels"] == 1, what
    assert sh.window_sweep == 1 and sh.small_plain == 0 and info["packed_index_bytes"] == 0, what
    assert info["grid_blocks"] == info["n_chunks"], what
    return info


def execute_twice(p, Ax, x, n, t, what):
    y = torch.full((n,), float("nan"), dtype=t, device=DEV)
    p.execute(Ax, x, y)
    again = torch.full((n,), float("nan"), dtype=t, device=DEV)
    p.execute(Ax, x, again)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert got.tobytes() == again.cpu().numpy().tobytes(), ("two executes differ", what)
    return got


_refs = {}


def reference(oracle, m, vb, integer):
    """The serial loop's y, and for real data the fp64 sum with its per-row bound; once per (matrix, value size, data)."""
    key = (m, vb, integer)
    if key not in _refs:
        Ap, Aj = sc.structure(m)
        Ax, x, _ = sc.operands(m, vb, integer)
        serial = oracle.spmv_serial(Ap, Aj, Ax, x)
        _refs[key] = (serial, None if integer else parity_bound(oracle, Ap, Aj, Ax, x))
    return _refs[key]


def compare(y, serial, bound, what):
    assert y.dtype == serial.dtype, what
    if bound is None:
        bad = np.nonzero(~(y == serial))[0]
        print(what, "rows that differ from the serial loop:", bad.size)
        assert bad.size == 0, ("rows differ from the serial loop", bad[:8], y[bad[:8]], serial[bad[:8]], what)
    else:
        y64, per_row = bound
        err = np.abs(y.astype(np.float64) - y64)
        bad = np.nonzero(~(err <= per_row))[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            print(what, "max error / bound:", float(np.nanmax(np.where(per_row > 0, err / per_row, 0.0))) if err.size else 0.0)
        assert bad.size == 0, ("rows outside the parity bound", bad[:8], err[bad[:8]], per_row[bad[:8]], what)


def run_case(sp, oracle, c, types, integer):
    m = c.matrix
    t_val, t_off = sc.TYPES[types]
    assert np.dtype(t_val).itemsize == c.vb
    Ap64, Aj = sc.structure(m)
    Ax, x, y0 = sc.operands(m, c.vb, integer)
    n, nnz = len(m.lens), int(Ap64[-1])
    serial, bound = reference(oracle, m, c.vb, integer)
    what = (c.name, types, "integer" if integer else "real")
    dAp, dAj, dAx, dx = d(Ap64.astype(t_off)), d(Aj), d(Ax), d(x)
    plans, fields = {}, {}
    try:
        for kind in ("vector", "light"):
            fields[kind] = sc.sweep_shape(kind, types, c.T, c.held, c.rounds, m.band, n, m.n_cols, nnz)
            plans[kind], _ = block_plan(sp, kind, fields[kind], 0, n, Ap64, dAp, dAj, dAx, m.n_cols)
            check_plan(plans[kind], kind, fields[kind], n, what)
        got = {kind: execute_twice(p, dAx, dx, n, dx.dtype, what + (kind,)) for kind, p in plans.items()}
        y = got["vector"]
        compare(y, serial, bound, what)
        assert got["light"].tobytes() == y.tobytes(), ("light differs from vector", np.nonzero(~(got["light"] == y))[0][:8], what)
        if integer and types == "f32-i32" and sc.ALPHA_BETA_CASES.get(c.family) == c.name:
            alpha, beta = sc.ALPHA_BETA
            for kind in ("vector", "light"):
                plans[kind].set_alpha_beta(alpha, beta)
                yab = d(y0)
                plans[kind].execute(dAx, dx, yab)
                torch.cuda.synchronize()
                out = yab.cpu().numpy()
                expect = (t_val(alpha) * serial + t_val(beta) * y0).astype(t_val)
                bad = np.nonzero(~(out == expect))[0]
                assert bad.size == 0, ("alpha / beta: rows differ", kind, bad[:8], out[bad[:8]], expect[bad[:8]], what)
        if c.family == "blocks":
            # the same shape cut at chunk boundaries where Ap % 4 is 1, 2 and 3 (the band shifted by row_begin,
            # nnz_begin_whole, nnz_read; the last block of the second cutting lies in the arrays' partial group)
            for kind in ("vector", "light"):
                for cuts in sc.block_cuts(c):
                    yb = torch.full((n,), float("nan"), dtype=dx.dtype, device=DEV)
                    for r0, r1 in cuts:
                        pb, v = block_plan(sp, kind, fields[kind], r0, r1, Ap64, dAp, dAj, dAx, m.n_cols)
                        try:
                            check_plan(pb, kind, fields[kind], r1 - r0, what + (r0, r1))
                            pb.execute(v, dx, yb[r0:r1])
                            torch.cuda.synchronize()
                        finally:
                            pb.destroy()
                    out = yb.cpu().numpy()
                    assert out.tobytes() == y.tobytes(), ("row blocks differ from the whole plan", kind, cuts,
                                                          np.nonzero(~(out == y))[0][:8], what)
    finally:
        for p in plans.values():
            p.destroy()


def groups():
    out = []
    for fam in sc.FAMILIES:
        for T in sc.FAMILY_LANES[fam]:
            for types in sc.FAMILY_TYPES[fam]:
                out.append(pytest.param(fam, T, types, id="%s-T%d-%s" % (fam, T, types)))
    return out


@pytest.mark.parametrize("fam,T,types", groups())
def test_family(sp, oracle, fam, T, types):
    cases = sc.family(fam, T, np.dtype(sc.TYPES[types][0]).itemsize)
    assert cases
    for c in cases:
        run_case(sp, oracle, c, types, True)
        if fam in sc.REAL_FAMILIES and c.matrix.data == "signs":
            run_case(sp, oracle, c, types, False)


@pytest.mark.parametrize("types", ["f32-i32", "f64-i64"])
def test_malformed_shapes_are_refused_on_the_host_before_any_launch(sp, types):
    """rows_per_chunk that is not (1024 / T) * held, eight rows per vector in fp64 or at T = 2, a window one element
    below a round, rows_cap below rows_per_chunk: launch_rows_sweep answers MI355_SPMV_EINVAL at execute and launches
    nothing — y keeps its NaN."""
    t_val, t_off = sc.TYPES[types]
    vb = np.dtype(t_val).itemsize
    c = [c for c in sc.family("rows", 8, vb) if c.name.startswith("rows_rowid") and c.held == 4][0]
    Ap64, Aj = sc.structure(c.matrix)
    Ax, x, _ = sc.operands(c.matrix, vb, True)
    n, nnz = len(c.matrix.lens), int(Ap64[-1])
    dAp, dAj, dAx, dx = d(Ap64.astype(t_off)), d(Aj), d(Ax), d(x)
    L = sp.capi.lib()
    names = [name for name, _ in sc.refused_shapes(types)]
    assert len(names) == (5 if vb == 8 else 4)
    for name, f in sc.refused_shapes(types):
        f = dict(f, n_rows=n, n_cols=c.matrix.n_cols, nnz=nnz)
        p = sp.Plan.block("vector", shape_struct(sp, f), 0, 0, -(-n // f["rows_per_chunk"]), 0, n, c.matrix.n_cols, nnz, dAp, dAj, dx.dtype)
        try:
            y = torch.full((n,), float("nan"), dtype=dx.dtype, device=DEV)
            st = L.mi355_spmv_plan_execute(p._h, ctypes.c_void_p(dAx.data_ptr()), ctypes.c_void_p(dx.data_ptr()),
                                           ctypes.c_void_p(y.data_ptr()), sp.capi._stream_ptr(None))
            torch.cuda.synchronize()
            assert st == EINVAL, (name, st, L.mi355_spmv_last_error().decode())
            assert b"sweep plan with" in L.mi355_spmv_last_error(), (name, L.mi355_spmv_last_error())
            assert bool(torch.isnan(y).all()), name
        finally:
            p.destroy()


@pytest.mark.parametrize("kind", ["vector", "light"])
@pytest.mark.parametrize("types", ["f32-i32", "f64-i64"])
def test_the_planner_sweeps_what_the_hand_written_shape_sweeps(sp, oracle, kind, types):
    """The smallest matrix the planner itself sweeps (sweep_cases.tie_matrix: 512 chunks at T = 64, two passes of nine
    rounds) under exactly the knobs that force the shape.  The planner's plan and a row-block plan of the field values
    sweep_shape() writes for the same geometry must give identical bytes, within the parity bound."""
    t_val, t_off = sc.TYPES[types]
    vb = np.dtype(t_val).itemsize
    Ap64, Aj, n_cols, band = sc.tie_matrix(vb)
    n, nnz = len(Ap64) - 1, int(Ap64[-1])
    Ax, x, _ = rc.operands_of(Ap64, Aj, n_cols, "signs", vb, False)
    dAp, dAj, dAx, dx = d(Ap64.astype(t_off)), d(Aj), d(Ax), d(x)
    what = ("tie", kind, types)
    with knobs(sp, sc.TIE_KNOBS):
        planner = sp.Plan(kind, n, n_cols, nnz, dAp, dAj, dx.dtype)
    hand = None
    try:
        sh = planner.shape()
        print(what, planner.info())
        assert sh.window_sweep == 1, (what, planner.info())
        held = sc.sweep_rows_for(vb, 64)
        fields = sc.sweep_shape(kind, types, 64, held, 9, band, n, n_cols, nnz)
        theirs = {k: getattr(sh, k) for k in fields}
        assert theirs == fields, (what, {k: (theirs[k], fields[k]) for k in fields if theirs[k] != fields[k]})
        check_plan(planner, kind, fields, n, what)
        hand, _ = block_plan(sp, kind, fields, 0, n, Ap64, dAp, dAj, dAx, n_cols)
        check_plan(hand, kind, fields, n, what)
        y_planner = execute_twice(planner, dAx, dx, n, dx.dtype, what + ("planner",))
        y_hand = execute_twice(hand, dAx, dx, n, dx.dtype, what + ("hand-written",))
        assert y_hand.tobytes() == y_planner.tobytes(), ("the hand-written shape differs from the planner's plan",
                                                         np.nonzero(~(y_hand == y_planner))[0][:8], what)
        compare(y_planner, oracle.spmv_serial(Ap64.astype(t_off), Aj, Ax, x), parity_bound(oracle, Ap64.astype(t_off), Aj, Ax, x), what)
    finally:
        planner.destroy()
        if hand is not None:
            hand.destroy()
