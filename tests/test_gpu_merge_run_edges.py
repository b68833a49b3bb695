"""GPU suite: merge_rows_kernel (csrc/merge_path.hip, the row-parallel run kernel of a MERGE plan) at every run, piece
and row edge — the table of tests/merge_run_cases.py, whose reach tests/test_merge_run_cases_cpu.py proves on the host.
Every case creates its plan under the knobs that force the run kernel on a small matrix (MI355_MERGE_ROWS=1, the tiles
per run, the search in the kernel or in front, the window on or off) and FAILS if info() reports another plan than the
one it was built for; nothing here skips.

Bar: integer-valued data is exact in any order, so y equals the serial loop (oracle.spmv_genl_serial) bit for bit, with
alpha = 2, beta = -1 on the run-edge, spanning and piece families as well (beta * y applied exactly once whether a row
is stored by its run or closed by the fix-up across several runs, alpha reaching every carry); real data (run_edges,
spanning, pieces, tail) within conftest.parity_bound; two executes give the same bits; merge_coords(), which a run plan
computes on demand, equals oracle.merge_tile_coords.  y is NaN before every execute, and the columns of x that no row
references hold NaN.

The executes of the same plans that the run kernel does not serve — min-plus, an Ax view one element off 16-byte
alignment, an fp32 matrix under fp64 vectors — walk the plan's tiles (merge_launch.hpp, launch_merge) and must equal the
oracle as well: test_executes_the_run_kernel_does_not_serve.  test_row_block_views_start_at_every_phase runs four of the
table's matrices as row-block plans whose nonzeros start at 1, 2 and 3: the one mutation of
profiles/merge_run_edges_mutations.txt that the table of whole matrices let through is caught there."""
import contextlib
import os

import numpy as np
import pytest
import torch

import merge_run_cases as rc
from conftest import parity_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_VAL = {"f32": torch.float32, "f64": torch.float64}


def d(a, off_by_one=False):
    """The array on the device; off_by_one: as a view one element off the allocation's (16-byte) alignment."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off_by_one:
        return t.to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.to(DEV)
    view = buf[1:]
    assert view.data_ptr() % 16 != 0
    return view


@contextlib.contextmanager
def knobs(sp, wanted):
    """Exactly `wanted` of the merge knobs while a plan is created (a plan keeps the knobs it was created under)."""
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


_refs = {}


def reference(oracle, m, val, integer, sr=0):
    """The serial loop's y, and for real plus-times data the fp64 sum and its per-row bound; computed once per (matrix,
    type, data, semiring) and left unchanged."""
    key = (m.name, m.seed, val, integer, sr)
    if key not in _refs:
        Ap = rc.arrays(m, integer)[0]
        Aj, Ax, x, _ = rc.operands(m, val, integer)
        serial = oracle.spmv_genl_serial(sr, Ap, Aj, Ax, x)
        assert not np.isnan(serial).any()
        _refs[key] = (serial, None if integer or sr else parity_bound(oracle, Ap, Aj, Ax, x))
    return _refs[key]


def poisoned(n, val):
    return torch.full((n,), float("nan"), dtype=T_VAL[val], device=DEV)


def check_plan(c, info, what):
    """The plan is the one the case was built for, or the case fails."""
    cs = rc.census_of(c)
    assert info["main_kernel"] == "merge_rows_kernel", what
    assert info["block_threads"] == rc.BLOCK, what
    assert info["tile_items"] == rc.TILE and info["n_tiles"] == cs.n_tiles, what
    assert info["grid_blocks"] == cs.n_super == -(-cs.n_tiles // c.tps), what
    assert info["n_kernels"] == rc.n_kernels_of(c), what
    assert info["window_segments"] <= 1, what
    if c.window:
        assert info["window_elems"] > 0, what
    else:
        assert info["window_elems"] == 0, what


def run_case(sp, oracle, c, off, val, integer):
    m = c.matrix
    t = rc.TYPES[val]
    Ap64 = rc.arrays(m, integer)[0]
    Aj, Ax, x, y0 = rc.operands(m, val, integer)
    n, nnz = len(m.lens), int(Ap64[-1])
    Ap = Ap64.astype(rc.NP_OFF[off])
    dAp, dAj, dAx, dx = d(Ap), d(Aj), d(Ax), d(x)
    assert (dAj.data_ptr() | dAx.data_ptr() | dx.data_ptr()) % 16 == 0            # (else the execute walks the tiles)
    with knobs(sp, c.knobs):
        p = sp.Plan("merge", n, m.n_cols, nnz, dAp, dAj, dx.dtype)
    try:
        info = p.info()
        what = (c.name, off, val, "integer" if integer else "real", info)
        check_plan(c, info, what)
        serial, bound = reference(oracle, m, val, integer)
        y = poisoned(n, val)
        p.execute(dAx, dx, y)
        again = poisoned(n, val)
        p.execute(dAx, dx, again)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert got.dtype == serial.dtype, what
        assert got.tobytes() == again.cpu().numpy().tobytes(), ("two executes differ", what)
        if bound is None:
            bad = np.nonzero(~(got == serial))[0]
            assert bad.size == 0, ("rows differ from the serial loop", bad[:8], got[bad[:8]], serial[bad[:8]], what)
        else:
            y64, per_row = bound
            err = np.abs(got.astype(np.float64) - y64)
            bad = np.nonzero(~(err <= per_row))[0]
            assert bad.size == 0, ("rows outside the parity bound", bad[:8], err[bad[:8]], per_row[bad[:8]], what)
        if integer and c.family in rc.ALPHA_BETA_FAMILIES:
            alpha, beta = rc.ALPHA_BETA
            p.set_alpha_beta(alpha, beta)
            y = d(y0)
            p.execute(dAx, dx, y)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            want = (t(alpha) * serial + t(beta) * y0).astype(t)
            bad = np.nonzero(~(got == want))[0]
            assert bad.size == 0, ("alpha / beta: rows differ", bad[:8], got[bad[:8]], want[bad[:8]], what)
            p.set_alpha_beta(1.0, 0.0)
        xs, ys = oracle.merge_tile_coords(Ap, rc.TILE)
        rows, nz = p.merge_coords()
        assert np.array_equal(rows, xs) and np.array_equal(nz, ys), ("merge_coords", what)
        y = poisoned(n, val)                                                       # ... which leaves the plan's executes as they were
        p.execute(dAx, dx, y)
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == again.cpu().numpy().tobytes(), ("the execute behind merge_coords differs", what)
    finally:
        p.destroy()


def groups():
    return [pytest.param(f, off, val, id="%s-%s-%s" % (f, off, val)) for f in rc.FAMILIES for off, val in rc.ALL_TYPES]


@pytest.mark.parametrize("family,off,val", groups())
def test_family(sp, oracle, family, off, val):
    cases = rc.family(family)
    assert cases
    for c in cases:
        run_case(sp, oracle, c, off, val, True)
        if family in rc.REAL_FAMILIES and c.matrix.data == "signs":
            run_case(sp, oracle, c, off, val, False)


BLOCK_VIEW_CASES = ("cut_middle_tps1", "whole_runs_1_2_3_tps1", "stored_PIECE_open", "tail2_phase3")


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64")])
def test_row_block_views_start_at_every_phase(sp, oracle, off, val):
    """The rows from r0 on as a row-block plan (a 16-byte-aligned view whose Ap[0] = nnz_begin is 1, 2 or 3) under the
    same forced run kernel: the merge then counts its nonzeros from nnz_begin, in the search kernel in front and in the
    kernel's own search alike (a search that dropped nnz_begin is right on every whole matrix).  Integer data, bit for
    bit the serial loop's rows from r0 on."""
    seen = set()
    for c in [c for c in rc.table() if c.matrix.name in BLOCK_VIEW_CASES and c.family != "search"]:
        m = c.matrix
        Ap64 = rc.arrays(m, True)[0]
        Aj, Ax, x, _ = rc.operands(m, val, True)
        n = len(m.lens)
        dAp, dAj, dAx, dx = d(Ap64.astype(rc.NP_OFF[off])), d(Aj), d(Ax), d(x)
        serial = reference(oracle, m, val, True)[0]
        for phase in (1, 2, 3):
            r0 = next(r for r in range(5, n) if Ap64[r] % 4 == phase and Ap64[r + 1] > Ap64[r])
            a, j, ax, lo = sp.dist.block_view(dAp, dAj, dAx, r0, n)
            assert int(a[0]) == phase and j.data_ptr() % 16 == 0 and ax.data_ptr() % 16 == 0
            nnz_end = int(Ap64[n]) - lo
            items = (n - r0) + int(Ap64[n] - Ap64[r0])
            for fused in ("0", "1"):
                with knobs(sp, dict(c.knobs, MI355_MERGE_FUSED=fused)):
                    p = sp.Plan.block("merge", None, r0, 0, 0, int(Ap64[r0]), n - r0, m.n_cols, nnz_end, a, j, dx.dtype)
                try:
                    info = p.info()
                    what = (c.name, off, val, phase, fused, info)
                    assert info["main_kernel"] == "merge_rows_kernel" and info["block_threads"] == rc.BLOCK, what
                    assert info["n_tiles"] == -(-items // rc.TILE) and info["grid_blocks"] == -(-info["n_tiles"] // c.tps), what
                    assert info["n_kernels"] == (2 if info["grid_blocks"] > 1 else 1) + (1 if fused == "0" else 0), what
                    y = poisoned(n - r0, val)
                    p.execute(ax, dx, y)
                    torch.cuda.synchronize()
                    got = y.cpu().numpy()
                    bad = np.nonzero(~(got == serial[r0:]))[0]
                    assert bad.size == 0, ("rows differ from the serial loop", bad[:8], got[bad[:8]], serial[r0:][bad[:8]], what)
                    seen.add((c.name, phase, fused))
                finally:
                    p.destroy()
    assert len(seen) == len(BLOCK_VIEW_CASES) * 6


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64")])
def test_executes_the_run_kernel_does_not_serve(sp, oracle, off, val):
    """The forced-run plans of the pieces and spanning matrices under min-plus and through an unaligned Ax (both walk the
    plan's tiles), and the plan of an fp32 matrix under fp64 vectors on the same structures: bit for bit the serial loop
    on integer data (min-plus: min never rounds, a + x is exact on integers).
    What is NOT asserted: that these executes take merge_tile_kernel.  info() describes the plan, not an execute, and
    keeps saying merge_rows_kernel; the dispatch is launch_merge's `p.merge_rows && vec && plus-times` (the run kernel is
    not instantiated for another semiring or value-type pair, and its 16-byte loads need the alignment), read there.  The
    test holds whichever kernel serves them to the oracle on the structures of this table."""
    for c in [c for f in rc.FALLBACK_FAMILIES for c in rc.family(f)]:
        m = c.matrix
        Ap64 = rc.arrays(m, True)[0]
        Aj, Ax, x, _ = rc.operands(m, val, True)
        n, nnz = len(m.lens), int(Ap64[-1])
        dAp, dAj, dAx, dx = d(Ap64.astype(rc.NP_OFF[off])), d(Aj), d(Ax), d(x)
        with knobs(sp, c.knobs):
            p = sp.Plan("merge", n, m.n_cols, nnz, dAp, dAj, dx.dtype)
            q = sp.Plan("merge", n, m.n_cols, nnz, dAp, dAj, torch.float64, mat_dtype=torch.float32) if val == "f64" else None
        try:
            what = (c.name, off, val, p.info())
            check_plan(c, p.info(), what)
            serial = reference(oracle, m, val, True)[0]
            y = poisoned(n, val)
            p.execute(d(Ax, off_by_one=True), dx, y)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            bad = np.nonzero(~(got == serial))[0]
            assert bad.size == 0, ("unaligned Ax: rows differ from the serial loop", bad[:8], got[bad[:8]], serial[bad[:8]], what)
            p.set_semiring("min_plus")
            want = reference(oracle, m, val, True, sp.capi.SEMIRINGS["min_plus"])[0]
            y = poisoned(n, val)
            p.execute(dAx, dx, y)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            bad = np.nonzero(~(got == want))[0]
            assert bad.size == 0, ("min-plus: rows differ from the serial loop", bad[:8], got[bad[:8]], want[bad[:8]], what)
            p.set_semiring("plus_times")
            y = poisoned(n, val)
            p.execute(dAx, dx, y)                                                  # ... and back on the run kernel
            torch.cuda.synchronize()
            assert np.array_equal(y.cpu().numpy(), serial), ("back under plus-times", what)
            if q is not None:
                assert q.info()["main_kernel"] == "merge_rows_kernel", (c.name, q.info())
                y = poisoned(n, val)
                q.execute(d(Ax.astype(np.float32)), dx, y)
                torch.cuda.synchronize()
                got = y.cpu().numpy()
                bad = np.nonzero(~(got == serial))[0]
                assert bad.size == 0, ("fp32 matrix under fp64 vectors: rows differ", bad[:8], got[bad[:8]], serial[bad[:8]], what)
        finally:
            p.destroy()
            if q is not None:
                q.destroy()
