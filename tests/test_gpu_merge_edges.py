"""GPU suite: merge_tile_kernel (csrc/merge_path.hip) at every thread, wave, tile and run edge — the table of
tests/merge_cases.py, whose reach tests/test_merge_cases_cpu.py proves on the host.  Every case creates its plan under
the knobs that force its shape (256 x 8 or 512 x 4 items, tiles per run, search in the kernel or in front, window on
or off, never the row-parallel run kernel) and FAILS if info() reports another plan than the one it was built for.

Bar: integer-valued data is exact in any order, so y equals the serial loop (oracle.spmv_genl_serial) bit for bit, with
alpha = 2, beta = -1 on the run family's float types as well (beta * y applied exactly once whether a row is closed inside a thread,
through the scan or by the fix-up); real data (thread-edge, tail and run families, float types) within conftest.parity_bound
under plus-times and bit for bit under min-plus (a + x rounds once, min never); two executes give the same bits; the
tile coordinates equal oracle.merge_tile_coords.  y is poisoned before every execute, and the columns of a float x that
no row references hold NaN."""
import contextlib
import os

import numpy as np
import pytest
import torch

import merge_cases as mc
from conftest import parity_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB_NAMES = ("MI355_MERGE_TPS", "MI355_MERGE_FUSED", "MI355_MERGE_SEARCH_LANES", "MI355_MERGE_BLOCK", "MI355_MERGE_ROWS",
              "MI355_SPMV_WINDOW")
POISON_INT = -77777777


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
    old = {k: os.environ.get(k) for k in KNOB_NAMES}
    try:
        for k in KNOB_NAMES:
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


def reference(sp, oracle, m, val, sr, integer):
    """The serial loop's y (the matrix widened to the type of x and y), and for real plus-times data the fp64 sum and
    its per-row bound; computed once per (matrix, types, semiring) and left unchanged."""
    key = (m.name, m.seed, val, sr, integer)
    if key not in _refs:
        Ap = mc.arrays(m, integer)[0]
        Aj, _, wide, x, _ = mc.operands(m, val, integer)
        serial = oracle.spmv_genl_serial(sp.capi.SEMIRINGS[sr], Ap, Aj, wide, x)
        bound = parity_bound(oracle, Ap, Aj, wide, x) if (not integer and sr == "plus_times") else None
        _refs[key] = (serial, bound)
    return _refs[key]


def poisoned(n, t_vec):
    if t_vec == np.int32:
        return torch.full((n,), POISON_INT, dtype=torch.int32, device=DEV)
    return torch.full((n,), float("nan"), dtype=torch.float32 if t_vec == np.float32 else torch.float64, device=DEV)


def run_case(sp, oracle, c, off, val, sr, integer):
    m = c.matrix
    t_vec, t_mat = mc.TYPES[val]
    Ap64 = mc.arrays(m, integer)[0]
    Aj, stored, wide, x, y0 = mc.operands(m, val, integer)
    n, nnz = len(m.lens), int(Ap64[-1])
    Ap = Ap64.astype(mc.NP_OFF[off])
    xs, ys = oracle.merge_tile_coords(Ap, mc.TILE)
    n_tiles = len(xs) - 1
    dAp, dAj, dx = d(Ap), d(Aj, c.unaligned), d(x)
    dAx = None if t_mat is None else d(stored, c.unaligned)
    with knobs(sp, c.knobs):
        p = sp.Plan("merge", n, m.n_cols, nnz, dAp, dAj, dx.dtype, mat_dtype="pattern" if t_mat is None else dAx.dtype)
    try:
        info = p.info()
        what = (c.name, off, val, sr, "integer" if integer else "real", info)
        assert info["main_kernel"] == "merge_tile_kernel", what
        assert info["tile_items"] == mc.TILE and info["n_tiles"] == n_tiles, what
        assert info["block_threads"] == c.block and info["elems_per_lane"] == mc.ipt_of(c.block), what
        assert info["grid_blocks"] == -(-n_tiles // mc.tps_of(c)), what
        assert info["n_kernels"] == mc.n_kernels_of(c, n_tiles), what
        if c.window:
            assert info["window_elems"] > 0, what
        if c.knobs.get("MI355_SPMV_WINDOW") == "0":
            assert info["window_elems"] == 0, what
        p.set_semiring(sr)
        serial, bound = reference(sp, oracle, m, val, sr, integer)
        y = poisoned(n, t_vec)
        p.execute(dAx, dx, y)
        again = poisoned(n, t_vec)
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
        rows, nz = p.merge_coords()
        assert np.array_equal(rows, xs) and np.array_equal(nz, ys), what
        # (mi355_spmv_plan_set_alpha_beta is for floating-point values: an int32 plan answers ENOTSUP)
        if c.family == "runs" and sr == "plus_times" and integer and t_vec != np.int32:
            alpha, beta = mc.ALPHA_BETA
            p.set_alpha_beta(alpha, beta)
            y = d(y0)
            p.execute(dAx, dx, y)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            want = (t_vec(alpha) * serial + t_vec(beta) * y0).astype(t_vec)
            bad = np.nonzero(~(got == want))[0]
            assert bad.size == 0, ("alpha / beta: rows differ", bad[:8], got[bad[:8]], want[bad[:8]], what)
    finally:
        p.destroy()


def groups():
    out = []
    for family in mc.FAMILIES:
        for block, _ in mc.VARIANTS:
            for off, val, sr in mc.FAMILY_TYPES[family]:
                if block == 512 and sr != "plus_times":      # (512 x 4 exists under plus-times only: merge_launch.hpp)
                    continue
                out.append(pytest.param(family, block, off, val, sr, id="%s-b%d-%s-%s-%s" % (family, block, off, val, sr)))
    return out


@pytest.mark.parametrize("family,block,off,val,sr", groups())
def test_family(sp, oracle, family, block, off, val, sr):
    cases = mc.family(family, block)
    assert cases
    for c in cases:
        run_case(sp, oracle, c, off, val, sr, True)
        if family in mc.REAL_FAMILIES and mc.TYPES[val][0] != np.int32:
            run_case(sp, oracle, c, off, val, sr, False)
