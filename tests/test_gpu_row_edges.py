"""GPU suite: chunk_rows (csrc/xwindow.hpp), the body of the vector and light kinds' window kernels, at every lane-width,
step, long-row, tail, group, window and per-chunk-width edge — the table of tests/row_cases.py, whose reach
tests/test_row_cases_cpu.py proves on the host.  Every case creates its plans under exactly the knobs that force its shape
(T, workgroup size, rows per chunk, long-row threshold, window kind, weight cut, giant length) and FAILS if info() or
get_shape report another plan than the one it was built for.

Bars, none of them new: integer-valued data is exact in any order, so y equals the serial loop (oracle.spmv_serial) bit
for bit; real data (steps, long, huge, tail, adapt) lies within conftest.parity_bound of the fp64 sum.  Identities: two
executes of one plan give the same bytes; light gives vector's bytes; the packed plan gives the unpacked plan's bytes; a
16-bit-matrix plan gives the fp32 plan's bytes on the widened values; and on one case per family alpha = 2, beta = -1 over a
known y0 equals 2 * serial - y0 exactly.  y is poisoned with NaN before every execute, and the columns of x that no row
references hold NaN."""
import contextlib
import os

import numpy as np
import pytest
import torch

import row_cases as rc
from conftest import parity_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = {"vector": "csr_vector_window_kernel", "light": "light_rows_window_kernel"}
HALF = {"f16": torch.float16, "bf16": torch.bfloat16}


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


_refs = {}


def reference(oracle, m, vb, integer):
    """The serial loop's y, and for real data the fp64 sum with its per-row bound; once per (matrix, value size, data)."""
    key = (m, vb, integer)
    if key not in _refs:
        Ap, Aj = rc.structure(m)
        Ax, x, _ = rc.operands(m, vb, integer)
        serial = oracle.spmv_serial(Ap, Aj, Ax, x)
        _refs[key] = (serial, None if integer else parity_bound(oracle, Ap, Aj, Ax, x))
    return _refs[key]


def check_plan(p, c, kind, what, packed=None, half=False):
    """The plan is the one the case was built for."""
    want = rc.plan_of(c)
    info, sh = p.info(), p.shape()
    what = what + (kind, info)
    assert info["main_kernel"] == KERNEL[kind], what
    assert info["lanes_per_row"] == want["lanes_per_row"] == sh.lanes_per_row, what
    assert info["block_threads"] == want["block_threads"] == sh.block_threads, what
    assert info["rows_per_chunk"] == want["rows_per_chunk"] == sh.rows_per_chunk, what
    assert info["n_chunks"] == want["n_chunks"] == sh.n_chunks, what
    assert info["balanced_chunks"] == want["balanced_chunks"] == sh.balanced_chunks, what
    assert info["rows_cap"] == want["rows_cap"], what
    assert sh.long_steps == want["long_steps"], what
    assert sh.window_sweep == 0 and sh.small_plain == 0, what
    if want["balanced_chunks"]:
        assert (sh.bal_k, sh.bal_q) == (want["bal_k"], want["bal_q"]), (what, sh.bal_k, sh.bal_q)
        if "MI355_SPMV_GIANT_ROW" in c.knobs:
            assert sh.giant_len == int(c.knobs["MI355_SPMV_GIANT_ROW"]) and sh.giant_rows_enabled == 1, what
            assert info["n_kernels"] == (1 if half else 3), what
    kind_of = ("none" if sh.window_elems == 0 else "segments" if sh.window_segments >= 2 else
               "band" if sh.window_from_band else "sampled")
    assert kind_of == want["window"] and info["window_elems"] == sh.window_elems, (what, kind_of)
    if want["window"] == "band" and c.family == "window":     # the window whose edges the planted columns sit on
        assert sh.window_elems == want["band_window_elems"] and (sh.band_lo, sh.band_hi) == (-rc.HW, rc.HW), what
    if want["window"] == "segments":
        assert sh.window_segments == 3, what
    if packed is None:
        packed = want["packed"] and kind == "vector"
    assert (info["packed_index_bytes"] > 0) == packed, what
    if packed and c.family == "window":
        assert info["packed_index_escapes"] > 0, what
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


def run_case(sp, oracle, c, types, integer, half=True):
    m = c.matrix
    t_val, t_off = rc.TYPES[types]
    assert np.dtype(t_val).itemsize == c.vb
    Ap64, Aj = rc.structure(m)
    Ax, x, y0 = rc.operands(m, c.vb, integer)
    n, nnz = len(m.lens), int(Ap64[-1])
    serial, bound = reference(oracle, m, c.vb, integer)
    what = (c.name, types, "integer" if integer else "real")
    want = rc.plan_of(c)
    dAp, dAj, dAx, dx = d(Ap64.astype(t_off)), d(Aj), d(Ax), d(x)
    plans = {}
    try:
        with knobs(sp, c.knobs):
            for kind in ("vector", "light"):
                plans[kind] = sp.Plan(kind, n, m.n_cols, nnz, dAp, dAj, dx.dtype)
        if want["packed"]:
            with knobs(sp, dict(c.knobs, MI355_SPMV_PACK="0")):
                plans["unpacked"] = sp.Plan("vector", n, m.n_cols, nnz, dAp, dAj, dx.dtype)
        for name, p in plans.items():
            check_plan(p, c, "vector" if name == "unpacked" else name, what, packed=False if name == "unpacked" else None)
        got = {name: execute_twice(p, dAx, dx, n, dx.dtype, what + (name,)) for name, p in plans.items()}
        y = got["vector"]
        assert y.dtype == serial.dtype, what
        if bound is None:
            bad = np.nonzero(~(y == serial))[0]
            assert bad.size == 0, ("rows differ from the serial loop", bad[:8], y[bad[:8]], serial[bad[:8]], what)
        else:
            y64, per_row = bound
            err = np.abs(y.astype(np.float64) - y64)
            bad = np.nonzero(~(err <= per_row))[0]
            assert bad.size == 0, ("rows outside the parity bound", bad[:8], err[bad[:8]], per_row[bad[:8]], what)
        assert got["light"].tobytes() == y.tobytes(), ("light differs from vector", np.nonzero(~(got["light"] == y))[0][:8], what)
        if "unpacked" in got:
            assert got["unpacked"].tobytes() == y.tobytes(), ("the packed plan differs from the unpacked one",
                                                              np.nonzero(~(got["unpacked"] == y))[0][:8], what)
        if integer and types == "f32-i32" and rc.ALPHA_BETA_CASES[c.family] == c.name:
            alpha, beta = rc.ALPHA_BETA
            for kind in ("vector", "light"):
                plans[kind].set_alpha_beta(alpha, beta)
                yab = d(y0)
                plans[kind].execute(dAx, dx, yab)
                torch.cuda.synchronize()
                out = yab.cpu().numpy()
                expect = (t_val(alpha) * serial + t_val(beta) * y0).astype(t_val)
                bad = np.nonzero(~(out == expect))[0]
                assert bad.size == 0, ("alpha / beta: rows differ", kind, bad[:8], out[bad[:8]], expect[bad[:8]], what)
        if half and integer and types == "f32-i32" and c.family in rc.HALF_FAMILIES:
            # the 16-bit matrix: the fp32 plan of the structure with another stored type; these integers are exact in both
            for tag, dtype in HALF.items():
                with knobs(sp, c.knobs):
                    ph = sp.Plan("vector", n, m.n_cols, nnz, dAp, dAj, torch.float32, mat_dtype=dtype)
                try:
                    check_plan(ph, c, "vector", what + (tag,), half=True)
                    Ah = dAx.to(dtype)
                    assert torch.equal(Ah.to(torch.float32), dAx), what
                    yh = execute_twice(ph, Ah, dx, n, torch.float32, what + (tag,))
                    assert yh.tobytes() == y.tobytes(), ("the %s plan differs from the fp32 plan" % tag,
                                                         np.nonzero(~(yh == y))[0][:8], what)
                finally:
                    ph.destroy()
    finally:
        for p in plans.values():
            p.destroy()


def groups():
    out = []
    for fam in rc.FAMILIES:
        for T in rc.FAMILY_LANES[fam]:
            for types in rc.FAMILY_TYPES[fam]:
                out.append(pytest.param(fam, T, types, id="%s-T%d-%s" % (fam, T, types)))
    return out


@pytest.mark.parametrize("fam,T,types", groups())
def test_family(sp, oracle, fam, T, types):
    cases = rc.family(fam, T, np.dtype(rc.TYPES[types][0]).itemsize)
    assert cases
    for c in cases:
        run_case(sp, oracle, c, types, True)
        if fam in rc.REAL_FAMILIES:
            run_case(sp, oracle, c, types, False)
