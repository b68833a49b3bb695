"""GPU suite: the executes of a merge plan built for its row-parallel run kernel (merge_rows_kernel) that the run kernel
does not serve — another semiring, the one-shot generalized entry points, an fp32 matrix under fp64 vectors, unaligned
views — and that walk the plan's tiles with merge_tile_kernel instead (merge_launch.hpp, launch_merge).  The plans are
the wide ones of tests/test_gpu_parity.py: 512- and 1 024-thread runs with one window of x, runs that sweep a band
wider than any window, and runs that stage a window segment per band.  Their window was sized for the run kernel
(up to ~155 KB of LDS): the tile kernel must not inherit it.

Bar: min / max semirings never round and a + x, a * x round once, so those are bit-exact against the serial loop;
plus-times within the per-row bound; the fp32 matrix under fp64 vectors within the fp64 bound around the widened
matrix (no fp32 rounding anywhere)."""
import numpy as np
import pytest
import torch

from conftest import parity_bound, seeded_x
from small_path import forced

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEMIRINGS = ("min_plus", "max_times", "max_plus", "or_and")


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def swept_band(val):
    """test_merge_runs_sweep_a_band_wider_than_any_window's matrix: 31 per row in a band of +-40 000 (fp32) or
    +-20 000 (fp64) columns, a few rows of 200 and empty rows the probe does not see."""
    rng = np.random.default_rng(37)
    n, per_row = 600_003, 31
    hw = 40_000 if val == "f32" else 20_000
    lens = np.full(n, per_row, dtype=np.int64)
    probed = set(((n - 1) * np.arange(256)) // 255)
    lens[[r for r in (5, 1001, 150_001, n - 2) if r not in probed]] = 200
    lens[[r for r in (7, 333_333) if r not in probed]] = 0
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    lo = np.clip(rows - hw, 0, n - 1)
    hi = np.clip(rows + hw, 0, n - 1)
    cols = lo + (rng.random(nnz) * (hi - lo + 1)).astype(np.int64)
    Aj = cols[np.lexsort((cols, rows))].astype(np.int32)
    return Ap, Aj, n


# (shape, off, val, what the plan must be: threads of the run kernel, window segments)
CASES = [
    pytest.param(("sweep", "i32", "f32", (1024, 1)), id="sweep-i32-f32"),
    pytest.param(("sweep", "i64", "f64", (1024, 1)), id="sweep-i64-f64"),
    pytest.param((("band", 4096), "i32", "f64", (512, 1)), id="band4096-i32-f64-512"),
    pytest.param((("band", 4096), "i64", "f64", (512, 1)), id="band4096-i64-f64-512"),
    pytest.param((("band", 16384), "i32", "f32", (1024, 1)), id="band16384-i32-f32-1024"),
    pytest.param((("band", 8192), "i64", "f64", (1024, 1)), id="band8192-i64-f64-1024"),
    pytest.param(("stencil", "i64", "f64", (256, 3)), id="stencil-i64-f64"),
    pytest.param(("stencil", "i32", "f32", (256, 3)), id="stencil-i32-f32"),
]


@pytest.fixture(scope="module", params=CASES)
def wide_plan(request, sp):
    shape, off, val, want = request.param
    to = {"i32": np.int32, "i64": np.int64}[off]
    tv = {"f32": np.float32, "f64": np.float64}[val]
    t_off = {"i32": torch.int32, "i64": torch.int64}[off]
    t_val = {"f32": torch.float32, "f64": torch.float64}[val]
    if shape == "sweep":
        Ap, Aj, n = swept_band(val)
        Ap, n_cols = Ap.astype(to), n
    elif shape == "stencil":
        m = sp.synth.stencil27(90, 90, 90, 4, DEV, val_dtype=t_val, off_dtype=t_off)
        Ap, Aj, _ = m.numpy()
        n_cols = m.n_cols
        del m
    else:
        m = sp.synth.banded_fixed(1_300_000, 32, shape[1], 8, DEV, val_dtype=t_val, off_dtype=t_off)
        Ap, Aj, _ = m.numpy()
        n_cols = m.n_cols
        del m
    rng = np.random.RandomState(len(Ap) % 9973)
    nnz = int(Ap[-1])
    Ax = (rng.rand(nnz) - 0.5).astype(tv)
    x = seeded_x(n_cols, tv)
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    p = sp.Plan("merge", len(Ap) - 1, n_cols, nnz, dAp, dAj, dAx.dtype)
    info = p.info()
    if not forced():                                  # the plan really is the row-parallel one, with its wide window
        block, segments = want
        assert info["main_kernel"] == "merge_rows_kernel" and info["block_threads"] == block, info
        assert info["window_segments"] == segments and info["window_elems"] > 0, info
        if block > 256:
            assert info["window_elems"] * Ax.itemsize > 64 * 1024, info
    yield dict(p=p, Ap=Ap, Aj=Aj, Ax=Ax, x=x, n_cols=n_cols, dAp=dAp, dAj=dAj, dAx=dAx, val=val, info=info, rng=rng)
    p.destroy()


def test_other_semirings_on_a_run_plan_are_bit_exact(sp, oracle, wide_plan):
    w = wide_plan
    p, Ap, Aj, n_rows = w["p"], w["Ap"], w["Aj"], len(w["Ap"]) - 1
    rng = np.random.RandomState(5)
    Ab = (rng.rand(Aj.size) < 0.5).astype(w["Ax"].dtype)            # or_and: booleans as 0.0 / 1.0
    xb = (rng.rand(w["n_cols"]) < 0.25).astype(w["Ax"].dtype)
    try:
        for sr in SEMIRINGS:
            Ax, x = (Ab, xb) if sr == "or_and" else (w["Ax"], w["x"])
            p.set_semiring(sr)
            y = torch.full((n_rows,), float("nan"), dtype=w["dAx"].dtype, device=DEV)
            p.execute(d(Ax), d(x), y)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            want = oracle.spmv_genl_serial(sp.capi.SEMIRINGS[sr], Ap, Aj, Ax, x)
            assert np.array_equal(got, want), (sr, int((got != want).sum()), w["info"])
            y1 = torch.full((n_rows,), float("nan"), dtype=w["dAx"].dtype, device=DEV)
            sp.spmv_genl(sr, n_rows, w["n_cols"], int(Ap[-1]), w["dAp"], w["dAj"], d(Ax), d(x), y1)
            assert torch.equal(y1, y), sr                                # the one-shot entry point: the same bits
    finally:
        p.set_semiring("plus_times")
        sp.capi.cache_release()


def test_fp32_matrix_under_fp64_vectors_on_a_run_plan(sp, oracle, wide_plan):
    """The typed plan of the same structure (shaped for fp64 vectors), with and without alpha / beta."""
    w = wide_plan
    Ap, Aj, n_rows = w["Ap"], w["Aj"], len(w["Ap"]) - 1
    A32 = w["Ax"].astype(np.float32)
    x = w["x"].astype(np.float64)
    q = sp.Plan("merge", n_rows, w["n_cols"], int(Ap[-1]), w["dAp"], w["dAj"], torch.float64, mat_dtype=torch.float32)
    try:
        info = q.info()
        if not forced():
            assert info["main_kernel"] == "merge_rows_kernel", info
        y = torch.full((n_rows,), float("nan"), dtype=torch.float64, device=DEV)
        q.execute(d(A32), d(x), y)
        torch.cuda.synchronize()
        y64, bound = parity_bound(oracle, Ap, Aj, A32.astype(np.float64), x, 8)
        err = np.abs(y.cpu().numpy() - y64)
        assert not np.isnan(err).any() and np.all(err <= bound), (int((err > bound).sum()), info)
        q.set_alpha_beta(-0.5, 0.25)
        y0 = w["rng"].rand(n_rows)
        y2 = d(y0)
        q.execute(d(A32), d(x), y2)
        torch.cuda.synchronize()
        assert np.all(np.abs(y2.cpu().numpy() - (-0.5 * y64 + 0.25 * y0)) <= 0.5 * bound + 2.0 ** -52 * np.abs(y0) + 1e-300)
    finally:
        q.destroy()


def test_plus_times_through_unaligned_views_on_a_run_plan(sp, oracle, wide_plan):
    w = wide_plan
    p, Ap, Aj, Ax, x, n_rows = w["p"], w["Ap"], w["Aj"], w["Ax"], w["x"], len(w["Ap"]) - 1
    nnz = int(Ap[-1])
    big_x = torch.zeros(nnz + 1, dtype=w["dAx"].dtype, device=DEV)
    big_x[1:] = w["dAx"]
    dAx = big_x[1:]
    assert dAx.data_ptr() % 16 != 0
    y = torch.full((n_rows,), float("nan"), dtype=dAx.dtype, device=DEV)
    p.execute(dAx, d(x), y)
    torch.cuda.synchronize()
    y64, bound = parity_bound(oracle, Ap, Aj, Ax, x, 8)
    got = y.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    bad = np.nonzero(np.abs(got - y64) > bound)[0]
    assert bad.size == 0, (bad[:5], w["info"])
