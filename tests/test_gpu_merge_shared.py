"""GPU suite: the two kernels every value type of the merge kind shares — merge_search_kernel in front of the main kernel
and merge_fixup_kernel behind it (merge_plan.hip: compiled once, launched for every typed instantiation of launch_merge).

One small ragged matrix under MI355_MERGE_FUSED=0 (the search kernel in front, never inside the tile kernel) and
MI355_MERGE_TPS=2 (runs of two tiles: ~15 runs, rows that straddle run boundaries, so the fix-up adds carries), for both
offset widths, every value-type instantiation, a rounding-free pair of semirings and every width of the search.

Bar: integer-valued data, so (+, *) is exact in any order and (min, +) never rounds: every result equals the serial
loop bit for bit; the tile coordinates the search kernel left behind equal the oracle's restatement of the reference's
search."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3001
KNOBS = {"MI355_MERGE_FUSED": "0", "MI355_MERGE_TPS": "2"}
NP_OFF = {"i32": np.int32, "i64": np.int64}
# value-type case -> (type of x and y, type the matrix is stored in; None: a pattern matrix)
TYPES = {"f32": (np.float32, np.float32), "f64": (np.float64, np.float64), "i32": (np.int32, np.int32),
         "f32-under-f64": (np.float64, np.float32), "pattern-f32": (np.float32, None)}


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def matrix():
    """3 001 rows whose lengths cycle through 0..40, 200 empty rows in the middle, nnz % 4 == 3."""
    lens = np.arange(N, dtype=np.int64) % 41
    lens[1400:1600] = 0
    lens[N - 1] += (3 - int(lens.sum())) % 4
    Ap = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    assert nnz % 4 == 3
    rng = np.random.RandomState(41)
    Aj = np.concatenate([np.sort(rng.choice(N, size=k, replace=False)) for k in lens]).astype(np.int32)
    Ax = rng.randint(-3, 4, size=nnz)
    x = rng.randint(-2, 3, size=N)
    return Ap, Aj, Ax, x


EXPECTED = {}


def expected(oracle, sr, val):
    """The serial loop's y (the matrix widened to the type of x and y; ones for the pattern), computed once per case."""
    if (sr, val) not in EXPECTED:
        Ap, Aj, Ax, x = matrix()
        t_vec, t_mat = TYPES[val]
        A = np.ones(Aj.size, dtype=t_vec) if t_mat is None else Ax.astype(t_mat).astype(t_vec)
        EXPECTED[sr, val] = oracle.spmv_genl_serial(sr, Ap, Aj, A, x.astype(t_vec))
    return EXPECTED[sr, val]


@pytest.fixture(params=[1, 4, 16], ids=lambda lanes: "lanes%d" % lanes)
def search_in_front(request, sp):
    """KNOBS and MI355_MERGE_SEARCH_LANES while the test creates its plan."""
    knobs = dict(KNOBS, MI355_MERGE_SEARCH_LANES=str(request.param))
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    sp.capi.lib().mi355_spmv_knobs_reload()
    yield request.param
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    sp.capi.lib().mi355_spmv_knobs_reload()


@pytest.mark.parametrize("sr", ["plus_times", "min_plus"])
@pytest.mark.parametrize("val", list(TYPES))
@pytest.mark.parametrize("off", ["i32", "i64"])
def test_search_in_front_and_fixup_behind(sp, oracle, search_in_front, off, val, sr):
    Ap, Aj, Ax, x = matrix()
    t_vec, t_mat = TYPES[val]
    nnz = int(Ap[-1])
    dAp, dAj, dx = d(Ap.astype(NP_OFF[off])), d(Aj), d(x.astype(t_vec))
    dAx = None if t_mat is None else d(Ax.astype(t_mat))
    mat_dtype = "pattern" if t_mat is None else dAx.dtype
    p = sp.Plan("merge", N, N, nnz, dAp, dAj, dx.dtype, mat_dtype=mat_dtype)
    try:
        info = p.info()
        # the search kernel, the tile kernel on several runs of two tiles, the fix-up
        assert info["main_kernel"] == "merge_tile_kernel" and info["n_kernels"] == 3, info
        assert info["grid_blocks"] >= 8 and info["n_tiles"] > info["grid_blocks"], info
        p.set_semiring(sr)
        y = torch.full((N,), -77777777, dtype=dx.dtype, device=DEV)
        p.execute(dAx, dx, y)
        torch.cuda.synchronize()
        got, want = y.cpu().numpy(), expected(oracle, sp.capi.SEMIRINGS[sr], val)
        assert got.dtype == want.dtype and np.array_equal(got, want), (int((got != want).sum()), info)
        rows, nz = p.merge_coords()
        want_rows, want_nz = oracle.merge_tile_coords(Ap.astype(NP_OFF[off]), info["tile_items"])
        assert info["n_tiles"] + 1 == len(want_rows)
        assert np.array_equal(rows, want_rows) and np.array_equal(nz, want_nz)
    finally:
        p.destroy()
