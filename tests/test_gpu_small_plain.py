"""GPU suite: the edges of the plain one-pass kernel (csr_vector_kernel) under the product's default — every lane width
the small-matrix rule picks (rows_plan.hip, shape_rows: 2 elements per lane up to 32 per row, 4 beyond; T = 2 .. 64), the
kSmallPlainNnz boundary itself, hub rows the structure probe does not see, tiny and degenerate matrices, alpha / beta.
Each case is checked row by row against the oracle (bound of tests/test_gpu_parity.py, bit-exact where integer-valued)."""
import numpy as np
import pytest
import torch

from conftest import parity_bound
from small_path import SMALL_PLAIN_NNZ, WEIGHT_CUT, check_kernel, plain_lanes, small_on  # noqa: F401  (small_on: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
COMBOS = [("i32", "f32"), ("i32", "f64"), ("i64", "f32"), ("i64", "f64")]
# mean row lengths: both sides of every lane-width step, and of the 2 -> 4 elements-per-lane switch at 32
MEANS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 300)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def regular_csr(rng, mean, n_rows, n_cols, hw=1500):
    """Rows of exactly `mean` nonzeros on average: pairs of rows mean + j and mean - j (j up to a quarter of the mean),
    sorted columns in a band of +-hw around the diagonal."""
    lens = np.full(n_rows, mean, dtype=np.int64)
    j = rng.randint(0, mean // 4 + 1, size=n_rows // 2)
    lens[0:2 * (n_rows // 2):2] += j
    lens[1:2 * (n_rows // 2):2] -= j
    Ap = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    centre = rows * n_cols // n_rows
    cols = np.clip(centre + rng.randint(-hw, hw + 1, size=rows.size), 0, n_cols - 1)
    cols = cols[np.lexsort((cols, rows))]
    return Ap, cols.astype(np.int32)


def run(sp, kind, n_rows, n_cols, Ap, Aj, Ax, x, y=None):
    p = sp.Plan(kind, n_rows, n_cols, int(Ap[-1]), d(Ap), d(Aj), d(Ax).dtype)
    if y is None:
        y = torch.full((n_rows,), float("nan"), dtype=d(Ax).dtype, device=DEV)
    p.execute(d(Ax), d(x), y)
    torch.cuda.synchronize()
    return p, y


def assert_rows(oracle, Ap, Aj, Ax, x, y, what):
    y = y.cpu().numpy()
    assert not np.isnan(y).any(), "%s: a row was skipped" % what
    y64, bound = parity_bound(oracle, Ap, Aj, Ax, x)
    bad = np.nonzero(np.abs(y.astype(np.float64) - y64) > bound)[0]
    assert bad.size == 0, "%s: rows outside the bound %s" % (what, bad[:5])


@pytest.mark.parametrize("off,val", COMBOS)
def test_every_lane_width_of_the_plain_kernel(sp, oracle, small_on, off, val):
    """The lane rule restated (small_path.plain_lanes) for every mean of MEANS; n_rows = 4 q + 2, so that no T divides
    the rows into whole workgroups (256 / T rows each).  Every row against the bound; integer values with x = 1
    bit-exact; alpha / beta, with beta = 0 on a NaN-poisoned y (y must come out finite) and beta != 0."""
    rng = np.random.RandomState(500 + MEANS[-1])
    reached = set()
    for mean in MEANS:
        n_rows = 4 * (max(2000, 400_000 // mean) // 4) + 2
        n_cols = n_rows + 77
        Ap, Aj = regular_csr(rng, mean, n_rows, n_cols)
        Ap = Ap.astype(NP[off])
        nnz = int(Ap[-1])
        assert nnz == mean * n_rows
        Ax = (rng.rand(nnz) * 2 - 1).astype(NP[val])
        x = (rng.rand(n_cols) * 2 - 1).astype(NP[val])
        T = plain_lanes(nnz, n_rows)
        what = "mean %d, %s/%s, T %d" % (mean, off, val, T)
        ys = {}
        for kind in ("vector", "light"):
            p, y = run(sp, kind, n_rows, n_cols, Ap, Aj, Ax, x)
            check_kernel(p, "default", lanes=T)
            assert_rows(oracle, Ap, Aj, Ax, x, y, "%s %s" % (what, kind))
            ys[kind] = y
            p.destroy()
        assert torch.equal(ys["vector"], ys["light"]), what
        reached.add(T)
        # integer values, x = 1: exact in any order
        Ai = rng.randint(-3, 4, size=nnz).astype(NP[val])
        ones = np.ones(n_cols, NP[val])
        p, y = run(sp, "vector", n_rows, n_cols, Ap, Aj, Ai, ones)
        assert np.array_equal(y.cpu().numpy(), oracle.spmv_serial(Ap, Aj, Ai, ones)), what
        # alpha / beta: beta = 0 never reads y (NaN-poisoned here); beta != 0 adds it
        p.set_alpha_beta(2.0, 0.0)
        y2 = torch.full((n_rows,), float("nan"), dtype=y.dtype, device=DEV)
        p.execute(d(Ai), d(ones), y2)
        y0 = (rng.rand(n_rows) * 2 - 1).astype(NP[val])
        y3 = d(y0)
        p.set_alpha_beta(1.5, -0.5)
        p.execute(d(Ax), d(x), y3)
        torch.cuda.synchronize()
        p.destroy()
        assert torch.isfinite(y2).all() and torch.equal(y2, 2.0 * y), what
        y64, bound = parity_bound(oracle, Ap, Aj, Ax, x)
        eps = 2.0 ** -24 if val == "f32" else 2.0 ** -53
        want = 1.5 * y64 - 0.5 * y0.astype(np.float64)
        tol = 1.5 * bound + 3 * eps * (np.abs(want) + 0.5 * np.abs(y0)) + 1e-300
        bad = np.nonzero(np.abs(y3.cpu().numpy().astype(np.float64) - want) > tol)[0]
        assert bad.size == 0, "%s: alpha / beta rows outside the bound %s" % (what, bad[:5])
    print("plain kernel, %s/%s: lanes per row reached %s" % (off, val, sorted(reached)))
    assert reached == {2, 4, 8, 16, 32, 64}


def test_the_small_matrix_threshold_is_inclusive(sp, oracle, small_on):
    """banded_fixed(128 125, 32) holds exactly kSmallPlainNnz = 4 100 000 nonzeros: the plain kernel (16 lanes per row);
    one row more is above it: the chunked kernels."""
    m = sp.synth.banded_fixed(128125, 32, 2048, 3, DEV)
    assert m.nnz == SMALL_PLAIN_NNZ
    x = sp.synth.dense_vector(m.n_cols, m.Ax.dtype, 3, DEV)
    Ap, Aj, Ax = m.numpy()
    for kind in ("vector", "light"):
        p = sp.Plan(kind, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, m.Ax.dtype)
        check_kernel(p, "default", lanes=plain_lanes(m.nnz, m.n_rows))
        y = torch.full((m.n_rows,), float("nan"), device=DEV)
        p.execute(m.Ax, x, y)
        torch.cuda.synchronize()
        p.destroy()
        assert_rows(oracle, Ap, Aj, Ax, x.cpu().numpy(), y, "threshold %s" % kind)
    m = sp.synth.banded_fixed(128126, 32, 2048, 3, DEV)
    assert m.nnz == SMALL_PLAIN_NNZ + 32
    for kind in ("vector", "light"):
        p = sp.Plan(kind, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, m.Ax.dtype)
        check_kernel(p, "chunked")
        p.destroy()


# where the rule sends a regular matrix with hub rows, and why: the probe does not see them, but decide_balance's pass
# over every chunk does — from 5 000 nonzeros on, in 1 M, the chunked kernels' weight-cut plan takes the matrix
HUBS = {5000: WEIGHT_CUT, 50_000: WEIGHT_CUT, 200_000: WEIGHT_CUT}


@pytest.mark.parametrize("hub", sorted(HUBS))
def test_hub_rows_the_probe_does_not_see(sp, oracle, small_on, hub):
    """A regular matrix (16 per row) with three rows of `hub` nonzeros placed where the 256-row structure probe does
    not look (analyze.hip, probe_structure samples rows (n - 1) i / 255): the plan it gets, every row, vector = light."""
    rng = np.random.RandomState(hub % 1000 + 7)
    n = 60_002
    Ap, Aj = regular_csr(rng, 16, n, n)
    lens = np.diff(Ap)
    probed = set(((n - 1) * np.arange(256)) // 255)
    hubs = [r for r in (3, n // 2 + 1, n - 3) if r not in probed]
    assert len(hubs) == 3
    lens[hubs] = hub
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows + rng.randint(-1500, 1501, size=nnz), 0, n - 1)
    for r in hubs:
        cols[Ap[r]:Ap[r + 1]] = rng.randint(0, n, size=hub)                   # a hub row spans every column
    Aj = cols.astype(np.int32)
    Ax = (rng.rand(nnz) * 2 - 1).astype(np.float32)
    x = (rng.rand(n) * 2 - 1).astype(np.float32)
    ys = []
    for kind in ("vector", "light"):
        p, y = run(sp, kind, n, n, Ap.astype(np.int32), Aj, Ax, x)
        print("hub %d, %s: %s" % (hub, kind, {k: p.info()[k] for k in ("main_kernel", "lanes_per_row", "balanced_chunks")}))
        check_kernel(p, "default", HUBS[hub], lanes=None if HUBS[hub] else plain_lanes(nnz, n))
        p.destroy()
        assert_rows(oracle, Ap, Aj, Ax, x, y, "hub %d %s" % (hub, kind))
        ys.append(y)
    assert torch.equal(ys[0], ys[1])


@pytest.mark.parametrize("off,val", COMBOS)
def test_tiny_and_degenerate_matrices(sp, oracle, small_on, off, val):
    """nnz < 4 (the 16-byte path needs 4), empty leading and trailing rows, one column, rows not a multiple of 256 / T;
    integer-valued, so every case is bit-exact against the serial sum."""
    rng = np.random.RandomState(61)
    cases = []
    for nnz in (0, 1, 2, 3):                                           # 7 rows, the nonzeros in the middle ones
        lens = np.zeros(7, np.int64)
        lens[2:2 + nnz] = 1
        cases.append((lens, 5))
    lens = np.zeros(1000, np.int64)                                    # empty leading and trailing rows
    lens[300:700] = rng.randint(1, 40, size=400)
    cases.append((lens, 3000))
    cases.append((rng.randint(0, 9, size=777), 1))                     # a single column
    for T in (2, 4, 8, 16, 32, 64):                                    # n_rows = 256 / T * q + 1
        mean = {2: 3, 4: 6, 8: 14, 16: 40, 32: 100, 64: 200}[T]
        cases.append((np.full(256 // T * 5 + 1, mean, np.int64), 500))
    for lens, n_cols in cases:
        n_rows = lens.size
        Ap = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(lens, out=Ap[1:])
        Ap = Ap.astype(NP[off])
        nnz = int(Ap[-1])
        Aj = rng.randint(0, n_cols, size=nnz).astype(np.int32)
        Ax = rng.randint(-3, 4, size=nnz).astype(NP[val])
        x = rng.randint(-2, 3, size=n_cols).astype(NP[val])
        want = oracle.spmv_serial(Ap, Aj, Ax, x)
        what = "%d rows, %d nonzeros, %d columns" % (n_rows, nnz, n_cols)
        for kind in ("vector", "light"):
            p, y = run(sp, kind, n_rows, n_cols, Ap, Aj, Ax, x)
            check_kernel(p, "default", lanes=plain_lanes(nnz, n_rows))
            p.destroy()
            assert np.array_equal(y.cpu().numpy(), want), "%s %s" % (what, kind)
            y1 = torch.full((n_rows,), float("nan"), dtype=y.dtype, device=DEV)
            sp.spmv(kind, n_rows, n_cols, nnz, d(Ap), d(Aj), d(Ax), d(x), y1)
            assert torch.equal(y1, y), "%s %s one-shot" % (what, kind)
