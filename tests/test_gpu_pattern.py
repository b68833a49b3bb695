"""GPU suite: pattern (value-free) matrices on the merge kind — MI355_VAL_PATTERN as the mat_type of a typed plan,
the mi355_spmv_merge_pattern_* one-shots, Plan(..., mat_dtype="pattern") / spmv_pattern, and the harness label
hip_merge_pattern.  Every stored entry counts as one in the type of x and y; Ax is never read.

Bar: expected values are oracle.spmv_genl_serial(semiring, Ap, Aj, ones, x) (the restatement pinned to the
reference's SpMV_genl_cpu_navie).  min / max never round and 1 + x, 1 * x round at most once, so int32 and the
min / max / or semirings are bit-exact; so is (+, *) on integer-valued x (every partial sum is exact); (+, *) on real x
is held to the per-row parity bound (len + 2) eps sum|x| around the fp64 serial sum (conftest.parity_bound, Ax = ones)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, parity_bound, random_csr, seeded_x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
TV = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32}
SEMIRINGS = ("plus_times", "min_plus", "max_times", "max_plus", "or_and")
N_ROWS, N_COLS = 20011, 5000


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(n, val):
    """y before a product: NaN, or a sentinel no result can be for the integer type."""
    if val == "i32":
        return torch.full((n,), -77777777, dtype=torch.int32, device=DEV)
    return torch.full((n,), float("nan"), dtype=TV[val], device=DEV)


def vectors(val, n_cols, seed=3):
    """x per semiring: real (integers for i32), integer-valued, booleans."""
    rng = np.random.RandomState(seed)
    t = NP[val]
    real = rng.randint(-50, 51, size=n_cols).astype(t) if val == "i32" else (rng.rand(n_cols) * 2 - 1).astype(t)
    return {"real": real, "int": rng.randint(-3, 4, size=n_cols).astype(t), "bool": (rng.rand(n_cols) < 0.3).astype(t)}


@pytest.fixture(scope="module")
def hub():
    """Ragged, with empty rows, several tiles, one row of 30 000 that spans tiles (carries through the fix-up launch)."""
    Ap, Aj, _ = random_csr(np.random.RandomState(20), N_ROWS, N_COLS, 12, long_row=30000)
    return Ap.astype(np.int64), Aj


def check(oracle, sr, Ap, Aj, x, got, exact=None):
    """got against the oracle with Ax = ones: bit-exact, or within the parity bound for (+, *) on real floats."""
    ones = np.ones(Aj.size, dtype=x.dtype)
    if exact is None:
        exact = sr != "plus_times" or x.dtype == np.int32
    if exact:
        want = oracle.spmv_genl_serial(SEMIRINGS.index(sr), Ap, Aj, ones, x)
        assert np.array_equal(got, want), (sr, x.dtype, int((got != want).sum()))
    else:
        y64, bound = parity_bound(oracle, Ap, Aj, ones, x)
        err = np.abs(got.astype(np.float64) - y64)
        assert not np.isnan(err).any() and np.all(err <= bound), (sr, x.dtype, int((~(err <= bound)).sum()))


def run_all_semirings(sp, oracle, Ap, Aj, n_rows, n_cols, val, dAj=None):
    """One-shot and a plan executed twice, all five semirings, y poisoned before every product."""
    nnz = int(Ap[-1])
    dAp = d(Ap)
    dAj = d(Aj) if dAj is None else dAj
    xs = vectors(val, n_cols)
    p = sp.Plan("merge", n_rows, n_cols, nnz, dAp, dAj, TV[val], mat_dtype="pattern")
    try:
        assert p.mat_type() == 3 and p.info()["main_kernel"] == "merge_tile_kernel", p.info()
        for sr in SEMIRINGS:
            for name in (("bool",) if sr == "or_and" else ("real", "int") if sr == "plus_times" else ("real",)):
                x = xs[name]
                exact = True if name == "int" else None
                y = poisoned(n_rows, val)
                sp.spmv_pattern(sr, n_rows, n_cols, nnz, dAp, dAj, d(x), y)
                check(oracle, sr, Ap, Aj, x, y.cpu().numpy(), exact)
                p.set_semiring(sr)
                for _ in range(2):
                    y2 = poisoned(n_rows, val)
                    p.execute(None, d(x), y2)
                    torch.cuda.synchronize()
                    assert torch.equal(y2.view(torch.uint8), y.view(torch.uint8)), (sr, name)   # the same bits as the one-shot
    finally:
        p.destroy()


@pytest.mark.parametrize("val", ["f32", "f64", "i32"])
@pytest.mark.parametrize("off", ["i32", "i64"])
def test_ragged_matrix_with_a_hub_row(sp, oracle, hub, off, val):
    Ap, Aj = hub
    run_all_semirings(sp, oracle, Ap.astype(NP[off]), Aj, N_ROWS, N_COLS, val)


@pytest.mark.parametrize("cut", [0, 1, 2, 3])
def test_array_tail(sp, oracle, hub, cut):
    """nnz % 4 = 0, 1, 2, 3: the nonzeros past the last whole 16-byte group are redone after the barrier."""
    Ap, Aj = hub
    nnz = int(Ap[-1]) - int(Ap[-1]) % 4 - cut            # ... % 4 == (4 - cut) % 4
    Ap2 = np.minimum(Ap, nnz)
    assert int(Ap2[-1]) % 4 == (4 - cut) % 4
    for off, val in (("i32", "f32"), ("i64", "f64"), ("i32", "i32")):
        run_all_semirings(sp, oracle, Ap2.astype(NP[off]), Aj[:nnz].copy(), N_ROWS, N_COLS, val)


@pytest.mark.parametrize("lens", [[0, 0, 0, 0, 0], [1], [3], [2, 0, 1], [0, 1, 0], [9001]],
                         ids=["all-empty", "nnz1", "one-row-nnz3", "nnz3", "nnz1-in-3-rows", "one-long-row"])
def test_degenerate_sizes(sp, oracle, lens):
    """nnz of 0, 1 and 3 (below the 16-byte path), one row, all rows empty."""
    rng = np.random.RandomState(len(lens))
    Ap = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Aj = rng.randint(0, 7, size=int(Ap[-1])).astype(np.int32)
    for off, val in (("i32", "f32"), ("i64", "f64"), ("i64", "i32")):
        run_all_semirings(sp, oracle, Ap.astype(NP[off]), Aj, len(lens), 7, val)


@pytest.fixture
def runs_of_8_tiles(sp):
    """MI355_MERGE_TPS=8 while the test creates its plans: the banded matrix below has 969 tiles, which the default rule
    leaves as runs of ONE tile each — and a run that short never stages a window of x."""
    old = os.environ.get("MI355_MERGE_TPS")
    os.environ["MI355_MERGE_TPS"] = "8"
    sp.capi.lib().mi355_spmv_knobs_reload()
    yield
    if old is None:
        os.environ.pop("MI355_MERGE_TPS", None)
    else:
        os.environ["MI355_MERGE_TPS"] = old
    sp.capi.lib().mi355_spmv_knobs_reload()


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64")])
def test_window_path(sp, oracle, runs_of_8_tiles, off, val):
    """The tile kernel's window of x: a band of +-700 columns as it is, then with a few dozen columns rewritten far outside
    the band (the rare out-of-window branch).  The valued plan of this shape is the row-parallel one; the pattern plan
    keeps its tiles, runs and window and walks the tiles."""
    n = 60_000
    m = sp.synth.banded_fixed(n, 32, 700, 5, DEV, val_dtype=TV[val], off_dtype={"i32": torch.int32, "i64": torch.int64}[off])
    Ap, Aj, _ = m.numpy()
    probed = set((((n - 1) * np.arange(256)) // 255).tolist())
    far = Aj.copy()
    rng = np.random.RandomState(8)
    rows = [r for r in rng.randint(0, n, size=60).tolist() if r not in probed][:40]
    for r in rows:                                         # not the first or last entry of a row: the window is placed from those
        far[int(Ap[r]) + 1 + rng.randint(30)] = (r + n // 2) % n
    assert len(rows) >= 24
    for cols in (Aj, far):
        dAp, dAj = d(Ap), d(cols)
        p = sp.Plan("merge", n, n, m.nnz, dAp, dAj, TV[val], mat_dtype="pattern")
        try:
            info = p.info()
            assert info["window_elems"] > 0 and info["main_kernel"] == "merge_tile_kernel", info
            xs = vectors(val, n)
            for sr, x in (("plus_times", xs["real"]), ("plus_times", xs["int"]), ("min_plus", xs["real"]), ("or_and", xs["bool"])):
                p.set_semiring(sr)
                y = poisoned(n, val)
                p.execute(None, d(x), y)
                torch.cuda.synchronize()
                check(oracle, sr, Ap, cols, x, y.cpu().numpy(), True if x is xs["int"] else None)
        finally:
            p.destroy()


@pytest.mark.parametrize("val", ["f32", "f64", "i32"])
def test_unaligned_view_of_aj(sp, oracle, hub, val):
    """Aj one element into its allocation: the 4-byte-per-lane form of the tile kernel."""
    Ap, Aj = hub
    big = torch.zeros(Aj.size + 1, dtype=torch.int32, device=DEV)
    big[1:] = d(Aj)
    view = big[1:]
    assert view.data_ptr() % 16 != 0
    run_all_semirings(sp, oracle, Ap.astype(np.int32), Aj, N_ROWS, N_COLS, val, dAj=view)


def test_ax_is_not_part_of_the_result(sp, hub):
    Ap, Aj = hub
    nnz = int(Ap[-1])
    dAp, dAj = d(Ap.astype(np.int32)), d(Aj)
    x = d(vectors("f32", N_COLS)["real"])
    p = sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, torch.float32, mat_dtype="pattern")
    ys = []
    for Ax in (None, torch.full((nnz,), float("nan"), device=DEV), torch.full((nnz + 1,), float("nan"), device=DEV)[1:]):
        y = poisoned(N_ROWS, "f32")
        p.execute(Ax, x, y)
        torch.cuda.synchronize()
        ys.append(y)
    p.destroy()
    assert not torch.isnan(ys[0]).any()
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32)) and torch.equal(ys[0].view(torch.int32), ys[2].view(torch.int32))


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64")])
def test_same_sums_as_the_valued_kernel(sp, hub, off, val):
    """Same tiles, same walk, same scan: y of the pattern plan equals, bit for bit, y of the valued tile kernel on Ax = ones."""
    Ap, Aj = hub
    nnz = int(Ap[-1])
    dAp, dAj = d(Ap.astype(NP[off])), d(Aj)
    x = d(vectors(val, N_COLS)["real"])
    pv = sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, TV[val])
    pp = sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, TV[val], mat_dtype="pattern")
    try:
        iv, ip = pv.info(), pp.info()
        assert iv["main_kernel"] == "merge_tile_kernel" and ip["main_kernel"] == "merge_tile_kernel", (iv, ip)
        for f in ("tile_items", "n_tiles", "grid_blocks", "block_threads", "n_kernels", "window_elems"):
            assert iv[f] == ip[f], (f, iv, ip)
        assert iv["n_tiles"] > 8 and iv["grid_blocks"] > 1
        yv, yp = poisoned(N_ROWS, val), poisoned(N_ROWS, val)
        pv.execute(torch.ones(nnz, dtype=TV[val], device=DEV), x, yv)
        pp.execute(None, x, yp)
        torch.cuda.synchronize()
        assert not torch.isnan(yp).any()
        assert torch.equal(yv.view(torch.uint8), yp.view(torch.uint8))
        (rv, nv), (rp, npp) = pv.merge_coords(), pp.merge_coords()
        assert np.array_equal(rv, rp) and np.array_equal(nv, npp)
    finally:
        pv.destroy()
        pp.destroy()


def test_no_plan_mix_up_between_valued_and_pattern_one_shots(sp, oracle, hub):
    """The valued one-shot keeps its plan, found again by the pointers of Ap / Aj: the pattern call in between must
    neither receive that plan nor leave its own behind for the next valued call."""
    Ap, Aj = hub
    Ap = Ap.astype(np.int32)
    nnz = int(Ap[-1])
    rng = np.random.RandomState(4)
    Ax = (rng.rand(nnz) * 2 - 1).astype(np.float32)
    x = vectors("f32", N_COLS)["real"]
    dAp, dAj, dAx, dx = d(Ap), d(Aj), d(Ax), d(x)
    y64, bound = parity_bound(oracle, Ap, Aj, Ax, x)
    try:
        for step in ("valued", "pattern", "valued", "pattern"):
            y = poisoned(N_ROWS, "f32")
            if step == "valued":
                sp.spmv_genl("plus_times", N_ROWS, N_COLS, nnz, dAp, dAj, dAx, dx, y)
                err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
                assert not np.isnan(err).any() and np.all(err <= bound), step
            else:
                sp.spmv_pattern("plus_times", N_ROWS, N_COLS, nnz, dAp, dAj, dx, y)
                check(oracle, "plus_times", Ap, Aj, x, y.cpu().numpy())
    finally:
        sp.capi.cache_release()


@pytest.mark.parametrize("val", ["f32", "f64"])
def test_alpha_beta(sp, oracle, hub, val):
    """The bound of test_gpu_parity.test_alpha_beta: (len + 3) eps (|alpha| sum|a x| + |beta y0|) around alpha y64 + beta y0."""
    Ap, Aj = hub
    Ap = Ap.astype(np.int32)
    nnz = int(Ap[-1])
    alpha, beta = -0.5, 0.25
    x = vectors(val, N_COLS)["real"]
    y0 = (np.random.RandomState(6).rand(N_ROWS) * 2 - 1).astype(NP[val])
    p = sp.Plan("merge", N_ROWS, N_COLS, nnz, d(Ap), d(Aj), TV[val], mat_dtype="pattern")
    y = d(y0.copy())
    p.set_alpha_beta(alpha, beta)
    p.execute(None, d(x), y)
    torch.cuda.synchronize()
    p.destroy()
    got = y.cpu().numpy().astype(np.float64)
    y64, yabs = oracle.spmv_ref64(Ap, Aj, np.ones(nnz, dtype=NP[val]), x)
    eps = 2.0 ** -24 if val == "f32" else 2.0 ** -53
    want = alpha * y64 + beta * y0.astype(np.float64)
    bound = (np.diff(Ap.astype(np.int64)) + 3) * eps * (abs(alpha) * yabs + np.abs(beta * y0.astype(np.float64))) + 1e-300
    assert not np.any(np.isnan(got)) and np.all(np.abs(got - want) <= bound)


def test_alpha_beta_refusals_and_mat_type(sp, hub):
    Ap, Aj = hub
    dAp, dAj = d(Ap.astype(np.int32)), d(Aj)
    p = sp.Plan("merge", N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, torch.float32, mat_dtype="pattern")
    assert p.mat_type() == 3
    p.set_semiring("min_plus")
    with pytest.raises(RuntimeError, match="not supported"):
        p.set_alpha_beta(2.0, 0.0)
    p.destroy()
    q = sp.Plan("merge", N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, torch.int32, mat_dtype="pattern")
    assert q.mat_type() == 3
    with pytest.raises(RuntimeError, match="not supported"):
        q.set_alpha_beta(2.0, 0.0)
    q.destroy()
    v = sp.Plan("merge", N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, torch.float64)
    assert v.mat_type() == sp.capi.VAL_TYPES[torch.float64][0]
    v.destroy()
    auto = sp.Plan("auto", N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, torch.float32, mat_dtype="pattern")
    assert auto.info()["kind"] == sp.capi.KINDS["merge"] and auto.mat_type() == 3
    auto.destroy()


def test_reuse_structure_side_stream_and_graph(sp, oracle, hub):
    Ap, Aj = hub
    Ap = Ap.astype(np.int32)
    nnz = int(Ap[-1])
    dAp, dAj = d(Ap), d(Aj)
    xs = [(np.random.RandomState(s).rand(N_COLS) * 2 - 1).astype(np.float32) for s in (1, 2, 3)]
    # MI355_PLAN_REUSE_STRUCTURE: the tile coordinates of the first execute serve the next ones
    p = sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, torch.float32, flags=sp.capi.PLAN_REUSE_STRUCTURE, mat_dtype="pattern")
    for x in xs:
        y = poisoned(N_ROWS, "f32")
        p.execute(None, d(x), y)
        torch.cuda.synchronize()
        check(oracle, "plus_times", Ap, Aj, x, y.cpu().numpy())
    p.destroy()
    p = sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, torch.float32, mat_dtype="pattern")
    # a side stream
    s = torch.cuda.Stream()
    dx = d(xs[0])
    y = poisoned(N_ROWS, "f32")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        p.execute(None, dx, y)
    s.synchronize()
    check(oracle, "plus_times", Ap, Aj, xs[0], y.cpu().numpy())
    # one capture, replayed on new x
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.execute(None, dx, y)
    dx.copy_(torch.from_numpy(xs[1]))
    y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    check(oracle, "plus_times", Ap, Aj, xs[1], got)
    y2 = poisoned(N_ROWS, "f32")
    p.execute(None, dx, y2)
    torch.cuda.synchronize()
    assert np.array_equal(got, y2.cpu().numpy())
    del g
    p.destroy()


def test_refusals(sp, hub):
    import ctypes as C
    Ap, Aj = hub
    dAp, dAj = d(Ap.astype(np.int32)), d(Aj)
    nnz = int(Ap[-1])
    for kind in ("vector", "light"):
        with pytest.raises(RuntimeError, match="not supported"):
            sp.Plan(kind, N_ROWS, N_COLS, nnz, dAp, dAj, torch.float32, mat_dtype="pattern")
    with pytest.raises((KeyError, TypeError, RuntimeError)):
        sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, "pattern")
    lib = sp.capi.lib()
    h = C.c_void_p()
    ptrs = (C.c_void_p(dAp.data_ptr()), C.c_void_p(dAj.data_ptr()))
    assert lib.mi355_spmv_plan_create(C.byref(h), 1, 0, 3, N_ROWS, N_COLS, nnz, *ptrs, 0) == 1 and not h.value
    for mat, xt, yt in ((3, 3, 3), (0, 3, 3), (3, 3, 0), (3, 0, 3)):             # pattern as the type of x or y
        assert lib.mi355_spmv_plan_create_typed(C.byref(h), 1, 0, mat, xt, yt, N_ROWS, N_COLS, nnz, *ptrs, 0) == 1 and not h.value
    assert lib.mi355_spmv_plan_create_typed(C.byref(h), 0, 0, 3, 0, 0, N_ROWS, N_COLS, nnz, *ptrs, 0) == 2 and not h.value
    assert b"pattern" in lib.mi355_spmv_last_error()
    assert lib.mi355_spmv_plan_acquire(C.byref(h), 1, 0, 3, N_ROWS, N_COLS, nnz, *ptrs) == 1 and not h.value


EXE = os.path.join(ROOT, "spmv-samples_amd", "bin", "spmv")


def test_harness_label(sp):
    """bin/spmv <pattern file> hip_merge_pattern passes the harness's own CPU check (the loader gives a pattern file's
    entries the value 1); on a matrix with real values the same label computes another product and the check shows it."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "spmv-samples_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "spmv-samples_amd", "host")], check=True)
    row = r"^\[hip_merge_pattern\] sum: +([0-9.eE+-]+|nan)  avg: +([0-9.eE+-]+|nan)$"
    for extra in ([], ["--dtype", "f64", "--offset", "64"]):
        r = subprocess.run([EXE, os.path.join(GOLD, "pat3x4_dup_unsorted.mtx"), "hip_merge_pattern", "hip_merge", "--iters", "3", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        m = re.search(row, r.stdout, re.M)
        assert m and float(m.group(1)) == 0.0, r.stdout
        assert re.search(r"^\[hip_merge_pattern\] total: +([0-9.]+) ms  kernel: +([0-9.]+) ms$", r.stdout, re.M), r.stdout
    r = subprocess.run([EXE, "--synthetic", "band:n=20000,k=32,w=600", "hip_merge_pattern", "hip_merge", "--iters", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(row, r.stdout, re.M)
    assert m and float(m.group(2)) > 1.0, r.stdout           # x = 1: every row sums to 32 instead of ~0
    m = re.search(r"^\[hip_merge   \] sum: +([0-9.eE+-]+|nan)  avg: +([0-9.eE+-]+|nan)$", r.stdout, re.M)
    assert m and float(m.group(2)) < 1e-4, r.stdout
