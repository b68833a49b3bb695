"""Multi-vector SpMV on the GPU (sp.MultiPlan / sp.spmm, csrc/multi.hip): every column of Y against the fp64 oracle
within the per-row parity bound (len + 2) eps sum|a x| — (len + 3) eps (|alpha| sum|a x| + |beta y0|) with alpha / beta,
as tests/test_gpu_parity.py::test_alpha_beta — and bit for bit against the serial oracle on integer-valued data.
Y is NaN-poisoned before every call; the padding columns of X hold NaN (a read that is used shows in the result) and
those of Y a canary that must survive."""
import numpy as np
import pytest
import torch

import multi_cases as mc
from conftest import parity_bound, random_csr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NP = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
CANARY = -777.25
K_MAX = 33
KS = (1, 3, 4, 8, 16, 17, 33)
N_ROWS, N_COLS = 3001, 700


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_ragged_cache = {}


def ragged(off, val, integer=False):
    """random_csr(rng, 3001, 700, 28, long_row=15000) with X of K_MAX columns and the oracle's answers, made once per
    type pair and left unchanged: (Ap, Aj, Ax, X, y64[j], bound[j], device copies)."""
    key = (off, val, integer)
    if key not in _ragged_cache:
        from oracle.oracle import Oracle
        orc = Oracle()
        rng = np.random.RandomState(1234)
        Ap, Aj, Ax = random_csr(rng, N_ROWS, N_COLS, 28, NP[off], NP[val], long_row=15000, integer_values=integer)
        if integer:
            X = rng.randint(-3, 4, size=(N_COLS, K_MAX)).astype(NP[val])
            ref = [orc.spmv_genl_serial(0, Ap, Aj, Ax, np.ascontiguousarray(X[:, j])) for j in range(K_MAX)]
            _ragged_cache[key] = (Ap, Aj, Ax, X, ref, None, (d(Ap), d(Aj), d(Ax)))
        else:
            X = (rng.rand(N_COLS, K_MAX) * 2 - 1).astype(NP[val])
            cols = [parity_bound(orc, Ap, Aj, Ax, np.ascontiguousarray(X[:, j])) for j in range(K_MAX)]
            _ragged_cache[key] = (Ap, Aj, Ax, X, [c[0] for c in cols], [c[1] for c in cols], (d(Ap), d(Aj), d(Ax)))
    return _ragged_cache[key]


def padded(A, ld, fill):
    """Device tensor of A's shape that is a view of rows of length ld, the padding columns filled with `fill`."""
    rows, k = A.shape
    buf = torch.full((max(rows, 1), ld), fill, dtype=torch.from_numpy(A[:0]).dtype, device=DEV)
    view = buf[:rows, :k]
    view.copy_(torch.from_numpy(np.ascontiguousarray(A)))
    return buf, view


def poisoned_y(rows, k, ldy, val):
    buf = torch.full((max(rows, 1), ldy), CANARY, dtype=torch.from_numpy(np.zeros(0, NP[val])).dtype, device=DEV)
    view = buf[:rows, :k]
    view.fill_(float("nan"))
    return buf, view


def check_columns(got, y64, bound, k):
    assert not np.any(np.isnan(got))
    for j in range(k):
        err = np.abs(got[:, j].astype(np.float64) - y64[j])
        assert np.all(err <= bound[j] + 1e-300), "column %d: max excess %g" % (j, (err - bound[j]).max())


def check_canary(ybuf, k):
    if ybuf.shape[1] > k:
        assert bool((ybuf[:, k:] == CANARY).all()), "a padding column of Y was written"


@pytest.fixture(scope="module")
def plans(sp):
    made = {}

    def get(off, val):
        if (off, val) not in made:
            Ap, Aj, Ax, X, _, _, (dAp, dAj, dAx) = ragged(off, val)
            made[(off, val)] = sp.MultiPlan(N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, dAx.dtype, K_MAX)
        return made[(off, val)]
    yield get
    for p in made.values():
        p.destroy()


@pytest.mark.parametrize("pad", [(0, 0), (3, 5)])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i32", "f64"), ("i64", "f32"), ("i64", "f64")])
def test_ragged(sp, plans, off, val, k, pad):
    Ap, Aj, Ax, X, y64, bound, (dAp, dAj, dAx) = ragged(off, val)
    p = plans(off, val)
    _, dX = padded(X[:, :k], k + pad[0], float("nan"))
    ybuf, dY = poisoned_y(N_ROWS, k, k + pad[1], val)
    assert dX.stride(0) == k + pad[0] and dY.stride(0) == k + pad[1]
    p.execute(dAx, dX, dY)
    torch.cuda.synchronize()
    check_columns(dY.cpu().numpy(), y64, bound, k)
    check_canary(ybuf, k)


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64")])
def test_integer_values_are_bit_exact(sp, off, val):
    Ap, Aj, Ax, X, ref, _, (dAp, dAj, dAx) = ragged(off, val, integer=True)
    p = sp.MultiPlan(N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, dAx.dtype, K_MAX)
    for k, pad in ((K_MAX, 0), (5, 2), (8, 0)):
        _, dX = padded(X[:, :k], k + pad, float("nan"))
        ybuf, dY = poisoned_y(N_ROWS, k, k + pad, val)
        p.execute(dAx, dX, dY)
        torch.cuda.synchronize()
        got = dY.cpu().numpy()
        for j in range(k):
            assert np.array_equal(got[:, j], ref[j]), j
        check_canary(ybuf, k)
    p.destroy()


def run_case(sp, oracle, Ap, Aj, Ax, n_cols, k, seed=5, alpha=1.0, beta=0.0, offset4=False):
    """One plan, one execute on a small matrix; all columns against the oracle."""
    n_rows = len(Ap) - 1
    nnz = int(Ap[-1])
    rng = np.random.RandomState(seed)
    X = (rng.rand(n_cols, k) * 2 - 1).astype(Ax.dtype)
    Y0 = (rng.rand(n_rows, k) * 2 - 1).astype(Ax.dtype) if beta != 0.0 else np.full((n_rows, k), np.nan, Ax.dtype)
    tdt = torch.from_numpy(Ax[:0]).dtype
    if offset4:         # every operand 4 bytes past a 16-byte boundary (fp32; one element)
        def off1(a):
            buf = torch.empty(a.size + 5, dtype=torch.from_numpy(a.ravel()[:0]).dtype, device=DEV)
            base = 1 + ((16 - buf.data_ptr() % 16) % 16) // buf.element_size()
            v = buf[base:base + a.size].view(a.shape)
            v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
            assert v.data_ptr() % 16 == 4
            return v
        dAj, dAx, dX, dY = off1(Aj), off1(Ax), off1(X), off1(Y0)
    else:
        dAj, dAx, dX, dY = d(Aj), d(Ax) if nnz else torch.empty(0, dtype=tdt, device=DEV), d(X), d(Y0)
    dAp = d(Ap)
    p = sp.MultiPlan(n_rows, n_cols, nnz, dAp, dAj, tdt, k)
    p.set_alpha_beta(alpha, beta)
    p.execute(dAx, dX, dY)
    torch.cuda.synchronize()
    info = p.info()
    p.destroy()
    got = dY.cpu().numpy().astype(np.float64)
    assert not np.any(np.isnan(got))
    eps = 2.0 ** -24 if Ax.dtype == np.float32 else 2.0 ** -53
    lens = np.diff(Ap.astype(np.int64))
    extra = 2 if (alpha, beta) == (1.0, 0.0) else 3
    Y0z = np.where(np.isnan(Y0), 0.0, Y0).astype(np.float64)
    for j in range(k):
        y64, yabs = oracle.spmv_ref64(Ap, Aj, Ax, np.ascontiguousarray(X[:, j]))
        want = alpha * y64 + beta * Y0z[:, j]
        bound = (lens + extra) * eps * (abs(alpha) * yabs + np.abs(beta * Y0z[:, j])) + 1e-300
        assert np.all(np.abs(got[:, j] - want) <= bound), j
    return info


def csr_from_lens(lens, n_cols, seed, val=np.float32):
    rng = np.random.RandomState(seed)
    Ap = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    return Ap, rng.randint(0, n_cols, size=nnz).astype(np.int32), (rng.rand(nnz) * 2 - 1).astype(val)


def test_no_rows(sp):
    Ap = torch.zeros(1, dtype=torch.int32, device=DEV)
    Aj = torch.zeros(0, dtype=torch.int32, device=DEV)
    p = sp.MultiPlan(0, 5, 0, Ap, Aj, torch.float32, 4)
    Y = torch.full((0, 4), float("nan"), device=DEV)
    p.execute(torch.zeros(0, device=DEV), torch.ones(5, 4, device=DEV), Y)
    torch.cuda.synchronize()
    assert p.info()["n_slices"] == 0
    p.destroy()


@pytest.mark.parametrize("beta", [0.0, 2.0])
def test_no_nonzeros_gives_beta_y(sp, oracle, beta):
    Ap, Aj, Ax = csr_from_lens([0] * 2500, 7, 1)
    run_case(sp, oracle, Ap, Aj, Ax, 7, 5, alpha=1.0, beta=beta)


def test_one_column(sp, oracle):
    rng = np.random.RandomState(2)
    Ap, Aj, Ax = random_csr(rng, 1500, 1, 9)
    run_case(sp, oracle, Ap, Aj, Ax, 1, 6)


@pytest.mark.parametrize("val", ["f32", "f64"])
def test_one_row_holds_every_nonzero(sp, oracle, val):
    for lens in ([5003], [0, 0, 5003, 0]):
        Ap, Aj, Ax = csr_from_lens(lens, 300, 3, NP[val])
        assert int(Ap[-1]) % 4 != 0
        run_case(sp, oracle, Ap, Aj, Ax, 300, 7)


@pytest.mark.parametrize("k", [4, 12, 32])
def test_empty_rows_first_last_and_at_every_slice_boundary(sp, oracle, k):
    Ap0 = torch.zeros(2, dtype=torch.int32, device=DEV)
    probe = sp.MultiPlan(1, 1, 0, Ap0, torch.zeros(0, dtype=torch.int32, device=DEV), torch.float32, k)
    L = probe.info()["slice_len"]
    probe.destroy()
    assert L >= 64
    # merge items = rows + nonzeros; rows are sized so that slice ends fall before, between and after runs of empty rows
    lens = [0, 0]
    for b in range(3):
        lens += [L - 3 - (2 if b == 0 else 0), 0, 0, 0]      # a row ends right at a slice end, empty rows straddle it
    lens += [L - 1, 0, 1, 0, L - 2, 0, 0, 2 * L + 1, 0, 17, 0, 0]
    Ap, Aj, Ax = csr_from_lens(lens, 211, 4)
    info = run_case(sp, oracle, Ap, Aj, Ax, 211, k, alpha=2.5, beta=0.0)
    assert info["n_slices"] == -(-(len(lens) + int(Ap[-1])) // L) >= 8
    run_case(sp, oracle, Ap, Aj, Ax, 211, k, alpha=-0.75, beta=3.0)


def test_operands_four_bytes_off_a_16_byte_boundary(sp, oracle):
    rng = np.random.RandomState(6)
    Ap, Aj, Ax = random_csr(rng, 2000, 300, 12, long_row=2100)
    run_case(sp, oracle, Ap, Aj, Ax, 300, 8, offset4=True)


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64")])
@pytest.mark.parametrize("alpha,beta", [(2.5, 0.0), (1.0, 1.0), (-0.75, 3.0), (0.0, 2.0)])
def test_alpha_beta(sp, oracle, off, val, alpha, beta):
    rng = np.random.RandomState(91)
    Ap, Aj, Ax = random_csr(rng, N_ROWS, N_COLS, 28, NP[off], NP[val], long_row=15000)
    run_case(sp, oracle, Ap, Aj, Ax, N_COLS, 6, alpha=alpha, beta=beta)


def test_wide_band_repeat_side_stream_and_graph(sp, oracle):
    k = 8
    m = sp.synth.banded_fixed(20000, 32, 700, seed=11, device=DEV)
    Ap, Aj, Ax = m.numpy()
    Xs = [(np.random.RandomState(s).rand(m.n_cols, k) * 2 - 1).astype(np.float32) for s in (1, 2)]

    def check(X, got):
        for j in range(k):
            y64, bound = parity_bound(oracle, Ap, Aj, Ax, np.ascontiguousarray(X[:, j]))
            assert np.all(np.abs(got[:, j].astype(np.float64) - y64) <= bound + 1e-300), j

    p = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, k)
    dX = d(Xs[0])
    Y = torch.full((m.n_rows, k), float("nan"), device=DEV)
    p.execute(m.Ax, dX, Y)
    torch.cuda.synchronize()
    first = Y.cpu().numpy()
    check(Xs[0], first)
    Y.fill_(float("nan"))
    p.execute(m.Ax, dX, Y)                      # two executes: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(first, Y.cpu().numpy())
    # a side stream
    s = torch.cuda.Stream()
    Y.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        p.execute(m.Ax, dX, Y)
    s.synchronize()
    assert np.array_equal(first, Y.cpu().numpy())
    # one capture, replayed on new X
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.execute(m.Ax, dX, Y)
    dX.copy_(torch.from_numpy(Xs[1]))
    Y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = Y.cpu().numpy()
    check(Xs[1], got)
    Y2 = torch.full((m.n_rows, k), float("nan"), device=DEV)
    p.execute(m.Ax, dX, Y2)
    torch.cuda.synchronize()
    assert np.array_equal(got, Y2.cpu().numpy())
    del g
    p.destroy()


def test_a_narrow_execute_after_a_full_one_sees_no_stale_carries(sp, plans):
    Ap, Aj, Ax, X, y64, bound, (dAp, dAj, dAx) = ragged("i32", "f32")
    p = plans("i32", "f32")
    _, dX = padded(X, K_MAX, float("nan"))
    _, dY = poisoned_y(N_ROWS, K_MAX, K_MAX, "f32")
    p.execute(dAx, dX, dY)
    k = 5
    X2 = np.ascontiguousarray(X[:, 7:7 + k])        # other vectors than the first execute's columns 0..4
    _, dX2 = padded(X2, k + 1, float("nan"))
    ybuf, dY2 = poisoned_y(N_ROWS, k, k + 2, "f32")
    p.execute(dAx, dX2, dY2)
    torch.cuda.synchronize()
    check_columns(dY2.cpu().numpy(), y64[7:7 + k], bound[7:7 + k], k)
    check_canary(ybuf, k)


def test_spmm_one_shot(sp):
    Ap, Aj, Ax, X, y64, bound, (dAp, dAj, dAx) = ragged("i64", "f32")
    k = 17
    _, dX = padded(X[:, :k], k, float("nan"))
    ybuf, dY = poisoned_y(N_ROWS, k, k + 1, "f32")
    out = sp.spmm(N_ROWS, N_COLS, int(Ap[-1]), dAp, dAj, dAx, dX, dY)
    assert out is dY
    check_columns(dY.cpu().numpy(), y64, bound, k)       # (the one-shot synchronises)
    check_canary(ybuf, k)


def test_info_and_device_side_refusals(sp, plans):
    Ap, Aj, Ax, X, _, _, (dAp, dAj, dAx) = ragged("i32", "f32")
    p = plans("i32", "f32")
    info = p.info()
    assert "multi_slice_kernel" in info["main_kernel"]
    assert info["scratch_bytes"] > 0 and info["slice_len"] > 0 and info["k_max"] == K_MAX
    assert info["n_slices"] == -(-(N_ROWS + int(Ap[-1])) // info["slice_len"])
    assert info["grid_blocks"] >= 1 and info["passes"] == 2 and info["n_kernels"] == 3
    with pytest.raises(RuntimeError, match="invalid argument"):          # k > k_max
        p.execute(dAx, torch.ones(N_COLS, K_MAX + 1, device=DEV), torch.zeros(N_ROWS, K_MAX + 1, device=DEV))
    import ctypes as C
    lib = sp.capi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    Xd, Yd = torch.ones(N_COLS, 4, device=DEV), torch.zeros(N_ROWS, 4, device=DEV)
    assert lib.mi355_spmv_multi_execute(p._h, None, ptr(Xd), 4, ptr(Yd), 4, 4, None) == 1      # null Ax with nonzeros
    assert lib.mi355_spmv_multi_execute(p._h, ptr(dAx), None, 4, ptr(Yd), 4, 4, None) == 1
    assert lib.mi355_spmv_multi_execute(p._h, ptr(dAx), ptr(Xd), 4, None, 4, 4, None) == 1
    assert lib.mi355_spmv_multi_execute(p._h, ptr(dAx), ptr(Xd), 3, ptr(Yd), 4, 4, None) == 1  # ldx < k


# ---- the table of tests/multi_cases.py: the cases that tests/test_multi_sim_cpu.py executes on the host, on the device ----
def on_device(flat, shift):
    """1-D device copy of `flat` whose base lies `shift` elements past a 16-byte boundary (an empty one has no base)."""
    t = torch.from_numpy(np.ascontiguousarray(flat))
    es = t.element_size()
    buf = torch.empty(t.numel() + 16 // es + 1, dtype=t.dtype, device=DEV)
    base = ((16 - buf.data_ptr() % 16) % 16) // es + shift
    v = buf[base:base + t.numel()]
    v.copy_(t)
    assert t.numel() == 0 or v.data_ptr() % 16 == shift * es
    return v


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_table(sp, oracle, family):
    """Every case of the family: plans are made per (structure, types, matrix offsets, k_max) and reused over k,
    alpha / beta, leading dimensions and the offsets of X and Y.  No case is skipped."""
    cases = mc.family(family)
    assert cases
    key, plan, dAx = None, None, None
    try:
        for c in cases:
            Ap, Aj, Ax, X, Y0 = mc.arrays(c.matrix, c.off, c.val, c.integer)
            n_rows, n_cols = len(c.matrix.lens), c.matrix.n_cols
            if mc.plan_key(c) != key:
                if plan is not None:
                    plan.destroy()
                    plan = None
                key = mc.plan_key(c)
                dAp, dAj, dAx = on_device(Ap, c.shift[0]), on_device(Aj, c.shift[1]), on_device(Ax, c.shift[2])
                plan = sp.MultiPlan(n_rows, n_cols, int(Ap[-1]), dAp, dAj, dAx.dtype, c.k_max)
                mc.assert_geometry(plan.info(), c.val)
            xh = np.full((n_cols, c.ldx), np.nan, dtype=X.dtype)
            xh[:, :c.k] = X[:, c.c0:c.c0 + c.k]
            yh = np.full((n_rows, c.ldy), mc.CANARY, dtype=X.dtype)
            yh[:, :c.k] = Y0[:, c.c0:c.c0 + c.k] if c.beta != 0.0 else np.nan
            xf, yf = on_device(xh.ravel(), c.shift[3]), on_device(yh.ravel(), c.shift[4])
            plan.set_alpha_beta(c.alpha, c.beta)
            plan.execute(dAx, torch.as_strided(xf, (n_cols, c.k), (c.ldx, 1)), torch.as_strided(yf, (n_rows, c.k), (c.ldy, 1)))
            mc.check(oracle, c, yf.cpu().numpy())       # (the copy synchronises)
    finally:
        if plan is not None:
            plan.destroy()
