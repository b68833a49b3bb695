"""GPU suite: permuted and transposed multi-vector SpMV (mi355_spmv_multi_create_permuted / _create_transposed;
sp.MultiPlan(perm=), sp.TransposedMultiPlan, sp.spmm_t).

The table of tests/multi_perm_cases.py runs through create_permuted against the bar of the host simulation: bit for bit the
plain MultiPlan on the same structure with Ax[perm] materialised.  TransposedMultiPlan is held to numpy exactly on integer
data, to the project's parity bound on real data, bit for bit to MultiPlan on its own .structure(), and to the adjoint
identity <A X, Z> = <X, A^T Z>.  The last test is the gap the feature closes: the whole backward of sparse attention
(sddmm -> row softmax -> spmm) with library calls only, against torch autograd on the dense masked formulation."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__
import multi_cases as mc
import multi_perm_cases as pc
from conftest import random_csr

pytestmark = pytest.mark.gpu
sp = __graft_entry__.load_package()
DEV = "cuda:0"
TV = {"f32": torch.float32, "f64": torch.float64}
NV = {"f32": np.float32, "f64": np.float64}
TO = {"i32": torch.int32, "i64": torch.int64}
CANARY = mc.CANARY


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def with_canary(a, extra=8):
    """A device copy of 1-D `a` with `extra` canaries behind it: (the view of a's length, the whole buffer)."""
    buf = torch.full((a.size + extra,), CANARY, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    buf[:a.size] = torch.from_numpy(np.ascontiguousarray(a))
    return buf[:a.size], buf


def canary_intact(buf, n):
    return bool((buf[n:] == CANARY).all())


# ---- layer 2: the table through create_permuted --------------------------------------------------------------------------
@pytest.mark.parametrize("perm", pc.PERMS)
def test_table_permuted_equals_plain_on_materialised_values_bit_for_bit(perm):
    cases = sorted((c for c in pc.table() if c.perm == perm), key=pc.plan_key)
    assert cases and max(sum(c.matrix.lens) for c in cases) < 10 ** 5
    key, plans = None, ()
    try:
        for c in cases:
            Ap, Aj, pm, nv, Ax, X, Y0 = pc.operands(c)
            n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, len(Aj)
            if pc.plan_key(c) != key:
                for p in plans:
                    p.destroy()
                key = pc.plan_key(c)
                dAp, dAj, dpm = d(Ap), d(Aj), d(pm)
                dAx, ax_buf = with_canary(Ax)
                dAxp = d(Ax[pm])
                plans = (sp.MultiPlan(n_rows, n_cols, nnz, dAp, dAj, TV[c.val], c.k_max, perm=dpm, n_values=nv),
                         sp.MultiPlan(n_rows, n_cols, nnz, dAp, dAj, TV[c.val], c.k_max))
                mc.assert_geometry(plans[0].info(), c.val)
                assert plans[0].info()["main_kernel"] == "multi_perm_slice_kernel"
                assert plans[0].perm_info() == {"n_values": nv, "held_bytes": 4 * nnz, "owns_structure": 0}
            xh = np.full((n_cols, c.ldx), np.nan, dtype=NV[c.val])
            xh[:, :c.k] = X
            dX, x_buf = with_canary(xh.ravel()[:(n_cols - 1) * c.ldx + c.k] if n_cols else xh.ravel())
            outs = []
            for p, values in zip(plans, (dAx, dAxp)):
                yh = np.full((n_rows, c.ldy), CANARY, dtype=NV[c.val])
                yh[:, :c.k] = Y0 if c.beta != 0.0 else np.nan       # poisoned first
                y_len = (n_rows - 1) * c.ldy + c.k if n_rows else 0
                dY, y_buf = with_canary(yh.ravel()[:y_len])
                p.set_alpha_beta(c.alpha, c.beta)
                p.execute(values, torch.as_strided(dX, (n_cols, c.k), (c.ldx, 1)), torch.as_strided(dY, (n_rows, c.k), (c.ldy, 1)))
                outs.append(dY.cpu().numpy())
                assert canary_intact(y_buf, y_len), c.name
            assert canary_intact(ax_buf, nv) and canary_intact(x_buf, dX.numel()), c.name
            pc.check(c, outs[0], outs[1])
    finally:
        for p in plans:
            p.destroy()


@pytest.mark.parametrize("poff", ["i32", "i64"])
def test_a_bad_index_is_refused_on_the_device_and_named(poff):
    c = next(c for c in pc.table() if c.matrix.name == "ragged" and c.perm == "random" and c.val == "f32" and c.k == 3)
    Ap, Aj, pm, nv, Ax, X, Y0 = pc.operands(c)
    for pos, value in ((17, nv), (4000, -1), (0, nv + 5)):
        bad = pm.astype({"i32": np.int32, "i64": np.int64}[poff])
        bad[pos] = value
        bad[pos + 100] = nv         # the first one is named
        with pytest.raises(RuntimeError, match=r"perm\[%d\] = %d is outside the %d values" % (pos, value, nv)):
            sp.MultiPlan(len(c.matrix.lens), c.matrix.n_cols, len(Aj), d(Ap), d(Aj), torch.float32, 4, perm=d(bad), n_values=nv)


def test_permuted_refusals():
    Ap, Aj, _ = random_csr(np.random.RandomState(1), 50, 40, 6)
    dAp, dAj, nnz = d(Ap), d(Aj), len(Aj)
    pm = d(np.arange(nnz, dtype=np.int32))
    p = sp.MultiPlan(50, 40, nnz, dAp, dAj, torch.float32, 8, perm=pm)
    with pytest.raises(RuntimeError, match="semiring only"):
        p.set_semiring("min_plus")
    X = torch.ones(40, 4, device=DEV)
    with pytest.raises(ValueError, match="shorter"):
        p.execute(torch.ones(nnz - 1, device=DEV), X, torch.zeros(50, 4, device=DEV))
    with pytest.raises(RuntimeError, match="invalid argument"):      # k > k_max
        p.execute(torch.ones(nnz, device=DEV), torch.ones(40, 9, device=DEV), torch.zeros(50, 9, device=DEV))
    p.destroy()
    for kw in (dict(val_dtype=torch.int32), dict(val_dtype=torch.float16), dict(val_dtype=torch.float32, mat_dtype="pattern"),
               dict(val_dtype=torch.float32, semiring="min_plus")):
        with pytest.raises(TypeError):
            sp.MultiPlan(50, 40, nnz, dAp, dAj, kw.pop("val_dtype"), 8, perm=pm, **kw)
    lib, h = sp.capi.lib(), C.c_void_p()
    args = (50, 40, nnz, C.c_void_p(dAp.data_ptr()), C.c_void_p(dAj.data_ptr()), 0, C.c_void_p(pm.data_ptr()), nnz, 8, None)
    for val_type in (2, 3, 4, 5):       # I32, PATTERN, F16, BF16
        assert lib.mi355_spmv_multi_create_permuted(C.byref(h), 0, val_type, *args) == 2 and not h.value


# ---- layer 3: the transposed plan ----------------------------------------------------------------------------------------
def graph(seed, n_rows, n_cols, off="i32", val="f32", integer=False, **kw):
    return random_csr(np.random.RandomState(seed), n_rows, n_cols, kw.pop("max_len", 30), {"i32": np.int32, "i64": np.int64}[off], NV[val],
                      integer_values=integer, **kw)


def dense_t(n_rows, n_cols, Ap, Aj, Ax, X):
    """(A^T X in fp64, |A|^T |X|, entries per column) by numpy."""
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))
    y, yabs = np.zeros((n_cols, X.shape[1])), np.zeros((n_cols, X.shape[1]))
    prod = Ax.astype(np.float64)[:, None] * X[rows].astype(np.float64)
    np.add.at(y, Aj, prod)
    np.add.at(yabs, Aj, np.abs(prod))
    return y, yabs, np.bincount(Aj, minlength=n_cols)


SHAPES_T = {"ragged_hub_row": dict(n_rows=900, n_cols=700, long_row=30000), "rect2x6": dict(n_rows=2, n_cols=6, max_len=6, empty_frac=0.0),
            "rect6x2": dict(n_rows=6, n_cols=2, max_len=2), "one_column": dict(n_rows=300, n_cols=1, max_len=1),
            "wide_empty_columns": dict(n_rows=40, n_cols=5000, max_len=9), "hub_columns": dict(n_rows=30000, n_cols=3, max_len=2)}


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i64", "f64"), ("i64", "f32"), ("i32", "f64")])
@pytest.mark.parametrize("shape", list(SHAPES_T))
def test_transposed_plan_exact_bounded_and_equal_to_a_plain_plan_on_its_structure(shape, off, val):
    kw = dict(SHAPES_T[shape])
    n_rows, n_cols = kw.pop("n_rows"), kw.pop("n_cols")
    k, k_max = (33, 40) if val == "f32" else (17, 20)
    rng = np.random.RandomState(3)
    for integer in (True, False):
        Ap, Aj, Ax = graph(11, n_rows, n_cols, off, val, integer, **dict(kw))
        nnz = len(Aj)
        X = (rng.randint(-3, 4, size=(n_rows, k)) if integer else rng.rand(n_rows, k) * 2 - 1).astype(NV[val])
        dAp, dAj, dAx, dX = d(Ap), d(Aj), d(Ax), d(X)
        plan = sp.TransposedMultiPlan(n_rows, n_cols, nnz, dAp, dAj, TV[val], k_max)
        info, pinfo = plan.info(), plan.perm_info()
        assert info["main_kernel"] == "multi_perm_slice_kernel" and info["off_type"] == ("i32", "i64").index(off)
        assert pinfo == {"n_values": nnz, "held_bytes": (n_cols + 1) * (4 if off == "i32" else 8) + 8 * nnz, "owns_structure": 1}
        Y = torch.full((n_cols, k), float("nan"), dtype=TV[val], device=DEV)
        assert plan.execute(dAx, dX, Y) is Y
        got = Y.cpu().numpy()
        y64, yabs, count = dense_t(n_rows, n_cols, Ap, Aj, Ax, X)
        if integer:
            assert np.array_equal(mc.bits(got), mc.bits(y64.astype(NV[val])))
        else:   # the project's bound, (len + 2) eps sum |a x| (conftest.parity_bound), len = the column's count
            eps = 2.0 ** -24 if val == "f32" else 2.0 ** -53
            assert np.all(np.abs(got.astype(np.float64) - y64) <= ((count + 2) * eps)[:, None] * yabs + 1e-300)
        assert np.all(got[count == 0] == 0)     # an empty column: beta * Y with beta = 0, over the NaN
        # the plan's own structure is layer 1's, and a plain plan on it with Ax[perm] gives the same bits
        Apt, Ajt, perm = plan.structure()
        for a, b in zip((Apt, Ajt, perm), sp.csr_transpose(n_rows, n_cols, dAp, dAj)):
            assert a.dtype == b.dtype and torch.equal(a, b)
        plain = sp.MultiPlan(n_cols, n_rows, nnz, Apt, Ajt, TV[val], k_max)
        Y2 = torch.full((n_cols, k), float("nan"), dtype=TV[val], device=DEV)
        plain.execute(dAx[perm.long()], dX, Y2)
        assert np.array_equal(got.view(np.uint8), Y2.cpu().numpy().view(np.uint8))
        plain.destroy()
        plan.destroy()


def test_transposed_no_rows_no_columns_no_nonzeros():
    e = torch.empty(0, dtype=torch.int32, device=DEV)
    for n_rows, n_cols in ((0, 5), (5, 0), (4, 3)):
        Ap = torch.zeros(n_rows + 1, dtype=torch.int32, device=DEV)
        plan = sp.TransposedMultiPlan(n_rows, n_cols, 0, Ap, e, torch.float32, 4)
        X = torch.ones(n_rows, 3, device=DEV)
        Y = torch.full((n_cols, 3), 2.0, device=DEV)
        plan.set_alpha_beta(1.0, 3.0)
        plan.execute(torch.empty(0, device=DEV), X, Y)
        assert bool((Y == 6.0).all())           # every column is empty: beta * Y
        assert tuple(t.numel() for t in plan.structure()) == (n_cols + 1, 0, 0)
        plan.destroy()


@pytest.mark.parametrize("off,val", [("i32", "f64"), ("i64", "f32")])
def test_adjoint_identity_on_small_integers(off, val):
    """<A X, Z> = <X, A^T Z>, exact, with A X by the existing MultiPlan."""
    n_rows, n_cols, k = 700, 450, 9
    Ap, Aj, Ax = graph(21, n_rows, n_cols, off, val, True, long_row=4000)
    rng = np.random.RandomState(4)
    X, Z = (rng.randint(-3, 4, size=s).astype(NV[val]) for s in ((n_cols, k), (n_rows, k)))
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    AX = torch.empty(n_rows, k, dtype=TV[val], device=DEV)
    fwd = sp.MultiPlan(n_rows, n_cols, len(Aj), dAp, dAj, TV[val], k)
    fwd.execute(dAx, d(X), AX)
    AtZ = torch.empty(n_cols, k, dtype=TV[val], device=DEV)
    bwd = sp.TransposedMultiPlan(n_rows, n_cols, len(Aj), dAp, dAj, TV[val], k)
    bwd.execute(dAx, d(Z), AtZ)
    lhs = (AX.cpu().numpy().astype(np.float64) * Z).sum(0)
    rhs = (X.astype(np.float64) * AtZ.cpu().numpy()).sum(0)
    assert np.array_equal(lhs, rhs) and np.abs(lhs).max() > 0
    fwd.destroy()
    bwd.destroy()


def test_beta_padding_unaligned_repeat_stream_graph_and_new_values():
    n_rows, n_cols, k = 3000, 2500, 12
    Ap, Aj, Ax = graph(31, n_rows, n_cols, "i32", "f32", True, long_row=9000)
    nnz = len(Aj)
    rng = np.random.RandomState(6)
    X, Y0 = (rng.randint(-3, 4, size=s).astype(np.float32) for s in ((n_rows, k), (n_cols, k)))
    want = lambda ax, x, alpha=1.0, beta=0.0: (alpha * dense_t(n_rows, n_cols, Ap, Aj, ax, x)[0] + beta * Y0).astype(np.float32)
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    plan = sp.TransposedMultiPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, 16)
    # beta != 0, padded leading dimensions, and views one element off a 16-byte boundary
    ldx, ldy = k + 3, k + 5
    xbuf = torch.full((n_rows * ldx + 1,), float("nan"), device=DEV)
    ybuf = torch.full((n_cols * ldy + 1,), CANARY, device=DEV)
    Xv, Yv = torch.as_strided(xbuf, (n_rows, k), (ldx, 1), 1), torch.as_strided(ybuf, (n_cols, k), (ldy, 1), 1)
    assert Xv.data_ptr() % 16 == 4 and Yv.data_ptr() % 16 == 4
    Xv.copy_(d(X)); Yv.copy_(d(Y0))
    plan.set_alpha_beta(-2.0, 3.0)
    plan.execute(dAx, Xv, Yv)
    assert np.array_equal(Yv.cpu().numpy(), want(Ax, X, -2.0, 3.0))
    pad = torch.as_strided(ybuf, (n_cols, ldy - k), (ldy, 1), 1 + k)
    assert bool((pad == CANARY).all()) and float(ybuf[0]) == CANARY
    plan.set_alpha_beta(1.0, 0.0)
    # repeat: the same bits; a side stream; new values in the SAME array and in another one are seen (nothing is cached)
    dX = d(X)
    Y = torch.full((n_cols, k), float("nan"), device=DEV)
    plan.execute(dAx, dX, Y)
    first = Y.cpu().numpy()
    assert np.array_equal(first, want(Ax, X))
    Y.fill_(float("nan"))
    plan.execute(dAx, dX, Y)
    assert np.array_equal(first, Y.cpu().numpy())
    s = torch.cuda.Stream()
    Y.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        plan.execute(dAx, dX, Y)
    s.synchronize()
    assert np.array_equal(first, Y.cpu().numpy())
    Ax2 = rng.randint(-3, 4, size=nnz).astype(np.float32)
    dAx.copy_(d(Ax2))
    plan.execute(dAx, dX, Y)
    assert np.array_equal(Y.cpu().numpy(), want(Ax2, X))
    Ax3 = np.roll(Ax2, 7)
    plan.execute(d(Ax3), dX, Y)
    assert np.array_equal(Y.cpu().numpy(), want(Ax3, X))
    # one capture of execute, replayed on new X and new values
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute(dAx, dX, Y)
    X2 = rng.randint(-3, 4, size=(n_rows, k)).astype(np.float32)
    dX.copy_(d(X2))
    dAx.copy_(d(Ax))
    Y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(Y.cpu().numpy(), want(Ax, X2))
    del g
    # k_max, shapes and aliasing are refused
    with pytest.raises(RuntimeError, match="invalid argument"):
        plan.execute(dAx, torch.ones(n_rows, 17, device=DEV), torch.zeros(n_cols, 17, device=DEV))
    with pytest.raises(ValueError):
        plan.execute(dAx, torch.ones(n_rows - 1, k, device=DEV), Y)
    with pytest.raises(ValueError):
        plan.execute(dAx, dX, torch.zeros(n_cols, k + 1, device=DEV))
    with pytest.raises(TypeError):
        plan.execute(dAx.double(), dX, Y)
    both = torch.zeros(max(n_rows, n_cols), k, device=DEV)
    with pytest.raises(ValueError, match="aliases"):
        plan.execute(dAx, both[:n_rows], both[:n_cols])
    with pytest.raises(RuntimeError, match="semiring only"):
        plan.set_semiring("min_plus")
    plan.destroy()
    with pytest.raises(RuntimeError, match="invalid argument"):
        sp.TransposedMultiPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, 0)


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i32", "f64"), ("i64", "f32"), ("i64", "f64")])
def test_the_four_one_shots(off, val):
    n_rows, n_cols, k = 800, 1100, 5
    Ap, Aj, Ax = graph(41, n_rows, n_cols, off, val, True, long_row=2500)
    X = np.random.RandomState(8).randint(-3, 4, size=(n_rows, k)).astype(NV[val])
    Y = torch.full((n_cols, k), float("nan"), dtype=TV[val], device=DEV)
    assert sp.spmm_t(n_rows, n_cols, len(Aj), d(Ap), d(Aj), d(Ax), d(X), Y) is Y
    assert np.array_equal(mc.bits(Y.cpu().numpy()), mc.bits(dense_t(n_rows, n_cols, Ap, Aj, Ax, X)[0].astype(NV[val])))
    with pytest.raises(ValueError):
        sp.spmm_t(n_rows, n_cols, len(Aj), d(Ap), d(Aj), d(Ax), d(X), Y[:, :4])


# ---- the gap this closes ----------------------------------------------------------------------------------------------------
def test_sparse_attention_backward_never_leaves_the_library():
    """Forward S = sddmm(Q, K) on the graph, P = row softmax(scale * S), O = spmm(P, V); backward with library calls only:
         dP = sddmm(dO, V)                        the gradient of spmm with respect to Ax
         dV = P^T dO                              TransposedMultiPlan: the gradient of spmm with respect to X
         dS = RowSoftmaxPlan.backward(P, dP)
         dQ = spmm(dS, K)                         the gradient of sddmm with respect to U
         dK = dS^T Q                              TransposedMultiPlan: the gradient of sddmm with respect to V
    against torch autograd on the dense masked formulation, within 1e-10 * max |ref| per tensor: a structural error is of
    order 1, fp64 rounding over these row lengths below 1e-13."""
    n_q, n_k, k = 300, 200, 8
    rng = np.random.RandomState(12)
    mask = rng.rand(n_q, n_k) < 4000.0 / (n_q * n_k)
    mask[7] = False                             # a query without edges
    mask[:, 11] = False                         # a key without edges
    rows, cols = np.nonzero(mask)
    nnz = len(rows)
    assert 3500 < nnz < 4500
    Ap = np.concatenate(([0], np.cumsum(mask.sum(1)))).astype(np.int32)
    dAp, dAj = d(Ap), d(cols.astype(np.int32))
    Q, K, V, dO = (torch.from_numpy(rng.randn(n, k)).to(DEV) for n in (n_q, n_k, n_k, n_q))
    scale = 1.0 / np.sqrt(k)
    f64 = torch.float64
    sddmm = sp.SddmmPlan(n_q, n_k, nnz, dAp, dAj, f64)
    soft = sp.RowSoftmaxPlan(n_q, n_k, nnz, dAp, dAj, f64)
    soft.set_scale(scale)
    spmm = sp.MultiPlan(n_q, n_k, nnz, dAp, dAj, f64, k)
    spmm_t = sp.TransposedMultiPlan(n_q, n_k, nnz, dAp, dAj, f64, k)
    # forward
    S = sddmm.execute(None, Q, K)
    P = soft.execute(S)
    O = spmm.execute(P, V, torch.empty(n_q, k, dtype=f64, device=DEV))
    # backward
    dP = sddmm.execute(None, dO, V)
    dV = spmm_t.execute(P, dO, torch.empty(n_k, k, dtype=f64, device=DEV))
    dS = soft.backward(P, dP)
    dQ = spmm.execute(dS, K, torch.empty(n_q, k, dtype=f64, device=DEV))
    dK = spmm_t.execute(dS, Q, torch.empty(n_k, k, dtype=f64, device=DEV))
    torch.cuda.synchronize()
    # the dense masked formulation under autograd
    q, kk, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    m = torch.from_numpy(mask).to(DEV)
    scores = torch.where(m, (q @ kk.t()) * scale, torch.full((), float("-inf"), dtype=f64, device=DEV))
    scores = torch.where(m.any(1, keepdim=True), scores, torch.zeros((), dtype=f64, device=DEV))   # a query without edges: no NaN
    p = torch.where(m, torch.softmax(scores, 1), torch.zeros((), dtype=f64, device=DEV))
    o = p @ v
    o.backward(dO)
    for name, got, ref in (("O", O, o.detach()), ("dQ", dQ, q.grad), ("dK", dK, kk.grad), ("dV", dV, v.grad)):
        err, top = float((got - ref).abs().max()), float(ref.abs().max())
        print("%s: max |got - ref| = %.3e, max |ref| = %.3e" % (name, err, top))
        assert top > 0.1 and err <= 1e-10 * top, name
    for p_ in (sddmm, soft, spmm, spmm_t):
        p_.destroy()
