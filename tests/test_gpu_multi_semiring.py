"""Multi-vector SpMV over semirings, int32 values and pattern matrices on the GPU (sp.MultiPlan(..., mat_dtype=,
semiring=), sp.spmm(semiring=), sp.spmm_pattern; csrc/multi_kernels.hpp): the table of tests/multi_semiring_cases.py
that tests/test_multi_semiring_sim_cpu.py executes on the host, the ragged matrix of tests/test_gpu_multi.py under
every semiring, type and k against the serial oracle and against the merge kind, pattern against valued plans, the
life cycle, the one-shots, and a multi-source BFS.  Y is poisoned before every call; the padding columns of X hold NaN
and those of Y a canary that must survive."""
import numpy as np
import pytest
import torch

import multi_cases as mc
import multi_semiring_cases as sc
import sim_runner as sr
from conftest import random_csr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NP = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32}
N_ROWS, N_COLS, K_MAX = 3001, 700, 33
KS = (1, 3, 8, 17, 33)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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


def bits(a):
    return sc.bits(np.ascontiguousarray(a))


# ---- the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["row_ends", "open_row", "slice_edges", "ragged"])
def test_table(sp, oracle, family):
    """Every case on the structures of the family, the sequences on one object among them: objects are made per
    (structure, types, valued / pattern, data, matrix offsets, k_max) and reused over k, semiring, alpha / beta,
    leading dimensions and the offsets of X and Y.  No case is skipped."""
    groups = [g for g in sr.consecutive_runs(sc.table(), sc.plan_key) if g[0].matrix.family == family]
    assert groups
    for g in groups:
        c = g[0]
        Ap, Aj, Ax, _, _ = sc.operands(c)
        n_rows, n_cols = len(c.matrix.lens), c.matrix.n_cols
        dAp, dAj = on_device(Ap, c.shift[0]), on_device(Aj, c.shift[1])
        dAx = None if c.pattern else on_device(Ax, c.shift[2])
        plan = sp.MultiPlan(n_rows, n_cols, int(Ap[-1]), dAp, dAj, TORCH[c.val], c.k_max,
                            mat_dtype="pattern" if c.pattern else TORCH[c.val])
        try:
            info = plan.info()
            assert info["slice_len"] == mc.SLICE_LEN and info["widest_tile"] == sc.TILE[c.val]
            assert plan.types() == {"mat_type": sc.VAL_PATTERN if c.pattern else sc.VAL_TYPE[c.val],
                                    "vec_type": sc.VAL_TYPE[c.val], "semiring": 0}
            for c in g:
                X, Y0 = sc.operands(c)[3:]
                xh = np.full((n_cols, c.ldx), sc.x_pad(c), dtype=X.dtype)
                xh[:, :c.k] = X[:, c.c0:c.c0 + c.k]
                yh = np.full((n_rows, c.ldy), NP[c.val](sc.CANARY), dtype=X.dtype)
                yh[:, :c.k] = Y0[:, c.c0:c.c0 + c.k] if c.beta != 0.0 else sc.y_poison(c)
                xf, yf = on_device(xh.ravel(), c.shift[3]), on_device(yh.ravel(), c.shift[4])
                plan.set_alpha_beta(1.0, 0.0)
                plan.set_semiring(c.semiring)
                plan.set_alpha_beta(c.alpha, c.beta)
                plan.execute(dAx, torch.as_strided(xf, (n_cols, c.k), (c.ldx, 1)), torch.as_strided(yf, (n_rows, c.k), (c.ldy, 1)))
                sc.check(oracle, c, yf.cpu().numpy())       # (the copy synchronises)
        finally:
            plan.destroy()


# ---- the ragged matrix of tests/test_gpu_multi.py ------------------------------------------------------------------------
_ragged = {}


def ragged(val):
    """random_csr(rng, 3001, 700, 28, long_row=15000): the long row spans about 15 slices.  Real-valued for the float
    types, small integers for int32; X of K_MAX columns, with +inf / -inf in a tenth of it for (min, +) / (max, +)."""
    if val not in _ragged:
        rng = np.random.RandomState(1234)
        Ap, Aj, Ax = random_csr(rng, N_ROWS, N_COLS, 28, np.int32, NP[val], long_row=15000, integer_values=val == "i32")
        if val == "i32":
            X = rng.randint(-3, 4, size=(N_COLS, K_MAX)).astype(np.int32)
            Xs = {s: X for s in sc.SEMIRINGS}
        else:
            X = (rng.rand(N_COLS, K_MAX) * 2 - 1).astype(NP[val])
            mask = rng.rand(N_COLS, K_MAX) < 0.1
            Xs = {s: X for s in sc.SEMIRINGS}
            Xs["min_plus"] = np.where(mask, NP[val](np.inf), X)
            Xs["max_plus"] = np.where(mask, NP[val](-np.inf), X)
        _ragged[val] = (Ap, Aj, Ax, Xs, (d(Ap), d(Aj), d(Ax)))
    return _ragged[val]


@pytest.mark.parametrize("pattern", [False, True], ids=["valued", "pattern"])
@pytest.mark.parametrize("val", sc.VALS)
def test_ragged_against_the_oracle_and_the_merge_kind(sp, oracle, val, pattern):
    Ap, Aj, Ax, Xs, (dAp, dAj, dAx) = ragged(val)
    nnz = int(Ap[-1])
    ones = np.ones_like(Ax)
    mat = "pattern" if pattern else TORCH[val]
    multi = sp.MultiPlan(N_ROWS, N_COLS, nnz, dAp, dAj, TORCH[val], K_MAX, mat_dtype=mat)
    merge = sp.Plan("merge", N_ROWS, N_COLS, nnz, dAp, dAj, TORCH[val], mat_dtype=mat)
    poison = lambda s: float("nan") if val != "i32" else sc.Y_POISON_I32[s]
    eps = 2.0 ** -24 if val == "f32" else 2.0 ** -53
    lens = np.diff(Ap.astype(np.int64))
    try:
        for s in sc.SEMIRINGS:
            X = Xs[s]
            cols = [np.ascontiguousarray(X[:, j]) for j in range(K_MAX)]
            exact = s != "plus_times" or val == "i32"
            if exact:
                ref = [oracle.spmv_genl_serial(sc.SEMIRINGS.index(s), Ap, Aj, ones if pattern else Ax, x) for x in cols]
            else:
                ref = [oracle.spmv_ref64(Ap, Aj, ones if pattern else Ax, x) for x in cols]
            multi.set_semiring(s)
            merge.set_semiring(s)
            for k in KS:
                pad = k % 3
                xbuf = torch.full((N_COLS, k + pad), sc.X_PAD_I32 if val == "i32" else float("nan"), dtype=TORCH[val], device=DEV)
                dX = xbuf[:, :k]
                dX.copy_(torch.from_numpy(np.ascontiguousarray(X[:, :k])))
                ybuf = torch.full((N_ROWS, k + pad), NP[val](sc.CANARY).item(), dtype=TORCH[val], device=DEV)
                dY = ybuf[:, :k]
                dY.fill_(poison(s))
                multi.execute(None if pattern else dAx, dX, dY)
                torch.cuda.synchronize()
                got = dY.cpu().numpy()
                if pad:
                    assert bool((ybuf[:, k:] == NP[val](sc.CANARY).item()).all()), "a padding column of Y was written"
                for j in range(k):
                    if exact:
                        assert np.array_equal(bits(got[:, j]), bits(ref[j])), (s, k, j)
                    else:
                        y64, yabs = ref[j]
                        assert np.all(np.abs(got[:, j].astype(np.float64) - y64) <= (lens + 2) * eps * yabs + 1e-300), (s, k, j)
                if k == K_MAX and exact:        # column j of the multi result is the merge plan's result on X[:, j], bit for bit
                    y = torch.empty(N_ROWS, dtype=TORCH[val], device=DEV)
                    for j in range(k):
                        y.fill_(poison(s))
                        merge.execute(None if pattern else dAx, d(cols[j]), y)
                        torch.cuda.synchronize()
                        assert np.array_equal(np.ascontiguousarray(got[:, j]).view(np.uint8), y.cpu().numpy().view(np.uint8)), (s, j)
    finally:
        multi.destroy()
        merge.destroy()


@pytest.mark.parametrize("val,k", [("f32", 17), ("f64", 9), ("f32", 33)])
def test_a_pattern_plan_equals_the_valued_plan_with_ones(sp, val, k):
    Ap, Aj, Ax, Xs, (dAp, dAj, dAx) = ragged(val)
    nnz = int(Ap[-1])
    dOnes = torch.ones(nnz, dtype=TORCH[val], device=DEV)
    valued = sp.MultiPlan(N_ROWS, N_COLS, nnz, dAp, dAj, TORCH[val], k, semiring="min_plus")
    pattern = sp.MultiPlan(N_ROWS, N_COLS, nnz, dAp, dAj, TORCH[val], k, mat_dtype="pattern")
    assert valued.types()["semiring"] == 1 and pattern.types()["mat_type"] == sc.VAL_PATTERN
    for s in sc.SEMIRINGS:
        dX = d(Xs[s][:, :k])
        valued.set_semiring(s)
        pattern.set_semiring(s)
        Y1 = torch.full((N_ROWS, k), float("nan"), dtype=TORCH[val], device=DEV)
        Y2 = torch.full((N_ROWS, k), float("nan"), dtype=TORCH[val], device=DEV)
        valued.execute(dOnes, dX, Y1)
        pattern.execute(None, dX, Y2)
        torch.cuda.synchronize()
        a, b = Y1.cpu().numpy(), Y2.cpu().numpy()
        assert not np.any(np.isnan(a))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), s
    valued.destroy()
    pattern.destroy()


# ---- life cycle ----------------------------------------------------------------------------------------------------------
def test_repeat_side_stream_graph_and_a_change_of_semiring(sp, oracle):
    k = 8
    Ap, Aj, Ax, Xs, (dAp, dAj, dAx) = ragged("f32")
    nnz = int(Ap[-1])
    want = {s: [oracle.spmv_genl_serial(sc.SEMIRINGS.index(s), Ap, Aj, Ax, np.ascontiguousarray(Xs[s][:, j])) for j in range(k)]
            for s in ("min_plus", "max_times")}

    def check(s, got):
        for j in range(k):
            assert np.array_equal(bits(got[:, j]), bits(want[s][j])), (s, j)

    p = sp.MultiPlan(N_ROWS, N_COLS, nnz, dAp, dAj, torch.float32, k, semiring="min_plus")
    dX = d(Xs["min_plus"][:, :k])
    Y = torch.full((N_ROWS, k), float("nan"), device=DEV)
    p.execute(dAx, dX, Y)
    torch.cuda.synchronize()
    first = Y.cpu().numpy()
    check("min_plus", first)
    Y.fill_(float("nan"))
    p.execute(dAx, dX, Y)                      # two executes: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(first.view(np.uint8), Y.cpu().numpy().view(np.uint8))
    s = torch.cuda.Stream()                     # a side stream
    Y.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        p.execute(dAx, dX, Y)
    s.synchronize()
    assert np.array_equal(first.view(np.uint8), Y.cpu().numpy().view(np.uint8))
    g = torch.cuda.CUDAGraph()                  # one capture, replayed
    with torch.cuda.graph(g):
        p.execute(dAx, dX, Y)
    Y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(first.view(np.uint8), Y.cpu().numpy().view(np.uint8))
    del g
    p.set_semiring("max_times")                 # the same object under another semiring, and back
    dX2 = d(Xs["max_times"][:, :k])
    Y.fill_(float("nan"))
    p.execute(dAx, dX2, Y)
    torch.cuda.synchronize()
    check("max_times", Y.cpu().numpy())
    p.set_semiring("min_plus")
    Y.fill_(float("nan"))
    p.execute(dAx, dX, Y)
    torch.cuda.synchronize()
    assert np.array_equal(first.view(np.uint8), Y.cpu().numpy().view(np.uint8))
    with pytest.raises(RuntimeError, match="not supported"):
        p.set_alpha_beta(2.0, 0.0)
    # a valued object with nonzeros refuses a NULL Ax at the C entry point (Python would refuse it first)
    import ctypes as C
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert sp.capi.lib().mi355_spmv_multi_execute(p._h, None, ptr(dX), k, ptr(Y), k, k, None) == 1
    assert b"null Ax or X" in sp.capi.lib().mi355_spmv_last_error()
    with pytest.raises(TypeError, match="only a pattern plan"):
        p.execute(None, dX, Y)
    p.destroy()


def test_one_shots(sp, oracle):
    Ap, Aj, Ax, Xs, (dAp, dAj, dAx) = ragged("f32")
    nnz, k = int(Ap[-1]), 5
    X = Xs["min_plus"]
    ybuf = torch.full((N_ROWS, k + 1), sc.CANARY, device=DEV)
    dY = ybuf[:, :k]
    dY.fill_(float("nan"))
    out = sp.spmm(N_ROWS, N_COLS, nnz, dAp, dAj, dAx, d(X[:, :k]), dY, semiring="min_plus")      # (the one-shot synchronises)
    assert out is dY
    got = dY.cpu().numpy()
    for j in range(k):
        assert np.array_equal(bits(got[:, j]), bits(oracle.spmv_genl_serial(1, Ap, Aj, Ax, np.ascontiguousarray(X[:, j])))), j
    assert bool((ybuf[:, k:] == sc.CANARY).all())
    # (or, and) on a pattern matrix, int32 vectors and 64-bit offsets
    Api, Aji, Axi, Xsi, _ = ragged("i32")
    Xi = Xsi["or_and"]
    Yi = torch.full((N_ROWS, k), 7, dtype=torch.int32, device=DEV)
    out = sp.spmm_pattern("or_and", N_ROWS, N_COLS, int(Api[-1]), d(Api.astype(np.int64)), d(Aji), d(Xi[:, :k]), Yi)
    assert out is Yi
    goti = Yi.cpu().numpy()
    ones = np.ones_like(Axi)
    for j in range(k):
        assert np.array_equal(goti[:, j], oracle.spmv_genl_serial(4, Api, Aji, ones, np.ascontiguousarray(Xi[:, j]))), j
    # int32 (+, *) through spmm
    Yi.fill_(7)
    sp.spmm(N_ROWS, N_COLS, int(Api[-1]), d(Api), d(Aji), d(Axi), d(Xi[:, :k]), Yi)
    goti = Yi.cpu().numpy()
    for j in range(k):
        assert np.array_equal(goti[:, j], oracle.spmv_genl_serial(0, Api, Aji, Axi, np.ascontiguousarray(Xi[:, j]))), j


# ---- a use of it: multi-source BFS -----------------------------------------------------------------------------------------
def test_multi_source_bfs_and_hop_counts(sp):
    """Row r of A lists the vertices r steps to: a vertex joins the frontier when one of them is visited.  Levels from
    successive (or, and) frontiers on the device equal a plain numpy BFS per source, and (min, +) on the same pattern
    matrix, started from 0 at the source and +inf elsewhere, converges to the same hop counts."""
    m = sp.synth.rmat(12, device=DEV)
    n, k = m.n_rows, 8
    assert n == m.n_cols == 1 << 12
    Ap, Aj, _ = m.numpy()
    sources = np.random.RandomState(3).choice(n, size=k, replace=False)
    rows = np.repeat(np.arange(n), np.diff(Ap))
    want = np.full((n, k), -1, dtype=np.int64)
    for j, src in enumerate(sources):
        level = np.full(n, -1, dtype=np.int64)
        level[src] = 0
        t = 0
        while True:
            hit = np.bincount(rows, weights=(level[Aj] >= 0).astype(np.float64), minlength=n) > 0
            new = hit & (level < 0)
            if not new.any():
                break
            t += 1
            level[new] = t
        want[:, j] = level
    assert want.max() >= 2 and (want < 0).any() and (want > 0).any()

    plan = sp.MultiPlan(n, n, m.nnz, m.Ap, m.Aj, torch.float32, k, mat_dtype="pattern", semiring="or_and")
    V = torch.zeros((n, k), device=DEV)
    V[torch.from_numpy(sources).to(DEV), torch.arange(k, device=DEV)] = 1.0
    level = torch.where(V > 0, 0, -1).to(torch.int64)
    Y = torch.empty_like(V)
    for t in range(1, n + 1):
        Y.fill_(float("nan"))
        plan.execute(None, V, Y)
        new = (Y > 0) & (V == 0)
        if not bool(new.any()):
            break
        level[new] = t
        V = torch.maximum(V, Y)
    assert np.array_equal(level.cpu().numpy(), want)

    plan.set_semiring("min_plus")
    D = torch.full((n, k), float("inf"), device=DEV)
    D[torch.from_numpy(sources).to(DEV), torch.arange(k, device=DEV)] = 0.0
    for t in range(n):
        Y.fill_(float("nan"))
        plan.execute(None, D, Y)
        nxt = torch.minimum(D, Y)
        if bool((nxt == D).all()):
            break
        D = nxt
    hops = D.cpu().numpy()
    assert np.array_equal(np.isinf(hops), want < 0)
    assert np.array_equal(hops[want >= 0], want[want >= 0].astype(np.float32))
    plan.destroy()
