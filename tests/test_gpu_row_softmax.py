"""Row softmax on the GPU (sp.RowSoftmaxPlan / sp.row_softmax, csrc/row_softmax.hip): the table of
tests/row_softmax_cases.py — the cases that tests/test_row_softmax_sim_cpu.py executes on the host — on the device, each
result against numpy's fp64 value as that module says (exact families bit for bit, real data within its stated bounds);
out starts as NaN, and one canary element before and one behind out must survive.  Then what only a device shows: two
executes give the same bits, a side stream, one graph capture replayed on new values, the one-shots, in place, the chain
sddmm -> row_softmax -> spmm, and the adjoint identity of the backward."""
import ctypes as C

import numpy as np
import pytest
import torch

import row_softmax_cases as rc
import sddmm_cases as sc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH = {"f32": torch.float32, "f64": torch.float64}


def on_device(flat, shift, guard=0, fill=0.0):
    """1-D device copy of `flat` whose base lies `shift` elements past a 16-byte boundary, with `guard` elements of `fill`
    before and behind it: (the view of flat.size elements, the view with its guards)."""
    t = torch.from_numpy(np.ascontiguousarray(flat))
    es = t.element_size()
    buf = torch.full((t.numel() + 2 * guard + 32 // es + 1,), fill, dtype=t.dtype, device=DEV)
    base = ((16 - buf.data_ptr() % 16) % 16) // es + 16 // es + shift
    v = buf[base:base + t.numel()]
    v.copy_(t)
    assert v.numel() == 0 or v.data_ptr() % 16 == shift * es
    return v, buf[base - guard:base + t.numel() + guard]


def execute_case(plan, c):
    """One case of the table on `plan`; returns out as numpy (the canaries checked)."""
    a, b = rc.operands(c)
    nnz, V = a.size, rc.NP[c.val]
    # an operand that is also the output carries the canaries
    da, ga = on_device(a, c.shift[2], 1, rc.CANARY)
    db, gb = on_device(b, c.shift[3], 1, rc.CANARY) if b is not None else (None, None)
    if c.in_place == 0:
        out, guard = on_device(np.full(nnz, np.nan, dtype=V), c.shift[4], 1, rc.CANARY)
    else:
        out, guard = (da, ga) if c.in_place == 1 else (db, gb)
    plan.set_scale(c.scale)
    got = plan.execute(da, out) if c.mode == "fwd" else plan.backward(da, db, out)
    assert nnz == 0 or got.data_ptr() == out.data_ptr()
    gh = guard.cpu().numpy()        # (the copy synchronises)
    assert gh[0] == V(rc.CANARY) and gh[-1] == V(rc.CANARY), "%s: a canary beside out was written" % c.name
    if c.in_place != 1:
        assert np.array_equal(da.cpu().numpy().view(np.uint8), a.view(np.uint8)), "%s: an input was written" % c.name
    if b is not None and c.in_place != 2:
        assert np.array_equal(db.cpu().numpy().view(np.uint8), b.view(np.uint8)), "%s: an input was written" % c.name
    return gh[1:-1].copy()


@pytest.fixture(scope="module")
def table(sp):
    """Every case of the table, run once: {case name: out}.  Plans are made per (structure, types, matrix offsets), as the
    host simulation's are, and the cases of a plan run in table order.  No case is skipped."""
    import sim_runner as sr
    results = {}
    for group in sr.groups_by(rc.table(), rc.plan_key):
        c = group[0]
        Ap, Aj = rc.csr(c.matrix, c.off)
        dAp, dAj = on_device(Ap, c.shift[0])[0], on_device(Aj, c.shift[1])[0]
        plan = sp.RowSoftmaxPlan(len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1]), dAp, dAj, TORCH[c.val])
        try:
            info = plan.info()
            rc.assert_geometry(info)
            assert info["n_slices"] == -(-(len(c.matrix.lens) + int(Ap[-1])) // rc.SLICE_LEN)
            assert (info["scratch_bytes"] > 0) == (int(Ap[-1]) > 0) and info["scratch_bytes"] <= 64 * info["n_slices"]
            for c in group:
                results[c.name] = execute_case(plan, c)
        finally:
            plan.destroy()
    return results


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_table(table, family):
    cases = rc.family(family)
    assert cases
    for c in cases:
        rc.check(c, table[c.name])


def test_in_place_equals_out_of_place_bit_for_bit(table):
    for a, b in rc.in_place_pairs():
        assert np.array_equal(table[a.name].view(np.uint8), table[b.name].view(np.uint8)), b.name


def test_two_executes_give_equal_bits(table):
    for a, b in rc.repeat_pairs():
        assert np.array_equal(table[a.name].view(np.uint8), table[b.name].view(np.uint8)), a.name


# ---- what only a device shows ---------------------------------------------------------------------------------------------
def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hub_real(mode, variant, off="i32", val="f32", scale=0.125):
    return rc._case(sc.hub_structure(), off, val, mode, "real", variant, scale, 0, rc.SHIFTS[0], "-device")


def test_repeat_side_stream_and_graph(sp):
    c = hub_real("fwd", 0)
    Ap, Aj = rc.csr(c.matrix, c.off)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj = d(Ap), d(Aj)
    plan = sp.RowSoftmaxPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32)
    plan.set_scale(c.scale)
    dx = d(rc.operands(c)[0])
    out = torch.full((nnz,), float("nan"), device=DEV)
    plan.execute(dx, out)
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    rc.check(c, first)
    out.fill_(float("nan"))
    plan.execute(dx, out)                       # two executes: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(first.view(np.uint32), out.cpu().numpy().view(np.uint32))
    made = plan.execute(dx)                     # out=None makes the result
    assert made.shape == (nnz,) and np.array_equal(first.view(np.uint32), made.cpu().numpy().view(np.uint32))
    s = torch.cuda.Stream()                     # a side stream
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        plan.execute(dx, out)
    s.synchronize()
    assert np.array_equal(first.view(np.uint32), out.cpu().numpy().view(np.uint32))
    # one capture of a forward and its backward, replayed on other values
    c_b = hub_real("bwd", 0)
    ddp = d(rc.operands(c_b)[1])
    grad = torch.full((nnz,), float("nan"), device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute(dx, out)
        plan.backward(out, ddp, grad)
    c2 = hub_real("fwd", 1)._replace(name=c.name + "-replayed")
    dx.copy_(d(rc.operands(c2)[0]))
    out.fill_(float("nan"))
    grad.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    rc.check(c2, got)
    assert not np.array_equal(got, first)
    # the gradient the graph made is the backward of the p it made
    want = plan.backward(out, ddp).cpu().numpy()
    assert np.array_equal(grad.cpu().numpy().view(np.uint32), want.view(np.uint32)) and not np.any(np.isnan(want))
    del g
    plan.destroy()


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i32", "f64"), ("i64", "f32"), ("i64", "f64")])
def test_one_shots_equal_the_plan(sp, off, val):
    c = rc._case(rc.structures("ragged")[0], off, val, "fwd", "real", 1, 0.125, 0, rc.SHIFTS[0], "-device")
    Ap, Aj = rc.csr(c.matrix, c.off)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dx = d(Ap), d(Aj), d(rc.operands(c)[0])
    plan = sp.RowSoftmaxPlan(n_rows, n_cols, nnz, dAp, dAj, TORCH[val])
    plan.set_scale(c.scale)
    want = plan.execute(dx)
    got = sp.row_softmax(n_rows, n_cols, nnz, dAp, dAj, dx, scale=c.scale)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    rc.check(c, got.cpu().numpy())
    # the C entry point itself, in place
    buf = dx.clone()
    f = getattr(sp.capi.lib(), "mi355_spmv_row_softmax_%s_%s" % (off, val))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert f(n_rows, n_cols, nnz, ptr(dAp), ptr(dAj), ptr(buf), ptr(buf), C.c_double(c.scale),
             C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    plan.destroy()


def test_in_place_on_the_hub_row(sp):
    """The 30-slice chain in place: forward into x, backward into dp and into p, bit for bit the out-of-place results."""
    c, c_b = hub_real("fwd", 2, "i64", "f64", -2.0), hub_real("bwd", 2, "i64", "f64", -2.0)
    Ap, Aj = rc.csr(c.matrix, c.off)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    plan = sp.RowSoftmaxPlan(n_rows, n_cols, nnz, d(Ap), d(Aj), torch.float64)
    plan.set_scale(c.scale)
    dx = d(rc.operands(c)[0])
    want = plan.execute(dx)
    assert plan.execute(dx, dx).data_ptr() == dx.data_ptr() and torch.equal(dx, want)
    rc.check(c, dx.cpu().numpy())
    p, dp = (d(a) for a in rc.operands(c_b))
    want = plan.backward(p, dp)
    rc.check(c_b, want.cpu().numpy())
    p2, dp2 = p.clone(), dp.clone()
    plan.backward(p, dp2, dp2)
    plan.backward(p2, dp, p2)
    assert torch.equal(dp2, want) and torch.equal(p2, want)
    plan.destroy()


def test_nothing_stored_launches_nothing(sp):
    for n_rows in (0, 2500):
        Ap = torch.zeros(n_rows + 1, dtype=torch.int32, device=DEV)
        Aj = torch.zeros(0, dtype=torch.int32, device=DEV)
        plan = sp.RowSoftmaxPlan(n_rows, 5, 0, Ap, Aj, torch.float32)
        x = torch.zeros(0, device=DEV)
        assert plan.execute(x).numel() == 0 and plan.backward(x, x).numel() == 0
        assert sp.row_softmax(n_rows, 5, 0, Ap, Aj, x).numel() == 0
        torch.cuda.synchronize()
        assert plan.info()["n_slices"] == -(-n_rows // 1024) and plan.info()["scratch_bytes"] == 0
        plan.destroy()


@pytest.mark.parametrize("val", ["f32", "f64"])
def test_the_chain_sddmm_softmax_spmm(sp, val):
    """Sparse attention on real data: P = row_softmax(sddmm(Q, K) / sqrt(k)), Y = spmm(P, Vv), against numpy in fp64 within
    the sum of the three stated bounds, each carried to Y at first order with its exact factor:
      scores   |ds| <= b1 = the SDDMM bound of tests/sddmm_cases.py (pattern, alpha = 1, beta = 0)
      softmax  an error dv = scale * ds of a row's inputs changes p by at most p * expm1(2 max_row |dv|); to that the
               forward bound b2 of tests/row_softmax_cases.py on the p of the perturbed scores
      spmm     |dY| <= sum_row dp |x|  +  (len + 2) eps sum_row (p + dp) |x|     (the multi-vector kind's row bound)"""
    m = rc.structures("ragged")[0]
    Ap, Aj, _, _, U, Vm = sc.arrays(m, "i32", val, False)
    n_rows, n_cols, nnz, k = len(m.lens), m.n_cols, int(Ap[-1]), 8
    scale = 1.0 / np.sqrt(k)
    Q, K = U[:, :k], Vm[:, :k]
    Vv = Vm[:, k:2 * k]
    dAp, dAj = d(Ap), d(Aj)
    scores = sp.sddmm(n_rows, n_cols, nnz, dAp, dAj, None, d(Q), d(K))
    plan = sp.RowSoftmaxPlan(n_rows, n_cols, nnz, dAp, dAj, TORCH[val])
    plan.set_scale(scale)
    P = plan.execute(scores)
    Y = torch.full((n_rows, k), float("nan"), dtype=TORCH[val], device=DEV)
    sp.spmm(n_rows, n_cols, nnz, dAp, dAj, P, d(Vv), Y)
    torch.cuda.synchronize()
    plan.destroy()
    eps, lens, rows = rc.EPS[val], np.asarray(m.lens), rc.rows_of(m)
    q, kk = Q.astype(np.float64)[rows], K.astype(np.float64)[Aj]
    s64, sabs = (q * kk).sum(1), np.abs(q * kk).sum(1)
    b1 = (k + 3) * eps * sabs + 4 * eps * np.abs(s64)
    assert np.all(np.abs(scores.cpu().numpy() - s64) <= b1)
    p64, v, vmax, spread = rc.forward_ref(s64, float(rc.NP[val](scale)), m)
    dv = np.zeros(n_rows)
    np.maximum.at(dv, rows, abs(scale) * b1)
    grow = np.exp(2 * dv[rows])
    b2 = eps * p64 * grow * (2 * lens[rows] + 2 * rc.E_EXP + 2 * (vmax + spread + 2 * dv)[rows] + 4)
    dp = p64 * np.expm1(2 * dv[rows]) + b2
    assert np.all(np.abs(P.cpu().numpy() - p64) <= dp)
    x = Vv.astype(np.float64)[Aj]
    want = np.zeros((n_rows, k))
    np.add.at(want, rows, p64[:, None] * x)
    bound = np.zeros((n_rows, k))
    np.add.at(bound, rows, dp[:, None] * np.abs(x) + ((lens[rows] + 2) * eps * (p64 + dp))[:, None] * np.abs(x))
    got = Y.cpu().numpy()
    assert not np.any(np.isnan(got[lens > 0])) and np.all(got[lens == 0] == 0)
    assert np.all(np.abs(got - want) <= bound + 1e-300)
    assert np.abs(got - want).max() > 0 or val == "f64"


@pytest.mark.parametrize("val", ["f32", "f64"])
def test_the_backward_is_the_adjoint_of_the_forwards_derivative(sp, val):
    """sum dx * d == sum dp * (J d), with J d = scale * p * (d - sum_row p d) the directional derivative of the forward,
    computed by numpy in fp64 from the fp64 p (no finite differences, none on the device).  Tolerance, at first order:
    the backward bound of tests/row_softmax_cases.py on each dx, plus what the forward bound b2 on the device's p does to
    dx = scale p (dp - t): |scale| (b2 (|dp| + |t|) + p sum_row b2 |dp|), each weighted by |d|."""
    m = sc.hub_structure()
    c = rc._case(m, "i64", val, "fwd", "real", 1, 0.125)
    x, _ = rc.operands(c)
    Ap, Aj = rc.csr(m, c.off)
    n_rows, nnz = len(m.lens), int(Ap[-1])
    rng = np.random.RandomState(77)
    dp, dd = (rng.rand(nnz) * 2 - 1).astype(rc.NP[val]), rng.rand(nnz) * 2 - 1
    plan = sp.RowSoftmaxPlan(n_rows, m.n_cols, nnz, d(Ap), d(Aj), TORCH[val])
    plan.set_scale(c.scale)
    p = plan.execute(d(x))
    dx = plan.backward(p, d(dp)).cpu().numpy().astype(np.float64)
    plan.destroy()
    eps, lens, rows = rc.EPS[val], np.asarray(m.lens), rc.rows_of(m)
    p64, v, vmax, spread = rc.forward_ref(x, c.scale, m)
    dp64 = dp.astype(np.float64)
    jd = c.scale * p64 * (dd - np.bincount(rows, weights=p64 * dd, minlength=n_rows)[rows])
    t = np.bincount(rows, weights=p64 * dp64, minlength=n_rows)
    tabs = np.bincount(rows, weights=np.abs(p64 * dp64), minlength=n_rows)
    b2 = eps * p64 * (2 * lens[rows] + 2 * rc.E_EXP + 2 * (vmax + spread)[rows] + 4)
    b_bwd = eps * abs(c.scale) * p64 * ((lens + 2)[rows] * tabs[rows] + 3 * (np.abs(dp64) + np.abs(t[rows]))) + rc.TINY[val]
    b_p = abs(c.scale) * (b2 * (np.abs(dp64) + np.abs(t[rows])) + p64 * np.bincount(rows, weights=b2 * np.abs(dp64), minlength=n_rows)[rows])
    lhs, rhs = np.dot(dx, dd), np.dot(dp64, jd)
    assert rhs != 0.0 and abs(lhs - rhs) <= 1.01 * np.dot(np.abs(dd), b_bwd + b_p)
