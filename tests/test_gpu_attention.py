"""Fused sparse attention on the GPU (sp.SparseAttentionPlan / sp.sparse_attention, csrc/attention.hip): the table of
tests/attention_cases.py — the cases that tests/test_attention_sim_cpu.py executes on the host — on the device, family by
family and plan by plan, each result against numpy's fp64 value as that module says (exact families bit for bit, real data
within its derived bound); O starts as a canary that must survive in its padding columns, lse as NaN, and one canary
element before and one behind every operand must survive.  Then what only a device shows: two executes give the same
bits, a side stream, one graph capture replayed on new values, the one-shots, lse=None, agreement with the chain
SddmmPlan -> RowSoftmaxPlan -> MultiPlan, exp(v - lse) against RowSoftmaxPlan's P, and info() of a one-pass and a two-pass
plan."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_cases as ac
import row_softmax_cases as rc
import sim_runner as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH = {"f32": torch.float32, "f64": torch.float64}


def on_device(flat, shift, guard=1, fill=ac.CANARY):
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


def strided(full, col0, width, ld, shift, fill):
    """Columns col0 .. col0 + width of `full` as a device matrix of leading dimension ld, (rows - 1) * ld + width elements
    long, its padding columns `fill`: (the rows x width view, the flat numpy it was made from, the guarded flat view)."""
    rows = full.shape[0]
    flat = np.full((rows - 1) * ld + width if rows else 0, fill, dtype=full.dtype)
    for r in range(rows):
        flat[r * ld:r * ld + width] = full[r, col0:col0 + width]
    v, g = on_device(flat, shift)
    return torch.as_strided(v, (rows, width), (ld, 1)) if rows else v.reshape(0, width), flat, g


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def execute_case(plan, c):
    """One case of the table on `plan`; returns (O, lse or None) as numpy, the canaries and the inputs checked."""
    T = ac.NP[c.val]
    n_rows = len(c.matrix.lens)
    Qf, Kf, Vf, bias = ac.operands(c)
    dQ, hq, gq = strided(Qf, c.c0, c.d, c.ldq, c.shift[2], np.nan)
    dK, hk, gk = strided(Kf, c.c0, c.d, c.ldk, c.shift[3], np.nan)
    dV, hv, gv = strided(Vf, c.cv0, c.dv, c.ldv, c.shift[4], np.nan)
    db, gb = on_device(bias, c.shift[5]) if bias is not None else (None, None)
    dO, ho, go = strided(np.full((n_rows, c.dv), ac.CANARY, dtype=T), 0, c.dv, c.ldo, c.shift[6], ac.CANARY)
    dl, gl = on_device(np.full(n_rows, np.nan, dtype=T), c.shift[7])
    plan.set_scale(c.scale)
    got = plan.execute(dQ, dK, dV, dO, dl if c.want_lse else None, db)
    assert n_rows == 0 or got.data_ptr() == dO.data_ptr()
    O = dO.cpu().numpy()        # (the copy synchronises)
    for g, h, name in ((gq, hq, "Q"), (gk, hk, "K"), (gv, hv, "V"), (gb, bias, "bias")):
        if g is None:
            continue
        gh = g.cpu().numpy()
        assert gh[0] == T(ac.CANARY) and gh[-1] == T(ac.CANARY), "%s: a canary beside %s was written" % (c.name, name)
        assert same_bits(gh[1:-1], h), "%s: %s was written" % (c.name, name)
    gh = go.cpu().numpy()
    assert gh[0] == T(ac.CANARY) and gh[-1] == T(ac.CANARY), "%s: a canary beside O was written" % c.name
    pad = np.ones(gh.size - 2, dtype=bool)
    for r in range(n_rows):
        pad[r * c.ldo:r * c.ldo + c.dv] = False
    assert np.all(gh[1:-1][pad] == T(ac.CANARY)), "%s: a padding column of O was written" % c.name
    gh = gl.cpu().numpy()
    assert gh[0] == T(ac.CANARY) and gh[-1] == T(ac.CANARY), "%s: a canary beside lse was written" % c.name
    assert c.want_lse or np.all(np.isnan(gh[1:-1])), "%s: lse was written without being asked for" % c.name
    return O, gh[1:-1].copy() if c.want_lse else None


def run_cases(sp, cases, ratios=None):
    """The cases, plan group by plan group in table order: {case name: (O, lse)}, each checked as the table says."""
    results = {}
    for group in sr.groups_by(cases, ac.plan_key):
        c = group[0]
        Ap, Aj = ac.csr(c.matrix, c.off)
        n_rows, nnz = len(c.matrix.lens), int(Ap[-1])
        dAp, dAj = on_device(Ap, c.shift[0], 0)[0], on_device(Aj, c.shift[1], 0)[0]
        plan = sp.SparseAttentionPlan(n_rows, c.matrix.n_cols, nnz, dAp, dAj, TORCH[c.val], ac.KF, ac.KV)
        try:
            info = plan.info()
            ac.assert_geometry(info, c.val)
            assert info["n_slices"] == -(-(n_rows + nnz) // ac.SLICE_LEN)
            es = 8 if c.val == "f64" else 4
            carry_ld = -(-ac.KV // ac.TILE[c.val]) * ac.TILE[c.val]
            assert info["scratch_bytes"] == info["n_slices"] * 2 * ((carry_ld + 2) * es + 4)
            for c in group:
                results[c.name] = execute_case(plan, c)
                ac.check(c, *results[c.name], ratios=ratios)
        finally:
            plan.destroy()
    return results


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_table(sp, family):
    cases = ac.family(family)
    assert cases
    ratios = []
    results = run_cases(sp, cases, ratios)
    assert len(results) == len(cases)
    if ratios:      # (shown with -s: DESIGN.md records the largest over the table)
        print("attention %s: largest error / derived bound over %d real cases: %.4f" % (family, len(ratios), max(ratios)))
    if family == "alignment":
        for a, b in ac.alignment_pairs():
            assert same_bits(results[a.name][0], results[b.name][0]) and same_bits(results[a.name][1], results[b.name][1]), b.name
    if family == "repeat":
        for a, b in ac.repeat_pairs():
            assert same_bits(results[a.name][0], results[b.name][0]) and same_bits(results[a.name][1], results[b.name][1]), a.name


# ---- what only a device shows ---------------------------------------------------------------------------------------------
def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_case(c):
    """(n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, dbias) of a case, contiguous."""
    Ap, Aj = ac.csr(c.matrix, c.off)
    Q, K, V, bias = ac.operands(c)
    return (len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1]), d(Ap), d(Aj), d(Q[:, c.c0:c.c0 + c.d]), d(K[:, c.c0:c.c0 + c.d]),
            d(V[:, c.cv0:c.cv0 + c.dv]), d(bias) if bias is not None else None)


def hub_real(variant, off="i32", val="f32", scale=0.125, d_=16, dv=32):
    return ac._case(ac.structures("hub")[0], off, val, "real", variant, scale, d_, dv, tag="-device")


def test_repeat_side_stream_graph_and_lse_none(sp):
    c = hub_real(0)
    n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, db = device_case(c)
    plan = sp.SparseAttentionPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, c.d, c.dv)
    plan.set_scale(c.scale)
    out = torch.full((n_rows, c.dv), float("nan"), device=DEV)
    lse = torch.full((n_rows,), float("nan"), device=DEV)
    plan.execute(dQ, dK, dV, out, lse, db)
    torch.cuda.synchronize()
    first, first_lse = out.cpu().numpy(), lse.cpu().numpy()
    ac.check(c, first, first_lse)
    out.fill_(float("nan"))
    lse.fill_(float("nan"))
    plan.execute(dQ, dK, dV, out, lse, db)                  # two executes: the same bits
    torch.cuda.synchronize()
    assert same_bits(first, out.cpu().numpy()) and same_bits(first_lse, lse.cpu().numpy())
    made = plan.execute(dQ, dK, dV, bias=db)                # out=None makes the result; lse=None: the same O, lse untouched
    assert made.shape == (n_rows, c.dv) and same_bits(first, made.cpu().numpy())
    s = torch.cuda.Stream()                                 # a side stream
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        plan.execute(dQ, dK, dV, out, lse, db)
    s.synchronize()
    assert same_bits(first, out.cpu().numpy())
    # one capture, replayed on other values
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute(dQ, dK, dV, out, lse, db)
    c2 = hub_real(1)
    _, _, _, _, _, dQ2, dK2, dV2, db2 = device_case(c2)
    dQ.copy_(dQ2)
    dK.copy_(dK2)
    dV.copy_(dV2)
    db.copy_(db2)
    out.fill_(float("nan"))
    lse.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ac.check(c2, got, lse.cpu().numpy())
    assert not np.array_equal(got, first)
    del g
    plan.destroy()


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i32", "f64"), ("i64", "f32"), ("i64", "f64")])
def test_one_shots_equal_the_plan(sp, off, val):
    dd, dv = (13, 33) if val == "f32" else (7, 17)
    c = ac._case(ac.structures("ragged")[0], off, val, "real", 1, 0.125, dd, dv, tag="-device")
    n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, db = device_case(c)
    plan = sp.SparseAttentionPlan(n_rows, n_cols, nnz, dAp, dAj, TORCH[val], c.d, c.dv)
    plan.set_scale(c.scale)
    want_lse = torch.empty(n_rows, dtype=TORCH[val], device=DEV)
    want = plan.execute(dQ, dK, dV, None, want_lse, db)
    lse = torch.empty_like(want_lse)
    got = sp.sparse_attention(n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, bias=db, scale=c.scale, lse=lse)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(lse, want_lse)
    ac.check(c, got.cpu().numpy(), lse.cpu().numpy())
    # the C entry point itself
    out2, lse2 = torch.full_like(want, float("nan")), torch.full_like(lse, float("nan"))
    f = getattr(sp.capi.lib(), "mi355_spmv_attention_%s_%s" % (off, val))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert f(n_rows, n_cols, nnz, ptr(dAp), ptr(dAj), c.d, c.dv, ptr(dQ), c.d, ptr(dK), c.d, ptr(dV), c.dv, ptr(db), C.c_double(c.scale),
             ptr(out2), c.dv, ptr(lse2), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2, want) and torch.equal(lse2, want_lse)
    plan.destroy()


def test_rows_without_entries_are_zero_and_minus_infinity(sp):
    for n_rows in (0, 2500):
        Ap = torch.zeros(n_rows + 1, dtype=torch.int32, device=DEV)
        Aj = torch.zeros(0, dtype=torch.int32, device=DEV)
        Q, K, V = torch.ones(n_rows, 4, device=DEV), torch.ones(5, 4, device=DEV), torch.ones(5, 40, device=DEV)
        out = torch.full((n_rows, 40), float("nan"), device=DEV)
        lse = torch.full((n_rows,), float("nan"), device=DEV)
        plan = sp.SparseAttentionPlan(n_rows, 5, 0, Ap, Aj, torch.float32, 4, 40)
        plan.execute(Q, K, V, out, lse)
        got = sp.sparse_attention(n_rows, 5, 0, Ap, Aj, Q, K, V)
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy().view(np.uint32) == 0) and np.all(np.isneginf(lse.cpu().numpy())) and torch.equal(got, out)
        assert plan.info()["n_slices"] == -(-n_rows // 1024)
        plan.destroy()


@pytest.mark.parametrize("val", ["f32", "f64"])
def test_the_fused_execute_agrees_with_the_chain_and_lse_gives_the_chains_p(sp, val):
    """On the ragged structure, without a bias (the chain has none): S = SddmmPlan(Q, K), P = RowSoftmaxPlan(scale * S),
    Y = MultiPlan(P, V).  The fused O and the chain's Y are each within the table's derived bound of the fp64 value — the
    chain's three stated bounds are the pieces that bound is composed of — so they differ by at most twice the bound.
    And P[n] = exp(scale * S[n] - lse[r]) from the fused lse: against the chain's P within the row-softmax forward bound on
    P plus what the bound on lse (and the error scale * b1 of S behind the fp64 lse) does to the exponent."""
    dd, dv = 16, 8
    c = ac._case(ac.structures("ragged")[0], "i32", val, "real", 2, 0.125, dd, dv, tag="-chain")
    n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, db = device_case(c)
    assert db is None
    T = TORCH[val]
    fused = sp.SparseAttentionPlan(n_rows, n_cols, nnz, dAp, dAj, T, dd, dv)
    fused.set_scale(c.scale)
    lse = torch.empty(n_rows, dtype=T, device=DEV)
    O = fused.execute(dQ, dK, dV, None, lse)
    p1, p2, p3 = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, T), sp.RowSoftmaxPlan(n_rows, n_cols, nnz, dAp, dAj, T), sp.MultiPlan(n_rows, n_cols, nnz, dAp, dAj, T, dv)
    p2.set_scale(c.scale)
    S = p1.execute(None, dQ, dK)
    P = p2.execute(S)
    Y = torch.full((n_rows, dv), float("nan"), dtype=T, device=DEV)
    p3.execute(P, dV, Y)
    torch.cuda.synchronize()
    for p in (fused, p1, p2, p3):
        p.destroy()
    ex = ac.expected(c)
    O, Y, lse = O.cpu().numpy(), Y.cpu().numpy(), lse.cpu().numpy()
    ac.check(c, O, lse)
    assert np.all(np.abs(O.astype(np.float64) - Y.astype(np.float64)) <= 2 * ex["bound"])
    # P from lse
    m, rows, lens, eps = c.matrix, ac.rows_of(c.matrix), np.asarray(c.matrix.lens), ac.EPS[val]
    s64 = S.cpu().numpy().astype(np.float64)
    scale = float(ac.NP[val](c.scale))
    p64, v, vmax, spread = rc.forward_ref(S.cpu().numpy(), scale, m)
    b2 = eps * p64 * (2 * lens[rows] + 2 * rc.E_EXP + 2 * (vmax + spread)[rows] + 4)
    Q, K = ac.operands(c)[0][:, c.c0:c.c0 + dd].astype(np.float64)[rows], ac.operands(c)[1][:, c.c0:c.c0 + dd].astype(np.float64)[ac.csr(m, c.off)[1]]
    b1 = np.zeros(n_rows)
    np.maximum.at(b1, rows, abs(scale) * ((dd + 3) * eps * np.abs(Q * K).sum(1) + 4 * eps * np.abs(s64)))
    live = lens > 0
    from_lse = np.exp(scale * s64 - lse.astype(np.float64)[rows])
    tol = b2 + p64 * np.expm1((ex["lse_bound"] + b1)[rows]) + 2 * eps * p64
    assert np.all(np.abs(from_lse - P.cpu().numpy().astype(np.float64)) <= tol) and live.any()


def test_info_of_a_one_pass_and_a_two_pass_plan(sp):
    m = ac.structures("ragged")[0]
    Ap, Aj = ac.csr(m, "i32")
    dAp, dAj = d(Ap), d(Aj)
    for val, one, two in (("f32", 32, 33), ("f64", 16, 17)):
        for dv_max, passes in ((one, 1), (two, 2), (3, 1)):
            plan = sp.SparseAttentionPlan(len(m.lens), m.n_cols, int(Ap[-1]), dAp, dAj, TORCH[val], 24, dv_max)
            info = plan.info()
            ac.assert_geometry(info, val)
            assert info["main_kernel"] == "attention_slice_kernel" and info["passes"] == passes
            assert (info["d_max"], info["dv_max"]) == (24, dv_max)
            assert info["lanes_per_slot"] == (8 if dv_max >= one else ac.lanes_per_slot(dv_max, val))
            assert info["grid_blocks"] == -(-info["n_slices"] // (info["block_threads"] // 64))
            plan.destroy()
