"""Fused sparse attention with 16-bit Q, K, V and O on the GPU (sp.SparseAttentionPlan(vec_dtype=) / sp.sparse_attention_half,
csrc/attention_half_kernel.hpp): the table of tests/attention_half_cases.py — the cases that
tests/test_attention_half_sim_cpu.py executes on the host — on the device, family by family and plan by plan, each result
as that module says (const and masked data bit for bit against one fp32 division narrowed once, real data within its derived
bound); O starts as a canary that must survive in its padding columns, lse as NaN, and one canary element before and one
behind every operand must survive.  Unaligned operands give the aligned bits, two executes the same bits, and where both
kinds run one lane per nonzero the 16-bit O is narrow(the fp32 kind's O on the widened operands).  Then what only a device
shows: a side stream, one graph capture replayed on new values, the four one-shots, lse=None, agreement with the 16-bit
chain SddmmPlan(vec_dtype) -> RowSoftmaxPlan in place -> MultiPlan(vec_dtype, mat_dtype=float32), rows without entries, and
info() of one-, two- and three-pass plans."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_cases as ac
import attention_half_cases as hc
import sim_runner as sr
from test_gpu_attention import DEV, on_device, same_bits

pytestmark = pytest.mark.gpu

TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}


def signed(bits):
    """A 16-bit pattern as the int16 that holds it."""
    return int(np.uint16(bits).astype(np.int16))


def canary_bits(vec):
    return int(hc.to_bits(np.float32(hc.CANARY), vec).reshape(-1)[0])


def bits16(a, vec):
    """fp32 values that `vec` holds, as the int16 array of their 16-bit patterns (the shape kept)."""
    return hc.to_bits(a, vec).reshape(np.shape(a)).view(np.int16)


def strided(full, col0, width, ld, shift, fill, guard_fill):
    """Columns col0 .. col0 + width of `full` as a device matrix of leading dimension ld, (rows - 1) * ld + width elements
    long, its padding columns `fill`, one element of guard_fill before and behind it: (the rows x width view, the flat numpy
    it was made from, the guarded flat view)."""
    rows = full.shape[0]
    flat = np.full((rows - 1) * ld + width if rows else 0, fill, dtype=full.dtype)
    for r in range(rows):
        flat[r * ld:r * ld + width] = full[r, col0:col0 + width]
    v, g = on_device(flat, shift, 1, guard_fill)
    return torch.as_strided(v, (rows, width), (ld, 1)) if rows else v.reshape(0, width), flat, g


def execute_case(plan, c):
    """One case of the table on `plan`; returns (O bits, lse or None) as numpy, the canaries and the inputs checked."""
    T, n_rows = TORCH[c.vec], len(c.matrix.lens)
    can, nan = signed(canary_bits(c.vec)), signed(hc.NAN_BITS[c.vec])
    Qf, Kf, Vf, bias = hc.operands(c)
    dQ, hq, gq = strided(bits16(Qf, c.vec), c.c0, c.d, c.ldq, c.shift[2], nan, can)
    dK, hk, gk = strided(bits16(Kf, c.vec), c.c0, c.d, c.ldk, c.shift[3], nan, can)
    dV, hv, gv = strided(bits16(Vf, c.vec), c.cv0, c.dv, c.ldv, c.shift[4], nan, can)
    db, gb = on_device(bias, c.shift[5]) if bias is not None else (None, None)
    dO, ho, go = strided(np.full((n_rows, c.dv), can, dtype=np.int16), 0, c.dv, c.ldo, c.shift[6], can, can)
    dl, gl = on_device(np.full(n_rows, np.nan, dtype=np.float32), c.shift[7])
    plan.set_scale(c.scale)
    got = plan.execute(dQ.view(T), dK.view(T), dV.view(T), dO.view(T), dl if c.want_lse else None, db)
    assert got.data_ptr() == dO.data_ptr() and got.dtype is T
    O = dO.cpu().numpy().view(np.uint16)        # (the copy synchronises)
    for g, h, name in ((gq, hq, "Q"), (gk, hk, "K"), (gv, hv, "V")):
        gh = g.cpu().numpy()
        assert gh[0] == can and gh[-1] == can, "%s: a canary beside %s was written" % (c.name, name)
        assert same_bits(gh[1:-1], h), "%s: %s was written" % (c.name, name)
    if gb is not None:
        gh = gb.cpu().numpy()
        assert gh[0] == np.float32(ac.CANARY) and gh[-1] == np.float32(ac.CANARY) and same_bits(gh[1:-1], bias), "%s: bias was written" % c.name
    gh = go.cpu().numpy()
    assert gh[0] == can and gh[-1] == can, "%s: a canary beside O was written" % c.name
    pad = np.ones(gh.size - 2, dtype=bool)
    for r in range(n_rows):
        pad[r * c.ldo:r * c.ldo + c.dv] = False
    assert np.all(gh[1:-1][pad] == can), "%s: a padding column of O was written" % c.name
    gh = gl.cpu().numpy()
    assert gh[0] == np.float32(ac.CANARY) and gh[-1] == np.float32(ac.CANARY), "%s: a canary beside lse was written" % c.name
    assert c.want_lse or np.all(np.isnan(gh[1:-1])), "%s: lse was written without being asked for" % c.name
    return O, gh[1:-1].copy() if c.want_lse else None


def run_cases(sp, cases, ratios=None):
    """The cases, plan group by plan group in table order: {case name: (O bits, lse)}, each checked as the table says."""
    results = {}
    for group in sr.groups_by(cases, hc.plan_key):
        c = group[0]
        Ap, Aj = hc.csr(c.matrix, c.off)
        n_rows, nnz = len(c.matrix.lens), int(Ap[-1])
        dAp, dAj = on_device(Ap, c.shift[0], 0)[0], on_device(Aj, c.shift[1], 0)[0]
        plan = sp.SparseAttentionPlan(n_rows, c.matrix.n_cols, nnz, dAp, dAj, torch.float32, hc.KF, hc.KV, vec_dtype=TORCH[c.vec])
        try:
            info = plan.info()
            hc.assert_geometry(info)
            assert info["n_slices"] == -(-(n_rows + nnz) // hc.SLICE_LEN)
            carry_ld = -(-hc.KV // hc.TILE) * hc.TILE       # fp32 pieces over whole 64-column tiles
            assert info["scratch_bytes"] == info["n_slices"] * 2 * ((carry_ld + 2) * 4 + 4)
            for c in group:
                results[c.name] = execute_case(plan, c)
                hc.check(c, *results[c.name], ratios=ratios)
        finally:
            plan.destroy()
    return results


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def d16(a, vec):
    return d(bits16(a, vec)).view(TORCH[vec])


def device_case(c):
    """(n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, dbias) of a case, contiguous, Q / K / V in the 16-bit type."""
    Ap, Aj = hc.csr(c.matrix, c.off)
    Q, K, V, bias = hc.operands(c)
    return (len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1]), d(Ap), d(Aj), d16(Q[:, c.c0:c.c0 + c.d], c.vec), d16(K[:, c.c0:c.c0 + c.d], c.vec),
            d16(V[:, c.cv0:c.cv0 + c.dv], c.vec), d(bias) if bias is not None else None)


def o_bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def fp32_kind(sp, c):
    """(O, lse) of the fp32 / fp64 kind's plan on the widened operands of a case."""
    Ap, Aj = hc.csr(c.matrix, c.off)
    Q, K, V, bias = hc.operands(c)
    n_rows = len(c.matrix.lens)
    plan = sp.SparseAttentionPlan(n_rows, c.matrix.n_cols, int(Ap[-1]), d(Ap), d(Aj), torch.float32, c.d, c.dv)
    plan.set_scale(c.scale)
    lse = torch.empty(n_rows, device=DEV)
    O = plan.execute(d(Q[:, c.c0:c.c0 + c.d]), d(K[:, c.c0:c.c0 + c.d]), d(V[:, c.cv0:c.cv0 + c.dv]), None, lse, d(bias) if bias is not None else None)
    torch.cuda.synchronize()
    plan.destroy()
    return O.cpu().numpy(), lse.cpu().numpy()


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_table(sp, family):
    cases = hc.family(family)
    assert cases
    ratios = []
    results = run_cases(sp, cases, ratios)
    assert len(results) == len(cases)
    if ratios:      # (shown with -s: DESIGN.md records the largest over the table)
        print("attention_half %s: largest error / derived bound over %d real cases: %.4f" % (family, len(ratios), max(ratios)))
    if family == "alignment":
        for a, b in hc.alignment_pairs():
            assert same_bits(results[a.name][0], results[b.name][0]) and same_bits(results[a.name][1], results[b.name][1]), b.name
    if family == "repeat":
        for a, b in hc.repeat_pairs():
            assert same_bits(results[a.name][0], results[b.name][0]) and same_bits(results[a.name][1], results[b.name][1]), a.name
    if family == "fp32_pairs":
        for c in cases:
            assert hc.lanes_per_slot(c.dv) == 1 and ac.lanes_per_slot(c.dv, "f32") == 1
            O32, lse32 = fp32_kind(sp, c)
            assert same_bits(results[c.name][0], hc.to_bits(O32, c.vec).reshape(O32.shape)), c.name
            assert same_bits(results[c.name][1], lse32), c.name


# ---- what only a device shows ---------------------------------------------------------------------------------------------
def hub_real(variant, vec, off="i32", scale=0.125, d_=16, dv=64):
    return hc._case(hc.structures("hub")[0], off, vec, "real", variant, scale, d_, dv, tag="-device")


@pytest.mark.parametrize("vec", hc.VECS)
def test_repeat_side_stream_graph_and_lse_none(sp, vec):
    c, T = hub_real(0, vec), TORCH[vec]
    n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, db = device_case(c)
    plan = sp.SparseAttentionPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, c.d, c.dv, vec_dtype=T)
    assert plan.info()["passes"] == 1
    plan.set_scale(c.scale)
    out = torch.full((n_rows, c.dv), float("nan"), dtype=T, device=DEV)
    lse = torch.full((n_rows,), float("nan"), device=DEV)
    plan.execute(dQ, dK, dV, out, lse, db)
    torch.cuda.synchronize()
    first, first_lse = o_bits(out), lse.cpu().numpy()
    hc.check(c, first, first_lse)
    out.fill_(float("nan"))
    lse.fill_(float("nan"))
    plan.execute(dQ, dK, dV, out, lse, db)                  # two executes: the same bits
    torch.cuda.synchronize()
    assert same_bits(first, o_bits(out)) and same_bits(first_lse, lse.cpu().numpy())
    made = plan.execute(dQ, dK, dV, bias=db)                # out=None makes the result in vec_dtype; lse=None: the same O
    assert made.shape == (n_rows, c.dv) and made.dtype is T and same_bits(first, o_bits(made))
    s = torch.cuda.Stream()                                 # a side stream
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        plan.execute(dQ, dK, dV, out, lse, db)
    s.synchronize()
    assert same_bits(first, o_bits(out))
    # one capture on a single stream, replayed on other values
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute(dQ, dK, dV, out, lse, db)
    c2 = hub_real(1, vec)
    _, _, _, _, _, dQ2, dK2, dV2, db2 = device_case(c2)
    dQ.copy_(dQ2)
    dK.copy_(dK2)
    dV.copy_(dV2)
    db.copy_(db2)
    out.fill_(float("nan"))
    lse.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = o_bits(out)
    hc.check(c2, got, lse.cpu().numpy())
    assert not np.array_equal(got, first)
    del g
    plan.destroy()


@pytest.mark.parametrize("off,vec", [(o, v) for o in hc.OFFS for v in hc.VECS])
def test_one_shots_equal_the_plan(sp, off, vec):
    c, T = hc._case(hc.structures("ragged")[0], off, vec, "real", 1, 0.125, 13, 65, tag="-device"), TORCH[vec]
    n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, db = device_case(c)
    plan = sp.SparseAttentionPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, c.d, c.dv, vec_dtype=T)
    plan.set_scale(c.scale)
    want_lse = torch.empty(n_rows, device=DEV)
    want = plan.execute(dQ, dK, dV, None, want_lse, db)
    lse = torch.empty_like(want_lse)
    got = sp.sparse_attention_half(n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, bias=db, scale=c.scale, lse=lse)
    torch.cuda.synchronize()
    assert got.dtype is T and same_bits(o_bits(got), o_bits(want)) and torch.equal(lse, want_lse)
    hc.check(c, o_bits(got), lse.cpu().numpy())
    # the C entry point itself
    out2, lse2 = torch.full_like(want, float("nan")), torch.full_like(lse, float("nan"))
    f = getattr(sp.capi.lib(), "mi355_spmv_attention_half_%s_%s" % (off, vec))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert f(n_rows, n_cols, nnz, ptr(dAp), ptr(dAj), c.d, c.dv, ptr(dQ), c.d, ptr(dK), c.d, ptr(dV), c.dv, ptr(db), C.c_double(c.scale),
             ptr(out2), c.dv, ptr(lse2), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert same_bits(o_bits(out2), o_bits(want)) and torch.equal(lse2, want_lse)
    plan.destroy()


def test_rows_without_entries_are_zero_and_minus_infinity(sp):
    for n_rows, T in ((0, torch.float16), (2500, torch.bfloat16), (2500, torch.float16)):
        Ap = torch.zeros(n_rows + 1, dtype=torch.int32, device=DEV)
        Aj = torch.zeros(0, dtype=torch.int32, device=DEV)
        Q, K, V = torch.ones(n_rows, 4, dtype=T, device=DEV), torch.ones(5, 4, dtype=T, device=DEV), torch.ones(5, 70, dtype=T, device=DEV)
        out = torch.full((n_rows, 70), float("nan"), dtype=T, device=DEV)
        lse = torch.full((n_rows,), float("nan"), device=DEV)
        plan = sp.SparseAttentionPlan(n_rows, 5, 0, Ap, Aj, torch.float32, 4, 70, vec_dtype=T)
        plan.execute(Q, K, V, out, lse)
        got = sp.sparse_attention_half(n_rows, 5, 0, Ap, Aj, Q, K, V)
        torch.cuda.synchronize()
        assert np.all(o_bits(out) == 0) and np.all(np.isneginf(lse.cpu().numpy())) and same_bits(o_bits(got), o_bits(out))
        assert plan.info()["n_slices"] == -(-n_rows // 1024)
        plan.destroy()


@pytest.mark.parametrize("vec", hc.VECS)
def test_the_fused_execute_agrees_with_the_16_bit_chain(sp, vec):
    """On the ragged structure, without a bias (the chain has none): S = SddmmPlan(vec_dtype)(Q, K) in fp32, P =
    RowSoftmaxPlan(scale * S) in place, Y = MultiPlan(vec_dtype, mat_dtype=float32)(P, V).  The chain's fp32 row sum is within
    attention_cases' fp32 bound of the fp64 value — the chain's three stated bounds are the pieces that bound is composed of —
    and is narrowed once, as the fused O is: each is within the table's bound, so they differ by at most the sum of both."""
    dd, dv, T = 16, 64, TORCH[vec]
    c = hc._case(hc.structures("ragged")[0], "i32", vec, "real", 2, 0.125, dd, dv, tag="-chain")
    n_rows, n_cols, nnz, dAp, dAj, dQ, dK, dV, db = device_case(c)
    assert db is None
    fused = sp.SparseAttentionPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, dd, dv, vec_dtype=T)
    fused.set_scale(c.scale)
    lse = torch.empty(n_rows, device=DEV)
    O = fused.execute(dQ, dK, dV, None, lse)
    p1 = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, vec_dtype=T)
    p2 = sp.RowSoftmaxPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32)
    p3 = sp.MultiPlan(n_rows, n_cols, nnz, dAp, dAj, T, dv, mat_dtype=torch.float32)
    p2.set_scale(c.scale)
    S = p1.execute(None, dQ, dK)
    P = p2.execute(S, S)
    assert P.data_ptr() == S.data_ptr()
    Y = torch.full((n_rows, dv), float("nan"), dtype=T, device=DEV)
    p3.execute(P, dV, Y)
    torch.cuda.synchronize()
    for p in (fused, p1, p2, p3):
        p.destroy()
    hc.check(c, o_bits(O), lse.cpu().numpy())
    bound = hc.o_bound(c)
    diff = np.abs(hc.from_bits(o_bits(O), vec).reshape(n_rows, dv).astype(np.float64) - hc.from_bits(o_bits(Y), vec).reshape(n_rows, dv).astype(np.float64))
    assert np.all(diff <= 2 * bound)


def test_info_of_one_two_and_three_pass_plans(sp):
    m = hc.structures("ragged")[0]
    Ap, Aj = hc.csr(m, "i32")
    dAp, dAj = d(Ap), d(Aj)
    for vec in hc.VECS:
        for dv_max, passes in ((64, 1), (65, 2), (128, 2), (129, 3), (3, 1), (32, 1)):
            plan = sp.SparseAttentionPlan(len(m.lens), m.n_cols, int(Ap[-1]), dAp, dAj, torch.float32, 24, dv_max, vec_dtype=TORCH[vec])
            info = plan.info()
            hc.assert_geometry(info)
            assert info["main_kernel"] == "attention_half_slice_kernel" and info["passes"] == passes
            assert (info["d_max"], info["dv_max"]) == (24, dv_max)
            assert info["lanes_per_slot"] == (8 if dv_max > 32 else hc.lanes_per_slot(dv_max))
            assert info["grid_blocks"] == -(-info["n_slices"] // (info["block_threads"] // 64))
            val, vt = C.c_int(), C.c_int()
            assert sp.capi.lib().mi355_spmv_attention_get_types(plan._h, C.byref(val), C.byref(vt)) == 0
            assert (val.value, vt.value) == (hc.VAL_TYPE["f32"], hc.VAL_TYPE[vec])
            plan.destroy()
