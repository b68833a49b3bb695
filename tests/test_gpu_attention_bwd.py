"""The fused attention backward on the GPU (sp.SparseAttentionBackwardPlan / sp.sparse_attention_backward /
sp.sparse_attention_function, csrc/attention_bwd.hip): the table of tests/attention_bwd_cases.py — the cases that
tests/test_attention_bwd_sim_cpu.py executes on the host — on the device, family by family and plan by plan, each result
against numpy's fp64 value as that module says (exact families equal, real data within its derived bound); every output
starts as a canary that must survive in its padding columns, and one canary element before and one behind every operand
must survive.  Then what only a device shows: two executes give the same bits, a side stream, one graph capture replayed on
new values, the one-shots, agreement with the call-by-call chain of DESIGN.md 3.14, rows and columns without entries, info()
of one- and multi-pass plans, and torch autograd on the dense masked formulation through sp.sparse_attention_function."""
import numpy as np
import pytest
import torch

import attention_bwd_cases as bc
import sim_runner as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH = {"f32": torch.float32, "f64": torch.float64}
RATIOS = []         # largest error / bound of every real case that ran (printed by the last test of the table)


def on_device(flat, shift, guard=1, fill=bc.CANARY):
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


def strided(full, ld, shift, fill):
    """`full` (rows x width) as a device matrix of leading dimension ld, (rows - 1) * ld + width elements long, its padding
    columns `fill`: (the rows x width view, the flat numpy it was made from, the guarded flat view)."""
    rows, width = full.shape
    flat = np.full((rows - 1) * ld + width if rows else 0, fill, dtype=full.dtype)
    for r in range(rows):
        flat[r * ld:r * ld + width] = full[r]
    v, g = on_device(flat, shift)
    return torch.as_strided(v, (rows, width), (ld, 1)) if rows else v.reshape(0, width), flat, g


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def execute_case(plan, c):
    """One case of the table on `plan`; returns (dQ, dK, dV, dbias) as numpy (None where not asked for), the canaries and
    the inputs checked."""
    T = bc.NP[c.val]
    n_rows, n_cols, Ap, Aj, _ = bc.csr(c)
    ops = bc.operands(c)
    ins = {}
    for name, pad in zip(bc.ORDER, c.pad[:5]):
        ins[name] = strided(ops[name], ops[name].shape[1] + pad, c.shift, np.nan)
    lse, glse = on_device(ops["lse"], c.shift)
    bias, gbias = on_device(ops["bias"], c.shift) if ops["bias"] is not None else (None, None)
    outs = {}
    for name, want, rows, width, pad in (("dQ", c.need[0], n_rows, c.d, c.pad[5]), ("dK", c.need[1], n_cols, c.d, c.pad[6]),
                                         ("dV", c.need[2], n_cols, c.dv, c.pad[7])):
        outs[name] = strided(np.full((rows, width), bc.CANARY, dtype=T), width + pad, c.shift, bc.CANARY) if want else (None, None, None)
    dbias, gdb = on_device(np.full(len(Aj), bc.CANARY, dtype=T), c.shift) if c.want_dbias else (None, None)
    plan.set_scale(c.scale)
    got = plan.execute(ins["Q"][0], ins["K"][0], ins["V"][0], ins["O"][0], ins["dO"][0], lse, bias=bias, dQ=outs["dQ"][0], dK=outs["dK"][0],
                       dV=outs["dV"][0], dbias=dbias, need=(False, False, False))
    res = [None if t is None else t.cpu().numpy() for t in got]       # (the copies synchronise)
    canary = T(bc.CANARY)
    for name, (v, h, g) in ins.items():
        gh = g.cpu().numpy()
        assert gh[0] == canary and gh[-1] == canary, "%s: a canary beside %s was written" % (c.name, name)
        assert same_bits(gh[1:-1], h), "%s: %s was written" % (c.name, name)
    for g, h, name in ((glse, ops["lse"], "lse"), (gbias, ops["bias"], "bias")):
        if g is not None:
            gh = g.cpu().numpy()
            assert gh[0] == canary and gh[-1] == canary and same_bits(gh[1:-1], h), "%s: %s or a canary beside it was written" % (c.name, name)
    for name, (v, h, g) in outs.items():
        if g is None:
            continue
        gh = g.cpu().numpy()
        assert gh[0] == canary and gh[-1] == canary, "%s: a canary beside %s was written" % (c.name, name)
        rows, width = v.shape
        ld = v.stride(0) if rows else width
        pad = np.ones(gh.size - 2, dtype=bool)
        for r in range(rows):
            pad[r * ld:r * ld + width] = False
        assert np.all(gh[1:-1][pad] == canary), "%s: a padding column of %s was written" % (c.name, name)
    if gdb is not None:
        gh = gdb.cpu().numpy()
        assert gh[0] == canary and gh[-1] == canary, "%s: a canary beside dbias was written" % c.name
    return tuple(res)


def make_plan(sp, c):
    n_rows, n_cols, Ap, Aj, _ = bc.csr(c)
    dAp, dAj = torch.from_numpy(Ap).to(DEV), torch.from_numpy(Aj).to(DEV)
    plan = sp.SparseAttentionBackwardPlan(n_rows, n_cols, len(Aj), dAp, dAj, TORCH[c.val], bc.D_MAX[c.val], bc.DV_MAX[c.val])
    bc.assert_geometry(plan.info(), c.val)
    return plan


def run_family(sp, name):
    """{case name: its outputs}, every case executed on its plan group's plan in table order and checked."""
    results = {}
    for group in sr.consecutive_runs(bc.family(name), bc.plan_key):
        plan = make_plan(sp, group[0])
        for c in group:
            results[c.name] = execute_case(plan, c)
            bc.check(c, *results[c.name], ratios=RATIOS)
        plan.destroy()
    return results


@pytest.mark.parametrize("family", [f for f in bc.FAMILIES if f not in ("alignment", "repeat", "need")])
def test_family(sp, family):
    run_family(sp, family)


def test_unaligned_operands_equal_aligned_ones_bit_for_bit(sp):
    results = run_family(sp, "alignment")
    for a, b in bc.alignment_pairs():
        for x, y in zip(results[a.name], results[b.name]):
            assert same_bits(x, y), b.name


def test_two_executes_give_equal_bits(sp):
    results = run_family(sp, "repeat")
    for a, b in bc.repeat_pairs():
        for x, y in zip(results[a.name], results[b.name]):
            assert same_bits(x, y), a.name


def test_each_output_alone_equals_the_all_three_execute_and_dbias_leaves_dq_unchanged(sp):
    results = run_family(sp, "need")
    for both, dq, dk, dv in bc.need_groups():
        assert results[dq.name][3] is None and results[both.name][3] is not None
        for alone, i in ((dq, 0), (dk, 1), (dv, 2)):
            assert same_bits(results[both.name][i], results[alone.name][i]), alone.name


def test_the_largest_error_over_bound_of_the_real_cases(sp):
    """Printed for DESIGN.md 3.15.2; above 1 the kernel or the derivation is wrong (each case has asserted it already)."""
    if not RATIOS:
        run_family(sp, "widths")
    print("attention backward: largest error / bound over %d outputs of real cases: %.3f" % (len(RATIOS), max(RATIOS)))
    assert max(RATIOS) <= 1.0


# ---- what only a device shows ------------------------------------------------------------------------------------------
def small_problem(val="f64", n_q=300, n_k=200, d=8, dv=8, seed=12, with_bias=True):
    """The shapes of test_sparse_attention_backward_never_leaves_the_library: a query and a key without edges."""
    rng = np.random.RandomState(seed)
    mask = rng.rand(n_q, n_k) < 4000.0 / (n_q * n_k)
    mask[7] = False
    mask[:, 11] = False
    rows, cols = np.nonzero(mask)
    Ap = np.concatenate(([0], np.cumsum(mask.sum(1)))).astype(np.int32)
    T = TORCH[val]
    t = lambda a: torch.from_numpy(a).to(DEV).to(T)
    Q, K, V, dO = t(rng.randn(n_q, d)), t(rng.randn(n_k, d)), t(rng.randn(n_k, dv)), t(rng.randn(n_q, dv))
    bias = t(rng.randn(len(rows))) if with_bias else None
    return dict(mask=mask, rows=rows, cols=cols, nnz=len(rows), Ap=torch.from_numpy(Ap).to(DEV), Aj=torch.from_numpy(cols.astype(np.int32)).to(DEV),
                Q=Q, K=K, V=V, dO=dO, bias=bias, n_q=n_q, n_k=n_k, d=d, dv=dv, T=T, scale=1.0 / np.sqrt(d))


def plans(sp, P):
    fwd = sp.SparseAttentionPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], P["T"], P["d"], P["dv"])
    bwd = sp.SparseAttentionBackwardPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], P["T"], P["d"], P["dv"])
    fwd.set_scale(P["scale"])
    bwd.set_scale(P["scale"])
    return fwd, bwd


def forward(fwd, P):
    lse = torch.empty(P["n_q"], dtype=P["T"], device=DEV)
    return fwd.execute(P["Q"], P["K"], P["V"], lse=lse, bias=P["bias"]), lse


def test_autograd_matches_the_dense_masked_formulation_and_repeats_its_bits(sp):
    P = small_problem()
    fwd, bwd = plans(sp, P)
    f = sp.sparse_attention_function(fwd, bwd)
    grads = []
    for _ in range(2):
        q, k, v, b = (t.clone().requires_grad_(True) for t in (P["Q"], P["K"], P["V"], P["bias"]))
        o = f(q, k, v, b)
        o.backward(P["dO"])
        grads.append((o.detach(), q.grad, k.grad, v.grad, b.grad))
    torch.cuda.synchronize()
    for x, y in zip(*grads):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    f64 = P["T"]
    q, k, v, b = (t.clone().requires_grad_(True) for t in (P["Q"], P["K"], P["V"], P["bias"]))
    m = torch.from_numpy(P["mask"]).to(DEV)
    dense_bias = torch.zeros(P["n_q"], P["n_k"], dtype=f64, device=DEV).index_put(
        (torch.from_numpy(P["rows"]).to(DEV), torch.from_numpy(P["cols"]).to(DEV)), b)
    scores = torch.where(m, (q @ k.t()) * P["scale"] + dense_bias, torch.full((), float("-inf"), dtype=f64, device=DEV))
    scores = torch.where(m.any(1, keepdim=True), scores, torch.zeros((), dtype=f64, device=DEV))   # a query without edges: no NaN
    p = torch.where(m, torch.softmax(scores, 1), torch.zeros((), dtype=f64, device=DEV))
    o = p @ v
    o.backward(P["dO"])
    for name, got, ref in zip(("O", "dQ", "dK", "dV", "dbias"), grads[0], (o.detach(), q.grad, k.grad, v.grad, b.grad)):
        err, top = float((got - ref).abs().max()), float(ref.abs().max())
        print("%s: max |got - ref| = %.3e, max |ref| = %.3e" % (name, err, top))
        assert top > 0.1 and err <= 1e-10 * top, name
    assert not grads[0][1][7].any() and not grads[0][2][11].any() and not grads[0][3][11].any()     # the lines without edges
    fwd.destroy()
    bwd.destroy()


def chain(sp, P, O_unused=None):
    """The call-by-call backward of DESIGN.md 3.14 on the parent's plans, P formed from one sddmm and lse."""
    n_q, n_k, nnz, T = P["n_q"], P["n_k"], P["nnz"], P["T"]
    sddmm = sp.SddmmPlan(n_q, n_k, nnz, P["Ap"], P["Aj"], T)
    soft = sp.RowSoftmaxPlan(n_q, n_k, nnz, P["Ap"], P["Aj"], T)
    soft.set_scale(P["scale"])
    spmm = sp.MultiPlan(n_q, n_k, nnz, P["Ap"], P["Aj"], T, max(P["d"], P["dv"]))
    spmm_t = sp.TransposedMultiPlan(n_q, n_k, nnz, P["Ap"], P["Aj"], T, max(P["d"], P["dv"]))
    rows = torch.from_numpy(P["rows"]).to(DEV)
    S = sddmm.execute(None, P["Q"], P["K"])
    prob = torch.exp(S * P["scale"] + (P["bias"] if P["bias"] is not None else 0) - P["lse"][rows])
    dP = sddmm.execute(None, P["dO"], P["V"])
    dV = spmm_t.execute(prob, P["dO"], torch.empty(n_k, P["dv"], dtype=T, device=DEV))
    dS = soft.backward(prob, dP)
    dQ = spmm.execute(dS, P["K"], torch.empty(n_q, P["d"], dtype=T, device=DEV))
    dK = spmm_t.execute(dS, P["Q"], torch.empty(n_k, P["d"], dtype=T, device=DEV))
    torch.cuda.synchronize()
    for p_ in (sddmm, soft, spmm, spmm_t):
        p_.destroy()
    return dQ, dK, dV


@pytest.mark.parametrize("side,off,val", [("A", "i32", "f32"), ("T", "i64", "f64"), ("T", "i32", "f32"), ("A", "i64", "f64")])
def test_agrees_with_the_call_by_call_chain_within_the_tables_bound(sp, side, off, val):
    """A real case of the table on the ragged structure: the fused outputs pass the table's check, the chain of DESIGN.md 3.14
    computes the same quantities from the same O and lse, and each lies within the case's derived bound of the fp64 value,
    so per element |fused - chain| <= 2 bound for dQ, dK and dV."""
    d, dv = bc.PAIRS[val][5]
    c = bc._case(bc.structures("ragged")[0], side, off, val, "real", 1, 0.125, d, dv, bc.PADS[0], 0, bc.NEED_ALL, True, "-chain")
    plan = make_plan(sp, c)
    fused = execute_case(plan, c)
    plan.destroy()
    bc.check(c, *fused)
    n_rows, n_cols, Ap, Aj, _ = bc.csr(c)
    ops = bc.operands(c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    P = dict(n_q=n_rows, n_k=n_cols, nnz=len(Aj), Ap=t(Ap), Aj=t(Aj), T=TORCH[val], d=c.d, dv=c.dv, scale=c.scale,
             rows=np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64))), Q=t(ops["Q"]), K=t(ops["K"]), V=t(ops["V"]), dO=t(ops["dO"]),
             bias=t(ops["bias"]), lse=t(ops["lse"]))
    bound = bc.expected(c)["bound"]
    for name, got, ref in zip(("dQ", "dK", "dV"), fused, chain(sp, P)):
        diff = np.abs(got.astype(np.float64) - ref.cpu().numpy().astype(np.float64))
        print("%s %s: largest |fused - chain| / (2 bound) = %.3f" % (c.name, name, float((diff / (2 * bound[name])).max())))
        assert np.all(diff <= 2 * bound[name]), name


def test_side_stream_and_graph_replay(sp):
    P = small_problem("f32", d=40, dv=36, seed=9)
    fwd, bwd = plans(sp, P)
    P["O"], P["lse"] = forward(fwd, P)
    torch.cuda.synchronize()
    args = lambda: (P["Q"], P["K"], P["V"], P["O"], P["dO"], P["lse"])
    base = [t.clone() for t in bwd.execute(*args(), bias=P["bias"], dbias=True)]
    torch.cuda.synchronize()        # one stream at a time per object: the executes share the plan's scratch
    # a side stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = bwd.execute(*args(), bias=P["bias"], dbias=True, stream=s)
    s.synchronize()
    for x, y in zip(base, side):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    # a graph capture replayed on new values
    outs = [torch.empty_like(t) for t in base]
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            bwd.execute(*args(), bias=P["bias"], dQ=outs[0], dK=outs[1], dV=outs[2], dbias=outs[3], stream=s)
    P["dO"].mul_(-0.5)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    again = bwd.execute(*args(), bias=P["bias"], dbias=True)
    torch.cuda.synchronize()
    for x, y in zip(again, outs):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    assert not same_bits(base[0].cpu().numpy(), outs[0].cpu().numpy())
    fwd.destroy()
    bwd.destroy()


@pytest.mark.parametrize("off,val", bc.ALL_TYPES)
def test_one_shots_equal_the_plan(sp, off, val):
    """sp.sparse_attention_backward and the C symbol mi355_spmv_attention_bwd_<off>_<val> called directly, against a plan's
    execute, bit for bit, for every (offset, value) pair."""
    import ctypes as C
    P = small_problem(val, d=20, dv=9, seed=3)
    if off == "i64":
        P["Ap"] = P["Ap"].to(torch.int64)
    fwd, bwd = plans(sp, P)
    P["O"], P["lse"] = forward(fwd, P)
    torch.cuda.synchronize()
    args = (P["Q"], P["K"], P["V"], P["O"], P["dO"], P["lse"])
    base = bwd.execute(*args, bias=P["bias"], dbias=True)
    once = sp.sparse_attention_backward(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], *args, bias=P["bias"], scale=P["scale"], dbias=True)
    direct = [torch.full_like(t, float("nan")) for t in base]
    ptr = lambda x: C.c_void_p(x.data_ptr())
    st = getattr(sp.capi.lib(), "mi355_spmv_attention_bwd_%s_%s" % (off, val))(
        P["n_q"], P["n_k"], P["nnz"], ptr(P["Ap"]), ptr(P["Aj"]), P["d"], P["dv"], ptr(P["Q"]), P["d"], ptr(P["K"]), P["d"], ptr(P["V"]), P["dv"],
        ptr(P["bias"]), C.c_double(P["scale"]), ptr(P["O"]), P["dv"], ptr(P["dO"]), P["dv"], ptr(P["lse"]), ptr(direct[0]), P["d"],
        ptr(direct[1]), P["d"], ptr(direct[2]), P["dv"], ptr(direct[3]), None)
    assert st == 0, sp.capi.lib().mi355_spmv_last_error().decode()
    torch.cuda.synchronize()
    for x, y, z in zip(base, once, direct):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy()) and same_bits(x.cpu().numpy(), z.cpu().numpy())
    assert float(base[0].abs().max()) > 0.01
    fwd.destroy()
    bwd.destroy()


def test_execute_refuses_widths_above_the_plans_maxima(sp):
    """The C execute on a live plan (the Python layer refuses first, and a one-shot's maxima are its widths)."""
    P = small_problem("f32")
    plan = sp.SparseAttentionBackwardPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], torch.float32, 8, 6)
    L = sp.capi.lib()
    x = torch.zeros(16, device=DEV)
    p = lambda: __import__("ctypes").c_void_p(x.data_ptr())
    for d, dv, word in ((9, 6, "d = 9 above d_max = 8"), (8, 7, "dv = 7 above dv_max = 6")):
        st = L.mi355_spmv_attention_bwd_execute(plan._h, d, dv, p(), 64, p(), 64, p(), 64, None, p(), 64, p(), 64, p(), p(), 64, p(), 64, p(), 64, None,
                                                None)
        assert st == 1 and word in L.mi355_spmv_last_error().decode(), (st, L.mi355_spmv_last_error().decode())
    plan.destroy()


def test_info_of_one_and_multi_pass_plans(sp):
    P = small_problem("f32")
    for d_max, dv_max in ((8, 8), (65, 33), (3, 100)):
        plan = sp.SparseAttentionBackwardPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], torch.float32, d_max, dv_max)
        info = plan.info()
        bc.assert_geometry(info, "f32")
        assert info["passes"] == {"dq": -(-d_max // 32), "dk": -(-d_max // 32), "dv": -(-dv_max // 32)}
        assert info["n_slices"] == -(-(P["n_q"] + P["nnz"]) // 1024) and info["n_slices_t"] == -(-(P["n_k"] + P["nnz"]) // 1024)
        assert info["held_bytes"] == 8 * P["nnz"] + 4 * (P["n_k"] + 1) and info["scratch_bytes"] > 0
        plan.destroy()
