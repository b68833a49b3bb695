"""The fused attention backward with 16-bit operands on the GPU (sp.SparseAttentionBackwardHalfPlan /
sp.sparse_attention_backward_half / sp.sparse_attention_function on a 16-bit pair, csrc/attention_bwd_half_kernel.hpp): the
table of tests/attention_bwd_half_cases.py — the cases that tests/test_attention_bwd_half_sim_cpu.py executes on the host —
on the device, family by family and plan by plan, each result as that module says (exact families bit for bit against the
exact value rounded once, real data within its derived bound); every output starts as a canary that must survive in its
padding columns, and one canary element before and one behind every operand must survive.  Unaligned operands give the
aligned bits, two executes the same bits, each output alone the all-three execute's, and on the exact families the 16-bit
outputs are narrow(the fp32 plan's outputs on the widened operands).  Then what only a device shows: a side stream, one
graph capture (a linear chain of launches) replayed on new values, the four one-shots, info() of one- and multi-pass plans,
execute refusals above the maxima, and torch autograd on the dense masked formulation through sp.sparse_attention_function
on a bf16 and an fp16 pair."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_bwd_half_cases as bh
import sim_runner as sr
from test_gpu_attention import DEV, on_device, same_bits
from test_gpu_attention_half import TORCH, bits16, canary_bits, signed

pytestmark = pytest.mark.gpu

RATIOS = []         # largest error / bound of every real case that ran (printed by the last test of the table)
F32_CANARY = np.float32(bh.CANARY)


def strided(full, ld, shift, fill, guard_fill):
    """`full` (rows x width, int16 patterns) as a device matrix of leading dimension ld, (rows - 1) * ld + width elements
    long, its padding columns `fill`: (the rows x width view, the flat numpy it was made from, the guarded flat view)."""
    rows, width = full.shape
    flat = np.full((rows - 1) * ld + width if rows else 0, fill, dtype=full.dtype)
    for r in range(rows):
        flat[r * ld:r * ld + width] = full[r]
    v, g = on_device(flat, shift, 1, guard_fill)
    return torch.as_strided(v, (rows, width), (ld, 1)) if rows else v.reshape(0, width), flat, g


def execute_case(plan, c):
    """One case of the table on `plan`; returns (dQ, dK, dV as uint16 patterns, dbias as float32) as numpy (None where not
    asked for), the canaries and the inputs checked."""
    T = TORCH[c.vec]
    can, nan = signed(canary_bits(c.vec)), signed(bh.NAN_BITS[c.vec])
    n_rows, n_cols, Ap, Aj, _ = bh.csr(c)
    ops = bh.operands(c)
    ins = {}
    for name, pad in zip(bh.ORDER, c.pad[:5]):
        ins[name] = strided(bits16(ops[name], c.vec), ops[name].shape[1] + pad, c.shift, nan, can)
    lse, glse = on_device(ops["lse"], c.shift, 1, F32_CANARY)
    bias, gbias = on_device(ops["bias"], c.shift, 1, F32_CANARY) if ops["bias"] is not None else (None, None)
    outs = {}
    for name, want, rows, width, pad in (("dQ", c.need[0], n_rows, c.d, c.pad[5]), ("dK", c.need[1], n_cols, c.d, c.pad[6]),
                                         ("dV", c.need[2], n_cols, c.dv, c.pad[7])):
        outs[name] = strided(np.full((rows, width), can, dtype=np.int16), width + pad, c.shift, can, can) if want else (None, None, None)
    dbias, gdb = on_device(np.full(len(Aj), F32_CANARY, dtype=np.float32), c.shift, 1, F32_CANARY) if c.want_dbias else (None, None)
    plan.set_scale(c.scale)
    view = lambda t: None if t is None else t.view(T)
    got = plan.execute(*(ins[n][0].view(T) for n in bh.ORDER), lse, bias=bias, dQ=view(outs["dQ"][0]), dK=view(outs["dK"][0]),
                       dV=view(outs["dV"][0]), dbias=dbias, need=(False, False, False))
    assert all(t is None or t.dtype is T for t in got[:3])
    res = [None if t is None else t.view(torch.int16).cpu().numpy().view(np.uint16) for t in got[:3]]       # (the copies synchronise)
    res.append(None if got[3] is None else got[3].cpu().numpy())
    for name, (v, h, g) in ins.items():
        gh = g.cpu().numpy()
        assert gh[0] == can and gh[-1] == can, "%s: a canary beside %s was written" % (c.name, name)
        assert same_bits(gh[1:-1], h), "%s: %s was written" % (c.name, name)
    for g, h, name in ((glse, ops["lse"], "lse"), (gbias, ops["bias"], "bias")):
        if g is not None:
            gh = g.cpu().numpy()
            assert gh[0] == F32_CANARY and gh[-1] == F32_CANARY and same_bits(gh[1:-1], h), "%s: %s or a canary beside it was written" % (c.name, name)
    for name, (v, h, g) in outs.items():
        if g is None:
            continue
        gh = g.cpu().numpy()
        assert gh[0] == can and gh[-1] == can, "%s: a canary beside %s was written" % (c.name, name)
        rows, width = v.shape
        ld = v.stride(0) if rows else width
        pad = np.ones(gh.size - 2, dtype=bool)
        for r in range(rows):
            pad[r * ld:r * ld + width] = False
        assert np.all(gh[1:-1][pad] == can), "%s: a padding column of %s was written" % (c.name, name)
    if gdb is not None:
        gh = gdb.cpu().numpy()
        assert gh[0] == F32_CANARY and gh[-1] == F32_CANARY, "%s: a canary beside dbias was written" % c.name
    return tuple(res)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_plan(sp, c):
    n_rows, n_cols, Ap, Aj, _ = bh.csr(c)
    plan = sp.SparseAttentionBackwardHalfPlan(n_rows, n_cols, len(Aj), dev(Ap), dev(Aj), TORCH[c.vec], bh.D_MAX, bh.DV_MAX)
    assert plan.val_dtype is torch.float32 and plan.vec_dtype is TORCH[c.vec]
    bh.assert_geometry(plan.info())
    return plan


def run_family(sp, name):
    """{case name: its outputs}, every case executed on its plan group's plan in table order and checked."""
    results = {}
    for group in sr.consecutive_runs(bh.family(name), bh.plan_key):
        plan = make_plan(sp, group[0])
        try:
            for c in group:
                results[c.name] = execute_case(plan, c)
                bh.check(c, *results[c.name], ratios=RATIOS)
        finally:
            plan.destroy()
    return results


@pytest.mark.parametrize("family", [f for f in bh.FAMILIES if f not in ("alignment", "repeat", "need", "fp32_pairs")])
def test_family(sp, family):
    run_family(sp, family)


def test_unaligned_operands_equal_aligned_ones_bit_for_bit(sp):
    results = run_family(sp, "alignment")
    for a, b in bh.alignment_pairs():
        for x, y in zip(results[a.name], results[b.name]):
            assert same_bits(x, y), b.name


def test_two_executes_give_equal_bits(sp):
    results = run_family(sp, "repeat")
    for a, b in bh.repeat_pairs():
        for x, y in zip(results[a.name], results[b.name]):
            assert same_bits(x, y), a.name


def test_each_output_alone_equals_the_all_three_execute_and_dbias_leaves_dq_unchanged(sp):
    results = run_family(sp, "need")
    for both, dq, dk, dv in bh.need_groups():
        assert results[dq.name][3] is None and results[both.name][3] is not None
        for alone, i in ((dq, 0), (dk, 1), (dv, 2)):
            assert same_bits(results[both.name][i], results[alone.name][i]), alone.name


def test_exact_families_equal_the_fp32_plans_outputs_narrowed(sp):
    """On data whose fp32 sums are exact, the 16-bit plan's outputs are narrow(the fp32 SparseAttentionBackwardPlan's
    outputs on the widened operands) bit for bit, whatever the two kernels' geometries; dbias equals outright."""
    results = run_family(sp, "fp32_pairs")
    for c in bh.family("fp32_pairs"):
        n_rows, n_cols, Ap, Aj, _ = bh.csr(c)
        ops = bh.operands(c)
        p32 = sp.SparseAttentionBackwardPlan(n_rows, n_cols, len(Aj), dev(Ap), dev(Aj), torch.float32, c.d, c.dv)
        p32.set_scale(c.scale)
        got = p32.execute(*(dev(ops[n]) for n in bh.ORDER), dev(ops["lse"]), bias=dev(ops["bias"]), dbias=True)
        torch.cuda.synchronize()
        p32.destroy()
        for name, x16, x32 in zip(("dQ", "dK", "dV"), results[c.name], got):
            want = bh.to_bits(x32.cpu().numpy(), c.vec).reshape(x16.shape)
            assert bh.same_but_zero_sign(x16, want).all(), "%s: %s" % (c.name, name)
        assert np.array_equal(results[c.name][3], got[3].cpu().numpy()), c.name


def test_the_largest_error_over_bound_of_the_real_cases(sp):
    """Printed for DESIGN.md 3.15.3; above 1 the kernel or the derivation is wrong (each case has asserted it already)."""
    if not RATIOS:
        run_family(sp, "widths")
    print("16-bit attention backward: largest error / bound over %d outputs of real cases: %.3f" % (len(RATIOS), max(RATIOS)))
    assert max(RATIOS) <= 1.0


# ---- what only a device shows ------------------------------------------------------------------------------------------
def small_problem(vec="bf16", n_q=300, n_k=200, d=8, dv=8, seed=12, off="i32"):
    """A query and a key without edges; Q, K, V, dO in the 16-bit type, bias in float32."""
    rng = np.random.RandomState(seed)
    mask = rng.rand(n_q, n_k) < 4000.0 / (n_q * n_k)
    mask[7] = False
    mask[:, 11] = False
    rows, cols = np.nonzero(mask)
    Ap = np.concatenate(([0], np.cumsum(mask.sum(1)))).astype(np.int32 if off == "i32" else np.int64)
    T = TORCH[vec]
    t = lambda a: torch.from_numpy(a).to(DEV).to(T)
    Q, K, V, dO = t(rng.randn(n_q, d)), t(rng.randn(n_k, d)), t(rng.randn(n_k, dv)), t(rng.randn(n_q, dv))
    bias = torch.from_numpy(rng.randn(len(rows)).astype(np.float32)).to(DEV)
    return dict(mask=mask, rows=rows, cols=cols, nnz=len(rows), Ap=dev(Ap), Aj=dev(cols.astype(np.int32)), Q=Q, K=K, V=V, dO=dO, bias=bias,
                n_q=n_q, n_k=n_k, d=d, dv=dv, T=T, scale=1.0 / np.sqrt(d))


def plans(sp, P):
    fwd = sp.SparseAttentionPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], torch.float32, P["d"], P["dv"], vec_dtype=P["T"])
    bwd = sp.SparseAttentionBackwardHalfPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], P["T"], P["d"], P["dv"])
    fwd.set_scale(P["scale"])
    bwd.set_scale(P["scale"])
    return fwd, bwd


def forward(fwd, P):
    lse = torch.empty(P["n_q"], dtype=torch.float32, device=DEV)
    return fwd.execute(P["Q"], P["K"], P["V"], lse=lse, bias=P["bias"]), lse


def raw(t):
    return t.view(torch.int16).cpu().numpy() if t.dtype in (torch.float16, torch.bfloat16) else t.cpu().numpy()


def test_side_stream_and_graph_replay(sp):
    P = small_problem("bf16", d=72, dv=36, seed=9)
    fwd, bwd = plans(sp, P)
    P["O"], P["lse"] = forward(fwd, P)
    torch.cuda.synchronize()
    args = lambda: (P["Q"], P["K"], P["V"], P["O"], P["dO"], P["lse"])
    base = [t.clone() for t in bwd.execute(*args(), bias=P["bias"], dbias=True)]
    torch.cuda.synchronize()        # one stream at a time per object: the executes share the plan's scratch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = bwd.execute(*args(), bias=P["bias"], dbias=True, stream=s)
    s.synchronize()
    for x, y in zip(base, side):
        assert same_bits(raw(x), raw(y))
    # a graph capture (delta, three roles with two DQ / DK passes, their fix-ups: one linear chain) replayed on new values
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
        assert same_bits(raw(x), raw(y))
    assert not same_bits(raw(base[0]), raw(outs[0]))
    fwd.destroy()
    bwd.destroy()


@pytest.mark.parametrize("off,vec", bh.TYPES)
def test_one_shots_equal_the_plan(sp, off, vec):
    """sp.sparse_attention_backward_half and the C symbol mi355_spmv_attention_bwd_half_<off>_<vec> called directly, against a
    plan's execute, bit for bit, for every (offset, 16-bit type) pair."""
    P = small_problem(vec, d=20, dv=9, seed=3, off=off)
    fwd, bwd = plans(sp, P)
    P["O"], P["lse"] = forward(fwd, P)
    torch.cuda.synchronize()
    args = (P["Q"], P["K"], P["V"], P["O"], P["dO"], P["lse"])
    base = bwd.execute(*args, bias=P["bias"], dbias=True)
    once = sp.sparse_attention_backward_half(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], *args, bias=P["bias"], scale=P["scale"], dbias=True)
    assert once[0].dtype is P["T"] and once[3].dtype is torch.float32
    direct = [torch.zeros_like(t) for t in base]
    ptr = lambda x: C.c_void_p(x.data_ptr())
    st = getattr(sp.capi.lib(), "mi355_spmv_attention_bwd_half_%s_%s" % (off, vec))(
        P["n_q"], P["n_k"], P["nnz"], ptr(P["Ap"]), ptr(P["Aj"]), P["d"], P["dv"], ptr(P["Q"]), P["d"], ptr(P["K"]), P["d"], ptr(P["V"]), P["dv"],
        ptr(P["bias"]), C.c_double(P["scale"]), ptr(P["O"]), P["dv"], ptr(P["dO"]), P["dv"], ptr(P["lse"]), ptr(direct[0]), P["d"],
        ptr(direct[1]), P["d"], ptr(direct[2]), P["dv"], ptr(direct[3]), None)
    assert st == 0, sp.capi.lib().mi355_spmv_last_error().decode()
    torch.cuda.synchronize()
    for x, y, z in zip(base, once, direct):
        assert same_bits(raw(x), raw(y)) and same_bits(raw(x), raw(z))
    assert float(base[0].float().abs().max()) > 0.01
    fwd.destroy()
    bwd.destroy()


def test_execute_refuses_widths_above_the_plans_maxima(sp):
    """The C execute on a live 16-bit plan (the Python layer refuses first, and a one-shot's maxima are its widths)."""
    P = small_problem("f16")
    plan = sp.SparseAttentionBackwardHalfPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], torch.float16, 8, 6)
    L = sp.capi.lib()
    x = torch.zeros(16, device=DEV)
    p = lambda: C.c_void_p(x.data_ptr())
    for d, dv, word in ((9, 6, "d = 9 above d_max = 8"), (8, 7, "dv = 7 above dv_max = 6")):
        st = L.mi355_spmv_attention_bwd_execute(plan._h, d, dv, p(), 64, p(), 64, p(), 64, None, p(), 64, p(), 64, p(), p(), 64, p(), 64, p(), 64, None,
                                                None)
        assert st == 1 and word in L.mi355_spmv_last_error().decode(), (st, L.mi355_spmv_last_error().decode())
    plan.destroy()


def test_info_of_one_and_multi_pass_plans(sp):
    P = small_problem("bf16")
    for d_max, dv_max in ((8, 8), (64, 64), (65, 33), (3, 130)):
        plan = sp.SparseAttentionBackwardHalfPlan(P["n_q"], P["n_k"], P["nnz"], P["Ap"], P["Aj"], torch.bfloat16, d_max, dv_max)
        info = plan.info()
        bh.assert_geometry(info)
        assert info["passes"] == {"dq": -(-d_max // 64), "dk": -(-d_max // 64), "dv": -(-dv_max // 64)}
        assert info["n_slices"] == -(-(P["n_q"] + P["nnz"]) // 1024) and info["n_slices_t"] == -(-(P["n_k"] + P["nnz"]) // 1024)
        assert info["held_bytes"] == 8 * P["nnz"] + 4 * (P["n_k"] + 1) and info["scratch_bytes"] > 0
        plan.destroy()


def unique_structure():
    """A structure without repeated entries (the dense formulation has one score per (row, column)): 600 x 97, rows of 0 ..
    60 entries that cross slices, a row and a column without entries; its arrays are handed to the tables' csr()."""
    import attention_cases as ac
    rng = np.random.RandomState(5)
    mask = rng.rand(600, 97) < rng.rand(600, 1) * 0.6
    mask[7] = False
    mask[:, 11] = False
    m = bh.bc.Matrix("autograd_unique", "autograd", tuple(int(x) for x in mask.sum(1)), 97, 977)
    Ap = np.concatenate(([0], np.cumsum(mask.sum(1)))).astype(np.int32)
    ac._csr.setdefault((m.name, "i32"), (Ap, np.nonzero(mask)[1].astype(np.int32)))
    return m


@pytest.mark.parametrize("vec,side", [("bf16", "A"), ("f16", "T")])
def test_autograd_through_a_16_bit_pair_against_the_dense_masked_formulation(sp, vec, side):
    """A real case on a structure without repeated entries through sp.sparse_attention_function: O is the library's own 16-bit
    forward, the reference torch autograd on the dense masked formulation in fp64 on the widened inputs, the bound the
    table's on (O', lse') plus attention_bwd_half_cases.autograd_extra()."""
    T = TORCH[vec]
    d, dv = bh.PAIRS[4]
    c = bh._case(unique_structure(), side, "i32", vec, "real", 1, 0.125, d, dv, bh.PADS[0], 0, bh.NEED_ALL, True, "-autograd")
    n_rows, n_cols, Ap, Aj, _ = bh.csr(c)
    ops = bh.operands(c)
    dAp, dAj = dev(Ap), dev(Aj)
    fwd = sp.SparseAttentionPlan(n_rows, n_cols, len(Aj), dAp, dAj, torch.float32, c.d, c.dv, vec_dtype=T)
    bwd = sp.SparseAttentionBackwardHalfPlan(n_rows, n_cols, len(Aj), dAp, dAj, T, c.d, c.dv)
    fwd.set_scale(c.scale)
    bwd.set_scale(c.scale)
    f = sp.sparse_attention_function(fwd, bwd)
    h = lambda a: dev(bits16(a, vec)).view(T)
    q, k, v = (h(ops[n]).requires_grad_(True) for n in ("Q", "K", "V"))
    b = dev(ops["bias"]).requires_grad_(True)
    o = f(q, k, v, b)
    assert o.dtype is T
    o.backward(h(ops["dO"]))
    torch.cuda.synchronize()
    assert q.grad.dtype is T and k.grad.dtype is T and v.grad.dtype is T and b.grad.dtype is torch.float32
    # the true forward and gradient: dense, masked, fp64, on the widened inputs
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))
    mask = np.zeros((n_rows, n_cols), dtype=bool)
    mask[rows, Aj] = True
    assert mask.sum() == len(Aj), "the dense formulation needs a structure without repeated entries"
    f64 = torch.float64
    q2, k2, v2, b2 = (dev(ops[n].astype(np.float64)).requires_grad_(True) for n in ("Q", "K", "V", "bias"))
    m = dev(mask)
    dense_bias = torch.zeros(n_rows, n_cols, dtype=f64, device=DEV).index_put((dev(rows), dev(Aj.astype(np.int64))), b2)
    scores = torch.where(m, (q2 @ k2.t()) * float(np.float32(c.scale)) + dense_bias, torch.full((), float("-inf"), dtype=f64, device=DEV))
    scores = torch.where(m.any(1, keepdim=True), scores, torch.zeros((), dtype=f64, device=DEV))
    p = torch.where(m, torch.softmax(scores, 1), torch.zeros((), dtype=f64, device=DEV))
    o2 = p @ v2
    o2.backward(dev(ops["dO"].astype(np.float64)))
    lse_true = torch.where(m.any(1), torch.logsumexp(scores, 1), torch.full((), float("-inf"), dtype=f64, device=DEV)).detach().cpu().numpy()
    # the case whose operands O and lse are what the backward was given: the saved forward outputs
    lse = torch.empty(n_rows, dtype=torch.float32, device=DEV)
    O = fwd.execute(q.detach(), k.detach(), v.detach(), lse=lse, bias=b.detach())
    assert same_bits(raw(O), raw(o.detach()))
    c2 = bh.with_forward(c, raw(O).view(np.uint16), lse.cpu().numpy())
    extra = bh.autograd_extra(c2, o2.detach().cpu().numpy(), lse_true)
    ex, true = bh.expected(c2), {}
    for name, ref in (("dQ", q2.grad), ("dK", k2.grad), ("dV", v2.grad), ("dbias", b2.grad)):
        gap = np.abs(ex[name] - ref.cpu().numpy())
        print("%s %s: the forward's terms: largest |reference on (O', lse') - true gradient| / extra = %.3f" % (
            c.name, name, float((gap / np.maximum(extra[name], 1e-300)).max())))
        true[name] = ref.cpu().numpy()      # the check below is against the TRUE gradient
    ratios = []
    bh.check(c2, raw(q.grad).view(np.uint16), raw(k.grad).view(np.uint16), raw(v.grad).view(np.uint16), b.grad.cpu().numpy(), ratios=ratios, extra=extra, want=true)
    print("%s: largest error / bound against the dense fp64 gradient: %.3f" % (c.name, max(ratios)))
    fwd.destroy()
    bwd.destroy()
