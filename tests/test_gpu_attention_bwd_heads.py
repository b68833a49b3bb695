"""The heads of sparse attention in one call on the GPU, backward (sp.SparseAttentionBackwardPlan / ...HalfPlan with 3-D
operands, mi355_spmv_attention_bwd_execute_heads): the backward cases of tests/attention_heads_cases.py — those that
tests/test_attention_bwd_heads_sim_cpu.py executes on the host.  The expected value of head h is the 2-D execute of the same
plan on head h's views, bit for bit; outputs start as a canary that must survive outside every head's rows x width and
around every buffer; reserve_heads goes up and down between the executes of a plan and never touches the held transpose.
Then: a captured graph replayed, the refusals of a real object, and sp.sparse_attention_function on 3-D operands — forward
and gradients equal, bit for bit, the per-head 2-D function on each head, and with an expanded K the gradient of K is the sum
of the per-head gradients to the rounding of that sum."""
import numpy as np
import pytest
import torch

import attention_heads_cases as hd
import attention_heads_device as dv
from attention_heads_device import small

pytestmark = pytest.mark.gpu

OUTS = ("dQ", "dK", "dV", "dbias")


def make_plan(sp, c, Ap, Aj):
    n_rows, n_cols, nnz = hd.sizes(c)
    if c.val in ("f16", "bf16"):
        return sp.SparseAttentionBackwardHalfPlan(n_rows, n_cols, nnz, Ap, Aj, dv.TORCH[c.val], hd.D_MAX, hd.DV_MAX)
    return sp.SparseAttentionBackwardPlan(n_rows, n_cols, nnz, Ap, Aj, dv.TORCH[c.val], hd.D_MAX, hd.DV_MAX)


def asked(c):
    return [n for n, want in zip(OUTS, c.need + (c.want_dbias,)) if want]


def run_heads(plan, c, ins, outs):
    H = c.H
    plan.execute(*[ins[n].view3(H) for n in ("Q", "K", "V", "O", "dO")], ins["lse"].vectors(H),
                 bias=None if ins["bias"] is None else ins["bias"].vectors(H), need=(False, False, False),
                 **{n: (outs[n].vectors(H) if n == "dbias" else outs[n].view3(H)) for n in outs})


def run_single(plan, c, ins, outs):
    H = c.H
    mats = {n: ins[n].view3(H) for n in ("Q", "K", "V", "O", "dO")}
    for h in range(H):
        bias = None if ins["bias"] is None else ins["bias"].vectors(H)
        plan.execute(*[mats[n][:, h] for n in ("Q", "K", "V", "O", "dO")], ins["lse"].vectors(H)[h],
                     bias=bias if bias is None or bias.dim() == 1 else bias[h], need=(False, False, False),
                     **{n: (outs[n].vectors(H)[h] if n == "dbias" else outs[n].view3(H)[:, h]) for n in outs})


@pytest.mark.parametrize("structure", hd.STRUCTURES)
def test_every_head_equals_the_single_head_execute_bit_for_bit(sp, structure):
    cases = [c for c in hd.backward_cases() if c.matrix is hd.structures()[structure]]
    plans = {}
    for c in cases:
        if hd.plan_key(c) not in plans:
            Ap, Aj = dv.structure_on_device(c)
            plans[hd.plan_key(c)] = make_plan(sp, c, Ap, Aj)
        plan = plans[hd.plan_key(c)]
        torch.cuda.synchronize()
        held = plan.info()["held_bytes"]
        plan.reserve_heads(c.H_max)
        assert plan.n_heads_max == c.H_max and plan.info()["held_bytes"] == held
        plan.set_scale(0.25)
        ins = dv.inputs(c, ("Q", "K", "V", "O", "dO"))
        sets = [{n: dv.output(c, n) for n in asked(c)} for _ in range(3)]
        run_heads(plan, c, ins, sets[0])
        run_single(plan, c, ins, sets[1])
        run_heads(plan, c, ins, sets[2])            # two executes give the same bits
        torch.cuda.synchronize()
        for n in asked(c):
            dv.assert_equal_heads(c, n, sets[0][n], sets[1][n])
            assert dv.same_bits(sets[0][n].bits(), sets[2][n].bits()), (c.name, n)
        for name, b in ins.items():
            if b is not None:
                assert dv.same_bits(b.bits()[dv.GUARD:dv.GUARD + b.elems], b.host), "%s: %s was written" % (c.name, name)
    for plan in plans.values():
        plan.destroy()


def plans_of(sp, P, H):
    fwd = sp.SparseAttentionPlan(P["n_rows"], P["n_cols"], P["nnz"], P["Ap"], P["Aj"], P["val"], P["d"], P["dv"], n_heads_max=H)
    bwd = sp.SparseAttentionBackwardPlan.with_heads(H, P["n_rows"], P["n_cols"], P["nnz"], P["Ap"], P["Aj"], P["val"], P["d"], P["dv"])
    fwd.set_scale(0.25)
    bwd.set_scale(0.25)
    return fwd, bwd


def test_a_captured_graph_replays_the_eager_bits_and_a_real_object_refuses_overlaps(sp):
    P = small(sp, seed=11)
    H = P["H"]
    fwd, bwd = plans_of(sp, P, H)
    lse = torch.empty((H, P["n_rows"]), dtype=P["val"], device=dv.DEV)
    O = fwd.execute(P["Q"], P["K"], P["V"], lse=lse, bias=P["bias"])
    dO = torch.ones_like(O) * 0.5
    eager = bwd.execute(P["Q"], P["K"], P["V"], O, dO, lse, bias=P["bias"], dbias=True)
    torch.cuda.synchronize()
    outs = [torch.zeros_like(t) for t in eager]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):         # a single linear capture: no parallel branches
            bwd.execute(P["Q"], P["K"], P["V"], O, dO, lse, bias=P["bias"], dQ=outs[0], dK=outs[1], dV=outs[2], dbias=outs[3], stream=s)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, outs):
        assert dv.same_bits(x.cpu().numpy(), y.cpu().numpy())
    # the refusals of a real object: all before any launch
    flat = torch.zeros(P["n_cols"] * H * P["d"], dtype=P["val"], device=dv.DEV)
    bad = torch.as_strided(flat, (P["n_cols"], H, P["d"]), (H * P["d"], P["d"] - 1, 1))
    with pytest.raises(RuntimeError, match="stride dk"):
        bwd.execute(P["Q"], P["K"], P["V"], O, dO, lse, dK=bad, need=(False, False, False))
    short = torch.as_strided(torch.zeros(H * P["nnz"], dtype=P["val"], device=dv.DEV), (H, P["nnz"]), (P["nnz"] - 1, 1))
    with pytest.raises(RuntimeError, match="stride dbias"):
        bwd.execute(P["Q"], P["K"], P["V"], O, dO, lse, dbias=short)
    bwd.reserve_heads(H - 1)
    with pytest.raises(RuntimeError, match="n_heads_max"):
        bwd.execute(P["Q"], P["K"], P["V"], O, dO, lse)
    fwd.destroy()
    bwd.destroy()


def test_the_3d_function_equals_the_per_head_2d_function_bit_for_bit(sp):
    P = small(sp, seed=13)
    H = P["H"]
    fwd, bwd = plans_of(sp, P, H)
    f = sp.sparse_attention_function(fwd, bwd)
    leaf = lambda t: t.clone().requires_grad_(True)
    Q, K, V, bias = leaf(P["Q"]), leaf(P["K"]), leaf(P["V"]), leaf(P["bias"])
    O = f(Q, K, V, bias)
    W = torch.linspace(-1, 1, O.numel(), dtype=P["val"], device=dv.DEV).reshape(O.shape)
    (O * W).sum().backward()
    torch.cuda.synchronize()
    assert O.shape == (P["n_rows"], H, P["dv"])
    for h in range(H):
        q, k, v, b = leaf(P["Q"][:, h]), leaf(P["K"][:, h]), leaf(P["V"][:, h]), leaf(P["bias"][h])
        o = f(q, k, v, b)
        (o * W[:, h]).sum().backward()
        torch.cuda.synchronize()
        for name, got, ref in (("O", O[:, h], o), ("dQ", Q.grad[:, h], q.grad), ("dK", K.grad[:, h], k.grad), ("dV", V.grad[:, h], v.grad),
                               ("dbias", bias.grad[h], b.grad)):
            assert dv.same_bits(got.detach().cpu().numpy(), ref.detach().cpu().numpy()), (name, h)
    fwd.destroy()
    bwd.destroy()


def test_an_expanded_k_gets_the_sum_of_the_heads_gradients(sp):
    """K of one head expanded to H: .contiguous() in the function materialises it, and autograd's backward of expand sums
    the heads' gradients — K.grad is the sum over h of the per-head dK, to the rounding of that sum: H - 1 additions of
    fp64 values, each within 2^-53 of the running sum's magnitude, so H eps sum_h |dK_h| bounds it in any order."""
    P = small(sp, val=torch.float64, seed=17)
    H = P["H"]
    fwd, bwd = plans_of(sp, P, H)
    f = sp.sparse_attention_function(fwd, bwd)
    K1 = P["K"][:, :1].clone().requires_grad_(True)
    Q, V = P["Q"].clone().requires_grad_(True), P["V"].clone().requires_grad_(True)
    O = f(Q, K1.expand(-1, H, -1), V)
    W = torch.linspace(-1, 1, O.numel(), dtype=P["val"], device=dv.DEV).reshape(O.shape)
    (O * W).sum().backward()
    per_head = []
    for h in range(H):
        k = K1[:, 0].detach().clone().requires_grad_(True)
        (f(P["Q"][:, h].clone(), k, P["V"][:, h].clone()) * W[:, h]).sum().backward()
        per_head.append(k.grad)
    torch.cuda.synchronize()
    total = torch.stack(per_head).sum(0)
    bound = H * np.finfo(np.float64).eps * torch.stack(per_head).abs().sum(0) + np.finfo(np.float64).tiny
    err = (K1.grad[:, 0] - total).abs()
    print("largest |K.grad - sum of the heads| / bound = %.3g" % float((err / bound).max()))
    assert bool((err <= bound).all())
    fwd.destroy()
    bwd.destroy()
