"""The heads of sparse attention in one call on the GPU, forward (sp.SparseAttentionPlan with 3-D operands,
mi355_spmv_attention_execute_heads): the forward cases of tests/attention_heads_cases.py — those that
tests/test_attention_heads_sim_cpu.py executes on the host — through the plans of both storage types.  The expected value of
head h is the 2-D execute of the same plan on head h's views, bit for bit; outputs start as a canary that must survive
outside every head's rows x width and around every buffer.  reserve_heads goes up and down between the executes of a plan.
Then: two executes give the same bits, one captured graph of one heads execute replayed, a shared K and V from expand, and
sp.sparse_attention_function on 3-D operands against the per-head 2-D function."""
import numpy as np
import pytest
import torch

import attention_heads_cases as hd
import attention_heads_device as dv
from attention_heads_device import small

pytestmark = pytest.mark.gpu


def make_plan(sp, c, Ap, Aj):
    n_rows, n_cols, nnz = hd.sizes(c)
    half = c.val in ("f16", "bf16")
    return sp.SparseAttentionPlan(n_rows, n_cols, nnz, Ap, Aj, dv.TORCH[hd.SIDE[c.val]], hd.D_MAX, hd.DV_MAX, vec_dtype=dv.TORCH[c.val] if half else None)


def run_heads(plan, c, ins, O, lse):
    plan.execute(ins["Q"].view3(c.H), ins["K"].view3(c.H), ins["V"].view3(c.H), out=O.view3(c.H), lse=None if lse is None else lse.vectors(c.H),
                 bias=None if ins["bias"] is None else ins["bias"].vectors(c.H))


def run_single(plan, c, ins, O, lse):
    Q, K, V, O3 = ins["Q"].view3(c.H), ins["K"].view3(c.H), ins["V"].view3(c.H), O.view3(c.H)
    for h in range(c.H):
        bias = None if ins["bias"] is None else ins["bias"].vectors(c.H)
        plan.execute(Q[:, h], K[:, h], V[:, h], out=O3[:, h], lse=None if lse is None else lse.vectors(c.H)[h],
                     bias=bias if bias is None or bias.dim() == 1 else bias[h])


@pytest.mark.parametrize("structure", hd.STRUCTURES)
def test_every_head_equals_the_single_head_execute_bit_for_bit(sp, structure):
    cases = [c for c in hd.forward_cases() if c.matrix is hd.structures()[structure]]
    plans, scratch = {}, {}
    for c in cases:
        if hd.plan_key(c) not in plans:
            Ap, Aj = dv.structure_on_device(c)
            plans[hd.plan_key(c)] = make_plan(sp, c, Ap, Aj)
        plan = plans[hd.plan_key(c)]
        torch.cuda.synchronize()
        plan.reserve_heads(c.H_max)                 # up and down between the executes of one plan
        assert plan.n_heads_max == c.H_max
        sizes = scratch.setdefault(hd.plan_key(c), {})
        assert sizes.setdefault(c.H_max, plan.info()["scratch_bytes"]) == plan.info()["scratch_bytes"]
        plan.set_scale(0.25)
        ins = dv.inputs(c, ("Q", "K", "V"))
        outs = [(dv.output(c, "O"), dv.output(c, "lse") if c.want_lse else None) for _ in range(3)]
        run_heads(plan, c, ins, *outs[0])
        run_single(plan, c, ins, *outs[1])
        run_heads(plan, c, ins, *outs[2])           # two executes give the same bits
        torch.cuda.synchronize()
        dv.assert_equal_heads(c, "O", outs[0][0], outs[1][0])
        assert dv.same_bits(outs[0][0].bits(), outs[2][0].bits()), c.name
        if c.want_lse:
            dv.assert_equal_heads(c, "lse", outs[0][1], outs[1][1])
            assert dv.same_bits(outs[0][1].bits(), outs[2][1].bits()), c.name
        for name in ("Q", "K", "V", "bias"):
            if ins[name] is not None:
                assert dv.same_bits(ins[name].bits()[dv.GUARD:dv.GUARD + ins[name].elems], ins[name].host), "%s: %s was written" % (c.name, name)
        if c.H > 1 and c.bias == "per_head":
            r = hd.whole_masked_row(c)
            assert not np.any(outs[0][0].head(1)[r]), "%s: the row masked whole in head 1 is not +0 there" % c.name
            if c.want_lse:
                row = np.array([outs[0][1].head(h).view(hd.NP[hd.SIDE[c.val]])[0, r] for h in range(c.H)])
                assert np.isneginf(row[1]) and np.all(np.isfinite(np.delete(row, 1))), c.name
    for sizes in scratch.values():                  # scratch_bytes grows with the reserve, one head's share per head
        assert [sizes[h] for h in sorted(sizes)] == sorted(sizes.values()) and len(set(sizes.values())) == len(sizes)
    for plan in plans.values():
        plan.destroy()


def test_a_captured_graph_of_one_heads_execute_replays_the_eager_bits(sp):
    P = small(sp)
    plan = sp.SparseAttentionPlan(P["n_rows"], P["n_cols"], P["nnz"], P["Ap"], P["Aj"], P["val"], P["d"], P["dv"], n_heads_max=P["H"])
    plan.set_scale(0.25)
    lse = torch.empty((P["H"], P["n_rows"]), dtype=P["val"], device=dv.DEV)
    eager = plan.execute(P["Q"], P["K"], P["V"], lse=lse, bias=P["bias"])
    torch.cuda.synchronize()
    out, lse2 = torch.zeros_like(eager), torch.zeros_like(lse)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):         # a single linear capture: no parallel branches
            plan.execute(P["Q"], P["K"], P["V"], out=out, lse=lse2, bias=P["bias"], stream=s)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert dv.same_bits(eager.cpu().numpy(), out.cpu().numpy()) and dv.same_bits(lse.cpu().numpy(), lse2.cpu().numpy())
    assert out.shape == (P["n_rows"], P["H"], P["dv"]) and out.is_contiguous()
    plan.destroy()


def test_expanded_k_and_v_and_a_head_major_q(sp):
    """One K and V for every head (multi-query attention) from expand, and Q head-major through permute: each head equals
    the 2-D execute."""
    P = small(sp, seed=5)
    plan = sp.SparseAttentionPlan(P["n_rows"], P["n_cols"], P["nnz"], P["Ap"], P["Aj"], P["val"], P["d"], P["dv"], n_heads_max=P["H"] + 1)
    K1, V1 = P["K"][:, :1].contiguous(), P["V"][:, :1].contiguous()
    Qhm = P["Q"].permute(1, 0, 2).contiguous()          # (H, n, d)
    out = plan.execute(Qhm.permute(1, 0, 2), K1.expand(-1, P["H"], -1), V1.expand(-1, P["H"], -1), bias=P["bias"][0])
    torch.cuda.synchronize()
    for h in range(P["H"]):
        ref = plan.execute(Qhm[h], K1[:, 0], V1[:, 0], bias=P["bias"][0])
        torch.cuda.synchronize()
        assert dv.same_bits(out[:, h].cpu().numpy(), ref.cpu().numpy()), h
    with pytest.raises(RuntimeError, match="n_heads_max"):
        plan.execute(P["Q"].repeat(1, 2, 1), P["K"].repeat(1, 2, 1), P["V"].repeat(1, 2, 1))
    plan.destroy()


def test_execute_heads_refuses_overlapping_outputs_of_a_real_object(sp):
    P = small(sp, seed=6)
    plan = sp.SparseAttentionPlan(P["n_rows"], P["n_cols"], P["nnz"], P["Ap"], P["Aj"], P["val"], P["d"], P["dv"], n_heads_max=P["H"])
    flat = torch.zeros(P["n_rows"] * P["H"] * P["dv"], dtype=P["val"], device=dv.DEV)
    overlapping = torch.as_strided(flat, (P["n_rows"], P["H"], P["dv"]), (P["H"] * P["dv"], P["dv"] - 1, 1))
    with pytest.raises(RuntimeError, match="stride o"):
        plan.execute(P["Q"], P["K"], P["V"], out=overlapping)
    lse = torch.as_strided(torch.zeros(P["H"] * P["n_rows"], dtype=P["val"], device=dv.DEV), (P["H"], P["n_rows"]), (P["n_rows"] - 1, 1))
    with pytest.raises(RuntimeError, match="stride lse"):
        plan.execute(P["Q"], P["K"], P["V"], lse=lse)
    plan.destroy()
