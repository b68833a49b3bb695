"""torch.autograd over the fused sparse attention: the forward of a SparseAttentionPlan and the backward of a
SparseAttentionBackwardPlan as one differentiable call.  No kernels here: both plans are capi.py's."""
import torch


def sparse_attention_function(fwd_plan, bwd_plan):
    """f(Q, K, V, bias=None) -> O = softmax(scale * Q K^T + bias, on the stored entries of A) V, differentiable in Q, K, V and
    (where it requires grad) bias.  The forward saves Q, K, V, bias, O and lse — nothing of nnz size but the caller's own
    bias.  Both plans are made on the same structure and value type, and the caller sets the same scale on both.  A 16-bit
    pair — SparseAttentionPlan(vec_dtype=) with a SparseAttentionBackwardHalfPlan of the same vec_dtype — takes Q, K, V in
    that type and returns O and the gradients in it; bias, lse and dbias are float32.
    Heads: where both plans reserve at least H heads (n_heads_max), Q, K and V may be 3-D, shaped (rows, H, width), and bias
    (H, nnz) or (nnz,) shared; O comes back as (n_rows, H, dv), and O and lse are saved per head ((H, n_rows) for lse).  The
    forward takes .contiguous() of every operand, so an expanded K or V (one K for all heads) is materialised per head, and
    autograd's own backward of expand sums the heads' gradients: the sum over heads is not fused into the kernel."""
    if (fwd_plan.n_rows, fwd_plan.n_cols, fwd_plan.nnz, fwd_plan.val_dtype) != (bwd_plan.n_rows, bwd_plan.n_cols, bwd_plan.nnz, bwd_plan.val_dtype):
        raise ValueError("the forward and the backward plan differ in structure or value type")
    if fwd_plan.vec_dtype != bwd_plan.vec_dtype:
        raise TypeError("the forward plan holds Q, K, V and O in %s, the backward plan in %s" % (fwd_plan.vec_dtype, bwd_plan.vec_dtype))

    class SparseAttention(torch.autograd.Function):
        @staticmethod
        def forward(ctx, Q, K, V, bias):
            Q, K, V = Q.detach().contiguous(), K.detach().contiguous(), V.detach().contiguous()
            bias = None if bias is None else bias.detach().contiguous()
            if Q.dim() == 3 and Q.size(1) > min(fwd_plan.n_heads_max, bwd_plan.n_heads_max):
                raise ValueError("%d heads above what both plans reserve (n_heads_max = %d forward, %d backward)"
                                 % (Q.size(1), fwd_plan.n_heads_max, bwd_plan.n_heads_max))
            lse = torch.empty((Q.size(1), fwd_plan.n_rows) if Q.dim() == 3 else (fwd_plan.n_rows,), dtype=fwd_plan.val_dtype, device=Q.device)
            O = fwd_plan.execute(Q, K, V, lse=lse, bias=bias)
            ctx.save_for_backward(Q, K, V, O, lse, *(() if bias is None else (bias,)))
            return O

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, dO):
            Q, K, V, O, lse = ctx.saved_tensors[:5]
            bias = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
            need = tuple(ctx.needs_input_grad[:3])
            want_dbias = bias is not None and ctx.needs_input_grad[3]
            if not any(need) and not want_dbias:
                return None, None, None, None
            dQ, dK, dV, dbias = bwd_plan.execute(Q, K, V, O, dO.contiguous(), lse, bias=bias, need=(need[0] or want_dbias, need[1], need[2]),
                                                 dbias=True if want_dbias else None)
            return (dQ if need[0] else None), dK, dV, dbias

    def f(Q, K, V, bias=None):
        return SparseAttention.apply(Q, K, V, bias)

    return f
