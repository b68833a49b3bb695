"""spmv-samples_amd — MI355X-native CSR SpMV engine behind the operator interface of
peakcrosser7/spmv-samples (`SpMV<...>(kind_str, n_rows, n_cols, nnz, Ap, Aj, Ax, x, y)`).

The directory name carries a hyphen (it mirrors the reference's repository name), so
it is imported under the alias `spmv_samples_amd`:

    import __graft_entry__          # registers the alias
    import spmv_samples_amd as sp

Contents (only what the hot path needs):
    csrc/      HIP kernels (gfx950) + the C ABI of include/mi355_spmv.h
    lib/       built libmi355spmv.so (git-ignored)
    host/      C++ mirror of the reference's include/spmv.h boundary (SpMV<>, SPMV_KINDS, Timer)
    capi.py    ctypes binding used by tests and bench.py: lib() declares the argument types, the shared helpers (_check, _require_*,
               _ptr, _stream_ptr) and the handle base _Handle (destroy, __del__, _info) come next, then the entry points (also coo_to_csr: COO -> CSR on the device, symmetric expansion included;
               MultiPlan / spmm / spmm_pattern: Y = A X for k vectors in one pass over A, over a semiring; narrow_values: fp32 -> fp16 / bf16 matrix values;
               SddmmPlan / sddmm / sddmm_half: dot(U[r], V[c]) at every stored entry (r, c) of A in one pass over A, U and V in fp32 / fp64 or in 16 bits;
               RowSoftmaxPlan / row_softmax: softmax over the stored entries of every row, and its gradient;
               SparseAttentionPlan / sparse_attention / sparse_attention_half: O = softmax(Q K^T on A) V fused into one pass over A, Q, K, V and O in fp32 / fp64 or in 16 bits;
               SparseAttentionBackwardPlan / sparse_attention_backward: dQ, dK, dV (and dbias) of that attention from O, dO and lse, nothing of nnz size kept;
               SparseAttentionBackwardHalfPlan / sparse_attention_backward_half: the same with the eight matrices in 16 bits;
               reserve_heads / n_heads_max / with_heads on the three attention plans, 3-D (rows, H, width) operands of their execute: the heads of a layer in one call;
               csr_transpose / MultiPlan(perm=) / TransposedMultiPlan / spmm_t: Y = A^T X with Ax read in place through a slot map)
    autograd.py  sparse_attention_function: the two attention plans as one torch.autograd.Function-backed callable
    synth.py   seeded synthetic CSR matrices (stand-ins for the BASELINE configs)
    dist.py    row-block sharding + allgatherv(y) for one process per GPU
    load.py    ctypes binding of the Matrix Market loader (include/mi355_load.h, host/load.hpp)
"""
from . import autograd, capi, dist, load, synth  # noqa: F401
from .autograd import sparse_attention_function  # noqa: F401
from .capi import (DistPlan, Functor, MultiPlan, Plan, PlanShape, RowSoftmaxPlan, SddmmPlan, SparseAttentionPlan, SparseAttentionBackwardPlan, SparseAttentionBackwardHalfPlan, sparse_attention_backward_half, sparse_attention, sparse_attention_backward, sparse_attention_half, coo_symmetric_nnz, coo_to_csr, spmm,  # noqa: F401
                   spmv, narrow_values, row_softmax, TransposedMultiPlan, csr_transpose, spmm_t, sddmm, sddmm_half, spmm_pattern, spmv_genl, spmv_mixed, spmv_pattern)
