"""ctypes binding of libmi355spmv.so (the C ABI of include/mi355_spmv.h).

This is plumbing for tests and bench.py: torch provides device memory and
streams, the library does the work.  There is NO fallback: if the shared library
is missing or a call fails, a RuntimeError is raised.

The reference interface this mirrors (same argument order and meaning):
    SpMV(kind_str, n_rows, n_cols, nnz, Ap, Aj, Ax, x, y)   include/spmv.h:29-34

Layout: the constants and the *Info structures; lib(), which declares the argument types (plan-level entries one by one,
as the header lists them; the <off>_<val> one-shot families from one table); the helpers every entry point shares (_check,
the _require_* checks, _ptr, _stream_ptr) and _Handle, the base of every class that owns a library object; then the entry
points in the header's order.
"""
import contextlib
import ctypes as C
import os

import torch  # imported before the library so both share one HIP runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355_SPMV_LIB") or os.path.join(_HERE, "lib", "libmi355spmv.so")

KINDS = {"vector": 0, "merge": 1, "light": 2, "auto": 100}   # auto: the library picks (MI355_KIND_AUTO)
KIND_NAMES = {0: "vector", 1: "merge", 2: "light"}
# labels the C++ host header registers in SPMV_KINDS (host/spmv.h)
LABELS = {"hip_vector": "vector", "hip_merge": "merge", "hip_light": "light", "hip_auto": "auto"}
OFF_TYPES = {torch.int32: (0, "i32"), torch.int64: (1, "i64")}
VAL_TYPES = {torch.float32: (0, "f32"), torch.float64: (1, "f64"), torch.int32: (2, "i32")}   # (int32 values: the merge kind only)
VAL_PATTERN = 3              # MI355_VAL_PATTERN: a matrix type only (Plan(..., mat_dtype="pattern"), spmv_pattern)
# MI355_VAL_F16 / MI355_VAL_BF16: matrix types only — 16-bit values under float32 x and y, the vector kind
# (Plan("vector", ..., torch.float32, mat_dtype=torch.float16), narrow_values).  Never in VAL_TYPES: that is x's and y's.
MAT_TYPES = {torch.float16: (4, "f16"), torch.bfloat16: (5, "bf16")}
PLAN_REUSE_STRUCTURE = 1
PLAN_NO_INDEX_COPY = 2       # the plan holds nothing derived from the contents of Aj (no packed index)
SEMIRINGS = {"plus_times": 0, "min_plus": 1, "max_times": 2, "max_plus": 3, "or_and": 4}

EXPORTS = (
    ["mi355_spmv_%s_%s_%s" % (k, o, v) for k in KINDS for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_merge_genl_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64", "i32")]
    + ["mi355_spmv_plan_set_semiring", "mi355_spmv_plan_set_alpha_beta"]
    + ["mi355_spmv_plan_create", "mi355_spmv_plan_execute", "mi355_spmv_plan_destroy",
       "mi355_spmv_plan_get_info", "mi355_spmv_stream_synchronize", "mi355_spmv_plan_merge_coords", "mi355_spmv_version",
       "mi355_spmv_status_string", "mi355_spmv_last_error", "mi355_spmv_device_count"]
    + ["mi355_spmv_plan_get_shape", "mi355_spmv_plan_partition", "mi355_spmv_plan_create_block",
       "mi355_spmv_knobs_reload", "mi355_spmv_cache_release", "mi355_spmv_plan_acquire", "mi355_spmv_plan_release",
       "mi355_spmv_plan_create_typed", "mi355_spmv_merge_f32mat_f64vec_i32",
       "mi355_spmv_merge_f32mat_f64vec_i64"]
    + ["mi355_spmv_dist_" + n for n in ("create_local", "unique_id", "create_rank", "scatter_values", "replicate_x",
                                        "execute", "execute_ex", "set_exchange", "get_info", "structure_changed",
                                        "set_alpha_beta", "parts", "cuts", "part_info", "device_y", "device_x",
                                        "destroy")]
    + ["mi355_spmv_functor_" + n for n in ("compile", "compile_log", "spmv", "destroy")]
    + ["mi355_spmv_coo_to_csr", "mi355_spmv_coo_symmetric_nnz", "mi355_spmv_coo_to_csr_symmetric"]
    + ["mi355_spmv_merge_pattern_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64", "i32")]
    + ["mi355_spmv_plan_get_mat_type", "mi355_spmv_narrow_values"]
    + ["mi355_spmv_multi_" + n for n in ("create", "set_alpha_beta", "execute", "get_info", "destroy")]
    + ["mi355_spmv_multi_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_multi_" + n for n in ("create_typed", "set_semiring", "get_types")]
    + ["mi355_spmv_multi_%s_%s_%s" % (g, o, v) for g in ("genl", "pattern") for o in ("i32", "i64") for v in ("f32", "f64", "i32")]
    + ["mi355_spmv_multi_create_half"]
    + ["mi355_spmv_multi_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")]
    + ["mi355_spmv_sddmm_" + n for n in ("create", "set_alpha_beta", "execute", "get_info", "destroy")]
    + ["mi355_spmv_sddmm_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_sddmm_create_half", "mi355_spmv_sddmm_get_types"]
    + ["mi355_spmv_sddmm_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")]
    + ["mi355_spmv_row_softmax_" + n for n in ("create", "set_scale", "execute", "backward", "get_info", "destroy")]
    + ["mi355_spmv_row_softmax_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_attention_" + n for n in ("create", "set_scale", "execute", "get_info", "destroy")]
    + ["mi355_spmv_attention_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_attention_create_half", "mi355_spmv_attention_get_types"]
    + ["mi355_spmv_attention_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")]
    + ["mi355_spmv_csr_transpose"]
    + ["mi355_spmv_multi_" + n for n in ("create_permuted", "create_transposed", "get_perm_info", "copy_structure")]
    + ["mi355_spmv_multi_transposed_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_attention_bwd_" + n for n in ("create", "set_scale", "execute", "get_info", "destroy")]
    + ["mi355_spmv_attention_bwd_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    + ["mi355_spmv_attention_bwd_create_half", "mi355_spmv_attention_bwd_get_types"]
    + ["mi355_spmv_attention_bwd_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")]
    + ["mi355_spmv_attention%s_%s" % (b, n) for b in ("", "_bwd") for n in ("reserve_heads", "get_heads_max", "execute_heads")]
)


def _struct_dict(s):
    """The fields of an *Info structure as a dict: character arrays as str, fields named reserved* left out."""
    d = {n: getattr(s, n) for n, _ in s._fields_ if not n.startswith("reserved")}
    return {n: v.decode() if isinstance(v, bytes) else v for n, v in d.items()}


class PlanInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("off_type", C.c_int32), ("val_type", C.c_int32),
                ("lanes_per_row", C.c_int32), ("elems_per_lane", C.c_int32), ("block_threads", C.c_int32),
                ("grid_blocks", C.c_int64), ("tile_items", C.c_int64), ("n_tiles", C.c_int64),
                ("rows_per_chunk", C.c_int64), ("scratch_bytes", C.c_int64), ("n_kernels", C.c_int32),
                ("window_elems", C.c_int32), ("window_segments", C.c_int32), ("main_kernel", C.c_char * 64),
                ("balanced_chunks", C.c_int32), ("rows_cap", C.c_int32), ("n_chunks", C.c_int64),
                ("knobs", C.c_char * 160), ("packed_index_bytes", C.c_int64), ("packed_index_escapes", C.c_int64)]

    def as_dict(self):
        return _struct_dict(self)


class PlanShape(C.Structure):
    """mi355_spmv_plan_shape: the launch-shape decisions of a plan as plain data (picklable via bytes(shape))."""
    _fields_ = [("struct_bytes", C.c_int32), ("kind", C.c_int32), ("off_type", C.c_int32), ("val_type", C.c_int32),
                ("n_rows", C.c_int32), ("n_cols", C.c_int32), ("nnz", C.c_int64),
                ("lanes_per_row", C.c_int32), ("elems_per_lane", C.c_int32), ("block_threads", C.c_int32),
                ("balanced_chunks", C.c_int32), ("rows_cap", C.c_int32), ("giant_rows_enabled", C.c_int32),
                ("rows_per_chunk", C.c_int64), ("n_chunks", C.c_int64), ("bal_k", C.c_int64), ("bal_q", C.c_int64),
                ("giant_len", C.c_int64),
                ("window_elems", C.c_int32), ("window_bytes", C.c_int32), ("window_from_band", C.c_int32),
                ("window_segments", C.c_int32), ("probe_ok", C.c_int32), ("long_steps", C.c_int32),
                ("band_lo", C.c_int64), ("band_hi", C.c_int64), ("seg_lo", C.c_int64 * 4), ("seg_hi", C.c_int64 * 4),
                ("window_sweep", C.c_int32), ("small_plain", C.c_int32)]


class DistInfo(C.Structure):
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("sub_blocks", C.c_int32), ("local_mode", C.c_int32),
                ("exchange", C.c_int32), ("auto_picked", C.c_int32), ("allgather_in_place", C.c_int32),
                ("reserved0", C.c_int32), ("trial_us", C.c_float * 4), ("max_block_rows", C.c_int64),
                ("staging_bytes", C.c_int64), ("exchange_name", C.c_char * 16)]


class MultiInfo(C.Structure):
    _fields_ = [("off_type", C.c_int32), ("val_type", C.c_int32), ("k_max", C.c_int32), ("slice_len", C.c_int32),
                ("block_threads", C.c_int32), ("widest_tile", C.c_int32), ("passes", C.c_int32), ("n_kernels", C.c_int32),
                ("n_slices", C.c_int64), ("grid_blocks", C.c_int64), ("scratch_bytes", C.c_int64),
                ("main_kernel", C.c_char * 64)]


class SddmmInfo(C.Structure):
    _fields_ = [("off_type", C.c_int32), ("val_type", C.c_int32), ("slice_len", C.c_int32), ("block_threads", C.c_int32),
                ("n_slices", C.c_int64), ("grid_blocks", C.c_int64), ("main_kernel", C.c_char * 64)]


class RowSoftmaxInfo(C.Structure):
    _fields_ = [("off_type", C.c_int32), ("val_type", C.c_int32), ("slice_len", C.c_int32), ("block_threads", C.c_int32),
                ("n_slices", C.c_int64), ("grid_blocks", C.c_int64), ("scratch_bytes", C.c_int64),
                ("main_kernel", C.c_char * 64)]


class AttentionInfo(C.Structure):
    _fields_ = [("off_type", C.c_int32), ("val_type", C.c_int32), ("slice_len", C.c_int32), ("block_threads", C.c_int32),
                ("d_max", C.c_int32), ("dv_max", C.c_int32), ("widest_tile", C.c_int32), ("passes", C.c_int32),
                ("lanes_per_slot", C.c_int32), ("reserved", C.c_int32),
                ("n_slices", C.c_int64), ("grid_blocks", C.c_int64), ("scratch_bytes", C.c_int64),
                ("main_kernel", C.c_char * 64)]


class AttentionHeadStrides(C.Structure):
    """mi355_spmv_attention_head_strides: elements between head h and head h + 1 of each operand (0: shared by all heads)."""
    _fields_ = [(n, C.c_int64) for n in ("q", "k", "v", "bias", "o", "lse")]


class AttentionBackwardHeadStrides(C.Structure):
    """mi355_spmv_attention_bwd_head_strides."""
    _fields_ = [(n, C.c_int64) for n in ("q", "k", "v", "bias", "o", "d_o", "lse", "dq", "dk", "dv", "dbias")]


class AttentionBackwardInfo(C.Structure):
    _fields_ = [("off_type", C.c_int32), ("val_type", C.c_int32), ("slice_len", C.c_int32), ("block_threads", C.c_int32),
                ("d_max", C.c_int32), ("dv_max", C.c_int32), ("widest_tile", C.c_int32), ("reserved", C.c_int32),
                ("lanes_per_slot", C.c_int32 * 3), ("passes", C.c_int32 * 3),
                ("n_slices", C.c_int64), ("grid_blocks", C.c_int64), ("n_slices_t", C.c_int64), ("grid_blocks_t", C.c_int64),
                ("scratch_bytes", C.c_int64), ("held_bytes", C.c_int64), ("main_kernel", C.c_char * 64)]


EXCHANGES = {"auto": 0, "bcast": 1, "sendrecv": 2, "allgather": 3}
EXEC_DEFAULT, EXEC_SKIP_EXCHANGE, EXEC_EXCHANGE_ONLY = 0, 1, 2

_lib = None


# the operands of an attention backward, execute and one-shots alike:
# (Q, ldq), (K, ldk), (V, ldv), bias, (O, ldo), (dO, lddo), lse, (dQ, lddq), (dK, lddk), (dV, lddv), dbias, stream
_BWD_OPERANDS = ([C.c_void_p, C.c_int64] * 3 + [C.c_void_p] + [C.c_void_p, C.c_int64] * 2 + [C.c_void_p] + [C.c_void_p, C.c_int64] * 3
                 + [C.c_void_p, C.c_void_p])


def _one_shot_signatures():
    """(stem, value suffixes, argument types) of the one-shot families mi355_spmv_<stem>_<off>_<val> that declare their
    types; "off" stands for nnz, int32_t or int64_t by <off>.  Families on one list share a signature in the header too.
    (The mi355_spmv_<kind>_*, merge_genl_*, merge_pattern_* and merge_f32mat_f64vec_* one-shots declare none: spmv and its
    kin wrap every argument themselves.)"""
    i32, i64, dbl, ptr = C.c_int32, C.c_int64, C.c_double, C.c_void_p
    # n_rows, n_cols, nnz, Ap, Aj, Ax, (X, ldx), (Y, ldy), k, stream
    multi = [i32, i32, "off", ptr, ptr, ptr, ptr, i64, ptr, i64, i32, ptr]
    # n_rows, n_cols, nnz, Ap, Aj, Ax, (U, ldu), (V, ldv), out, k, stream
    sddmm = [i32, i32, "off", ptr, ptr, ptr, ptr, i64, ptr, i64, ptr, i32, ptr]
    # n_rows, n_cols, nnz, Ap, Aj, d, dv, (Q, ldq), (K, ldk), (V, ldv), bias, scale, (O, ldo), lse, stream
    attention = [i32, i32, "off", ptr, ptr, i32, i32, ptr, i64, ptr, i64, ptr, i64, ptr, dbl, ptr, i64, ptr, ptr]
    # ... bias, scale, (O, ldo), ...: the one-shots take the scale behind bias
    attention_bwd = [i32, i32, "off", ptr, ptr, i32, i32] + _BWD_OPERANDS[:7] + [dbl] + _BWD_OPERANDS[7:]
    floats, halves = ("f32", "f64"), ("f16", "bf16")
    return (
        ("multi", floats, multi), ("multi_half", halves, multi), ("multi_transposed", floats, multi),
        ("multi_genl", floats + ("i32",), [C.c_int] + multi),                      # the semiring first
        ("multi_pattern", floats + ("i32",), [C.c_int] + multi[:5] + multi[6:]),   # ... and no Ax
        ("sddmm", floats, sddmm), ("sddmm_half", halves, sddmm),
        ("row_softmax", floats, [i32, i32, "off", ptr, ptr, ptr, ptr, dbl, ptr]),
        ("attention", floats, attention), ("attention_half", halves, attention),
        ("attention_bwd", floats, attention_bwd), ("attention_bwd_half", halves, attention_bwd),
    )


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.mi355_spmv_status_string.restype = C.c_char_p
        L.mi355_spmv_last_error.restype = C.c_char_p
        L.mi355_spmv_plan_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int32,
                                             C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        L.mi355_spmv_plan_create_typed.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        L.mi355_spmv_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_plan_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_plan_acquire.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int32,
                                              C.c_int64, C.c_void_p, C.c_void_p]
        L.mi355_spmv_plan_release.argtypes = [C.c_void_p, C.c_int]
        L.mi355_spmv_plan_set_semiring.argtypes = [C.c_void_p, C.c_int]
        L.mi355_spmv_plan_set_alpha_beta.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.mi355_spmv_plan_get_info.argtypes = [C.c_void_p, C.POINTER(PlanInfo)]
        L.mi355_spmv_plan_merge_coords.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_plan_get_mat_type.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.mi355_spmv_narrow_values.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_plan_get_shape.argtypes = [C.c_void_p, C.POINTER(PlanShape)]
        L.mi355_spmv_plan_partition.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_plan_create_block.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                                   C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        L.mi355_spmv_dist_create_local.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int32,
                                                   C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                   C.c_int, C.c_int]
        L.mi355_spmv_dist_unique_id.argtypes = [C.c_void_p]
        L.mi355_spmv_dist_create_rank.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        L.mi355_spmv_dist_scatter_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_dist_replicate_x.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_dist_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_dist_execute_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mi355_spmv_dist_set_exchange.argtypes = [C.c_void_p, C.c_int]
        L.mi355_spmv_dist_get_info.argtypes = [C.c_void_p, C.POINTER(DistInfo)]
        L.mi355_spmv_dist_structure_changed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.POINTER(C.c_int)]
        L.mi355_spmv_dist_set_alpha_beta.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.mi355_spmv_dist_parts.argtypes = [C.c_void_p]
        L.mi355_spmv_dist_cuts.argtypes = [C.c_void_p, C.c_void_p]
        L.mi355_spmv_dist_part_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(PlanInfo)]
        L.mi355_spmv_dist_device_y.argtypes = [C.c_void_p, C.c_int]
        L.mi355_spmv_dist_device_y.restype = C.c_void_p
        L.mi355_spmv_dist_device_x.argtypes = [C.c_void_p, C.c_int]
        L.mi355_spmv_dist_device_x.restype = C.c_void_p
        L.mi355_spmv_dist_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_functor_compile.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p,
                                                 C.c_char_p, C.c_char_p]
        L.mi355_spmv_functor_compile_log.restype = C.c_char_p
        L.mi355_spmv_functor_spmv.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 6
        L.mi355_spmv_functor_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_coo_to_csr.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_size_t), C.c_void_p]
        L.mi355_spmv_coo_symmetric_nnz.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.mi355_spmv_coo_to_csr_symmetric.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t),
                                                      C.c_void_p]
        L.mi355_spmv_multi_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_int32]
        L.mi355_spmv_multi_set_alpha_beta.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.mi355_spmv_multi_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                               C.c_int32, C.c_void_p]
        L.mi355_spmv_multi_get_info.argtypes = [C.c_void_p, C.POINTER(MultiInfo)]
        L.mi355_spmv_multi_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_multi_create_typed.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int32,
                                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
        L.mi355_spmv_multi_set_semiring.argtypes = [C.c_void_p, C.c_int]
        L.mi355_spmv_multi_get_types.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355_spmv_multi_create_half.argtypes = L.mi355_spmv_multi_create_typed.argtypes
        L.mi355_spmv_sddmm_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64,
                                              C.c_void_p, C.c_void_p]
        L.mi355_spmv_sddmm_set_alpha_beta.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.mi355_spmv_sddmm_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_int32, C.c_void_p]
        L.mi355_spmv_sddmm_get_info.argtypes = [C.c_void_p, C.POINTER(SddmmInfo)]
        L.mi355_spmv_sddmm_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_sddmm_create_half.argtypes = L.mi355_spmv_sddmm_create.argtypes
        L.mi355_spmv_sddmm_get_types.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355_spmv_row_softmax_create.argtypes = L.mi355_spmv_sddmm_create.argtypes
        L.mi355_spmv_row_softmax_set_scale.argtypes = [C.c_void_p, C.c_double]
        L.mi355_spmv_row_softmax_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_row_softmax_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_row_softmax_get_info.argtypes = [C.c_void_p, C.POINTER(RowSoftmaxInfo)]
        L.mi355_spmv_row_softmax_destroy.argtypes = [C.c_void_p]
        # Deliberate: this create alone takes the handle LAST (include/mi355_spmv.h, mi355_spmv_attention_create); create_half
        # and every other create take it first.
        L.mi355_spmv_attention_create.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int32,
                                                  C.c_int32, C.POINTER(C.c_void_p)]
        L.mi355_spmv_attention_set_scale.argtypes = [C.c_void_p, C.c_double]
        L.mi355_spmv_attention_execute.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.mi355_spmv_attention_get_info.argtypes = [C.c_void_p, C.POINTER(AttentionInfo)]
        L.mi355_spmv_attention_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_attention_create_half.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                                       C.c_void_p, C.c_int32, C.c_int32]
        L.mi355_spmv_attention_get_types.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355_spmv_csr_transpose.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
        L.mi355_spmv_multi_create_permuted.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64,
                                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int32,
                                                       C.c_void_p]
        L.mi355_spmv_multi_create_transposed.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64,
                                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.mi355_spmv_multi_get_perm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.mi355_spmv_multi_copy_structure.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355_spmv_attention_bwd_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.mi355_spmv_attention_bwd_set_scale.argtypes = [C.c_void_p, C.c_double]
        L.mi355_spmv_attention_bwd_execute.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + _BWD_OPERANDS   # the handle, d, dv
        L.mi355_spmv_attention_bwd_get_info.argtypes = [C.c_void_p, C.POINTER(AttentionBackwardInfo)]
        L.mi355_spmv_attention_bwd_destroy.argtypes = [C.c_void_p]
        L.mi355_spmv_attention_bwd_create_half.argtypes = L.mi355_spmv_attention_bwd_create.argtypes
        L.mi355_spmv_attention_bwd_get_types.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        for stem, strides in (("mi355_spmv_attention", AttentionHeadStrides), ("mi355_spmv_attention_bwd", AttentionBackwardHeadStrides)):
            getattr(L, stem + "_reserve_heads").argtypes = [C.c_void_p, C.c_int32]
            getattr(L, stem + "_get_heads_max").argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
            # the handle, n_heads, hs, then exactly execute's arguments behind its handle
            getattr(L, stem + "_execute_heads").argtypes = [C.c_void_p, C.c_int32, C.POINTER(strides)] + getattr(L, stem + "_execute").argtypes[1:]
        for stem, vals, args in _one_shot_signatures():
            for o, off_c in (("i32", C.c_int32), ("i64", C.c_int64)):
                for v in vals:
                    getattr(L, "mi355_spmv_%s_%s_%s" % (stem, o, v)).argtypes = [off_c if a == "off" else a for a in args]
        _lib = L
    return _lib


# ---- what every entry point shares


def _check(status, what):
    if status != 0:
        L = lib()
        raise RuntimeError("%s failed: %s (%s)" % (
            what, L.mi355_spmv_status_string(status).decode(), L.mi355_spmv_last_error().decode()))


_NO_CPU_PATH = "mi355 spmv takes device tensors only (no CPU path exists)"


def _require_device(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU_PATH)
        if not t.is_contiguous():
            raise RuntimeError("mi355 spmv takes contiguous tensors")


def _require_structure(Ap, Aj, *more):
    """Ap and Aj (and `more`, a one-shot's Ax) are contiguous device tensors and Aj is int32."""
    _require_device(Ap, Aj, *more)
    if Aj.dtype != torch.int32:
        raise TypeError("Aj must be int32")


def _require_on_device(t):
    """A one-shot's first operand, asked before its type is: whatever it is, it must say that it is on the device."""
    if not getattr(t, "is_cuda", False):
        raise RuntimeError(_NO_CPU_PATH)


def _require_matrix(t, name, rows, dtype):
    """A 2-D device tensor of `rows` rows whose rows are contiguous (stride(1) == 1); returns its leading dimension."""
    if not t.is_cuda:
        raise RuntimeError(_NO_CPU_PATH)
    if t.dim() != 2:
        raise ValueError("%s must be 2-D (one row per matrix column / row, one column per vector)" % name)
    if t.dtype != dtype:
        raise TypeError("value type differs from the plan's")
    if t.size(0) < rows:
        raise ValueError("operand shorter than the plan's sizes")
    if t.size(1) > 1 and t.stride(1) != 1:
        raise ValueError("%s must be row-major: stride(1) == 1 (column-major operands are not built)" % name)
    ld = t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))
    if ld < t.size(1):
        raise ValueError("%s: rows overlap (stride(0) below the number of columns)" % name)
    return ld


def _edge_values(t, name, nnz, val_dtype):
    """An operand of nnz values in CSR order: a contiguous 1-D device tensor of the plan's value type."""
    _require_device(t)
    if t.dtype != val_dtype:
        raise TypeError("value type differs from the plan's (%s)" % name)
    if t.dim() != 1 or t.numel() < nnz:
        raise ValueError("operand shorter than the plan's sizes (%s)" % name)
    return t


def _require_vectors(X, x_rows, Y, y_rows, dtype):
    """The k vectors of a multi-vector call, X of x_rows rows and Y of y_rows: (ldx, ldy)."""
    ldx = _require_matrix(X, "X", x_rows, dtype)
    ldy = _require_matrix(Y, "Y", y_rows, dtype)
    if X.size(1) != Y.size(1):
        raise ValueError("X and Y hold different numbers of vectors")
    return ldx, ldy


def _refuse_alias(X, Y):
    """Y must not lie over X: a slice writes rows of Y while other slices still gather rows of X."""
    span = lambda t: (t.data_ptr(), t.data_ptr() + ((t.size(0) - 1) * t.stride(0) + t.size(1)) * t.element_size()) if t.numel() else (0, 0)
    (x0, x1), (y0, y1) = span(X), span(Y)
    if x0 < y1 and y0 < x1:
        raise ValueError("Y aliases X")


def _semiring_id(semiring):
    return SEMIRINGS[semiring] if isinstance(semiring, str) else int(semiring)


def _ptr(t):
    """The address of a tensor's first element as a void*; NULL for None (an optional operand left out)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptr_or_null(t):
    """_ptr that also gives NULL for a tensor without elements, whose address means nothing."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream_ptr(stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


# Deliberate: which calls run under torch.cuda.device(...) — include/mi355_spmv.h has every entry point work on the CURRENT device.
# No guard (the caller's current device is the operands', as with the reference's operator; bench.py times the issue rate of
# the first of these): the mi355_spmv_<kind>_* / merge_* one-shots, narrow_values, coo_to_csr, every mi355_spmv_plan_* call but
# acquire / release, MultiPlan.execute, SddmmPlan's create (no device call), the functor, DistPlan.scatter_values /
# replicate_x, every setter and query.  Entered under the device of Ap (rows, y): plan acquire / release, coo_symmetric_nnz,
# csr_transpose, the multi / row_softmax / attention creates, the sddmm / row_softmax / attention / dist executes, every
# one-shot from spmm_t on, DistPlan's creates and structure_changed.  Add none and remove none.


class _Handle:
    """Owner of one library object: `_h` is its handle, `_destroy` names the entry that frees it."""
    _destroy = None

    def _call(self, entry, *args):
        """entry(handle, *args), checked."""
        _check(getattr(lib(), entry)(self._h, *args), entry)

    def _info(self, struct_type, entry, *args):
        """entry(handle, *args, &struct) as a dict (_struct_dict)."""
        si = struct_type()
        self._call(entry, *args, C.byref(si))
        return _struct_dict(si)

    def destroy(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ---- SpMV: one-shots, COO -> CSR, Plan


def spmv(kind, n_rows, n_cols, nnz, Ap, Aj, Ax, x, y, stream=None):
    """One-shot call: the reference's `SpMV(kind_str, n_rows, n_cols, nnz, Ap, Aj, Ax, x, y)`
    (include/spmv.h:29-34) for kind in {"vector","merge","light"} (or their
    SPMV_KINDS labels "hip_vector", ...).  Synchronises the stream before returning."""
    kind = LABELS.get(kind, kind)
    if kind not in KINDS:
        # the reference prints 'SpMV kind "<k>" is NOT SUPPROT' and exits (spmv.h:46-47)
        raise ValueError('SpMV kind "%s" is NOT SUPPORTED' % kind)
    _require_device(Ap, Aj, Ax, x, y)
    if Aj.dtype != torch.int32 or Ax.dtype != x.dtype or Ax.dtype != y.dtype:
        raise TypeError("Aj must be int32 and Ax, x, y one value type")
    if Ax.dtype == torch.int32:            # integer values exist for the (generalized) merge kind only
        if LABELS.get(kind, kind) not in ("merge", "auto"):
            raise RuntimeError("mi355_spmv: integer values are not supported by the %s kind (merge only)" % kind)
        return spmv_genl("plus_times", n_rows, n_cols, nnz, Ap, Aj, Ax, x, y, stream)
    o = OFF_TYPES[Ap.dtype][1]
    v = VAL_TYPES[Ax.dtype][1]
    fn = getattr(lib(), "mi355_spmv_%s_%s_%s" % (kind, o, v))
    nnz_c = C.c_int32(nnz) if o == "i32" else C.c_int64(nnz)
    st = fn(C.c_int32(n_rows), C.c_int32(n_cols), nnz_c, C.c_void_p(Ap.data_ptr()), C.c_void_p(Aj.data_ptr()),
            C.c_void_p(Ax.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), _stream_ptr(stream))
    _check(st, "mi355_spmv_%s_%s_%s" % (kind, o, v))
    return y


def spmv_mixed(n_rows, n_cols, nnz, Ap, Aj, Ax, x, y, stream=None):
    """One-shot merge-path SpMV with an fp32 matrix under fp64 vectors (mi355_spmv_merge_f32mat_f64vec_*)."""
    _require_device(Ap, Aj, Ax, x, y)
    if Aj.dtype != torch.int32 or Ax.dtype != torch.float32 or x.dtype != torch.float64 or y.dtype != torch.float64:
        raise TypeError("Aj int32, Ax float32, x and y float64")
    o = OFF_TYPES[Ap.dtype][1]
    fn = getattr(lib(), "mi355_spmv_merge_f32mat_f64vec_%s" % o)
    nnz_c = C.c_int32(nnz) if o == "i32" else C.c_int64(nnz)
    st = fn(C.c_int32(n_rows), C.c_int32(n_cols), nnz_c, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), _stream_ptr(stream))
    _check(st, "mi355_spmv_merge_f32mat_f64vec_%s" % o)
    return y


def narrow_values(Ax, dtype, out=None, stream=None):
    """Device float32 values rounded to torch.float16 / torch.bfloat16 (mi355_spmv_narrow_values: nearest even, overflow
    to +-inf, NaN stays NaN, subnormals kept): the Ax of a Plan(..., mat_dtype=dtype).  Asynchronous on `stream`."""
    if dtype not in MAT_TYPES:
        raise TypeError("narrow_values: dtype is torch.float16 or torch.bfloat16")
    _require_device(Ax)
    if Ax.dtype != torch.float32:
        raise TypeError("narrow_values takes float32 values")
    if out is None:
        out = torch.empty(Ax.shape, dtype=dtype, device=Ax.device)
    else:
        _require_device(out)
        if out.dtype != dtype or out.numel() < Ax.numel():
            raise TypeError("narrow_values: out must hold Ax.numel() values of the asked dtype")
    st = lib().mi355_spmv_narrow_values(MAT_TYPES[dtype][0], Ax.numel(), _ptr(Ax), _ptr(out), _stream_ptr(stream))
    _check(st, "mi355_spmv_narrow_values")
    return out


def cache_release():
    """Destroy the plans the one-shot entry points keep between calls (mi355_spmv_cache_release)."""
    _check(lib().mi355_spmv_cache_release(), "mi355_spmv_cache_release")


def spmv_genl(semiring, n_rows, n_cols, nnz, Ap, Aj, Ax, x, y, stream=None):
    """Generalized merge-path SpMV: the reference's SpMV_merge_based_generalized
    (include/spmv/merge_genl/merge_genl.cuh:41-79) with the semiring as an argument."""
    sr = SEMIRINGS[semiring] if isinstance(semiring, str) else int(semiring)
    _require_device(Ap, Aj, Ax, x, y)
    if Aj.dtype != torch.int32 or Ax.dtype != x.dtype or Ax.dtype != y.dtype:
        raise TypeError("Aj must be int32 and Ax, x, y one value type")
    o = OFF_TYPES[Ap.dtype][1]
    v = VAL_TYPES[Ax.dtype][1]
    fn = getattr(lib(), "mi355_spmv_merge_genl_%s_%s" % (o, v))
    nnz_c = C.c_int32(nnz) if o == "i32" else C.c_int64(nnz)
    st = fn(C.c_int(sr), C.c_int32(n_rows), C.c_int32(n_cols), nnz_c, C.c_void_p(Ap.data_ptr()),
            C.c_void_p(Aj.data_ptr()), C.c_void_p(Ax.data_ptr()), C.c_void_p(x.data_ptr()),
            C.c_void_p(y.data_ptr()), _stream_ptr(stream))
    _check(st, "mi355_spmv_merge_genl_%s_%s" % (o, v))
    return y


def spmv_pattern(semiring, n_rows, n_cols, nnz, Ap, Aj, x, y, stream=None):
    """One-shot generalized merge-path SpMV with a PATTERN matrix — a structure and no values, every entry one
    (mi355_spmv_merge_pattern_*): the arguments of spmv_genl without Ax.  Synchronises the stream."""
    sr = _semiring_id(semiring)
    _require_device(Ap, Aj, x, y)
    if Aj.dtype != torch.int32 or x.dtype != y.dtype:
        raise TypeError("Aj must be int32 and x, y one value type")
    o = OFF_TYPES[Ap.dtype][1]
    v = VAL_TYPES[x.dtype][1]
    fn = getattr(lib(), "mi355_spmv_merge_pattern_%s_%s" % (o, v))
    nnz_c = C.c_int32(nnz) if o == "i32" else C.c_int64(nnz)
    st = fn(C.c_int(sr), C.c_int32(n_rows), C.c_int32(n_cols), nnz_c, _ptr(Ap), _ptr(Aj), _ptr(x), _ptr(y), _stream_ptr(stream))
    _check(st, "mi355_spmv_merge_pattern_%s_%s" % (o, v))
    return y


def coo_to_csr_workspace_bytes(n_rows, nnz, off_dtype=torch.int32, val_dtype=None):
    """Device workspace mi355_spmv_coo_to_csr needs (the size query: no device is touched)."""
    ws = C.c_size_t(0)
    st = lib().mi355_spmv_coo_to_csr(OFF_TYPES[off_dtype][0], VAL_TYPES[val_dtype or torch.float32][0],
                                     C.c_int32(n_rows), C.c_int32(0), C.c_int64(nnz), None, None, None, None, None,
                                     None, None, None, C.byref(ws), None)
    _check(st, "mi355_spmv_coo_to_csr (size query)")
    return ws.value


def coo_to_csr_symmetric_workspace_bytes(n_rows, nnz_stored, nnz_expanded, off_dtype=torch.int32, val_dtype=None):
    """Device workspace mi355_spmv_coo_to_csr_symmetric needs (the size query: no device is touched)."""
    ws = C.c_size_t(0)
    st = lib().mi355_spmv_coo_to_csr_symmetric(OFF_TYPES[off_dtype][0], VAL_TYPES[val_dtype or torch.float32][0],
                                               C.c_int32(n_rows), C.c_int32(0), C.c_int64(nnz_stored),
                                               C.c_int64(nnz_expanded), None, None, None, None, None, None, None, None,
                                               C.byref(ws), None)
    _check(st, "mi355_spmv_coo_to_csr_symmetric (size query)")
    return ws.value


def coo_symmetric_nnz(rows, cols, stream=None):
    """Entries the stored entries (rows, cols) of a symmetric matrix expand to: their number plus the off-diagonal
    ones (mi355_spmv_coo_symmetric_nnz, a device reduction).  Synchronises the stream."""
    _require_device(rows, cols)
    if rows.dtype != torch.int32 or cols.dtype != torch.int32:
        raise TypeError("rows and cols must be int32")
    if cols.numel() != rows.numel():
        raise ValueError("rows and cols must have the same length")
    out = C.c_int64(0)
    with torch.cuda.device(rows.device):
        st = lib().mi355_spmv_coo_symmetric_nnz(C.c_int64(rows.numel()), _ptr_or_null(rows), _ptr_or_null(cols),
                                                _stream_ptr(stream), C.byref(out))
    _check(st, "mi355_spmv_coo_symmetric_nnz")
    return out.value


def coo_to_csr(n_rows, n_cols, rows, cols, vals=None, off_dtype=torch.int32, return_perm=False, stream=None,
               symmetric=False):
    """COO -> CSR on the device (mi355_spmv_coo_to_csr): the reference's ToCsr result (include/load.hpp:420-474) —
    entries of a row in input order, duplicates kept, columns not sorted.  rows / cols: int32 device tensors; vals:
    a float32 / float64 / int32 device tensor or None (then Ax is None).  Returns a synth.Csr, or (Csr, perm) with
    perm[k] = the source index of CSR slot k (int64) when return_perm.  Synchronises the stream.
    symmetric=True: rows / cols / vals are the STORED entries of a symmetric file; the result is ToCsr of LoadCoo's
    expansion (entry, then its mirror if off the diagonal), built by mi355_spmv_coo_to_csr_symmetric after
    coo_symmetric_nnz has sized it; perm[k] is then the index of the stored entry behind slot k."""
    from .synth import Csr
    _require_device(rows, cols, *([vals] if vals is not None else []))
    if rows.dtype != torch.int32 or cols.dtype != torch.int32:
        raise TypeError("rows and cols must be int32")
    n_in = rows.numel()
    if cols.numel() != n_in or (vals is not None and vals.numel() != n_in):
        raise ValueError("rows, cols and vals must have the same length")
    if vals is not None and vals.dtype not in VAL_TYPES:
        raise TypeError("vals must be float32, float64 or int32")
    dev = rows.device
    nnz = coo_symmetric_nnz(rows, cols, stream) if symmetric else n_in
    Ap = torch.empty(n_rows + 1, dtype=off_dtype, device=dev)
    Aj = torch.empty(nnz, dtype=torch.int32, device=dev)
    Ax = torch.empty(nnz, dtype=vals.dtype, device=dev) if vals is not None else None
    perm = torch.empty(nnz, dtype=torch.int64, device=dev) if return_perm else None
    val_dtype = vals.dtype if vals is not None else torch.float32
    ptr = _ptr_or_null
    if symmetric:       # the symmetric entry takes both counts: stored, expanded
        what, counts = "coo_to_csr_symmetric", (C.c_int64(n_in), C.c_int64(nnz))
        nbytes = coo_to_csr_symmetric_workspace_bytes(n_rows, n_in, nnz, off_dtype, val_dtype)
    else:
        what, counts = "coo_to_csr", (C.c_int64(nnz),)
        nbytes = coo_to_csr_workspace_bytes(n_rows, nnz, off_dtype, val_dtype)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    size = C.c_size_t(nbytes)
    st = getattr(lib(), "mi355_spmv_" + what)(OFF_TYPES[off_dtype][0], VAL_TYPES[val_dtype][0], C.c_int32(n_rows), C.c_int32(n_cols),
                                              *counts, ptr(rows), ptr(cols), ptr(vals), ptr(Ap), ptr(Aj), ptr(Ax), ptr(perm),
                                              _ptr(ws), C.byref(size), _stream_ptr(stream))
    _check(st, "mi355_spmv_" + what)
    csr = Csr(n_rows, n_cols, nnz, Ap, Aj, Ax, what, {"synthetic": False})
    return (csr, perm) if return_perm else csr


class Plan(_Handle):
    """Scratch + launch shapes kept across calls (mi355_spmv_plan_*).  Holds
    references to Ap and Aj so they outlive the plan."""
    _destroy = "mi355_spmv_plan_destroy"

    def __init__(self, kind, n_rows, n_cols, nnz, Ap, Aj, val_dtype, flags=0, mat_dtype=None):
        """val_dtype: the type of x and y (and of all arithmetic).  mat_dtype: the type the matrix values are stored
        in — None = val_dtype; torch.float32 under torch.float64 vectors is built for the merge kind
        (mi355_spmv_plan_create_typed; the reference's operator keeps the three value types apart, spmv.h:29-34).
        mat_dtype="pattern": the matrix stores no values, every entry is one (MI355_VAL_PATTERN; merge kind, float32 /
        float64 / int32 vectors) — execute() then ignores Ax, which may be None.
        mat_dtype=torch.float16 / torch.bfloat16: the matrix values are stored in 16 bits under float32 x and y
        (MI355_VAL_F16 / MI355_VAL_BF16; kind "vector", or "auto", which becomes it) — execute() takes Ax of that dtype."""
        kind = LABELS.get(kind, kind)
        if kind not in KINDS:
            raise ValueError('SpMV kind "%s" is NOT SUPPORTED' % kind)
        _require_structure(Ap, Aj)
        self.kind, self.n_rows, self.n_cols, self.nnz = kind, n_rows, n_cols, nnz
        self.Ap, self.Aj, self.val_dtype = Ap, Aj, val_dtype
        self.mat_dtype = mat_dtype if mat_dtype is not None else val_dtype
        self._h = C.c_void_p()
        if isinstance(self.mat_dtype, str):
            if self.mat_dtype != "pattern":
                raise ValueError('mat_dtype is a torch dtype or "pattern"')
            if val_dtype not in VAL_TYPES:
                raise TypeError("val_dtype must be float32, float64 or int32")
            types = (VAL_PATTERN, VAL_TYPES[val_dtype][0], VAL_TYPES[val_dtype][0])
        elif self.mat_dtype in MAT_TYPES:
            if val_dtype != torch.float32:
                raise TypeError("a float16 / bfloat16 matrix is built under float32 x and y only")
            types = (MAT_TYPES[self.mat_dtype][0], 0, 0)
        elif self.mat_dtype == val_dtype:
            st = lib().mi355_spmv_plan_create(C.byref(self._h), KINDS[kind], OFF_TYPES[Ap.dtype][0],
                                              VAL_TYPES[val_dtype][0], n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), flags)
            _check(st, "mi355_spmv_plan_create")
            return
        else:
            types = (VAL_TYPES[self.mat_dtype][0], VAL_TYPES[val_dtype][0], VAL_TYPES[val_dtype][0])
        # (mat_type, x_type, y_type)
        st = lib().mi355_spmv_plan_create_typed(C.byref(self._h), KINDS[kind], OFF_TYPES[Ap.dtype][0], *types, n_rows, n_cols,
                                                nnz, _ptr(Ap), _ptr(Aj), flags)
        _check(st, "mi355_spmv_plan_create_typed")

    def execute(self, Ax, x, y, stream=None):
        """Asynchronous on `stream` (default: torch's current stream).  A pattern plan ignores Ax: None or any tensor."""
        if getattr(self, "mat_dtype", None) == "pattern":
            _require_device(x, y)
            if x.dtype != self.val_dtype or y.dtype != self.val_dtype:
                raise TypeError("value type differs from the plan's")
            if x.numel() < self.n_cols or y.numel() < self.n_rows:
                raise ValueError("operand shorter than the plan's sizes")
            st = lib().mi355_spmv_plan_execute(self._h, None, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                               _stream_ptr(stream))
            _check(st, "mi355_spmv_plan_execute")
            return y
        _require_device(Ax, x, y)
        if Ax.dtype != getattr(self, "mat_dtype", self.val_dtype) or x.dtype != self.val_dtype or y.dtype != self.val_dtype:
            raise TypeError("value type differs from the plan's")
        if Ax.numel() < self.nnz or x.numel() < self.n_cols or y.numel() < self.n_rows:
            raise ValueError("operand shorter than the plan's sizes")
        st = lib().mi355_spmv_plan_execute(self._h, C.c_void_p(Ax.data_ptr()), C.c_void_p(x.data_ptr()),
                                           C.c_void_p(y.data_ptr()), _stream_ptr(stream))
        _check(st, "mi355_spmv_plan_execute")
        return y

    def set_semiring(self, semiring):
        self._call("mi355_spmv_plan_set_semiring", C.c_int(_semiring_id(semiring)))

    def set_alpha_beta(self, alpha, beta):
        """y = alpha * A x + beta * y for the following executes (default 1, 0)."""
        self._call("mi355_spmv_plan_set_alpha_beta", C.c_double(alpha), C.c_double(beta))

    def mat_type(self):
        """The MI355_VAL_* the plan's matrix values are stored in (3 = VAL_PATTERN: none)."""
        out = C.c_int(-1)
        self._call("mi355_spmv_plan_get_mat_type", C.byref(out))
        return out.value

    def info(self):
        return self._info(PlanInfo, "mi355_spmv_plan_get_info")

    def shape(self):
        """The plan's launch-shape decisions (mi355_spmv_plan_get_shape)."""
        sh = PlanShape()
        self._call("mi355_spmv_plan_get_shape", C.byref(sh))
        return sh

    def partition(self, parts):
        """nnz-balanced cuts on the plan's chunk boundaries: (row_cuts, chunk_cuts, nnz_cuts), parts + 1 each."""
        import numpy as np
        arrs = [np.zeros(parts + 1, dtype=np.int64) for _ in range(3)]
        self._call("mi355_spmv_plan_partition", parts, *[a.ctypes.data_as(C.c_void_p) for a in arrs])
        return tuple(a.tolist() for a in arrs)

    @classmethod
    def block(cls, kind, whole_shape, row_begin, chunk_begin, n_chunks, nnz_begin_whole, n_rows, n_cols, nnz_end,
              Ap, Aj, val_dtype, flags=0):
        """Plan for a row block given as a 16-byte-aligned VIEW of the whole CSR (Ap[0] in 0..3, nnz_end =
        Ap[n_rows]); inherits `whole_shape` (a PlanShape, or None) — mi355_spmv_plan_create_block."""
        kind = LABELS.get(kind, kind)
        _require_device(Ap, Aj)
        self = cls.__new__(cls)
        self.kind, self.n_rows, self.n_cols, self.nnz = kind, n_rows, n_cols, nnz_end
        self.Ap, self.Aj, self.val_dtype = Ap, Aj, val_dtype
        self._h = C.c_void_p()
        st = lib().mi355_spmv_plan_create_block(
            C.byref(self._h), KINDS[kind], OFF_TYPES[Ap.dtype][0], VAL_TYPES[val_dtype][0],
            C.cast(C.byref(whole_shape), C.c_void_p) if whole_shape is not None else None,
            row_begin, chunk_begin, n_chunks, nnz_begin_whole, n_rows, n_cols, nnz_end, _ptr(Ap), _ptr(Aj), flags)
        _check(st, "mi355_spmv_plan_create_block")
        return self

    @classmethod
    def acquire(cls, kind, n_rows, n_cols, nnz, Ap, Aj, val_dtype):
        """The plan a one-shot call on these arrays would run (mi355_spmv_plan_acquire): the one kept from the previous
        call on the same pointers, sizes, types, kind and device, else a new one.  Give it back with release() once
        the stream it ran on has been synchronised; destroy() instead drops it without keeping it."""
        kind = LABELS.get(kind, kind)
        if kind not in KINDS:
            raise ValueError('SpMV kind "%s" is NOT SUPPORTED' % kind)
        _require_structure(Ap, Aj)
        self = cls.__new__(cls)
        self.kind, self.n_rows, self.n_cols, self.nnz = kind, n_rows, n_cols, nnz
        self.Ap, self.Aj, self.val_dtype, self.mat_dtype = Ap, Aj, val_dtype, val_dtype
        self._h = C.c_void_p()
        with torch.cuda.device(Ap.device):
            st = lib().mi355_spmv_plan_acquire(C.byref(self._h), KINDS[kind], OFF_TYPES[Ap.dtype][0],
                                               VAL_TYPES[val_dtype][0], n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj))
        _check(st, "mi355_spmv_plan_acquire")
        return self

    def release(self, executed_ok=True):
        """Hand an acquired plan back (mi355_spmv_plan_release): kept for the next acquire / one-shot call on the same
        arrays when that is safe, destroyed otherwise.  The handle is gone either way."""
        if self._h:
            h, self._h = self._h, C.c_void_p()
            with torch.cuda.device(self.Ap.device):
                _check(lib().mi355_spmv_plan_release(h, 1 if executed_ok else 0), "mi355_spmv_plan_release")

    def merge_coords(self):
        import numpy as np
        n = self.info()["n_tiles"] + 1
        rows = np.empty(n, dtype=np.int64)
        nz = np.empty(n, dtype=np.int64)
        self._call("mi355_spmv_plan_merge_coords", rows.ctypes.data_as(C.c_void_p), nz.ctypes.data_as(C.c_void_p))
        return rows, nz


# ---- multi-vector SpMV


class MultiPlan(_Handle):
    """mi355_spmv_multi_*: Y = A X for up to k_max vectors in one pass over A — Y = alpha * A X + beta * Y under (+, *),
    Y[r, j] = reduce over the row of combine(Ax, X[Aj, j]) under another semiring (set_semiring, or semiring=).  X
    (n_cols x k) and Y (n_rows x k) are 2-D row-major device tensors; views with a larger stride(0) are taken as they
    are.  val_dtype (the type of X, Y and all arithmetic) is float32, float64 or int32; mat_dtype="pattern" makes a
    matrix without values (every entry one): execute then takes Ax=None.  int32 needs one of mat_dtype=torch.int32,
    mat_dtype="pattern" or a semiring other than "plus_times" spelled out: MultiPlan(..., torch.int32, k_max) alone is
    refused, as it was before int32 existed here.  val_dtype float16 / bfloat16 (mi355_spmv_multi_create_half): X and Y
    in 16 bits, fp32 arithmetic, Y rounded once; mat_dtype is then None or val_dtype (Ax in the same 16 bits) or
    torch.float32, and the semiring "plus_times".  Holds references to Ap and Aj so they outlive the object."""
    _destroy = "mi355_spmv_multi_destroy"

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, val_dtype, k_max, mat_dtype=None, semiring="plus_times", perm=None,
                 n_values=None, stream=None):
        """perm (nnz int32 or int64 device indices) makes a PERMUTED plan (mi355_spmv_multi_create_permuted): execute reads
        nonzero n's value as Ax[perm[n]], Ax holding n_values values (default nnz).  float32 / float64 under "plus_times"
        only.  Every index is checked on the device at create (on `stream`, which is synchronised); the plan keeps its own
        copy of perm."""
        _require_structure(Ap, Aj)
        self.n_values = nnz
        if perm is not None:
            self._init_permuted(n_rows, n_cols, nnz, Ap, Aj, val_dtype, k_max, mat_dtype, semiring, perm, n_values, stream)
            return
        if n_values is not None:
            raise TypeError("n_values comes with perm")
        pattern = isinstance(mat_dtype, str) and mat_dtype == "pattern"
        half = val_dtype in MAT_TYPES
        if half and mat_dtype not in (None, val_dtype, torch.float32):
            raise TypeError("mat_dtype under 16-bit vectors must be val_dtype or torch.float32")
        if not half and mat_dtype is not None and not pattern and mat_dtype != val_dtype:
            raise TypeError('mat_dtype must be val_dtype or "pattern" (mixed precision is not built on the multi path)')
        sr = _semiring_id(semiring)
        if half and sr != 0:
            raise TypeError('16-bit vectors are built under the "plus_times" semiring only')
        typed = pattern or sr != 0 or val_dtype == torch.int32 and mat_dtype is not None
        if val_dtype not in (torch.float32, torch.float64) and not half and not (typed and val_dtype == torch.int32):
            raise TypeError("val_dtype must be float32 or float64"
                            " (or int32 under a semiring, a pattern matrix or mat_dtype=torch.int32)")
        self.n_rows, self.n_cols, self.nnz, self.k_max = n_rows, n_cols, nnz, k_max
        self.Ap, self.Aj, self.val_dtype, self.pattern = Ap, Aj, val_dtype, pattern
        self.mat_dtype = val_dtype if mat_dtype is None or pattern else mat_dtype      # the type of Ax
        self._h = C.c_void_p()
        if half:            # (mat_type, vec_type)
            what = "mi355_spmv_multi_create_half"
            types = (VAL_TYPES[torch.float32][0] if self.mat_dtype == torch.float32 else MAT_TYPES[val_dtype][0], MAT_TYPES[val_dtype][0])
        elif typed:         # (mat_type, vec_type)
            what = "mi355_spmv_multi_create_typed"
            types = (VAL_PATTERN if pattern else VAL_TYPES[val_dtype][0], VAL_TYPES[val_dtype][0])
        else:               # plain fp32 / fp64 (+, *) objects: one type
            what = "mi355_spmv_multi_create"
            types = (VAL_TYPES[val_dtype][0],)
        with torch.cuda.device(Ap.device):
            st = getattr(lib(), what)(C.byref(self._h), OFF_TYPES[Ap.dtype][0], *types, n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), k_max)
        _check(st, what)
        if sr != 0:
            self.set_semiring(sr)

    def _init_permuted(self, n_rows, n_cols, nnz, Ap, Aj, val_dtype, k_max, mat_dtype, semiring, perm, n_values, stream):
        if val_dtype not in (torch.float32, torch.float64) or mat_dtype not in (None, val_dtype):
            raise TypeError("a permuted plan is float32 or float64 (matrix and vectors alike)")
        if _semiring_id(semiring) != 0:
            raise TypeError('a permuted plan is built under the "plus_times" semiring only')
        _require_device(perm)
        if perm.dtype not in OFF_TYPES:
            raise TypeError("perm must be int32 or int64")
        if perm.dim() != 1 or perm.numel() < nnz:
            raise ValueError("perm must hold nnz indices")
        n_values = nnz if n_values is None else int(n_values)
        if n_values < 0:
            raise ValueError("n_values is negative")
        self.n_rows, self.n_cols, self.nnz, self.k_max, self.n_values = n_rows, n_cols, nnz, k_max, n_values
        self.Ap, self.Aj, self.val_dtype, self.pattern, self.mat_dtype = Ap, Aj, val_dtype, False, val_dtype
        self.permuted = True
        self._h = C.c_void_p()
        with torch.cuda.device(Ap.device):
            st = lib().mi355_spmv_multi_create_permuted(
                C.byref(self._h), OFF_TYPES[Ap.dtype][0], VAL_TYPES[val_dtype][0], n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj),
                OFF_TYPES[perm.dtype][0], _ptr(perm), n_values, k_max, _stream_ptr(stream))
        _check(st, "mi355_spmv_multi_create_permuted")

    def perm_info(self):
        """{"n_values", "held_bytes", "owns_structure"} (mi355_spmv_multi_get_perm_info)."""
        n, b, o = C.c_int64(), C.c_int64(), C.c_int()
        self._call("mi355_spmv_multi_get_perm_info", C.byref(n), C.byref(b), C.byref(o))
        return {"n_values": n.value, "held_bytes": b.value, "owns_structure": o.value}

    def execute(self, Ax, X, Y, stream=None):
        """Asynchronous on `stream` (default: torch's current stream).  k = X.size(1) = Y.size(1).  Ax is None for a
        pattern plan (one that is given is ignored); a permuted plan takes n_values values."""
        if getattr(self, "pattern", False):
            Ax = None       # ignored: never checked, never passed on
        elif Ax is None:
            raise TypeError("Ax is None: only a pattern plan has no values")
        else:
            _require_device(Ax)
            if Ax.dtype != getattr(self, "mat_dtype", self.val_dtype):
                raise TypeError("value type differs from the plan's")
            if Ax.numel() < (self.n_values if getattr(self, "permuted", False) else self.nnz):
                raise ValueError("operand shorter than the plan's sizes")
        ldx, ldy = _require_vectors(X, self.n_cols, Y, self.n_rows, self.val_dtype)
        if getattr(self, "permuted", False):
            _refuse_alias(X, Y)
        st = lib().mi355_spmv_multi_execute(self._h, _ptr(Ax), _ptr(X), ldx, _ptr(Y), ldy, X.size(1), _stream_ptr(stream))
        _check(st, "mi355_spmv_multi_execute")
        return Y

    def set_alpha_beta(self, alpha, beta):
        """Y = alpha * A X + beta * Y for the following executes (default 1, 0); (+, *) on float types only."""
        self._call("mi355_spmv_multi_set_alpha_beta", C.c_double(alpha), C.c_double(beta))

    def set_semiring(self, semiring):
        """The semiring of the following executes: a name of SEMIRINGS or its number."""
        self._call("mi355_spmv_multi_set_semiring", C.c_int(_semiring_id(semiring)))

    def types(self):
        """{"mat_type", "vec_type", "semiring"} as the library holds them (MI355_VAL_*, MI355_SEMIRING_*)."""
        m, v, s = C.c_int(), C.c_int(), C.c_int()
        self._call("mi355_spmv_multi_get_types", C.byref(m), C.byref(v), C.byref(s))
        return {"mat_type": m.value, "vec_type": v.value, "semiring": s.value}

    def info(self):
        return self._info(MultiInfo, "mi355_spmv_multi_get_info")


def csr_transpose(n_rows, n_cols, Ap, Aj, stream=None):
    """The structure of A^T on the device (mi355_spmv_csr_transpose): (Apt, Ajt, perm) with Apt of n_cols + 1 offsets in
    Ap's dtype, Ajt[t] = the row of A behind transposed slot t and perm[t] = its CSR slot in A (int32 tensors holding the
    library's unsigned 32-bit indices), so that Axt = Ax[perm.long()].  Inside a column the slots ascend (a stable sort by
    column): deterministic.  Synchronises the stream."""
    _require_structure(Ap, Aj)
    if Ap.dtype not in OFF_TYPES:
        raise TypeError("Ap must be int32 or int64")
    if Ap.dim() != 1 or Ap.numel() < n_rows + 1:
        raise ValueError("Ap must hold n_rows + 1 offsets")
    nnz = Aj.numel()
    dev = Ap.device
    Apt = torch.empty(n_cols + 1, dtype=Ap.dtype, device=dev)
    Ajt = torch.empty(nnz, dtype=torch.int32, device=dev)
    perm = torch.empty(nnz, dtype=torch.int32, device=dev)
    nbytes = csr_transpose_workspace_bytes(n_cols, nnz, Ap.dtype)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    size = C.c_size_t(nbytes)
    with torch.cuda.device(dev):
        st = lib().mi355_spmv_csr_transpose(OFF_TYPES[Ap.dtype][0], n_rows, n_cols, nnz, _ptr(Ap), _ptr_or_null(Aj), _ptr(Apt),
                                            _ptr_or_null(Ajt), _ptr_or_null(perm), _ptr(ws), C.byref(size), _stream_ptr(stream))
    _check(st, "mi355_spmv_csr_transpose")
    return Apt, Ajt, perm


def csr_transpose_workspace_bytes(n_cols, nnz, off_dtype=torch.int32):
    """Device workspace mi355_spmv_csr_transpose needs (the size query: no device is touched)."""
    ws = C.c_size_t(0)
    st = lib().mi355_spmv_csr_transpose(OFF_TYPES[off_dtype][0], 1 if nnz else 0, n_cols, nnz, None, None, None, None, None, None,
                                        C.byref(ws), None)
    _check(st, "mi355_spmv_csr_transpose (size query)")
    return ws.value


class TransposedMultiPlan(MultiPlan):
    """mi355_spmv_multi_create_transposed: Y = alpha * A^T X + beta * Y for up to k_max vectors, with A given as it is held —
    Ap, Aj (n_rows x n_cols) — and Ax, at execute, in A's own CSR order: the plan builds the structure of A^T once and
    reads the values through a slot map, so values that change on every step are never gathered or copied.  X is
    n_rows x k, Y is n_cols x k.  float32 / float64.  The plan owns its structure: Ap and Aj are not retained."""

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, val_dtype, k_max, stream=None):
        _require_structure(Ap, Aj)
        if val_dtype not in (torch.float32, torch.float64):
            raise TypeError("val_dtype must be float32 or float64")
        if Ap.dtype not in OFF_TYPES:
            raise TypeError("Ap must be int32 or int64")
        if Ap.numel() < n_rows + 1 or Aj.numel() < nnz:
            raise ValueError("Ap or Aj shorter than the matrix")
        # as a MultiPlan sees it: the rows of A^T are the columns of A
        self.n_rows, self.n_cols, self.nnz, self.k_max, self.n_values = n_cols, n_rows, nnz, k_max, nnz
        self.val_dtype, self.mat_dtype, self.pattern, self.permuted = val_dtype, val_dtype, False, True
        self.off_dtype, self.device = Ap.dtype, Ap.device
        self.Ap = self.Aj = None
        self._h = C.c_void_p()
        with torch.cuda.device(Ap.device):
            st = lib().mi355_spmv_multi_create_transposed(
                C.byref(self._h), OFF_TYPES[Ap.dtype][0], VAL_TYPES[val_dtype][0], n_rows, n_cols, nnz, _ptr(Ap), _ptr_or_null(Aj),
                k_max, _stream_ptr(stream))
        _check(st, "mi355_spmv_multi_create_transposed")

    def structure(self, stream=None):
        """(Apt, Ajt, perm): copies of the plan's CSR structure of A^T and its slot map, as csr_transpose returns them."""
        Apt = torch.empty(self.n_rows + 1, dtype=self.off_dtype, device=self.device)
        Ajt = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        perm = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            st = lib().mi355_spmv_multi_copy_structure(self._h, _ptr_or_null(Apt), _ptr_or_null(Ajt), _ptr_or_null(perm),
                                                       _stream_ptr(stream))
        _check(st, "mi355_spmv_multi_copy_structure")
        return Apt, Ajt, perm


def spmm_t(n_rows, n_cols, nnz, Ap, Aj, Ax, X, Y, stream=None):
    """One-shot Y = A^T X for the k = X.size(1) vectors of a row-major X (n_rows x k; Y is n_cols x k), Ax in A's CSR order:
    mi355_spmv_multi_transposed_<off>_<val> — create, execute, synchronise the stream, destroy."""
    _require_structure(Ap, Aj, Ax)
    if Ax.dtype not in (torch.float32, torch.float64):
        raise TypeError("Ax must be float32 or float64")
    if Ax.numel() < nnz or Aj.numel() < nnz or Ap.numel() < n_rows + 1:
        raise ValueError("operand shorter than the matrix")
    ldx, ldy = _require_vectors(X, n_rows, Y, n_cols, Ax.dtype)
    _refuse_alias(X, Y)
    name = "mi355_spmv_multi_transposed_%s_%s" % (OFF_TYPES[Ap.dtype][1], VAL_TYPES[Ax.dtype][1])
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(X), ldx, _ptr(Y), ldy, X.size(1),
                                  _stream_ptr(stream))
    _check(st, name)
    return Y


def spmm(n_rows, n_cols, nnz, Ap, Aj, Ax, X, Y, stream=None, semiring="plus_times"):
    """One-shot Y = A X for the k = X.size(1) vectors of a row-major X: create, execute, synchronise the stream,
    destroy.  (+, *) on float values: mi355_spmv_multi_<off>_<val>; another semiring, or int32 values:
    mi355_spmv_multi_genl_<off>_<val>; float16 / bfloat16 Ax, X and Y under (+, *): mi355_spmv_multi_half_<off>_<val>
    (fp32 arithmetic, Y rounded once)."""
    _require_structure(Ap, Aj, Ax)
    sr = _semiring_id(semiring)
    genl = sr != 0 or Ax.dtype == torch.int32
    half = sr == 0 and Ax.dtype in MAT_TYPES
    if not half and Ax.dtype not in ((torch.float32, torch.float64, torch.int32) if genl else (torch.float32, torch.float64)):
        raise TypeError("Ax must be float32 or float64" + (" or int32" if genl else ""))
    if Ax.numel() < nnz:
        raise ValueError("operand shorter than the matrix")
    ldx, ldy = _require_vectors(X, n_cols, Y, n_rows, Ax.dtype)
    o, v = OFF_TYPES[Ap.dtype][1], (MAT_TYPES if half else VAL_TYPES)[Ax.dtype][1]
    name = "mi355_spmv_multi_%s%s_%s" % ("half_" if half else "genl_" if genl else "", o, v)
    args = (n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(X), ldx, _ptr(Y), ldy, X.size(1), _stream_ptr(stream))
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(*(((sr,) if genl else ()) + args))
    _check(st, name)
    return Y


def spmm_pattern(semiring, n_rows, n_cols, nnz, Ap, Aj, X, Y, stream=None):
    """One-shot multi-vector SpMV with a PATTERN matrix — a structure and no values, every entry one
    (mi355_spmv_multi_pattern_<off>_<val>): the arguments of spmm without Ax, the semiring first as in spmv_pattern."""
    sr = _semiring_id(semiring)
    _require_structure(Ap, Aj)
    _require_on_device(X)
    if X.dtype not in VAL_TYPES:
        raise TypeError("X must be float32, float64 or int32")
    ldx, ldy = _require_vectors(X, n_cols, Y, n_rows, X.dtype)
    name = "mi355_spmv_multi_pattern_%s_%s" % (OFF_TYPES[Ap.dtype][1], VAL_TYPES[X.dtype][1])
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(sr, n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), _ptr(X), ldx, _ptr(Y), ldy, X.size(1),
                                  _stream_ptr(stream))
    _check(st, name)
    return Y


# ---- SDDMM, row softmax, fused sparse attention and its backward

# What separates a one-shot on 16-bit matrices from its full-precision sibling: (the types its first operand may have,
# each with its entry suffix; how the refusal names them; the value type — None: the operand's own; the entry stem).
_FULL = ({torch.float32: "f32", torch.float64: "f64"}, "float32 or float64", None, "")
_HALF = ({dt: s for dt, (_, s) in MAT_TYPES.items()}, "float16 or bfloat16", torch.float32, "half_")


def _one_shot_value_type(variant, Ap, Aj, first, first_name):
    """The opening of such a one-shot: the structure, then its first operand's device and type -> the value type."""
    types, words, val_dtype, _ = variant
    _require_structure(Ap, Aj)
    _require_on_device(first)
    if first.dtype not in types:
        raise TypeError("%s must be %s" % (first_name, words))
    return val_dtype or first.dtype


def _one_shot_entry(variant, family, Ap, first):
    """mi355_spmv_<family>_[half_]<off>_<val>, named once every operand has passed."""
    types, _, _, stem = variant
    return "mi355_spmv_%s_%s%s_%s" % (family, stem, OFF_TYPES[Ap.dtype][1], types[first.dtype])


def _sddmm_operands(n_rows, n_cols, nnz, val_dtype, Ax, U, V, out, k, vec_dtype=None):
    """The checks of an SDDMM execute, in MultiPlan's words: (Ax or None, ldu, ldv, out, k).  vec_dtype: the type of U and V
    where it is not val_dtype (a 16-bit plan)."""
    vec_dtype = val_dtype if vec_dtype is None else vec_dtype
    if Ax is not None:
        _require_device(Ax)
        if Ax.dtype != val_dtype:
            raise TypeError("value type differs from the plan's")
        if Ax.numel() < nnz:
            raise ValueError("operand shorter than the plan's sizes")
    ldu = _require_matrix(U, "U", n_rows, vec_dtype)
    ldv = _require_matrix(V, "V", n_cols, vec_dtype)
    if k is None:
        k = U.size(1)
    if k < 1 or k > U.size(1) or k > V.size(1):
        raise ValueError("k outside 1 .. the columns U and V hold")
    if out is None:
        out = torch.empty(nnz, dtype=val_dtype, device=U.device)
    else:
        _require_device(out)
        if out.dtype != val_dtype:
            raise TypeError("value type differs from the plan's")
        if out.dim() != 1 or out.numel() < nnz:
            raise ValueError("operand shorter than the plan's sizes")
    return Ax, ldu, ldv, out, k


class SddmmPlan(_Handle):
    """mi355_spmv_sddmm_*: out[n] = alpha * s[n] * dot(U[r(n), :k], V[Aj[n], :k]) + beta * out[n] for every stored entry n
    of A, in one pass over A and one kernel for any k; s = Ax, or 1 with Ax=None (a pattern matrix).  U (n_rows x k) and
    V (n_cols x k) are 2-D row-major device tensors; views with a larger stride(0) are taken as they are.  out holds nnz
    values in CSR order.  val_dtype is float32 or float64.  The gradient of spmm with respect to Ax is
    SddmmPlan.execute(None, dY, X).  Holds references to Ap and Aj so they outlive the object; creating one touches no
    device memory.

    vec_dtype=torch.float16 / torch.bfloat16 (mi355_spmv_sddmm_create_half; val_dtype must be float32): U and V are held
    in that type, Ax and out stay float32, every stored value is widened exactly and products and sums are float32.
    plan.vec_dtype is the type of U and V (val_dtype without the argument)."""
    _destroy = "mi355_spmv_sddmm_destroy"

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, val_dtype, vec_dtype=None):
        _require_structure(Ap, Aj)
        if val_dtype not in (torch.float32, torch.float64):
            raise TypeError("val_dtype must be float32 or float64")
        if vec_dtype is not None:
            if vec_dtype not in MAT_TYPES:
                raise TypeError("vec_dtype must be float16 or bfloat16 (or None: U and V in val_dtype)")
            if val_dtype != torch.float32:
                raise TypeError("vec_dtype needs val_dtype float32 (16-bit U and V under float32 Ax and out)")
        self.n_rows, self.n_cols, self.nnz = n_rows, n_cols, nnz
        self.Ap, self.Aj, self.val_dtype = Ap, Aj, val_dtype
        self.vec_dtype = val_dtype if vec_dtype is None else vec_dtype
        self._h = C.c_void_p()
        args = (n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj))
        if vec_dtype is None:
            _check(lib().mi355_spmv_sddmm_create(C.byref(self._h), OFF_TYPES[Ap.dtype][0], VAL_TYPES[val_dtype][0], *args),
                   "mi355_spmv_sddmm_create")
        else:
            _check(lib().mi355_spmv_sddmm_create_half(C.byref(self._h), OFF_TYPES[Ap.dtype][0], MAT_TYPES[vec_dtype][0], *args),
                   "mi355_spmv_sddmm_create_half")

    def execute(self, Ax, U, V, out=None, k=None, stream=None):
        """Asynchronous on `stream` (default: torch's current stream); returns out (made when None: then beta must be 0).
        k defaults to U.size(1); ldu / ldv are the operands' stride(0)."""
        Ax, ldu, ldv, out, k = _sddmm_operands(self.n_rows, self.n_cols, self.nnz, self.val_dtype, Ax, U, V, out, k, self.vec_dtype)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_sddmm_execute(self._h, _ptr(Ax), _ptr(U), ldu, _ptr(V), ldv, _ptr(out), k, _stream_ptr(stream))
        _check(st, "mi355_spmv_sddmm_execute")
        return out

    def set_alpha_beta(self, alpha, beta):
        """out = alpha * s * dot + beta * out for the following executes (default 1, 0)."""
        self._call("mi355_spmv_sddmm_set_alpha_beta", C.c_double(alpha), C.c_double(beta))

    def info(self):
        return self._info(SddmmInfo, "mi355_spmv_sddmm_get_info")


def _sddmm(variant, n_rows, n_cols, nnz, Ap, Aj, Ax, U, V, out, stream):
    val_dtype = _one_shot_value_type(variant, Ap, Aj, U, "U")
    Ax, ldu, ldv, out, k = _sddmm_operands(n_rows, n_cols, nnz, val_dtype, Ax, U, V, out, None, U.dtype)
    name = _one_shot_entry(variant, "sddmm", Ap, U)
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(U), ldu, _ptr(V), ldv, _ptr(out), k,
                                  _stream_ptr(stream))
    _check(st, name)
    return out


def sddmm(n_rows, n_cols, nnz, Ap, Aj, Ax, U, V, out=None, stream=None):
    """One-shot SDDMM (mi355_spmv_sddmm_<off>_<val>): out[n] = s[n] * dot(U[r(n)], V[Aj[n]]) for the k = U.size(1) columns
    of row-major U and V; Ax=None is a pattern matrix.  Asynchronous on `stream`: it does not synchronise."""
    return _sddmm(_FULL, n_rows, n_cols, nnz, Ap, Aj, Ax, U, V, out, stream)


def sddmm_half(n_rows, n_cols, nnz, Ap, Aj, Ax, U, V, out=None, stream=None):
    """One-shot SDDMM on 16-bit U and V (mi355_spmv_sddmm_half_<off>_<f16|bf16>): sddmm's arguments with U and V in one of
    float16 / bfloat16, Ax (or None) and out in float32.  Asynchronous on `stream`: it does not synchronise."""
    return _sddmm(_HALF, n_rows, n_cols, nnz, Ap, Aj, Ax, U, V, out, stream)


class RowSoftmaxPlan(_Handle):
    """mi355_spmv_row_softmax_*: the softmax of scale * x over the stored entries of every row of A ("edge softmax"), and
    its gradient.  x, out, p, dp and the gradient are contiguous 1-D device tensors of nnz values in CSR order, float32 or
    float64 (val_dtype).  An entry of -inf is a masked edge and gives exactly 0; a row that is masked whole gives zeros;
    empty rows write nothing.  In place is allowed: execute(x, out=x), backward(p, dp, out=dp) or out=p.  Holds
    references to Ap and Aj (Aj is not read) so they outlive the object; creating one allocates O(n_slices) bytes of
    scratch on Ap's device (info()["scratch_bytes"]).  Executes are asynchronous and never synchronise."""
    _destroy = "mi355_spmv_row_softmax_destroy"

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, val_dtype):
        _require_structure(Ap, Aj)
        if val_dtype not in (torch.float32, torch.float64):
            raise TypeError("val_dtype must be float32 or float64")
        self.n_rows, self.n_cols, self.nnz = n_rows, n_cols, nnz
        self.Ap, self.Aj, self.val_dtype = Ap, Aj, val_dtype
        self._h = C.c_void_p()
        # (nothing stored: create makes no device call, and no device need exist)
        with torch.cuda.device(Ap.device) if nnz > 0 and n_rows > 0 else contextlib.nullcontext():
            st = lib().mi355_spmv_row_softmax_create(C.byref(self._h), OFF_TYPES[Ap.dtype][0], VAL_TYPES[val_dtype][0], n_rows, n_cols,
                                                     nnz, _ptr(Ap), _ptr(Aj))
        _check(st, "mi355_spmv_row_softmax_create")

    def _out(self, out, like):
        if out is None:
            return torch.empty(self.nnz, dtype=self.val_dtype, device=like.device)
        return _edge_values(out, "out", self.nnz, self.val_dtype)

    def execute(self, x, out=None, stream=None):
        """out = softmax over each row of scale * x; asynchronous on `stream` (default: torch's current stream); returns
        out (made when None; out may be x)."""
        x = _edge_values(x, "x", self.nnz, self.val_dtype)
        out = self._out(out, x)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_row_softmax_execute(self._h, _ptr(x), _ptr(out), _stream_ptr(stream))
        _check(st, "mi355_spmv_row_softmax_execute")
        return out

    def backward(self, p, dp, out=None, stream=None):
        """out = scale * p * (dp - sum over the row of p * dp), p an execute's output; returns out (made when None; out
        may be dp or p)."""
        p = _edge_values(p, "p", self.nnz, self.val_dtype)
        dp = _edge_values(dp, "dp", self.nnz, self.val_dtype)
        out = self._out(out, p)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_row_softmax_backward(self._h, _ptr(p), _ptr(dp), _ptr(out), _stream_ptr(stream))
        _check(st, "mi355_spmv_row_softmax_backward")
        return out

    def set_scale(self, s):
        """scale for the following executes and backwards (default 1): the 1 / sqrt(d) of attention."""
        self._call("mi355_spmv_row_softmax_set_scale", C.c_double(s))

    def info(self):
        return self._info(RowSoftmaxInfo, "mi355_spmv_row_softmax_get_info")


def row_softmax(n_rows, n_cols, nnz, Ap, Aj, x, out=None, scale=1.0, stream=None):
    """One-shot row softmax (mi355_spmv_row_softmax_<off>_<val>): out = softmax over each row of scale * x, x and out nnz
    values in CSR order (out may be x).  Synchronises `stream` before returning: its scratch lives for the call."""
    _one_shot_value_type(_FULL, Ap, Aj, x, "x")
    x = _edge_values(x, "x", nnz, x.dtype)
    out = torch.empty(nnz, dtype=x.dtype, device=x.device) if out is None else _edge_values(out, "out", nnz, x.dtype)
    name = _one_shot_entry(_FULL, "row_softmax", Ap, x)
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), _ptr(x), _ptr(out), C.c_double(scale), _stream_ptr(stream))
    _check(st, name)
    return out


def _heads_of(matrices):
    """The ranks of an attention execute's matrices [(tensor or None, name)]: 0 when every one is 2-D (the single-head call),
    else H of 3-D operands shaped (rows, H, width), which must all agree (the library refuses H above the plan's reserve)."""
    given = [(t, name) for t, name in matrices if t is not None]
    for t, _ in given:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU_PATH)
    ranks = {t.dim() for t, _ in given}
    if ranks == {2}:
        return 0
    if ranks != {3}:
        raise ValueError("%s: %s (every matrix 2-D, or every matrix 3-D shaped (rows, H, width))"
                         % ("mixed ranks" if len(ranks) > 1 else "matrices must be 2-D or 3-D",
                            ", ".join("%s is %d-D" % (name, t.dim()) for t, name in given)))
    heads = {t.size(1) for t, _ in given}
    if len(heads) != 1:
        raise ValueError("the matrices differ in their heads: %s" % ", ".join("%s has %d" % (name, t.size(1)) for t, name in given))
    H = heads.pop()
    if H < 1:
        raise ValueError("3-D operands need at least one head")
    return H


def _head0(t):
    """Head 0 of a 3-D matrix as the 2-D operand that every matrix check takes (None stays None)."""
    return None if t is None else t.select(1, 0)


def _head_vector(t, name, H, n):
    """A per-head vector operand, (H, n) with unit stride along n — or, for an input, (n,) shared by all heads: (head 0 as a
    1-D tensor, the head stride).  None: (None, 0)."""
    if t is None:
        return None, 0
    if t.dim() == 1:
        return t, 0
    if t.dim() != 2 or t.size(0) != H:
        raise ValueError("%s must be (H, %s) = (%d, %d)" % (name, name, H, n))
    if t.size(1) > 1 and t.stride(1) != 1:
        raise ValueError("%s must have unit stride along its last dimension" % name)
    return t[0], (t.stride(0) if H > 1 else 0)


class _AttentionHeads:
    """reserve_heads and n_heads_max of the three attention plans (`_stem` names the C object's entry points)."""
    _stem = None

    @classmethod
    def with_heads(cls, n_heads_max, *args, **kwargs):
        """cls(*args, **kwargs) with scratch reserved for n_heads_max heads."""
        plan = cls(*args, **kwargs)
        if n_heads_max > 1:
            plan.reserve_heads(n_heads_max)
        return plan

    def reserve_heads(self, n_heads_max):
        """Scratch for up to n_heads_max heads in one execute (mi355_spmv_attention[_bwd]_reserve_heads): a device call
        like the create — not during stream capture, not with an execute in flight."""
        with torch.cuda.device(self.Ap.device) if self.n_rows > 0 else contextlib.nullcontext():
            self._call(self._stem + "_reserve_heads", int(n_heads_max))

    @property
    def n_heads_max(self):
        n = C.c_int32()
        self._call(self._stem + "_get_heads_max", C.byref(n))
        return n.value


def _attention_operands(n_rows, n_cols, nnz, val_dtype, Q, K, V, out, lse, bias, d_max=None, dv_max=None, vec_dtype=None):
    """The operand checks of a fused sparse attention: (d, dv, ldq, ldk, ldv, out, ldo).  Q, K, V and out are 2-D device
    tensors of vec_dtype (the value type when None) with unit stride along their columns (any row stride >= the width: a
    column slice of a wider tensor is taken as it is); bias and lse are contiguous 1-D tensors of nnz and n_rows values of
    the value type, or None."""
    vec_dtype = val_dtype if vec_dtype is None else vec_dtype
    ldq, ldk, ldv = _require_matrix(Q, "Q", n_rows, vec_dtype), _require_matrix(K, "K", n_cols, vec_dtype), _require_matrix(V, "V", n_cols, vec_dtype)
    d, dv = Q.size(1), V.size(1)
    if K.size(1) != d:
        raise ValueError("Q and K differ in their columns (%d, %d)" % (d, K.size(1)))
    if d < 1 or dv < 1:
        raise ValueError("Q, K and V need at least one column")
    if (d_max is not None and d > d_max) or (dv_max is not None and dv > dv_max):
        raise ValueError("d = %d or dv = %d above the plan's d_max = %s, dv_max = %s" % (d, dv, d_max, dv_max))
    if out is None:
        out = torch.empty((n_rows, dv), dtype=vec_dtype, device=Q.device)
    ldo = _require_matrix(out, "out", n_rows, vec_dtype)
    if out.size(1) != dv:
        raise ValueError("out has %d columns, V has %d" % (out.size(1), dv))
    if lse is not None:
        _edge_values(lse, "lse", n_rows, val_dtype)
    if bias is not None:
        _edge_values(bias, "bias", nnz, val_dtype)
    return d, dv, ldq, ldk, ldv, out, ldo


class SparseAttentionPlan(_AttentionHeads, _Handle):
    """mi355_spmv_attention_*: fused sparse attention on the structure of A, O = softmax(scale * Q K^T + bias, over the
    stored entries of every row) V in ONE pass over A — the chain SddmmPlan -> RowSoftmaxPlan -> MultiPlan without the
    nnz-sized scores and probabilities.  Q is n_rows x d, K n_cols x d, V n_cols x dv (row-major device tensors of
    val_dtype, float32 or float64; d <= d_max, dv <= dv_max; a row stride above the width is taken as the leading
    dimension), bias nnz values in CSR order or None; bias[n] = -inf masks an edge.  A row that is empty or masked whole
    gives zeros and lse = -inf.  out and lse must not overlap an input.  Holds references to Ap and Aj so they outlive the
    object; creating one allocates O(n_slices * dv_max) bytes of scratch on Ap's device (info()["scratch_bytes"]).
    Executes are asynchronous and never synchronise.
    vec_dtype=torch.float16 / torch.bfloat16 (mi355_spmv_attention_create_half; val_dtype must be float32): Q, K, V and out
    are held in that type; bias, lse, the scale and every operation stay float32, every stored value is widened exactly and
    an element of out is rounded to vec_dtype once.  plan.vec_dtype is the type of Q, K, V and out (val_dtype without the
    argument).
    Heads in one call: n_heads_max=H (or reserve_heads(H)) reserves H copies of the scratch; execute then takes 3-D
    operands shaped (rows, H, width) — see execute."""
    _destroy = "mi355_spmv_attention_destroy"
    _stem = "mi355_spmv_attention"

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, val_dtype, d_max, dv_max, vec_dtype=None, n_heads_max=1):
        _require_structure(Ap, Aj)
        if val_dtype not in (torch.float32, torch.float64):
            raise TypeError("val_dtype must be float32 or float64")
        if vec_dtype is not None:
            if vec_dtype not in MAT_TYPES:
                raise TypeError("vec_dtype must be float16 or bfloat16 (or None: Q, K, V and out in val_dtype)")
            if val_dtype != torch.float32:
                raise TypeError("vec_dtype needs val_dtype float32 (16-bit Q, K, V and out under float32 bias and lse)")
        self.n_rows, self.n_cols, self.nnz = n_rows, n_cols, nnz
        self.Ap, self.Aj, self.val_dtype = Ap, Aj, val_dtype
        self.vec_dtype = val_dtype if vec_dtype is None else vec_dtype
        self.d_max, self.dv_max = d_max, dv_max
        self._h = C.c_void_p()
        # (no rows: create makes no device call, and no device need exist)
        with torch.cuda.device(Ap.device) if n_rows > 0 else contextlib.nullcontext():
            if vec_dtype is None:
                # Deliberate: the handle goes LAST here, and here alone (include/mi355_spmv.h, mi355_spmv_attention_create)
                st, name = lib().mi355_spmv_attention_create(n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), OFF_TYPES[Ap.dtype][0],
                                                             VAL_TYPES[val_dtype][0], d_max, dv_max, C.byref(self._h)), "mi355_spmv_attention_create"
            else:
                st, name = lib().mi355_spmv_attention_create_half(C.byref(self._h), OFF_TYPES[Ap.dtype][0], MAT_TYPES[vec_dtype][0], n_rows,
                                                                  n_cols, nnz, _ptr(Ap), _ptr(Aj), d_max, dv_max), "mi355_spmv_attention_create_half"
        _check(st, name)
        if n_heads_max > 1:
            self.reserve_heads(n_heads_max)

    def execute(self, Q, K, V, out=None, lse=None, bias=None, stream=None):
        """out[r] = sum over the row of softmax(scale * Q[r] . K[c] + bias)[n] * V[c]; lse (n_rows values, optional) takes
        the row's log-sum-exp.  Asynchronous on `stream` (default: torch's current stream); returns out (made when None).
        Heads in one call (mi355_spmv_attention_execute_heads): Q, K, V (and out) 3-D, shaped (rows, H, width) with unit
        stride in the last dimension and ANY other strides — (n, H, d) contiguous is the interleaved layout, a head-major
        (H, n, d) tensor is passed as t.permute(1, 0, 2), and a stride of 0 from expand shares K, V or Q between the heads.
        bias is (H, nnz), or (nnz,) shared by all heads; lse is (H, n_rows); out is made as a contiguous (n_rows, H, dv)
        when None.  Head h equals the 2-D call on head h's operands bit for bit.  Mixed ranks are a ValueError."""
        H = _heads_of(((Q, "Q"), (K, "K"), (V, "V"), (out, "out")))
        if H:
            return self._execute_heads(H, Q, K, V, out, lse, bias, stream)
        d, dv, ldq, ldk, ldv, out, ldo = _attention_operands(self.n_rows, self.n_cols, self.nnz, self.val_dtype, Q, K, V, out, lse, bias,
                                                             self.d_max, self.dv_max, self.vec_dtype)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_attention_execute(self._h, d, dv, _ptr(Q), ldq, _ptr(K), ldk, _ptr(V), ldv, _ptr(bias), _ptr(out), ldo,
                                                    _ptr(lse), _stream_ptr(stream))
        _check(st, "mi355_spmv_attention_execute")
        return out

    def _execute_heads(self, H, Q, K, V, out, lse, bias, stream):
        if out is None:
            out = torch.empty((self.n_rows, H, V.size(2)), dtype=self.vec_dtype, device=Q.device)
        lse0, s_lse = _head_vector(lse, "lse", H, self.n_rows)
        if lse is not None and lse.dim() != 2:
            raise ValueError("lse must be (H, n_rows) with 3-D operands")
        bias0, s_bias = _head_vector(bias, "bias", H, self.nnz)
        d, dv, ldq, ldk, ldv, out0, ldo = _attention_operands(self.n_rows, self.n_cols, self.nnz, self.val_dtype, _head0(Q), _head0(K), _head0(V),
                                                              _head0(out), lse0, bias0, self.d_max, self.dv_max, self.vec_dtype)
        hs = AttentionHeadStrides(Q.stride(1), K.stride(1), V.stride(1), s_bias, out.stride(1), s_lse)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_attention_execute_heads(self._h, H, C.byref(hs), d, dv, _ptr(Q), ldq, _ptr(K), ldk, _ptr(V), ldv, _ptr(bias), _ptr(out),
                                                          ldo, _ptr(lse), _stream_ptr(stream))
        _check(st, "mi355_spmv_attention_execute_heads")
        return out

    def set_scale(self, s):
        """scale for the following executes (default 1): the 1 / sqrt(d) of attention; one scale for all heads."""
        self._call("mi355_spmv_attention_set_scale", C.c_double(s))

    def info(self):
        return self._info(AttentionInfo, "mi355_spmv_attention_get_info")


def _sparse_attention(variant, n_rows, n_cols, nnz, Ap, Aj, Q, K, V, bias, scale, out, lse, stream):
    val_dtype = _one_shot_value_type(variant, Ap, Aj, Q, "Q")
    d, dv, ldq, ldk, ldv, out, ldo = _attention_operands(n_rows, n_cols, nnz, val_dtype, Q, K, V, out, lse, bias, vec_dtype=Q.dtype)
    name = _one_shot_entry(variant, "attention", Ap, Q)
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), d, dv, _ptr(Q), ldq, _ptr(K), ldk, _ptr(V), ldv, _ptr(bias),
                                  C.c_double(scale), _ptr(out), ldo, _ptr(lse), _stream_ptr(stream))
    _check(st, name)
    return out


def sparse_attention(n_rows, n_cols, nnz, Ap, Aj, Q, K, V, bias=None, scale=1.0, out=None, lse=None, stream=None):
    """One-shot fused sparse attention (mi355_spmv_attention_<off>_<val>): SparseAttentionPlan's execute on a plan made for
    the call.  Synchronises `stream` before returning: its scratch lives for the call."""
    return _sparse_attention(_FULL, n_rows, n_cols, nnz, Ap, Aj, Q, K, V, bias, scale, out, lse, stream)


def sparse_attention_half(n_rows, n_cols, nnz, Ap, Aj, Q, K, V, bias=None, scale=1.0, out=None, lse=None, stream=None):
    """One-shot fused sparse attention on 16-bit Q, K, V and out (mi355_spmv_attention_half_<off>_<f16|bf16>):
    sparse_attention's arguments with Q, K, V (and out) in one of float16 / bfloat16, bias and lse in float32.  Synchronises
    `stream` before returning: its scratch lives for the call."""
    return _sparse_attention(_HALF, n_rows, n_cols, nnz, Ap, Aj, Q, K, V, bias, scale, out, lse, stream)


def _attention_backward_operands(n_rows, n_cols, nnz, val_dtype, Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias, need, d_max=None, dv_max=None,
                                 vec_dtype=None):
    """The operand checks of a fused attention backward: (d, dv, the leading dimensions of Q, K, V, O, dO, then dQ, dK, dV,
    dbias — made where asked for by `need` and not given — and their leading dimensions, 0 for an output that is None).
    Q, K, V, O, dO and dQ, dK, dV are of vec_dtype (the value type when None); lse, bias and dbias of the value type."""
    vec_dtype = val_dtype if vec_dtype is None else vec_dtype
    if vec_dtype != val_dtype:      # the 16-bit object: which of the eight matrices is in another type
        for t, name in ((Q, "Q"), (K, "K"), (V, "V"), (O, "O"), (dO, "dO"), (dQ, "dQ"), (dK, "dK"), (dV, "dV")):
            if t is not None and getattr(t, "dtype", vec_dtype) != vec_dtype:
                raise TypeError("%s is %s: the plan's vec_dtype is %s" % (name, t.dtype, vec_dtype))
    ldq, ldk, ldv = _require_matrix(Q, "Q", n_rows, vec_dtype), _require_matrix(K, "K", n_cols, vec_dtype), _require_matrix(V, "V", n_cols, vec_dtype)
    ldo, lddo = _require_matrix(O, "O", n_rows, vec_dtype), _require_matrix(dO, "dO", n_rows, vec_dtype)
    d, dv = Q.size(1), V.size(1)
    if K.size(1) != d:
        raise ValueError("Q and K differ in their columns (%d, %d)" % (d, K.size(1)))
    if O.size(1) != dv or dO.size(1) != dv:
        raise ValueError("O and dO need V's %d columns (%d, %d)" % (dv, O.size(1), dO.size(1)))
    if d < 1 or dv < 1:
        raise ValueError("Q, K and V need at least one column")
    if (d_max is not None and d > d_max) or (dv_max is not None and dv > dv_max):
        raise ValueError("d = %d or dv = %d above the plan's d_max = %s, dv_max = %s" % (d, dv, d_max, dv_max))
    _edge_values(lse, "lse", n_rows, val_dtype)
    if bias is not None:
        _edge_values(bias, "bias", nnz, val_dtype)
    need = tuple(bool(x) for x in need)
    if len(need) != 3:
        raise ValueError("need is (dQ, dK, dV)")
    outs, lds = [], []
    for t, name, want, rows, width in ((dQ, "dQ", need[0], n_rows, d), (dK, "dK", need[1], n_cols, d), (dV, "dV", need[2], n_cols, dv)):
        if t is None and want:
            t = torch.empty((rows, width), dtype=vec_dtype, device=Q.device)
        if t is not None:
            lds.append(_require_matrix(t, name, rows, vec_dtype))
            if t.size(1) != width:
                raise ValueError("%s has %d columns, not %d" % (name, t.size(1), width))
        else:
            lds.append(0)
        outs.append(t)
    if not any(t is not None for t in outs):
        raise ValueError("none of dQ, dK and dV is asked for")
    if dbias is True:
        dbias = torch.empty((nnz,), dtype=val_dtype, device=Q.device)
    if dbias is not None:
        if outs[0] is None:
            raise ValueError("dbias needs dQ (it comes from the walk that makes dQ)")
        _edge_values(dbias, "dbias", nnz, val_dtype)
    return d, dv, ldq, ldk, ldv, ldo, lddo, outs[0], outs[1], outs[2], dbias, lds


class SparseAttentionBackwardPlan(_AttentionHeads, _Handle):
    """mi355_spmv_attention_bwd_*: the fused backward of SparseAttentionPlan — dQ, dK, dV (and dbias) from Q, K, V, bias, the
    forward's O and lse, and dO, with nothing of nnz size kept between forward and backward.  One plan per STRUCTURE: it
    holds the transpose of A (info()["held_bytes"]), built at create on `stream` (which is synchronised), and serves every
    head, layer and step on that structure.  dtype is float32 or float64; Q is n_rows x d, K n_cols x d, V n_cols x dv, O
    and dO n_rows x dv (row-major device tensors, d <= d_max, dv <= dv_max, a row stride above the width is the leading
    dimension); lse n_rows values, bias nnz values in CSR order or None.  Holds references to Ap and Aj.  Executes are
    asynchronous and never synchronise.
    Heads in one call: reserve_heads(H), or making the plan with with_heads(H, ...), reserves H copies of the scratch (not of
    the transpose, which the heads share); execute then takes 3-D operands shaped (rows, H, width) — see execute."""
    _destroy = "mi355_spmv_attention_bwd_destroy"
    _stem = "mi355_spmv_attention_bwd"

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, dtype, d_max, dv_max, stream=None):
        _require_structure(Ap, Aj)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("dtype must be float32 or float64 (16-bit operands: SparseAttentionBackwardHalfPlan)")
        self._create("mi355_spmv_attention_bwd_create", VAL_TYPES[dtype][0], n_rows, n_cols, nnz, Ap, Aj, dtype, dtype, d_max, dv_max, stream)

    def _create(self, entry, type_code, n_rows, n_cols, nnz, Ap, Aj, val_dtype, vec_dtype, d_max, dv_max, stream):
        """The object of checked arguments: `entry` is create (type_code a value type) or create_half (a 16-bit type)."""
        self.n_rows, self.n_cols, self.nnz = n_rows, n_cols, nnz
        self.Ap, self.Aj, self.val_dtype = Ap, Aj, val_dtype
        self.vec_dtype = vec_dtype
        self.d_max, self.dv_max = d_max, dv_max
        self._h = C.c_void_p()
        with torch.cuda.device(Ap.device):
            st = getattr(lib(), entry)(C.byref(self._h), OFF_TYPES[Ap.dtype][0], type_code, n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), d_max,
                                       dv_max, _stream_ptr(stream))
        _check(st, entry)

    def execute(self, Q, K, V, O, dO, lse, bias=None, dQ=None, dK=None, dV=None, dbias=None, need=(True, True, True), stream=None):
        """-> (dQ, dK, dV, dbias).  need = which of dQ, dK, dV to compute (a given tensor is computed whatever need says; an
        output neither given nor needed is None and its walk is not launched).  dbias: a tensor of nnz values, True to have
        one made, or None.  Asynchronous on `stream` (default: torch's current stream).
        Heads in one call (mi355_spmv_attention_bwd_execute_heads): every matrix 3-D, shaped (rows, H, width) as
        SparseAttentionPlan.execute takes them (any strides but the last, 0 from expand on an input); lse is (H, n_rows),
        bias (H, nnz) or (nnz,) shared, dbias (H, nnz); outputs are made as contiguous (rows, H, width) where needed."""
        H = _heads_of(((Q, "Q"), (K, "K"), (V, "V"), (O, "O"), (dO, "dO"), (dQ, "dQ"), (dK, "dK"), (dV, "dV")))
        if H:
            return self._execute_heads(H, Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias, need, stream)
        d, dv, ldq, ldk, ldv, ldo, lddo, dQ, dK, dV, dbias, lds = _attention_backward_operands(
            self.n_rows, self.n_cols, self.nnz, self.val_dtype, Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias, need, self.d_max, self.dv_max,
            self.vec_dtype)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_attention_bwd_execute(self._h, d, dv, _ptr(Q), ldq, _ptr(K), ldk, _ptr(V), ldv, _ptr(bias), _ptr(O), ldo,
                                                        _ptr(dO), lddo, _ptr(lse), _ptr(dQ), lds[0], _ptr(dK), lds[1], _ptr(dV), lds[2],
                                                        _ptr(dbias), _stream_ptr(stream))
        _check(st, "mi355_spmv_attention_bwd_execute")
        return dQ, dK, dV, dbias

    def _execute_heads(self, H, Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias, need, stream):
        need = tuple(bool(x) for x in need)
        if len(need) != 3:
            raise ValueError("need is (dQ, dK, dV)")
        make = lambda t, want, rows, width: torch.empty((rows, H, width), dtype=self.vec_dtype, device=Q.device) if t is None and want else t
        dQ, dK, dV = (make(dQ, need[0], self.n_rows, Q.size(2)), make(dK, need[1], self.n_cols, K.size(2)),
                      make(dV, need[2], self.n_cols, V.size(2)))
        if dbias is True:
            dbias = torch.empty((H, self.nnz), dtype=self.val_dtype, device=Q.device)
        if lse.dim() != 2 or (dbias is not None and dbias.dim() != 2):
            raise ValueError("lse must be (H, n_rows) and dbias (H, nnz) with 3-D operands")
        lse0, s_lse = _head_vector(lse, "lse", H, self.n_rows)
        bias0, s_bias = _head_vector(bias, "bias", H, self.nnz)
        dbias0, s_dbias = _head_vector(dbias, "dbias", H, self.nnz)
        d, dv, ldq, ldk, ldv, ldo, lddo, _, _, _, _, lds = _attention_backward_operands(
            self.n_rows, self.n_cols, self.nnz, self.val_dtype, _head0(Q), _head0(K), _head0(V), _head0(O), _head0(dO), lse0, bias0, _head0(dQ),
            _head0(dK), _head0(dV), dbias0, (False, False, False), self.d_max, self.dv_max, self.vec_dtype)
        stride = lambda t: 0 if t is None else t.stride(1)
        hs = AttentionBackwardHeadStrides(Q.stride(1), K.stride(1), V.stride(1), s_bias, O.stride(1), dO.stride(1), s_lse, stride(dQ), stride(dK),
                                          stride(dV), s_dbias)
        with torch.cuda.device(self.Ap.device):
            st = lib().mi355_spmv_attention_bwd_execute_heads(self._h, H, C.byref(hs), d, dv, _ptr(Q), ldq, _ptr(K), ldk, _ptr(V), ldv, _ptr(bias),
                                                              _ptr(O), ldo, _ptr(dO), lddo, _ptr(lse), _ptr(dQ), lds[0], _ptr(dK), lds[1], _ptr(dV),
                                                              lds[2], _ptr(dbias), _stream_ptr(stream))
        _check(st, "mi355_spmv_attention_bwd_execute_heads")
        return dQ, dK, dV, dbias

    def set_scale(self, s):
        """scale for the following executes (default 1): the forward plan's."""
        self._call("mi355_spmv_attention_bwd_set_scale", C.c_double(s))

    def info(self):
        d = self._info(AttentionBackwardInfo, "mi355_spmv_attention_bwd_get_info")
        d["lanes_per_slot"] = dict(zip(("dq", "dk", "dv"), d["lanes_per_slot"]))      # one per walk
        d["passes"] = dict(zip(("dq", "dk", "dv"), d["passes"]))
        return d


class SparseAttentionBackwardHalfPlan(SparseAttentionBackwardPlan):
    """mi355_spmv_attention_bwd_create_half: SparseAttentionBackwardPlan with Q, K, V, O, dO and dQ, dK, dV held in vec_dtype
    (torch.float16 or torch.bfloat16) — the backward of SparseAttentionPlan(vec_dtype=).  lse, bias and dbias are float32
    (val_dtype), and so is every operation; every stored value is widened exactly and an element of dQ, dK or dV is rounded
    to vec_dtype once, from the float32 sum of its line.  execute, set_scale, info and destroy are the base class's."""

    def __init__(self, n_rows, n_cols, nnz, Ap, Aj, vec_dtype, d_max, dv_max, stream=None):
        if vec_dtype not in MAT_TYPES:
            raise TypeError("vec_dtype must be float16 or bfloat16 (float32 / float64 operands: SparseAttentionBackwardPlan)")
        _require_structure(Ap, Aj)
        self._create("mi355_spmv_attention_bwd_create_half", MAT_TYPES[vec_dtype][0], n_rows, n_cols, nnz, Ap, Aj, torch.float32, vec_dtype, d_max,
                     dv_max, stream)


def _sparse_attention_backward(variant, n_rows, n_cols, nnz, Ap, Aj, Q, K, V, O, dO, lse, bias, scale, dQ, dK, dV, dbias, need, stream):
    val_dtype = _one_shot_value_type(variant, Ap, Aj, Q, "Q")
    d, dv, ldq, ldk, ldv, ldo, lddo, dQ, dK, dV, dbias, lds = _attention_backward_operands(
        n_rows, n_cols, nnz, val_dtype, Q, K, V, O, dO, lse, bias, dQ, dK, dV, dbias, need, vec_dtype=Q.dtype)
    name = _one_shot_entry(variant, "attention_bwd", Ap, Q)
    with torch.cuda.device(Ap.device):
        st = getattr(lib(), name)(n_rows, n_cols, nnz, _ptr(Ap), _ptr(Aj), d, dv, _ptr(Q), ldq, _ptr(K), ldk, _ptr(V), ldv, _ptr(bias),
                                  C.c_double(scale), _ptr(O), ldo, _ptr(dO), lddo, _ptr(lse), _ptr(dQ), lds[0], _ptr(dK), lds[1], _ptr(dV),
                                  lds[2], _ptr(dbias), _stream_ptr(stream))
    _check(st, name)
    return dQ, dK, dV, dbias


def sparse_attention_backward(n_rows, n_cols, nnz, Ap, Aj, Q, K, V, O, dO, lse, bias=None, scale=1.0, dQ=None, dK=None, dV=None, dbias=None,
                              need=(True, True, True), stream=None):
    """One-shot fused attention backward (mi355_spmv_attention_bwd_<off>_<val>): SparseAttentionBackwardPlan's execute on a
    plan made for the call -> (dQ, dK, dV, dbias).  Synchronises `stream` before returning."""
    return _sparse_attention_backward(_FULL, n_rows, n_cols, nnz, Ap, Aj, Q, K, V, O, dO, lse, bias, scale, dQ, dK, dV, dbias, need, stream)


def sparse_attention_backward_half(n_rows, n_cols, nnz, Ap, Aj, Q, K, V, O, dO, lse, bias=None, scale=1.0, dQ=None, dK=None, dV=None, dbias=None,
                                   need=(True, True, True), stream=None):
    """One-shot fused attention backward on 16-bit matrices (mi355_spmv_attention_bwd_half_<off>_<f16|bf16>):
    sparse_attention_backward's arguments with Q, K, V, O, dO (and dQ, dK, dV) in one of float16 / bfloat16, lse, bias and
    dbias in float32 -> (dQ, dK, dV, dbias).  Synchronises `stream` before returning."""
    return _sparse_attention_backward(_HALF, n_rows, n_cols, nnz, Ap, Aj, Q, K, V, O, dO, lse, bias, scale, dQ, dK, dV, dbias, need, stream)


# ---- run-time functors, row blocks over the GPUs of a node

C_TYPE_NAMES = {torch.float32: "float", torch.float64: "double", torch.int32: "int", torch.int64: "long long"}


class Functor(_Handle):
    """mi355_spmv_functor_*: a generalized SpMV whose functor is C++ source text, compiled for gfx950 at run time.

    source        text defining the functor the way the reference writes one (merge_genl.cuh:19-38): a struct with
                  static initialize() / combine(nonzero, x) / reduce(lhs, rhs)
    functor_type  the type to use ("MyFunctor", "MergeFunctor<float, float, double>")
    off_dtype     torch.int32 / torch.int64;  mat / x / y: torch dtypes or C++ type names (a struct of the source)
    Compiling needs no device; .spmv() runs on the tensors' device, asynchronously on `stream`."""
    _destroy = "mi355_spmv_functor_destroy"

    def __init__(self, source, functor_type, off_dtype=torch.int32, mat=torch.float32, x=torch.float32, y=torch.float32):
        self._h = C.c_void_p()
        self.off_dtype = off_dtype
        names = [t if isinstance(t, str) else C_TYPE_NAMES[t] for t in (mat, x, y)]
        L = lib()
        st = L.mi355_spmv_functor_compile(C.byref(self._h), source.encode(), functor_type.encode(), OFF_TYPES[off_dtype][0],
                                          names[0].encode(), names[1].encode(), names[2].encode())
        self.log = (L.mi355_spmv_functor_compile_log() or b"").decode(errors="replace")
        _check(st, "mi355_spmv_functor_compile")

    def spmv(self, n_rows, n_cols, nnz, Ap, Aj, Ax, x, y, stream=None):
        _require_device(Ap, Aj, Ax, x, y)
        if Ap.dtype != self.off_dtype or Aj.dtype != torch.int32:
            raise TypeError("Functor.spmv: Ap must be %s and Aj int32" % self.off_dtype)
        # (bare addresses: the declared void* slots of lib() take them)
        self._call("mi355_spmv_functor_spmv", n_rows, n_cols, nnz, Ap.data_ptr(), Aj.data_ptr(), Ax.data_ptr(), x.data_ptr(), y.data_ptr(),
                   _stream_ptr(stream))


class DistPlan(_Handle):
    """mi355_spmv_dist_*: row blocks over the GPUs of a node, x replicated, allgatherv(y) over RCCL.

    DistPlan.local(...)  one process drives `devices` (the whole structure lives on the current device)
    DistPlan.rank(...)   one process per GPU: this rank's slice + the global cut lists + a 128-byte id
    """
    _destroy = "mi355_spmv_dist_destroy"

    def __init__(self):
        self._h = C.c_void_p()
        self._keep = ()

    @classmethod
    def local(cls, kind, n_rows, n_cols, nnz, Ap, Aj, val_dtype, parts=None, devices=None, sub_blocks=None, flags=0):
        kind = LABELS.get(kind, kind)
        _require_device(Ap, Aj)
        devices = list(devices) if devices is not None else [Ap.device.index or 0]
        if sub_blocks is None:
            sub_blocks = (parts // len(devices)) if parts else 1
        if parts is not None and parts != sub_blocks * len(devices):
            raise ValueError("parts must be len(devices) * sub_blocks")
        self = cls()
        self.kind, self.n_rows, self.n_cols, self.nnz, self.val_dtype = kind, n_rows, n_cols, nnz, val_dtype
        self._keep = (Ap, Aj)
        devs = (C.c_int * len(devices))(*devices)
        with torch.cuda.device(Ap.device):
            st = lib().mi355_spmv_dist_create_local(
                C.byref(self._h), KINDS[kind], OFF_TYPES[Ap.dtype][0], VAL_TYPES[val_dtype][0], n_rows, n_cols, nnz,
                _ptr(Ap), _ptr(Aj), len(devices), C.cast(devs, C.c_void_p), sub_blocks, flags)
        _check(st, "mi355_spmv_dist_create_local")
        return self

    @staticmethod
    def unique_id():
        """128 bytes from ONE rank; hand them to every rank by your own means."""
        buf = (C.c_char * 128)()
        _check(lib().mi355_spmv_dist_unique_id(C.cast(buf, C.c_void_p)), "mi355_spmv_dist_unique_id")
        return bytes(buf)

    @classmethod
    def rank(cls, kind, rank, world, unique_id, parts_per_rank, row_cuts, chunk_cuts, nnz_cuts, whole_shape,
             n_cols, n_rows_local, nnz_end_local, Ap_local, Aj_local, val_dtype, flags=0):
        import numpy as np
        kind = LABELS.get(kind, kind)
        _require_device(Ap_local, Aj_local)
        self = cls()
        self.kind, self.n_rows, self.n_cols, self.val_dtype = kind, int(row_cuts[-1]), n_cols, val_dtype
        self.nnz = int(nnz_cuts[-1]) - int(nnz_cuts[0])
        self._keep = (Ap_local, Aj_local)
        rc = np.ascontiguousarray(row_cuts, dtype=np.int64)
        cc = np.ascontiguousarray(chunk_cuts if chunk_cuts is not None else [0] * len(row_cuts), dtype=np.int64)
        nc = np.ascontiguousarray(nnz_cuts, dtype=np.int64)
        idbuf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        with torch.cuda.device(Ap_local.device):
            st = lib().mi355_spmv_dist_create_rank(
                C.byref(self._h), KINDS[kind], OFF_TYPES[Ap_local.dtype][0], VAL_TYPES[val_dtype][0], rank, world,
                C.cast(idbuf, C.c_void_p) if idbuf is not None else None, parts_per_rank,
                rc.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                C.cast(C.byref(whole_shape), C.c_void_p) if whole_shape is not None else None,
                n_cols, n_rows_local, nnz_end_local, _ptr(Ap_local), _ptr(Aj_local), flags)
        _check(st, "mi355_spmv_dist_create_rank")
        return self

    def cuts(self):
        import numpy as np
        n = lib().mi355_spmv_dist_parts(self._h)
        a = np.zeros(n + 1, dtype=np.int64)
        self._call("mi355_spmv_dist_cuts", a.ctypes.data_as(C.c_void_p))
        return a.tolist()

    def info(self, part=0):
        """Launch shape of this process's block `part`."""
        return self._info(PlanInfo, "mi355_spmv_dist_part_info", part)

    def scatter_values(self, Ax, stream=None):
        _require_device(Ax)
        self._call("mi355_spmv_dist_scatter_values", _ptr(Ax), _stream_ptr(stream))

    def replicate_x(self, x, stream=None):
        _require_device(x)
        self._call("mi355_spmv_dist_replicate_x", _ptr(x), _stream_ptr(stream))

    def execute(self, Ax, x, y, stream=None, flags=EXEC_DEFAULT):
        """Asynchronous on `stream`.  LOCAL: home-device Ax / x (None = unchanged since scatter_values /
        replicate_x) and the full y; RANK: this rank's values view, its x, its full-length y.
        flags: EXEC_SKIP_EXCHANGE (kernels only) / EXEC_EXCHANGE_ONLY (the allgatherv of whatever y holds)."""
        for t in (Ax, x, y):
            if t is not None:
                _require_device(t)
                if t.dtype != self.val_dtype:
                    raise TypeError("value type differs from the plan's")
        if y.numel() < self.n_rows:
            raise ValueError("y is shorter than the matrix has rows")
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(y.device):
            st = lib().mi355_spmv_dist_execute_ex(self._h, p(Ax), p(x), p(y), _stream_ptr(stream), flags)
        _check(st, "mi355_spmv_dist_execute_ex")
        return y

    def set_exchange(self, name):
        """'bcast' | 'sendrecv' | 'allgather' (collective: every rank the same)."""
        self._call("mi355_spmv_dist_set_exchange", EXCHANGES[name])

    def dist_info(self):
        d = self._info(DistInfo, "mi355_spmv_dist_get_info")
        trial_us = d.pop("trial_us")       # one time per exchange that the auto pick tried
        d["trial_us"] = {k: float(trial_us[v]) for k, v in EXCHANGES.items() if v}
        return d

    def structure_changed(self, Ap, Aj, stream=None):
        """LOCAL mode: does the caller's Ap / Aj still match the fingerprint taken at create?"""
        _require_device(Ap, Aj)
        out = C.c_int(0)
        with torch.cuda.device(Ap.device):
            st = lib().mi355_spmv_dist_structure_changed(self._h, _ptr(Ap), _ptr(Aj), _stream_ptr(stream), C.byref(out))
        _check(st, "mi355_spmv_dist_structure_changed")
        return bool(out.value)

    def set_alpha_beta(self, alpha, beta):
        self._call("mi355_spmv_dist_set_alpha_beta", C.c_double(alpha), C.c_double(beta))
