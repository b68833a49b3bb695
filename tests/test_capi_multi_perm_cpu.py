"""Transposed and permuted multi-vector SpMV without a device (mi355_spmv_csr_transpose, mi355_spmv_multi_create_permuted /
_create_transposed / _get_perm_info / _transposed_*): the names are declared with the header's signatures, exported and
bound, and the feature macro is defined; every argument error is refused before any device call with a status and a text
(on dummy pointers: nothing is dereferenced); the workspace query of csr_transpose runs without a GPU; the Python checks."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

ONE_SHOTS = ["mi355_spmv_multi_transposed_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
NAMES = ["mi355_spmv_csr_transpose", "mi355_spmv_multi_create_permuted", "mi355_spmv_multi_create_transposed",
         "mi355_spmv_multi_get_perm_info", "mi355_spmv_multi_copy_structure"] + ONE_SHOTS
OK, EINVAL, ENOTSUP = 0, 1, 2
OFF_I32, OFF_I64 = 0, 1
F32, F64, I32, PATTERN, F16, BF16 = 0, 1, 2, 3, 4, 5
DUMMY = C.c_void_p(256)


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mi355_spmv.h")).read())


def test_the_names_are_declared_exported_and_bound(sp):
    text = header()
    lib = sp.capi.lib()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, text), n
        assert hasattr(lib, n), n
        assert n in sp.capi.EXPORTS, n
    assert "#define MI355_SPMV_HAS_MULTI_TRANSPOSED 1" in text
    # the signatures, as the issue states them
    assert ("int mi355_spmv_csr_transpose(int off_type, int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, "
            "void* Apt, int32_t* Ajt, uint32_t* perm, void* workspace, size_t* workspace_bytes, void* stream);") in text
    assert ("int mi355_spmv_multi_create_permuted(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, "
            "int64_t nnz, const void* Ap, const int32_t* Aj, int perm_type, const void* perm, int64_t n_values, int32_t k_max, "
            "void* stream);") in text
    assert ("int mi355_spmv_multi_create_transposed(mi355_spmv_multi** out, int off_type, int val_type, int32_t n_rows, int32_t n_cols, "
            "int64_t nnz, const void* Ap, const int32_t* Aj, int32_t k_max, void* stream);") in text
    assert ("int mi355_spmv_multi_get_perm_info(const mi355_spmv_multi* multi, int64_t* n_values, int64_t* held_bytes, "
            "int* owns_structure);") in text
    # mi355_spmv_multi_info did not grow: 8 int32, 3 int64, 64 chars
    assert C.sizeof(sp.capi.MultiInfo) == 8 * 4 + 3 * 8 + 64
    assert sp.TransposedMultiPlan is sp.capi.TransposedMultiPlan and sp.csr_transpose is sp.capi.csr_transpose and sp.spmm_t is sp.capi.spmm_t


def refused(lib, status, want, *words):
    assert status == want, (status, lib.mi355_spmv_last_error())
    text = lib.mi355_spmv_last_error().decode()
    for w in words:
        assert w in text, (w, text)


def test_csr_transpose_refuses_bad_arguments_and_answers_the_size_query_without_a_device(sp):
    lib = sp.capi.lib()
    ws = C.c_size_t(0)
    call = lambda off, n_rows, n_cols, nnz, Ap=DUMMY, Aj=DUMMY, Apt=DUMMY, Ajt=DUMMY, perm=DUMMY, w=None, size=C.byref(ws): \
        lib.mi355_spmv_csr_transpose(off, n_rows, n_cols, nnz, Ap, Aj, Apt, Ajt, perm, w, size, None)
    refused(lib, call(7, 4, 4, 4), EINVAL, "offset type")
    refused(lib, call(OFF_I32, -1, 4, 4), EINVAL, "negative")
    refused(lib, call(OFF_I32, 4, 4, 2 ** 31), EINVAL, "32-bit offsets")
    refused(lib, call(OFF_I64, 4, 4, 2 ** 32), ENOTSUP, "2^32")
    refused(lib, call(OFF_I32, 0, 4, 4), EINVAL, "n_rows or n_cols is 0")
    refused(lib, call(OFF_I32, 4, 4, 4, size=None), EINVAL, "workspace_bytes")
    # the query: no device is touched, and the answer is the sort's for n_cols keys
    for off in (OFF_I32, OFF_I64):
        for n_cols, nnz in ((1, 100), (256, 100), (257, 5000), (70000, 5000), (10, 0)):
            assert call(off, 4, n_cols, nnz) == OK
            assert ws.value == sp.capi.coo_to_csr_workspace_bytes(n_cols, nnz) >= 256
            assert ws.value == sp.capi.csr_transpose_workspace_bytes(n_cols, nnz, {0: torch.int32, 1: torch.int64}[off])
    # with a workspace: its size and the pointers, still before any device call
    small = C.c_size_t(16)
    refused(lib, call(OFF_I32, 4, 4, 4, w=DUMMY, size=C.byref(small)), EINVAL, "workspace of 16 bytes")
    big = C.c_size_t(1 << 30)
    refused(lib, call(OFF_I32, 4, 4, 4, Apt=None, w=DUMMY, size=C.byref(big)), EINVAL, "Apt")
    refused(lib, call(OFF_I32, 4, 4, 4, Ap=None, w=DUMMY, size=C.byref(big)), EINVAL, "Ap")
    for kw in (dict(Aj=None), dict(Ajt=None), dict(perm=None)):
        refused(lib, call(OFF_I32, 4, 4, 4, w=DUMMY, size=C.byref(big), **kw), EINVAL, "Aj, Ajt or perm")


def test_create_permuted_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p(77)
    create = lambda off, val, n_rows, n_cols, nnz, Ap, Aj, ptype, perm, n_values, k_max: \
        lib.mi355_spmv_multi_create_permuted(C.byref(h), off, val, n_rows, n_cols, nnz, Ap, Aj, ptype, perm, n_values, k_max, None)
    good = (OFF_I32, F32, 4, 4, 4, DUMMY, DUMMY, OFF_I32, DUMMY, 4, 8)
    change = lambda **kw: [kw.get(n, v) for n, v in zip("off val n_rows n_cols nnz Ap Aj ptype perm n_values k_max".split(), good)]
    refused(lib, lib.mi355_spmv_multi_create_permuted(None, *good, None), EINVAL, "null object pointer")
    refused(lib, create(*change(ptype=2)), EINVAL, "perm_type")
    refused(lib, create(*change(ptype=-1)), EINVAL, "perm_type")
    refused(lib, create(*change(n_values=-1)), EINVAL, "n_values")
    refused(lib, create(*change(n_values=2 ** 32)), ENOTSUP, "2^32")
    refused(lib, create(*change(perm=None)), EINVAL, "null perm")
    refused(lib, create(*change(Ap=None)), EINVAL, "Ap")
    refused(lib, create(*change(Aj=None)), EINVAL, "Aj")
    refused(lib, create(*change(k_max=0)), EINVAL, "k_max")
    refused(lib, create(*change(k_max=2 ** 20 + 1)), EINVAL, "k_max")
    refused(lib, create(*change(nnz=2 ** 31)), EINVAL, "32-bit offsets")
    refused(lib, create(*change(off=3)), EINVAL, "offset type")
    refused(lib, create(*change(n_rows=-1)), EINVAL, "n_rows")
    refused(lib, create(*change(val=9)), EINVAL, "value type")
    for val in (I32, PATTERN, F16, BF16):
        refused(lib, create(*change(val=val)), ENOTSUP, "fp32 and fp64")
        assert not h.value          # *out is cleared on every refusal
        h.value = 77


def test_create_transposed_and_the_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p(77)
    create = lambda off, val, n_rows, n_cols, nnz, Ap, Aj, k_max: \
        lib.mi355_spmv_multi_create_transposed(C.byref(h), off, val, n_rows, n_cols, nnz, Ap, Aj, k_max, None)
    refused(lib, lib.mi355_spmv_multi_create_transposed(None, OFF_I32, F32, 4, 4, 4, DUMMY, DUMMY, 8, None), EINVAL, "null object pointer")
    refused(lib, create(5, F32, 4, 4, 4, DUMMY, DUMMY, 8), EINVAL, "offset type")
    for val in (I32, PATTERN, F16, BF16):
        refused(lib, create(OFF_I32, val, 4, 4, 4, DUMMY, DUMMY, 8), ENOTSUP, "fp32 and fp64")
    refused(lib, create(OFF_I32, 9, 4, 4, 4, DUMMY, DUMMY, 8), EINVAL, "value type")
    refused(lib, create(OFF_I32, F32, 4, 4, 4, DUMMY, DUMMY, 0), EINVAL, "k_max")
    refused(lib, create(OFF_I32, F32, 4, -1, 4, DUMMY, DUMMY, 8), EINVAL, "n_cols")
    refused(lib, create(OFF_I32, F64, 4, 4, 2 ** 31, DUMMY, DUMMY, 8), EINVAL, "32-bit offsets")
    refused(lib, create(OFF_I64, F64, 4, 4, 2 ** 32, DUMMY, DUMMY, 8), ENOTSUP, "2^32")
    refused(lib, create(OFF_I32, F32, 4, 4, 4, None, DUMMY, 8), EINVAL, "Ap")
    refused(lib, create(OFF_I32, F32, 4, 4, 4, DUMMY, None, 8), EINVAL, "Aj")
    refused(lib, create(OFF_I32, F32, 0, 4, 4, DUMMY, DUMMY, 8), EINVAL, "n_rows or n_cols is 0")
    assert not h.value
    for name in ONE_SHOTS:
        fn = getattr(lib, name)
        shot = lambda Ap=DUMMY, Aj=DUMMY, Ax=DUMMY, X=DUMMY, ldx=4, Y=DUMMY, ldy=4, k=4, nnz=4: fn(4, 4, nnz, Ap, Aj, Ax, X, ldx, Y, ldy, k, None)
        refused(lib, shot(Ap=None), EINVAL, "Ap")
        refused(lib, shot(Ax=None), EINVAL, "Ax or X")
        refused(lib, shot(X=None), EINVAL, "Ax or X")
        refused(lib, shot(Y=None), EINVAL, "Y")
        refused(lib, shot(k=0), EINVAL, "k = 0")
        refused(lib, shot(ldx=3), EINVAL, "leading dimension")
        refused(lib, shot(ldy=3), EINVAL, "leading dimension")
        refused(lib, shot(nnz=-1), EINVAL, "nnz")
    refused(lib, lib.mi355_spmv_multi_get_perm_info(None, None, None, None), EINVAL, "null object")
    refused(lib, lib.mi355_spmv_multi_copy_structure(None, None, None, None, None), EINVAL, "null object")


def test_python_checks_come_before_any_device_call(sp):
    cpu = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.csr_transpose(4, 4, cpu, cpu)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.TransposedMultiPlan(4, 4, 4, cpu, cpu, torch.float32, 8)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.MultiPlan(4, 4, 4, cpu, cpu, torch.float32, 8, perm=cpu)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.spmm_t(4, 4, 4, cpu, cpu, cpu.float(), torch.zeros(4, 2), torch.zeros(4, 2))
