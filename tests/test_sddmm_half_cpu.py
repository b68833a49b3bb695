"""SDDMM with 16-bit U and V without a device (mi355_spmv_sddmm_create_half / _get_types / _half_*, sp.SddmmPlan(...,
vec_dtype=), sp.sddmm_half): the names are declared, exported and bound; every argument error is refused before any device
call with a status and a text that names the argument (on dummy pointers: nothing is dereferenced); create_half /
get_types / get_info / destroy make no device call at all; the Python checks."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NAMES = (["mi355_spmv_sddmm_create_half", "mi355_spmv_sddmm_get_types"]
         + ["mi355_spmv_sddmm_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")])
OK, EINVAL, ENOTSUP = 0, 1, 2
OFF_I32, OFF_I64 = 0, 1
F32, F64, I32, PATTERN, F16, BF16 = 0, 1, 2, 3, 4, 5
DUMMY = C.c_void_p(256)


def test_the_names_are_declared_exported_and_bound(sp):
    text = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    lib = sp.capi.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
        assert n in sp.capi.EXPORTS, n
        assert getattr(lib, n).argtypes, n
    assert re.search(r"^#define MI355_SPMV_HAS_SDDMM_HALF 1\b", text, flags=re.M)
    assert re.search(r"^#define MI355_SPMV_VERSION 310\b", text, flags=re.M) and lib.mi355_spmv_version() == 310
    assert sp.sddmm_half is sp.capi.sddmm_half
    assert "16-bit U / V, semirings" not in text        # the sentence that said they are not built went


def refused(lib, status, want, *words):
    assert status == want, (status, lib.mi355_spmv_last_error())
    text = lib.mi355_spmv_last_error().decode()
    for w in words:
        assert w in text, (w, text)


def test_create_half_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a: lib.mi355_spmv_sddmm_create_half(C.byref(h), *a)
    for vt in (F32, F64, I32, PATTERN, 9, -1):
        h.value = 1234
        refused(lib, create(OFF_I32, vt, 4, 4, 4, DUMMY, DUMMY), EINVAL, "vec_type")
        assert not h.value                      # *out cleared on failure
    for vt in (F16, BF16):
        refused(lib, create(5, vt, 4, 4, 4, DUMMY, DUMMY), EINVAL, "off_type")
        refused(lib, create(OFF_I32, vt, -1, 4, 4, DUMMY, DUMMY), EINVAL, "n_rows")
        refused(lib, create(OFF_I32, vt, 4, -1, 4, DUMMY, DUMMY), EINVAL, "n_cols")
        refused(lib, create(OFF_I32, vt, 4, 4, -1, DUMMY, DUMMY), EINVAL, "nnz")
        refused(lib, create(OFF_I32, vt, 4, 4, 2 ** 31, DUMMY, DUMMY), EINVAL, "nnz", "32-bit")
        refused(lib, create(OFF_I32, vt, 4, 4, 4, None, DUMMY), EINVAL, "Ap")
        refused(lib, create(OFF_I64, vt, 4, 4, 4, DUMMY, None), EINVAL, "Aj")
        refused(lib, create(OFF_I32, vt, 4, 0, 4, DUMMY, DUMMY), EINVAL, "n_cols")
        assert not h.value
        refused(lib, lib.mi355_spmv_sddmm_create_half(None, OFF_I32, vt, 4, 4, 4, DUMMY, DUMMY), EINVAL, "out")
        assert create(OFF_I64, vt, 4, 4, 2 ** 31, DUMMY, DUMMY) == OK       # 64-bit offsets hold it
        assert lib.mi355_spmv_sddmm_destroy(h) == OK
    # the typed create keeps refusing the 16-bit types as a val_type
    for vt in (F16, BF16):
        refused(lib, lib.mi355_spmv_sddmm_create(C.byref(h), OFF_I32, vt, 4, 4, 4, DUMMY, DUMMY), EINVAL, "val_type")


@pytest.mark.parametrize("n_rows,nnz", [(4, 4), (0, 0), (3001, 70017), (1, 1024)])
def test_get_types_and_get_info_on_both_kinds_of_object(sp, n_rows, nnz):
    lib = sp.capi.lib()
    for make, arg, want, kernel in ((lib.mi355_spmv_sddmm_create_half, F16, (F32, F16), b"sddmm_half_slice_kernel"),
                                    (lib.mi355_spmv_sddmm_create_half, BF16, (F32, BF16), b"sddmm_half_slice_kernel"),
                                    (lib.mi355_spmv_sddmm_create, F32, (F32, F32), b"sddmm_slice_kernel"),
                                    (lib.mi355_spmv_sddmm_create, F64, (F64, F64), b"sddmm_slice_kernel")):
        h = C.c_void_p()
        assert make(C.byref(h), OFF_I64, arg, n_rows, 7, nnz, DUMMY, DUMMY) == OK
        val, vec = C.c_int(-1), C.c_int(-1)
        assert lib.mi355_spmv_sddmm_get_types(h, C.byref(val), C.byref(vec)) == OK
        assert (val.value, vec.value) == want
        assert lib.mi355_spmv_sddmm_get_types(h, None, None) == OK      # either pointer may be null
        info = sp.capi.SddmmInfo()
        assert lib.mi355_spmv_sddmm_get_info(h, C.byref(info)) == OK
        assert (info.off_type, info.val_type) == (OFF_I64, want[0])
        assert info.slice_len == 1024 and info.n_slices == -(-(n_rows + nnz) // 1024)
        assert info.grid_blocks == -(-info.n_slices // (info.block_threads // 64))
        assert info.main_kernel == kernel
        assert lib.mi355_spmv_sddmm_destroy(h) == OK
    refused(lib, lib.mi355_spmv_sddmm_get_types(None, None, None), EINVAL, "object")


def test_execute_and_the_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    for vt in (F16, BF16):
        h = C.c_void_p()
        assert lib.mi355_spmv_sddmm_create_half(C.byref(h), OFF_I32, vt, 4, 4, 4, DUMMY, DUMMY) == OK
        ex = lambda *a: lib.mi355_spmv_sddmm_execute(h, *a)
        refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 0, None), EINVAL, "k = 0")
        refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, -3, None), EINVAL, "k = -3")
        refused(lib, ex(DUMMY, DUMMY, 3, DUMMY, 4, DUMMY, 4, None), EINVAL, "ldu")
        refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 3, DUMMY, 4, None), EINVAL, "ldv")
        refused(lib, ex(DUMMY, None, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "null U")
        refused(lib, ex(DUMMY, DUMMY, 4, None, 4, DUMMY, 4, None), EINVAL, "null V")
        refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 4, None, 4, None), EINVAL, "null out")
        assert lib.mi355_spmv_sddmm_set_alpha_beta(h, 2.5, -1.0) == OK
        assert lib.mi355_spmv_sddmm_destroy(h) == OK
    for o in ("i32", "i64"):
        for v in ("f16", "bf16"):
            f = getattr(lib, "mi355_spmv_sddmm_half_%s_%s" % (o, v))
            refused(lib, f(4, 4, 4, None, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "Ap")
            refused(lib, f(4, 4, 4, DUMMY, None, DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "Aj")
            refused(lib, f(4, 4, -1, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "nnz")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, None, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "null U")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, None, 4, DUMMY, 4, None), EINVAL, "null V")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, None, 4, None), EINVAL, "null out")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 0, None), EINVAL, "k = 0")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 3, DUMMY, 4, DUMMY, 4, None), EINVAL, "ldu")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 3, DUMMY, 4, None), EINVAL, "ldv")
            # nothing stored: nothing to launch, no device call, OK — also with every pointer null
            assert f(0, 4, 0, None, None, None, None, 4, None, 4, None, 4, None) == OK
            assert f(4, 4, 0, DUMMY, None, None, None, 4, None, 4, None, 4, None) == OK


class _OnDevice:
    """A tensor that says it lives on the device: the other checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_python_checks(sp):
    Ap = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    Aj = torch.tensor([0, 1, 0], dtype=torch.int32)
    dAp, dAj = _OnDevice(Ap), _OnDevice(Aj)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.SddmmPlan(3, 2, 3, Ap, Aj, torch.float32, vec_dtype=torch.float16)
    with pytest.raises(TypeError, match="val_dtype float32"):
        sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.float64, vec_dtype=torch.bfloat16)       # vec_dtype with float64 values
    for dt in (torch.float32, torch.float64, torch.int32, torch.int16, "f16"):
        with pytest.raises(TypeError, match="float16 or bfloat16"):
            sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.float32, vec_dtype=dt)
    # what stays locked: a 16-bit val_dtype, with or without vec_dtype
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.float16)
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.bfloat16, vec_dtype=torch.bfloat16)
    # today's plan: vec_dtype is val_dtype
    plain = sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.float64)
    assert plain.vec_dtype is torch.float64 and plain.info()["main_kernel"] == "sddmm_slice_kernel"
    plain.destroy()
    for vec, other in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)):
        plan = sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.float32, vec_dtype=vec)    # made without a device
        assert plan.vec_dtype is vec and plan.val_dtype is torch.float32
        info = plan.info()
        assert info["n_slices"] == 1 and info["slice_len"] == 1024 and info["main_kernel"] == "sddmm_half_slice_kernel"
        assert info["val_type"] == F32
        plan.set_alpha_beta(2.0, 0.0)
        U, V = _OnDevice(torch.ones(3, 4, dtype=vec)), _OnDevice(torch.ones(2, 4, dtype=vec))
        Ax, out = _OnDevice(torch.ones(3)), _OnDevice(torch.zeros(3))
        with pytest.raises(RuntimeError, match="device tensors only"):
            plan.execute(Ax, torch.ones(3, 4, dtype=vec), V, out)
        with pytest.raises(TypeError, match="differs from the plan's"):
            plan.execute(Ax, _OnDevice(torch.ones(3, 4, dtype=other)), V, out)      # U in the wrong 16-bit type
        with pytest.raises(TypeError, match="differs from the plan's"):
            plan.execute(Ax, U, _OnDevice(torch.ones(2, 4, dtype=other)), out)
        with pytest.raises(TypeError, match="differs from the plan's"):
            plan.execute(Ax, _OnDevice(torch.ones(3, 4)), V, out)                   # fp32 U on a half plan
        with pytest.raises(TypeError, match="differs from the plan's"):
            plan.execute(Ax, U, _OnDevice(torch.ones(2, 4)), out)
        with pytest.raises(TypeError, match="differs from the plan's"):
            plan.execute(_OnDevice(torch.ones(3, dtype=vec)), U, V, out)            # 16-bit Ax
        with pytest.raises(TypeError, match="differs from the plan's"):
            plan.execute(Ax, U, V, _OnDevice(torch.zeros(3, dtype=vec)))            # 16-bit out
        with pytest.raises(ValueError, match="shorter than"):
            plan.execute(Ax, _OnDevice(torch.ones(2, 4, dtype=vec)), V, out)
        with pytest.raises(ValueError, match="row-major"):
            plan.execute(Ax, _OnDevice(torch.ones(4, 3, dtype=vec).t()), V, out)
        for k in (0, 5):
            with pytest.raises(ValueError, match="k outside"):
                plan.execute(Ax, U, V, out, k=k)
        plan.destroy()
        plan.destroy()
        # the one-shot
        with pytest.raises(RuntimeError, match="device tensors only"):
            sp.sddmm_half(3, 2, 3, Ap, Aj, None, U, V)
        with pytest.raises(RuntimeError, match="device tensors only"):
            sp.sddmm_half(3, 2, 3, dAp, dAj, None, torch.ones(3, 4, dtype=vec), V)
        with pytest.raises(TypeError, match="Aj must be int32"):
            sp.sddmm_half(3, 2, 3, dAp, _OnDevice(Aj.long()), None, U, V)
        with pytest.raises(TypeError, match="float16 or bfloat16"):
            sp.sddmm_half(3, 2, 3, dAp, dAj, None, _OnDevice(torch.ones(3, 4)), V)  # fp32 U
        with pytest.raises(TypeError, match="differs from the plan's"):
            sp.sddmm_half(3, 2, 3, dAp, dAj, None, U, _OnDevice(torch.ones(2, 4, dtype=other)))
        with pytest.raises(TypeError, match="differs from the plan's"):
            sp.sddmm_half(3, 2, 3, dAp, dAj, _OnDevice(torch.ones(3, dtype=vec)), U, V, out)
        # and sp.sddmm keeps refusing 16-bit U
        with pytest.raises(TypeError, match="float32 or float64"):
            sp.sddmm(3, 2, 3, dAp, dAj, None, U, V)
