"""SDDMM without a device (mi355_spmv_sddmm_*, sp.SddmmPlan, sp.sddmm): the names are declared, exported and bound;
every argument error is refused before any device call with a status and a text that names the argument (on dummy
pointers: nothing is dereferenced); create / get_info / destroy make no device call at all; the Python checks."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NAMES = (["mi355_spmv_sddmm_" + n for n in ("create", "set_alpha_beta", "execute", "get_info", "destroy")]
         + ["mi355_spmv_sddmm_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")])
OK, EINVAL, ENOTSUP = 0, 1, 2
OFF_I32, OFF_I64 = 0, 1
F32, F64, I32, PATTERN, F16, BF16 = 0, 1, 2, 3, 4, 5
DUMMY = C.c_void_p(256)


def header():
    return open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()


def test_the_names_are_declared_exported_and_bound(sp):
    text = header()
    lib = sp.capi.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
        assert n in sp.capi.EXPORTS, n
    assert re.search(r"^#define MI355_SPMV_HAS_SDDMM 1\b", text, flags=re.M)
    assert re.search(r"^#define MI355_SPMV_VERSION 310\b", text, flags=re.M) and lib.mi355_spmv_version() == 310
    assert sp.SddmmPlan is sp.capi.SddmmPlan and sp.sddmm is sp.capi.sddmm
    for status, name in ((ENOTSUP, b"not supported"), (EINVAL, b"invalid argument")):
        assert lib.mi355_spmv_status_string(status) == name


def refused(lib, status, want, *words):
    assert status == want, (status, lib.mi355_spmv_last_error())
    text = lib.mi355_spmv_last_error().decode()
    for w in words:
        assert w in text, (w, text)


def test_create_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a: lib.mi355_spmv_sddmm_create(C.byref(h), *a)
    refused(lib, create(5, F32, 4, 4, 4, DUMMY, DUMMY), EINVAL, "off_type")
    refused(lib, create(OFF_I32, I32, 4, 4, 4, DUMMY, DUMMY), ENOTSUP, "val_type", "I32")
    for vt in (PATTERN, F16, BF16, 9, -1):
        refused(lib, create(OFF_I32, vt, 4, 4, 4, DUMMY, DUMMY), EINVAL, "val_type")
    refused(lib, create(OFF_I32, F32, -1, 4, 4, DUMMY, DUMMY), EINVAL, "n_rows")
    refused(lib, create(OFF_I32, F32, 4, -1, 4, DUMMY, DUMMY), EINVAL, "n_cols")
    refused(lib, create(OFF_I32, F32, 4, 4, -1, DUMMY, DUMMY), EINVAL, "nnz")
    refused(lib, create(OFF_I32, F64, 4, 4, 2 ** 31, DUMMY, DUMMY), EINVAL, "nnz", "32-bit")
    refused(lib, create(OFF_I32, F32, 4, 4, 4, None, DUMMY), EINVAL, "Ap")
    refused(lib, create(OFF_I64, F32, 4, 4, 4, DUMMY, None), EINVAL, "Aj")
    refused(lib, create(OFF_I32, F32, 4, 0, 4, DUMMY, DUMMY), EINVAL, "n_cols")
    assert not h.value
    refused(lib, lib.mi355_spmv_sddmm_create(None, OFF_I32, F32, 4, 4, 4, DUMMY, DUMMY), EINVAL, "out")
    assert lib.mi355_spmv_sddmm_create(C.byref(h), OFF_I64, F64, 4, 4, 2 ** 31, DUMMY, DUMMY) == OK     # 64-bit offsets hold it
    assert lib.mi355_spmv_sddmm_destroy(h) == OK


def test_execute_and_the_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_sddmm_create(C.byref(h), OFF_I32, F32, 4, 4, 4, DUMMY, DUMMY) == OK
    ex = lambda *a: lib.mi355_spmv_sddmm_execute(h, *a)
    refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 0, None), EINVAL, "k = 0")
    refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, -3, None), EINVAL, "k = -3")
    refused(lib, ex(DUMMY, DUMMY, 3, DUMMY, 4, DUMMY, 4, None), EINVAL, "ldu")
    refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 3, DUMMY, 4, None), EINVAL, "ldv")
    refused(lib, ex(DUMMY, None, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "null U")
    refused(lib, ex(DUMMY, DUMMY, 4, None, 4, DUMMY, 4, None), EINVAL, "null V")
    refused(lib, ex(DUMMY, DUMMY, 4, DUMMY, 4, None, 4, None), EINVAL, "null out")
    refused(lib, lib.mi355_spmv_sddmm_execute(None, DUMMY, DUMMY, 4, DUMMY, 4, DUMMY, 4, None), EINVAL, "object")
    refused(lib, lib.mi355_spmv_sddmm_set_alpha_beta(None, 1.0, 0.0), EINVAL, "object")
    assert lib.mi355_spmv_sddmm_set_alpha_beta(h, 2.5, -1.0) == OK
    assert lib.mi355_spmv_sddmm_destroy(h) == OK
    assert lib.mi355_spmv_sddmm_destroy(None) == OK
    for o in ("i32", "i64"):
        for v in ("f32", "f64"):
            f = getattr(lib, "mi355_spmv_sddmm_%s_%s" % (o, v))
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


@pytest.mark.parametrize("n_rows,nnz", [(4, 4), (0, 0), (5000, 0), (3001, 70017), (1, 1023), (1, 1024), (2 ** 31 - 1, 2 ** 33)])
def test_create_info_destroy_need_no_device(sp, n_rows, nnz):
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_sddmm_create(C.byref(h), OFF_I64, F32, n_rows, 7, nnz, DUMMY, DUMMY) == OK
    info = sp.capi.SddmmInfo()
    assert lib.mi355_spmv_sddmm_get_info(h, C.byref(info)) == OK
    assert (info.off_type, info.val_type) == (OFF_I64, F32)
    assert info.slice_len == 1024 and info.block_threads % 64 == 0
    assert info.n_slices == -(-(n_rows + nnz) // info.slice_len)
    waves = info.block_threads // 64
    assert info.grid_blocks == -(-info.n_slices // waves)
    assert info.main_kernel == b"sddmm_slice_kernel"
    assert lib.mi355_spmv_sddmm_get_info(h, None) == EINVAL and lib.mi355_spmv_sddmm_get_info(None, C.byref(info)) == EINVAL
    assert lib.mi355_spmv_sddmm_destroy(h) == OK


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
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.SddmmPlan(3, 2, 3, Ap, Aj, torch.float32)
    dAp, dAj = _OnDevice(Ap), _OnDevice(Aj)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.SddmmPlan(3, 2, 3, dAp, _OnDevice(Aj.long()), torch.float32)
    for dt in (torch.int32, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32 or float64"):
            sp.SddmmPlan(3, 2, 3, dAp, dAj, dt)
    # the object itself: made without a device (create reads nothing and calls nothing on one)
    plan = sp.SddmmPlan(3, 2, 3, dAp, dAj, torch.float32)
    info = plan.info()
    assert info["n_slices"] == 1 and info["slice_len"] == 1024 and info["main_kernel"] == "sddmm_slice_kernel"
    plan.set_alpha_beta(2.0, 0.0)
    U, V, Ax = _OnDevice(torch.ones(3, 4)), _OnDevice(torch.ones(2, 4)), _OnDevice(torch.ones(3))
    out = _OnDevice(torch.zeros(3))
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(Ax, torch.ones(3, 4), V, out)
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(torch.ones(3), U, V, out)
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(Ax, U, V, torch.zeros(3))
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(_OnDevice(torch.ones(3, dtype=torch.float64)), U, V, out)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(Ax, _OnDevice(torch.ones(3, 4, dtype=torch.float64)), V, out)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(Ax, U, _OnDevice(torch.ones(2, 4, dtype=torch.float16)), out)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(Ax, U, V, _OnDevice(torch.zeros(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(_OnDevice(torch.ones(2)), U, V, out)
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(Ax, _OnDevice(torch.ones(2, 4)), V, out)                   # rows of U
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(Ax, U, _OnDevice(torch.ones(1, 4)), out)                   # rows of V
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(Ax, U, V, _OnDevice(torch.zeros(2)))                       # out
    with pytest.raises(ValueError, match="must be 2-D"):
        plan.execute(Ax, _OnDevice(torch.ones(12)), V, out)
    with pytest.raises(ValueError, match="row-major"):
        plan.execute(Ax, _OnDevice(torch.ones(4, 3).t()), V, out)
    with pytest.raises(ValueError, match="row-major"):
        plan.execute(Ax, U, _OnDevice(torch.ones(4, 2).t()), out)
    for k in (0, 5):
        with pytest.raises(ValueError, match="k outside"):
            plan.execute(Ax, U, V, out, k=k)
    with pytest.raises(ValueError, match="k outside"):
        plan.execute(Ax, U, _OnDevice(torch.ones(2, 3)), out)                   # V holds fewer columns than k = U's
    plan.destroy()
    plan.destroy()
    # the one-shot
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.sddmm(3, 2, 3, Ap, Aj, None, U, V)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.sddmm(3, 2, 3, dAp, dAj, None, torch.ones(3, 4), V)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.sddmm(3, 2, 3, dAp, _OnDevice(Aj.long()), None, U, V)
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.sddmm(3, 2, 3, dAp, dAj, None, _OnDevice(torch.ones(3, 4, dtype=torch.float16)), V)
    with pytest.raises(TypeError, match="differs from the plan's"):
        sp.sddmm(3, 2, 3, dAp, dAj, _OnDevice(torch.ones(3, dtype=torch.float64)), U, V, out)
