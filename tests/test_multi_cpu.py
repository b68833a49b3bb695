"""Multi-vector SpMV (mi355_spmv_multi_*, sp.MultiPlan, sp.spmm), without a GPU: the header's new names are exported,
every argument-only error is refused before any device call and no object comes back, and the Python entry points
refuse what their siblings refuse."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mi355_spmv.h")
OBJECT_CALLS = ["mi355_spmv_multi_" + n for n in ("create", "set_alpha_beta", "execute", "get_info", "destroy")]
ONE_SHOTS = ["mi355_spmv_multi_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
EINVAL, ENOTSUP = 1, 2
DUMMY = C.c_void_p(256)


def test_symbols_are_declared_and_exported(sp):
    text = open(HEADER).read()
    lib = sp.capi.lib()
    assert re.search(r"#define\s+MI355_SPMV_HAS_MULTI\s+1\b", text)
    assert re.search(r"#define\s+MI355_SPMV_VERSION\s+310\b", text) and lib.mi355_spmv_version() == 310
    assert re.search(r"typedef struct mi355_spmv_multi mi355_spmv_multi;", text)
    for name in OBJECT_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for name in ONE_SHOTS:
        assert re.search(r"\bint\s+%s\(int32_t n_rows, int32_t n_cols, int(32|64)_t nnz, const int(32|64)_t\* Ap, const int32_t\* Aj,"
                         r"\s*const (float|double)\* Ax, const (float|double)\* X, int64_t ldx, (float|double)\* Y, int64_t ldy, "
                         r"int32_t k, void\* stream\);" % name, text), name
    for name in OBJECT_CALLS + ONE_SHOTS:
        assert hasattr(lib, name), name
        assert name in sp.capi.EXPORTS, name
    assert callable(sp.spmm) and callable(sp.MultiPlan)


def test_create_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a: lib.mi355_spmv_multi_create(C.byref(h), *a)
    #                 off val rows cols nnz Ap     Aj     k_max
    assert lib.mi355_spmv_multi_create(None, 0, 0, 4, 4, 4, DUMMY, DUMMY, 4) == EINVAL           # null out
    for args in ((7, 0, 4, 4, 4, DUMMY, DUMMY, 4),       # unknown offset type
                 (0, 9, 4, 4, 4, DUMMY, DUMMY, 4),       # unknown value type
                 (0, 0, -1, 4, 4, DUMMY, DUMMY, 4),      # negative sizes
                 (0, 0, 4, -1, 4, DUMMY, DUMMY, 4),
                 (0, 0, 4, 4, -1, DUMMY, DUMMY, 4),
                 (0, 0, 4, 4, 4, DUMMY, DUMMY, 0),       # k_max < 1
                 (0, 0, 4, 4, 4, DUMMY, DUMMY, -3),
                 (0, 0, 4, 4, 4, None, DUMMY, 4),        # null Ap with rows
                 (0, 0, 4, 4, 4, DUMMY, None, 4),        # null Aj with nonzeros
                 (0, 0, 4, 0, 4, DUMMY, DUMMY, 4),       # nonzeros but no columns
                 (0, 0, 4, 4, 2 ** 31, DUMMY, DUMMY, 4)):   # nnz beyond 32-bit offsets
        h.value = 12345
        assert create(*args) == EINVAL and not h.value, args
        assert lib.mi355_spmv_last_error() != b""
    for val in (2, 3):                                   # MI355_VAL_I32, MI355_VAL_PATTERN
        h.value = 12345
        assert create(0, val, 4, 4, 4, DUMMY, DUMMY, 4) == ENOTSUP and not h.value


def test_execute_refuses_bad_arguments_on_an_empty_object(sp):
    """A matrix without rows needs no scratch, so its object exists without a device; execute's checks come first."""
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_multi_create(C.byref(h), 0, 0, 0, 5, 0, None, None, 8) == 0 and h.value
    ex = lambda X, ldx, Y, ldy, k: lib.mi355_spmv_multi_execute(h, None, X, ldx, Y, ldy, k, None)
    assert ex(DUMMY, 8, DUMMY, 8, 0) == EINVAL            # k < 1
    assert ex(DUMMY, 16, DUMMY, 16, 9) == EINVAL          # k > k_max
    assert ex(DUMMY, 3, DUMMY, 8, 4) == EINVAL            # ldx < k
    assert ex(DUMMY, 8, DUMMY, 3, 4) == EINVAL            # ldy < k
    assert lib.mi355_spmv_multi_execute(None, None, DUMMY, 8, DUMMY, 8, 4, None) == EINVAL
    assert lib.mi355_spmv_multi_set_alpha_beta(None, 1.0, 0.0) == EINVAL
    assert lib.mi355_spmv_multi_get_info(None, None) == EINVAL
    info = sp.capi.MultiInfo()
    assert lib.mi355_spmv_multi_get_info(h, C.byref(info)) == 0
    assert info.k_max == 8 and info.n_slices == 0 and info.scratch_bytes == 0 and info.slice_len > 0
    assert info.passes == 1 and info.widest_tile == 32 and b"multi_slice_kernel" in info.main_kernel
    assert ex(None, 8, None, 8, 4) == 0                   # nothing to do: no rows, no nonzeros, no launch
    assert lib.mi355_spmv_multi_destroy(h) == 0
    assert lib.mi355_spmv_multi_destroy(None) == 0


def test_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    for name in ONE_SHOTS:
        fn = getattr(lib, name)
        #          rows cols nnz Ap     Aj     Ax     X      ldx Y      ldy k  stream
        assert fn(4, 4, 4, DUMMY, DUMMY, None, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL    # null Ax with nonzeros
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, None, 4, DUMMY, 4, 4, None) == EINVAL    # null X with nonzeros
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, None, 4, 4, None) == EINVAL    # null Y with rows
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 0, None) == EINVAL   # k < 1
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 3, DUMMY, 4, 4, None) == EINVAL   # ldx < k
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 3, 4, None) == EINVAL   # ldy < k
        assert fn(-1, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL  # negative size
        assert fn(4, 4, 4, None, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL    # null Ap


class _OnDevice:
    """A tensor that says it lives on the device: the dtype and shape checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_python_entry_points_refuse_cpu_tensors(sp):
    Ap = torch.tensor([0, 1, 2], dtype=torch.int32)
    Aj = torch.tensor([0, 1], dtype=torch.int32)
    Ax = torch.ones(2)
    X, Y = torch.ones(2, 4), torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.MultiPlan(2, 2, 2, Ap, Aj, torch.float32, 4)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.spmm(2, 2, 2, Ap, Aj, Ax, X, Y)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.spmm(2, 2, 2, _OnDevice(Ap), _OnDevice(Aj), _OnDevice(Ax), X, _OnDevice(Y))


def test_python_entry_points_refuse_a_wide_aj_a_flat_x_and_strided_columns(sp):
    Ap = _OnDevice(torch.tensor([0, 1, 2], dtype=torch.int32))
    Aj32 = _OnDevice(torch.tensor([0, 1], dtype=torch.int32))
    Aj64 = _OnDevice(torch.tensor([0, 1], dtype=torch.int64))
    Ax = _OnDevice(torch.ones(2))
    X, Y = _OnDevice(torch.ones(2, 4)), _OnDevice(torch.zeros(2, 4))
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.MultiPlan(2, 2, 2, Ap, Aj64, torch.float32, 4)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.spmm(2, 2, 2, Ap, Aj64, Ax, X, Y)
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.MultiPlan(2, 2, 2, Ap, Aj32, torch.int32, 4)
    with pytest.raises(ValueError, match="2-D"):
        sp.spmm(2, 2, 2, Ap, Aj32, Ax, _OnDevice(torch.ones(8)), Y)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        sp.spmm(2, 2, 2, Ap, Aj32, Ax, _OnDevice(torch.ones(4, 2).t()), Y)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        sp.spmm(2, 2, 2, Ap, Aj32, Ax, X, _OnDevice(torch.zeros(2, 8)[:, ::2]))
    with pytest.raises(TypeError, match="value type"):
        sp.spmm(2, 2, 2, Ap, Aj32, Ax, _OnDevice(torch.ones(2, 4, dtype=torch.float64)), Y)
    with pytest.raises(ValueError, match="different numbers of vectors"):
        sp.spmm(2, 2, 2, Ap, Aj32, Ax, X, _OnDevice(torch.zeros(2, 3)))
    with pytest.raises(ValueError, match="shorter"):
        sp.spmm(2, 3, 2, Ap, Aj32, Ax, X, Y)
    # MultiPlan.execute runs the same checks (an object made without the library: the checks come before any call)
    plan = sp.MultiPlan.__new__(sp.MultiPlan)
    plan.n_rows, plan.n_cols, plan.nnz, plan.k_max, plan.val_dtype, plan._h = 2, 2, 2, 4, torch.float32, C.c_void_p()
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(torch.ones(2), X, Y)
    with pytest.raises(ValueError, match="2-D"):
        plan.execute(Ax, _OnDevice(torch.ones(8)), Y)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        plan.execute(Ax, _OnDevice(torch.ones(4, 2).t()), Y)
    with pytest.raises(TypeError, match="value type"):
        plan.execute(_OnDevice(torch.ones(2, dtype=torch.float64)), X, Y)
