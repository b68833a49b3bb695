"""Pattern (value-free) matrices, without a GPU: the C ABI's new names are declared and exported, the version the
library reports is the header's, and the Python entry points refuse what their siblings refuse before any device call."""
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mi355_spmv.h")
ONE_SHOTS = ["mi355_spmv_merge_pattern_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64", "i32")]


def test_symbols_are_declared_and_exported(sp):
    text = open(HEADER).read()
    lib = sp.capi.lib()
    assert re.search(r"\bMI355_VAL_PATTERN\s*=\s*3\b", text)
    assert re.search(r"\bint\s+mi355_spmv_plan_get_mat_type\s*\(\s*const\s+mi355_spmv_plan\s*\*", text)
    for name in ONE_SHOTS:            # the arguments of merge_genl without Ax
        assert re.search(r"\bint\s+%s\(int semiring, int32_t n_rows, int32_t n_cols, int(32|64)_t nnz, const int(32|64)_t\* Ap,"
                         r"\s*const int32_t\* Aj, const (float|double|int32_t)\* x, (float|double|int32_t)\* y, void\* stream\);" % name, text), name
    for name in ONE_SHOTS + ["mi355_spmv_plan_get_mat_type"]:
        assert hasattr(lib, name), name
        assert name in sp.capi.EXPORTS, name
    assert sp.capi.VAL_PATTERN == 3 and 3 not in [v[0] for v in sp.capi.VAL_TYPES.values()]
    assert callable(sp.spmv_pattern)


def test_version_is_the_headers(sp):
    m = re.search(r"#define\s+MI355_SPMV_VERSION\s+(\d+)", open(HEADER).read())
    assert m and sp.capi.lib().mi355_spmv_version() == int(m.group(1))
    assert re.search(r"#define\s+MI355_SPMV_HAS_PATTERN\s+1\b", open(HEADER).read())


def test_get_mat_type_rejects_null(sp):
    import ctypes as C
    lib = sp.capi.lib()
    out = C.c_int(-1)
    assert lib.mi355_spmv_plan_get_mat_type(None, C.byref(out)) == 1
    assert lib.mi355_spmv_plan_get_mat_type(None, None) == 1


def test_python_entry_points_refuse_cpu_tensors_and_a_wide_aj(sp):
    Ap = torch.tensor([0, 1, 2], dtype=torch.int32)
    Aj = torch.tensor([0, 1], dtype=torch.int32)
    x = torch.ones(2)
    y = torch.zeros(2)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.spmv_pattern("plus_times", 2, 2, 2, Ap, Aj, x, y)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.Plan("merge", 2, 2, 2, Ap, Aj, torch.float32, mat_dtype="pattern")
    with pytest.raises(ValueError, match="NOT SUPPORTED"):
        sp.Plan("no_such_kind", 2, 2, 2, Ap, Aj, torch.float32, mat_dtype="pattern")
    with pytest.raises(KeyError):
        sp.spmv_pattern("no_such_semiring", 2, 2, 2, Ap, Aj, x, y)


class _OnDevice:
    """A tensor that says it lives on the device: the dtype checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_python_entry_points_refuse_a_non_int32_aj(sp):
    Ap = _OnDevice(torch.tensor([0, 1, 2], dtype=torch.int32))
    Aj = _OnDevice(torch.tensor([0, 1], dtype=torch.int64))
    x, y = _OnDevice(torch.ones(2)), _OnDevice(torch.zeros(2))
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.spmv_pattern("plus_times", 2, 2, 2, Ap, Aj, x, y)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.Plan("merge", 2, 2, 2, Ap, Aj, torch.float32, mat_dtype="pattern")
    Aj32 = _OnDevice(torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(TypeError, match="one value type"):
        sp.spmv_pattern("plus_times", 2, 2, 2, Ap, Aj32, x, _OnDevice(torch.zeros(2, dtype=torch.float64)))
    with pytest.raises(ValueError, match='"pattern"'):
        sp.Plan("merge", 2, 2, 2, Ap, Aj32, torch.float32, mat_dtype="ones")


def test_c_abi_refuses_pattern_everywhere_but_a_typed_merge_plan(sp):
    """All refused from the arguments alone, before any device call; no plan comes back."""
    import ctypes as C
    lib = sp.capi.lib()
    h = C.c_void_p()
    dummy = C.c_void_p(256)
    assert lib.mi355_spmv_plan_create(C.byref(h), 1, 0, 3, 4, 4, 4, dummy, dummy, 0) == 1 and not h.value       # as a val_type
    assert lib.mi355_spmv_plan_acquire(C.byref(h), 1, 0, 3, 4, 4, 4, dummy, dummy) == 1 and not h.value
    for kind in (0, 2):                                                                                          # VECTOR, LIGHT
        assert lib.mi355_spmv_plan_create_typed(C.byref(h), kind, 0, 3, 0, 0, 4, 4, 4, dummy, dummy, 0) == 2 and not h.value
        assert b"merge kind only" in lib.mi355_spmv_last_error()
    assert lib.mi355_spmv_plan_create_typed(C.byref(h), 7, 0, 3, 0, 0, 4, 4, 4, dummy, dummy, 0) == 1 and not h.value
    for mat, xt, yt in ((3, 3, 3), (0, 3, 3), (3, 3, 0), (3, 0, 3), (3, 0, 1)):
        assert lib.mi355_spmv_plan_create_typed(C.byref(h), 1, 0, mat, xt, yt, 4, 4, 4, dummy, dummy, 0) in (1, 2) and not h.value
    for name in ONE_SHOTS:                                                                                       # unknown semiring
        assert getattr(lib, name)(9, 0, 0, 0, None, None, None, None, None) == 1
