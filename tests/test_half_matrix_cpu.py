"""16-bit matrix values under fp32 vectors (MI355_VAL_F16 / MI355_VAL_BF16, the vector kind), without a GPU: the C ABI's
new names are declared and exported, and every refusal comes from the arguments alone — dummy pointers, no device call, no
plan handed back — with its status code and its text."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mi355_spmv.h")
OK, EINVAL, ENOTSUP = 0, 1, 2
VECTOR, MERGE, LIGHT, AUTO = 0, 1, 2, 100
F32, F64, I32, PATTERN, F16, BF16 = 0, 1, 2, 3, 4, 5
HALF = (F16, BF16)


def typed(lib, kind, mat, xt, yt):
    """plan_create_typed on dummy pointers: (status, last_error, whether a plan came back)."""
    h = C.c_void_p()
    dummy = C.c_void_p(256)
    st = lib.mi355_spmv_plan_create_typed(C.byref(h), kind, 0, mat, xt, yt, 4, 4, 4, dummy, dummy, 0)
    return st, lib.mi355_spmv_last_error().decode(), bool(h.value)


def test_names_are_declared_and_exported(sp):
    text = open(HEADER).read()
    assert re.search(r"#define\s+MI355_SPMV_HAS_HALF_MATRIX\s+1\b", text)
    assert re.search(r"\bMI355_VAL_F16\s*=\s*4\b", text) and re.search(r"\bMI355_VAL_BF16\s*=\s*5\b", text)
    assert re.search(r"\bint\s+mi355_spmv_narrow_values\(int dst_type, int64_t n, const float\* src, void\* dst, void\* stream\);", text)
    m = re.search(r"#define\s+MI355_SPMV_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 310 and sp.capi.lib().mi355_spmv_version() == 310
    assert hasattr(sp.capi.lib(), "mi355_spmv_narrow_values") and "mi355_spmv_narrow_values" in sp.capi.EXPORTS
    assert sp.capi.MAT_TYPES == {torch.float16: (4, "f16"), torch.bfloat16: (5, "bf16")}
    assert sorted(v[0] for v in sp.capi.VAL_TYPES.values()) == [0, 1, 2]        # x's and y's types: unchanged
    assert callable(sp.narrow_values)


@pytest.mark.parametrize("mat", HALF)
def test_merge_and_light_are_not_supported_and_the_text_names_the_vector_kind(sp, mat):
    lib = sp.capi.lib()
    for kind in (MERGE, LIGHT):
        st, err, plan = typed(lib, kind, mat, F32, F32)
        assert st == ENOTSUP and not plan, (kind, st, err)
        assert "vector kind" in err, err
    st, err, plan = typed(lib, 7, mat, F32, F32)                                 # no such kind
    assert st == EINVAL and not plan and "unknown kind" in err, (st, err)


@pytest.mark.parametrize("mat", HALF)
def test_x_and_y_other_than_fp32_are_not_supported(sp, mat):
    lib = sp.capi.lib()
    for kind in (VECTOR, AUTO, MERGE):
        for xt, yt in ((F64, F64), (I32, I32), (F32, F64), (F64, F32)):
            st, err, plan = typed(lib, kind, mat, xt, yt)
            assert st == ENOTSUP and not plan, (kind, xt, yt, st, err)
            assert "fp32 x and y only" in err or "different types" in err, err


@pytest.mark.parametrize("half", HALF)
def test_a_16_bit_x_or_y_is_invalid(sp, half):
    lib = sp.capi.lib()
    for mat, xt, yt in ((half, half, half), (half, half, F32), (half, F32, half), (F32, half, half), (F32, F32, half),
                        (F64, half, F64), (PATTERN, half, half)):
        st, err, plan = typed(lib, VECTOR, mat, xt, yt)
        assert st == EINVAL and not plan and "unknown value type" in err, (mat, xt, yt, st, err)


@pytest.mark.parametrize("half", HALF)
def test_every_other_entry_point_takes_them_for_an_unknown_value_type(sp, half):
    lib = sp.capi.lib()
    h = C.c_void_p()
    dummy = C.c_void_p(256)

    def refused(st, text):
        err = lib.mi355_spmv_last_error().decode()
        assert st == EINVAL and not h.value and text in err, (st, err)

    for kind in (VECTOR, MERGE, LIGHT, AUTO):
        refused(lib.mi355_spmv_plan_create(C.byref(h), kind, 0, half, 4, 4, 4, dummy, dummy, 0), "unknown value type")
        refused(lib.mi355_spmv_plan_acquire(C.byref(h), kind, 0, half, 4, 4, 4, dummy, dummy), "unknown value type")
    refused(lib.mi355_spmv_plan_create_block(C.byref(h), VECTOR, 0, half, None, 0, 0, 1, 0, 4, 4, 4, dummy, dummy, 0),
            "unknown value type")
    refused(lib.mi355_spmv_dist_create_local(C.byref(h), VECTOR, 0, half, 4, 4, 4, dummy, dummy, 1, None, 1, 0),
            "a matrix type of mi355_spmv_plan_create_typed only")
    cuts = (C.c_int64 * 2)(0, 4)
    refused(lib.mi355_spmv_dist_create_rank(C.byref(h), VECTOR, 0, half, 0, 1, None, 1, cuts, cuts, cuts, None, 4, 4, 4,
                                            dummy, dummy, 0), "a matrix type of mi355_spmv_plan_create_typed only")
    refused(lib.mi355_spmv_multi_create(C.byref(h), 0, half, 4, 4, 4, dummy, dummy, 2), "unknown value type")
    size = C.c_size_t(0)
    refused(lib.mi355_spmv_coo_to_csr(0, half, 4, 4, 4, dummy, dummy, dummy, dummy, dummy, dummy, None, None,
                                      C.byref(size), None), "unknown value type")
    refused(lib.mi355_spmv_coo_to_csr_symmetric(0, half, 4, 4, 4, 8, dummy, dummy, dummy, dummy, dummy, dummy, None, None,
                                                C.byref(size), None), "unknown value type")


def test_what_answered_before_answers_as_before(sp):
    """The neighbours of the new branch in plan_create_typed: pattern and fp32-under-fp64 on the row kinds, an unknown
    matrix type."""
    lib = sp.capi.lib()
    for kind in (VECTOR, LIGHT):
        st, err, plan = typed(lib, kind, PATTERN, F32, F32)
        assert st == ENOTSUP and not plan and "merge kind only" in err, (st, err)
        st, err, plan = typed(lib, kind, F32, F64, F64)
        assert st == ENOTSUP and not plan and "merge kind only" in err, (st, err)
    st, err, plan = typed(lib, MERGE, F64, F32, F32)
    assert st == ENOTSUP and not plan and "only mixed combination" in err, (st, err)
    for mat in (6, -1, 99):
        st, err, plan = typed(lib, VECTOR, mat, F32, F32)
        assert st == EINVAL and not plan and "unknown value type" in err, (mat, st, err)


def test_narrow_values_refuses_bad_arguments(sp):
    lib = sp.capi.lib()
    dummy = C.c_void_p(256)
    for dst_type in (F32, F64, I32, PATTERN, 6, -1):
        assert lib.mi355_spmv_narrow_values(dst_type, 4, dummy, dummy, None) == EINVAL
        assert b"MI355_VAL_F16 or MI355_VAL_BF16" in lib.mi355_spmv_last_error()
    for half in HALF:
        assert lib.mi355_spmv_narrow_values(half, -1, dummy, dummy, None) == EINVAL
        assert lib.mi355_spmv_narrow_values(half, 4, None, dummy, None) == EINVAL
        assert lib.mi355_spmv_narrow_values(half, 4, dummy, None, None) == EINVAL
        assert lib.mi355_spmv_narrow_values(half, 0, None, None, None) == OK      # nothing to do, nothing launched


class _OnDevice:
    """A tensor that says it lives on the device: the dtype checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_python_plan_checks_its_dtypes(sp, dtype):
    Ap = torch.tensor([0, 1, 2], dtype=torch.int32)
    Aj = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.Plan("vector", 2, 2, 2, Ap, Aj, torch.float32, mat_dtype=dtype)
    dAp, dAj = _OnDevice(Ap), _OnDevice(Aj)
    with pytest.raises(TypeError, match="float32 x and y only"):
        sp.Plan("vector", 2, 2, 2, dAp, dAj, torch.float64, mat_dtype=dtype)
    with pytest.raises(TypeError, match="float32 x and y only"):
        sp.Plan("auto", 2, 2, 2, dAp, dAj, dtype, mat_dtype=torch.bfloat16 if dtype == torch.float16 else torch.float16)
    for kind in ("merge", "light"):       # the library's own refusal, from the arguments alone
        with pytest.raises(RuntimeError, match="not supported.*vector kind only"):
            sp.Plan(kind, 2, 2, 2, dAp, dAj, torch.float32, mat_dtype=dtype)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.Plan("vector", 2, 2, 2, dAp, _OnDevice(Aj.to(torch.int64)), torch.float32, mat_dtype=dtype)

    # execute holds Ax to the plan's matrix dtype, x and y to float32 (a plan object without a handle: no device)
    plan = sp.Plan.__new__(sp.Plan)
    plan._h = None
    plan.kind, plan.n_rows, plan.n_cols, plan.nnz = "vector", 2, 2, 2
    plan.val_dtype, plan.mat_dtype = torch.float32, dtype
    x, y = _OnDevice(torch.ones(2)), _OnDevice(torch.zeros(2))
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(_OnDevice(torch.ones(2)), x, y)                                   # float32 values
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(_OnDevice(torch.ones(2, dtype=other)), x, y)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(_OnDevice(torch.ones(2, dtype=dtype)), _OnDevice(torch.ones(2, dtype=dtype)), y)
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(_OnDevice(torch.ones(1, dtype=dtype)), x, y)


def test_python_narrow_values_checks_its_arguments(sp):
    ax = torch.ones(4)
    with pytest.raises(TypeError, match="float16 or torch.bfloat16"):
        sp.narrow_values(_OnDevice(ax), torch.float32)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.narrow_values(ax, torch.float16)
    with pytest.raises(TypeError, match="takes float32"):
        sp.narrow_values(_OnDevice(ax.double()), torch.float16)
    with pytest.raises(TypeError, match="out must hold"):
        sp.narrow_values(_OnDevice(ax), torch.float16, out=_OnDevice(torch.ones(4, dtype=torch.bfloat16)))
    with pytest.raises(TypeError, match="out must hold"):
        sp.narrow_values(_OnDevice(ax), torch.float16, out=_OnDevice(torch.ones(3, dtype=torch.float16)))
