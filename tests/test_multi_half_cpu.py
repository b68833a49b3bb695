"""Multi-vector SpMV with 16-bit vectors (mi355_spmv_multi_create_half / multi_half_*, sp.MultiPlan(..., torch.float16 |
torch.bfloat16, k_max, mat_dtype=), sp.spmm on 16-bit operands), without a GPU: the header's new names are exported,
every argument-only error is refused before any device call, the typed create keeps its refusals, and the case table
of tests/multi_half_cases.py keeps its promises."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import multi_half_cases as hc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mi355_spmv.h")
ONE_SHOTS = ["mi355_spmv_multi_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")]
OK, EINVAL, ENOTSUP = 0, 1, 2
F32, F64, I32, PAT, F16, BF16 = 0, 1, 2, 3, 4, 5
PLUS_TIMES, MIN_PLUS, OR_AND = 0, 1, 4
DUMMY = C.c_void_p(256)


def empty_object(lib, mat, vec, k_max=8):
    """An object of a matrix without rows: no scratch, so no device is needed."""
    h = C.c_void_p()
    assert lib.mi355_spmv_multi_create_half(C.byref(h), 0, mat, vec, 0, 5, 0, None, None, k_max) == OK and h.value
    return h


def test_symbols_are_declared_and_exported(sp):
    text = open(HEADER).read()
    lib = sp.capi.lib()
    assert re.search(r"#define\s+MI355_SPMV_HAS_MULTI_HALF\s+1\b", text)
    assert re.search(r"\bint\s+mi355_spmv_multi_create_half\s*\(", text)
    for name in ONE_SHOTS:
        o = name.split("_")[-2]
        assert re.search(r"\bint\s+%s\(int32_t n_rows, int32_t n_cols, int%s_t nnz, const int%s_t\* Ap, const int32_t\* Aj,"
                         r"\s*const void\* Ax, const void\* X, int64_t ldx, void\* Y, int64_t ldy, int32_t k, void\* stream\);"
                         % (name, o[1:], o[1:]), text), name
    for name in ["mi355_spmv_multi_create_half"] + ONE_SHOTS:
        assert hasattr(lib, name), name
        assert name in sp.capi.EXPORTS, name
        assert getattr(lib, name).argtypes, name


def test_create_half_refusals(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a: lib.mi355_spmv_multi_create_half(C.byref(h), *a)
    assert lib.mi355_spmv_multi_create_half(None, 0, F16, F16, 4, 4, 4, DUMMY, DUMMY, 4) == EINVAL     # null out
    #            off mat  vec  rows cols nnz Ap     Aj     k_max
    for args in ((0, F32, F32, 4, 4, 4, DUMMY, DUMMY, 4),        # vec_type outside {F16, BF16}
                 (0, F16, F32, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, F64, F64, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, I32, I32, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, PAT, PAT, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, F16, 9, 4, 4, 4, DUMMY, DUMMY, 4),          # unknown types
                 (0, F16, -1, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, 9, F16, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, -1, BF16, 4, 4, 4, DUMMY, DUMMY, 4),
                 (7, F16, F16, 4, 4, 4, DUMMY, DUMMY, 4),        # unknown offset type
                 (0, F16, F16, -1, 4, 4, DUMMY, DUMMY, 4),       # the size and pointer checks of multi_create
                 (0, F32, BF16, 4, -1, 4, DUMMY, DUMMY, 4),
                 (0, BF16, BF16, 4, 4, -1, DUMMY, DUMMY, 4),
                 (0, F16, F16, 4, 4, 4, DUMMY, DUMMY, 0),
                 (0, F16, F16, 4, 4, 4, DUMMY, DUMMY, 2 ** 20 + 1),
                 (0, F32, F16, 4, 4, 4, None, DUMMY, 4),
                 (0, F32, F16, 4, 4, 4, DUMMY, None, 4),
                 (0, BF16, BF16, 4, 0, 4, DUMMY, DUMMY, 4),
                 (0, BF16, BF16, 4, 4, 2 ** 31, DUMMY, DUMMY, 4)):
        h.value = 12345
        assert create(*args) == EINVAL and not h.value, args
        assert lib.mi355_spmv_last_error() != b""
    for mat, vec in ((F16, BF16), (BF16, F16), (F64, F16), (F64, BF16), (I32, F16), (I32, BF16), (PAT, F16), (PAT, BF16)):
        h.value = 12345
        assert create(0, mat, vec, 4, 4, 4, DUMMY, DUMMY, 4) == ENOTSUP and not h.value, (mat, vec)
        assert lib.mi355_spmv_last_error() != b""


def test_the_typed_and_plain_creates_refuse_16_bit_types_as_before(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    for mat, vec in ((F16, F16), (BF16, BF16), (F32, F16), (F32, BF16)):
        h.value = 12345
        assert lib.mi355_spmv_multi_create_typed(C.byref(h), 0, mat, vec, 4, 4, 4, DUMMY, DUMMY, 4) == EINVAL and not h.value
    for mat in (F16, BF16):
        h.value = 12345
        assert lib.mi355_spmv_multi_create_typed(C.byref(h), 0, mat, F32, 4, 4, 4, DUMMY, DUMMY, 4) == ENOTSUP and not h.value
    for val in (I32, PAT):
        h.value = 12345
        assert lib.mi355_spmv_multi_create(C.byref(h), 0, val, 4, 4, 4, DUMMY, DUMMY, 4) == ENOTSUP and not h.value
    for val in (F16, BF16):
        h.value = 12345
        assert lib.mi355_spmv_multi_create(C.byref(h), 0, val, 4, 4, 4, DUMMY, DUMMY, 4) == EINVAL and not h.value


def test_get_types_get_info_and_the_semiring_on_an_empty_object(sp):
    lib = sp.capi.lib()
    for mat, vec in ((F16, F16), (F32, F16), (BF16, BF16), (F32, BF16)):
        h = empty_object(lib, mat, vec, k_max=130)
        m, v, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.mi355_spmv_multi_get_types(h, C.byref(m), C.byref(v), C.byref(s)) == OK
        assert (m.value, v.value, s.value) == (mat, vec, PLUS_TIMES)
        info = sp.capi.MultiInfo()
        assert lib.mi355_spmv_multi_get_info(h, C.byref(info)) == OK
        assert info.val_type == vec and info.widest_tile == 64 and info.k_max == 130 and info.passes == 3
        assert info.scratch_bytes == 0 and info.n_slices == 0 and info.n_kernels == 3 and info.slice_len == 1024
        assert info.main_kernel == b"multi_half_slice_kernel"
        for bad in (-1, 5, 99):
            assert lib.mi355_spmv_multi_set_semiring(h, bad) == EINVAL
        for sr in (1, 2, 3, 4):
            assert lib.mi355_spmv_multi_set_semiring(h, sr) == ENOTSUP and b"16-bit" in lib.mi355_spmv_last_error()
        assert lib.mi355_spmv_multi_set_semiring(h, PLUS_TIMES) == OK
        assert lib.mi355_spmv_multi_get_types(h, None, None, C.byref(s)) == OK and s.value == PLUS_TIMES
        assert lib.mi355_spmv_multi_set_alpha_beta(h, -0.75, 3.0) == OK
        assert lib.mi355_spmv_multi_set_semiring(h, PLUS_TIMES) == OK
        ex = lambda X, ldx, Y, ldy, k: lib.mi355_spmv_multi_execute(h, None, X, ldx, Y, ldy, k, None)
        assert ex(DUMMY, 8, DUMMY, 8, 0) == EINVAL            # k < 1
        assert ex(DUMMY, 200, DUMMY, 200, 131) == EINVAL      # k > k_max
        assert ex(DUMMY, 3, DUMMY, 8, 4) == EINVAL            # ldx < k
        assert ex(DUMMY, 8, DUMMY, 3, 4) == EINVAL            # ldy < k
        assert ex(None, 8, None, 8, 4) == OK                  # nothing to do: no rows, no nonzeros, no launch
        assert lib.mi355_spmv_multi_destroy(h) == OK


def test_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    for name in ONE_SHOTS:
        fn = getattr(lib, name)
        #         rows cols nnz Ap     Aj     Ax     X      ldx Y      ldy k  stream
        assert fn(4, 4, 4, DUMMY, DUMMY, None, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL    # null Ax with nonzeros
        assert b"null Ax or X" in lib.mi355_spmv_last_error()
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, None, 4, DUMMY, 4, 4, None) == EINVAL    # null X with nonzeros
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, None, 4, 4, None) == EINVAL    # null Y with rows
        assert b"null Y" in lib.mi355_spmv_last_error()
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 0, None) == EINVAL   # k < 1
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 3, DUMMY, 4, 4, None) == EINVAL   # ldx < k
        assert fn(4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 3, 4, None) == EINVAL   # ldy < k
        assert fn(-1, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL
        assert fn(4, 4, 4, None, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL    # null Ap
        assert fn(4, 4, 4, DUMMY, None, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL    # null Aj with nonzeros
        assert fn(4, 0, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL   # nonzeros but no columns


class _OnDevice:
    """A tensor that says it lives on the device: the dtype and shape checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_python_entry_points_refuse_what_the_library_would(sp, dtype):
    Ap = _OnDevice(torch.tensor([0, 1, 2], dtype=torch.int32))
    Aj = _OnDevice(torch.tensor([0, 1], dtype=torch.int32))
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    X, Y = _OnDevice(torch.ones(2, 4, dtype=dtype)), _OnDevice(torch.zeros(2, 4, dtype=dtype))
    Ax = _OnDevice(torch.ones(2, dtype=dtype))
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.MultiPlan(2, 2, 2, torch.tensor([0, 1, 2], dtype=torch.int32), Aj, dtype, 4)
    for semiring in ("min_plus", "or_and", 3):
        with pytest.raises(TypeError, match="plus_times"):
            sp.MultiPlan(2, 2, 2, Ap, Aj, dtype, 4, semiring=semiring)
    for mat in (other, torch.float64, torch.int32, "pattern"):
        with pytest.raises(TypeError, match="mat_dtype under 16-bit vectors"):
            sp.MultiPlan(2, 2, 2, Ap, Aj, dtype, 4, mat_dtype=mat)
    with pytest.raises(TypeError, match="mixed precision"):         # the older refusals keep their words
        sp.MultiPlan(2, 2, 2, Ap, Aj, torch.float32, 4, mat_dtype=dtype)
    with pytest.raises(TypeError, match="mixed precision"):
        sp.MultiPlan(2, 2, 2, Ap, Aj, torch.float64, 4, mat_dtype=torch.float32)
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.MultiPlan(2, 2, 2, Ap, Aj, torch.int32, 4)
    with pytest.raises(TypeError, match="float32 or float64 or int32"):
        sp.spmm(2, 2, 2, Ap, Aj, Ax, X, Y, semiring="min_plus")
    # sp.spmm on 16-bit operands: X and Y in the type of Ax
    with pytest.raises(TypeError, match="value type"):
        sp.spmm(2, 2, 2, Ap, Aj, Ax, _OnDevice(torch.ones(2, 4)), Y)
    with pytest.raises(TypeError, match="value type"):
        sp.spmm(2, 2, 2, Ap, Aj, Ax, X, _OnDevice(torch.zeros(2, 4, dtype=other)))
    with pytest.raises(ValueError, match="different numbers of vectors"):
        sp.spmm(2, 2, 2, Ap, Aj, Ax, X, _OnDevice(torch.zeros(2, 3, dtype=dtype)))
    with pytest.raises(ValueError, match="shorter than the matrix"):
        sp.spmm(2, 2, 3, Ap, Aj, Ax, X, Y)
    # execute checks Ax against the matrix type and X / Y against the vectors' (objects made without the library)
    for mat in (dtype, torch.float32):
        plan = sp.MultiPlan.__new__(sp.MultiPlan)
        plan.n_rows, plan.n_cols, plan.nnz, plan.k_max, plan.val_dtype, plan.mat_dtype, plan.pattern, plan._h = (
            2, 2, 2, 4, dtype, mat, False, C.c_void_p())
        wrong = torch.float32 if mat == dtype else dtype
        with pytest.raises(TypeError, match="value type"):
            plan.execute(_OnDevice(torch.ones(2, dtype=wrong)), X, Y)
        good = _OnDevice(torch.ones(2, dtype=mat))
        with pytest.raises(TypeError, match="value type"):
            plan.execute(good, _OnDevice(torch.ones(2, 4)), Y)
        with pytest.raises(TypeError, match="value type"):
            plan.execute(good, X, _OnDevice(torch.zeros(2, 4)))
        with pytest.raises(ValueError, match="2-D"):
            plan.execute(good, _OnDevice(torch.ones(8, dtype=dtype)), Y)
        with pytest.raises(TypeError, match="only a pattern plan"):
            plan.execute(None, X, Y)


def test_the_table_keeps_its_promises():
    """Names of their own, every combination, and carried hub rows whose sums lie far above 256."""
    hc.self_test()


def test_the_16_bit_roundings_of_the_table_are_the_formats_own():
    """The bf16 rounding built from integer operations against torch's on the CPU (NaN as NaN), and both formats' exact
    widening; ties go to even and the largest finite value's upper neighbours overflow to inf."""
    rng = np.random.RandomState(5)
    a = (rng.randn(200000) * np.exp(rng.randn(200000) * 20)).astype(np.float32)
    a[:12] = [np.inf, -np.inf, 0.0, -0.0, 3.4e38, -3.4e38, 1.00390625, 1.01171875, 257.0, 259.0, 65520.0, 1e-40]
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(hc.to_bits(a, "bf16"), want)
    assert np.array_equal(hc.from_bits(want, "bf16"), torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy())
    assert hc.is_nan_bits(hc.to_bits(np.float32("nan"), "bf16"), "bf16").all()
    assert hc.is_nan_bits(hc.to_bits(np.float32("nan"), "f16"), "f16").all()
    want16 = torch.from_numpy(a).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(hc.to_bits(a, "f16"), want16)
    for t in hc.VECS:
        assert hc.from_bits(hc.to_bits(np.float32(hc.CANARY), t), t)[0] == hc.CANARY
        ints = np.arange(-256, 257, dtype=np.float32)
        assert np.array_equal(hc.from_bits(hc.to_bits(ints, t), t), ints)
    assert hc.from_bits(hc.to_bits(np.float32([257.0, 259.0]), "bf16"), "bf16").tolist() == [256.0, 260.0]
