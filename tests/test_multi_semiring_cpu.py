"""Multi-vector SpMV over semirings, int32 values and pattern matrices (mi355_spmv_multi_create_typed / set_semiring /
get_types / genl_* / pattern_*, sp.MultiPlan(..., mat_dtype=, semiring=), sp.spmm(semiring=), sp.spmm_pattern), without a
GPU: the header's new names are exported, every argument-only error is refused before any device call, and the
interplay of set_semiring with set_alpha_beta is that of the merge kind's plans."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mi355_spmv.h")
OBJECT_CALLS = ["mi355_spmv_multi_" + n for n in ("create_typed", "set_semiring", "get_types")]
GENL = ["mi355_spmv_multi_genl_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64", "i32")]
PATTERN = ["mi355_spmv_multi_pattern_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64", "i32")]
OK, EINVAL, ENOTSUP = 0, 1, 2
F32, F64, I32, PAT, F16, BF16 = 0, 1, 2, 3, 4, 5
PLUS_TIMES, MIN_PLUS, OR_AND = 0, 1, 4
DUMMY = C.c_void_p(256)


def empty_object(lib, mat, vec, k_max=8):
    """An object of a matrix without rows: no scratch, so no device is needed."""
    h = C.c_void_p()
    assert lib.mi355_spmv_multi_create_typed(C.byref(h), 0, mat, vec, 0, 5, 0, None, None, k_max) == OK and h.value
    return h


def test_symbols_are_declared_and_exported(sp):
    text = open(HEADER).read()
    lib = sp.capi.lib()
    assert re.search(r"#define\s+MI355_SPMV_HAS_MULTI_SEMIRING\s+1\b", text)
    assert re.search(r"#define\s+MI355_SPMV_VERSION\s+310\b", text) and lib.mi355_spmv_version() == 310
    for name in OBJECT_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    c = {"f32": "float", "f64": "double", "i32": "int32_t"}
    for name in GENL + PATTERN:
        o, v = name.split("_")[-2:]
        ax = r"const %s\* Ax, " % c[v] if "genl" in name else ""
        assert re.search(r"\bint\s+%s\(int semiring, int32_t n_rows, int32_t n_cols, int%s_t nnz, const int%s_t\* Ap, const int32_t\* Aj,"
                         r"\s*%sconst %s\* X, int64_t ldx, %s\* Y, int64_t ldy, int32_t k, void\* stream\);"
                         % (name, o[1:], o[1:], ax, c[v], c[v]), text), name
    for name in OBJECT_CALLS + GENL + PATTERN:
        assert hasattr(lib, name), name
        assert name in sp.capi.EXPORTS, name
        assert getattr(lib, name).argtypes, name
    assert callable(sp.spmm_pattern) and callable(sp.MultiPlan.set_semiring) and callable(sp.MultiPlan.types)


def test_create_typed_refusals(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a: lib.mi355_spmv_multi_create_typed(C.byref(h), *a)
    assert lib.mi355_spmv_multi_create_typed(None, 0, F32, F32, 4, 4, 4, DUMMY, DUMMY, 4) == EINVAL     # null out
    #            off mat  vec  rows cols nnz Ap     Aj     k_max
    for args in ((0, F32, PAT, 4, 4, 4, DUMMY, DUMMY, 4),        # PATTERN / F16 / BF16 are not types of X and Y
                 (0, PAT, PAT, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, F32, F16, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, F16, F16, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, F32, BF16, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, F32, 9, 4, 4, 4, DUMMY, DUMMY, 4),          # unknown types
                 (0, 9, F32, 4, 4, 4, DUMMY, DUMMY, 4),
                 (0, -1, F32, 4, 4, 4, DUMMY, DUMMY, 4),
                 (7, F32, F32, 4, 4, 4, DUMMY, DUMMY, 4),        # unknown offset type
                 (0, I32, I32, -1, 4, 4, DUMMY, DUMMY, 4),       # the size and pointer checks of multi_create
                 (0, PAT, F32, 4, -1, 4, DUMMY, DUMMY, 4),
                 (0, PAT, I32, 4, 4, -1, DUMMY, DUMMY, 4),
                 (0, I32, I32, 4, 4, 4, DUMMY, DUMMY, 0),
                 (0, PAT, F64, 4, 4, 4, None, DUMMY, 4),
                 (0, PAT, F64, 4, 4, 4, DUMMY, None, 4),
                 (0, I32, I32, 4, 0, 4, DUMMY, DUMMY, 4),
                 (0, PAT, F32, 4, 4, 2 ** 31, DUMMY, DUMMY, 4)):
        h.value = 12345
        assert create(*args) == EINVAL and not h.value, args
        assert lib.mi355_spmv_last_error() != b""
    for mat, vec in ((F32, F64), (F64, F32), (F16, F32), (BF16, F32), (F16, F64), (I32, F32), (F32, I32), (F64, I32), (BF16, I32)):
        h.value = 12345
        assert create(0, mat, vec, 4, 4, 4, DUMMY, DUMMY, 4) == ENOTSUP and not h.value, (mat, vec)
        assert lib.mi355_spmv_last_error() != b""
    for val in (I32, PAT):       # the plain create keeps its refusal
        h.value = 12345
        assert lib.mi355_spmv_multi_create(C.byref(h), 0, val, 4, 4, 4, DUMMY, DUMMY, 4) == ENOTSUP and not h.value


def test_get_types_and_info(sp):
    lib = sp.capi.lib()
    for mat, vec, tile in ((F32, F32, 32), (F64, F64, 16), (I32, I32, 32), (PAT, F32, 32), (PAT, F64, 16), (PAT, I32, 32)):
        h = empty_object(lib, mat, vec)
        m, v, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.mi355_spmv_multi_get_types(h, C.byref(m), C.byref(v), C.byref(s)) == OK
        assert (m.value, v.value, s.value) == (mat, vec, PLUS_TIMES)
        assert lib.mi355_spmv_multi_set_semiring(h, OR_AND) == OK
        assert lib.mi355_spmv_multi_get_types(h, None, None, C.byref(s)) == OK and s.value == OR_AND
        info = sp.capi.MultiInfo()
        assert lib.mi355_spmv_multi_get_info(h, C.byref(info)) == OK
        assert info.val_type == vec and info.widest_tile == tile and info.k_max == 8 and info.scratch_bytes == 0
        assert lib.mi355_spmv_multi_destroy(h) == OK
    assert lib.mi355_spmv_multi_get_types(None, None, None, None) == EINVAL
    h = C.c_void_p()        # an object of the plain create reports its one type twice
    assert lib.mi355_spmv_multi_create(C.byref(h), 0, F64, 0, 5, 0, None, None, 8) == OK
    m, v, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.mi355_spmv_multi_get_types(h, C.byref(m), C.byref(v), C.byref(s)) == OK
    assert (m.value, v.value, s.value) == (F64, F64, PLUS_TIMES)
    assert lib.mi355_spmv_multi_destroy(h) == OK


def test_set_semiring_and_set_alpha_beta_refuse_each_other_in_both_orders(sp):
    lib = sp.capi.lib()
    assert lib.mi355_spmv_multi_set_semiring(None, 0) == EINVAL
    h = empty_object(lib, F32, F32)
    for bad in (-1, 5, 99):
        assert lib.mi355_spmv_multi_set_semiring(h, bad) == EINVAL
    # alpha / beta first: another semiring is refused until they are back at 1 / 0
    assert lib.mi355_spmv_multi_set_alpha_beta(h, 2.0, 0.0) == OK
    assert lib.mi355_spmv_multi_set_semiring(h, MIN_PLUS) == ENOTSUP and lib.mi355_spmv_last_error() != b""
    assert lib.mi355_spmv_multi_set_semiring(h, PLUS_TIMES) == OK
    assert lib.mi355_spmv_multi_set_alpha_beta(h, 1.0, 0.5) == OK
    assert lib.mi355_spmv_multi_set_semiring(h, OR_AND) == ENOTSUP
    assert lib.mi355_spmv_multi_set_alpha_beta(h, 1.0, 0.0) == OK
    for s in range(5):
        assert lib.mi355_spmv_multi_set_semiring(h, s) == OK
    # the semiring first: alpha / beta other than 1 / 0 are refused, 1 / 0 pass
    assert lib.mi355_spmv_multi_set_semiring(h, MIN_PLUS) == OK
    assert lib.mi355_spmv_multi_set_alpha_beta(h, 2.0, 0.0) == ENOTSUP and lib.mi355_spmv_last_error() != b""
    assert lib.mi355_spmv_multi_set_alpha_beta(h, 1.0, 1.0) == ENOTSUP
    assert lib.mi355_spmv_multi_set_alpha_beta(h, 1.0, 0.0) == OK
    s = C.c_int(-1)
    assert lib.mi355_spmv_multi_get_types(h, None, None, C.byref(s)) == OK and s.value == MIN_PLUS     # a refusal changes nothing
    assert lib.mi355_spmv_multi_set_semiring(h, PLUS_TIMES) == OK
    assert lib.mi355_spmv_multi_set_alpha_beta(h, -0.75, 3.0) == OK
    assert lib.mi355_spmv_multi_destroy(h) == OK


def test_int32_objects_have_no_alpha_beta(sp):
    lib = sp.capi.lib()
    for mat in (I32, PAT):
        h = empty_object(lib, mat, I32)
        assert lib.mi355_spmv_multi_set_alpha_beta(h, 2.0, 0.0) == ENOTSUP
        assert lib.mi355_spmv_multi_set_alpha_beta(h, 1.0, 1.0) == ENOTSUP
        assert lib.mi355_spmv_multi_set_alpha_beta(h, 1.0, 0.0) == OK
        assert lib.mi355_spmv_multi_destroy(h) == OK


def test_execute_checks_on_objects_without_rows(sp):
    lib = sp.capi.lib()
    for mat, vec in ((PAT, F32), (I32, I32), (PAT, I32)):
        h = empty_object(lib, mat, vec)
        ex = lambda X, ldx, Y, ldy, k: lib.mi355_spmv_multi_execute(h, None, X, ldx, Y, ldy, k, None)
        assert ex(DUMMY, 8, DUMMY, 8, 0) == EINVAL            # k < 1
        assert ex(DUMMY, 16, DUMMY, 16, 9) == EINVAL          # k > k_max
        assert ex(DUMMY, 3, DUMMY, 8, 4) == EINVAL            # ldx < k
        assert ex(DUMMY, 8, DUMMY, 3, 4) == EINVAL            # ldy < k
        assert lib.mi355_spmv_multi_set_semiring(h, MIN_PLUS) == OK
        assert ex(None, 8, None, 8, 4) == OK                  # nothing to do: no rows, no nonzeros, no launch
        assert lib.mi355_spmv_multi_destroy(h) == OK


def test_a_null_ax_passes_on_a_pattern_one_shot_and_is_refused_on_a_valued_one(sp):
    """The one-shots run check_execute_args with the object's kind before they create anything: with nonzeros, a
    valued matrix needs Ax (EINVAL before any device call); a pattern entry point has no Ax to give, and its next
    refusal is about something else — here the null Y."""
    lib = sp.capi.lib()
    for name in GENL:
        assert getattr(lib, name)(MIN_PLUS, 4, 4, 4, DUMMY, DUMMY, None, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL
        assert b"null Ax or X" in lib.mi355_spmv_last_error()
    for name in PATTERN:
        assert getattr(lib, name)(MIN_PLUS, 4, 4, 4, DUMMY, DUMMY, DUMMY, 4, None, 4, 4, None) == EINVAL
        assert b"null Y" in lib.mi355_spmv_last_error()
    # an object without rows: a NULL Ax is whatever the kind, and the pattern object takes a non-NULL one too
    h = empty_object(lib, PAT, F64)
    assert lib.mi355_spmv_multi_execute(h, None, DUMMY, 8, DUMMY, 8, 4, None) == OK
    assert lib.mi355_spmv_multi_execute(h, DUMMY, DUMMY, 8, DUMMY, 8, 4, None) == OK
    assert lib.mi355_spmv_multi_destroy(h) == OK


def test_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    for name in GENL:
        fn = getattr(lib, name)
        #       semiring  rows cols nnz Ap     Aj     Ax     X      ldx Y      ldy k  stream
        assert fn(5, 4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL          # unknown semiring
        assert fn(-1, 4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL
        assert fn(MIN_PLUS, 4, 4, 4, DUMMY, DUMMY, None, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL    # null Ax with nonzeros
        assert fn(MIN_PLUS, 4, 4, 4, DUMMY, DUMMY, DUMMY, None, 4, DUMMY, 4, 4, None) == EINVAL    # null X with nonzeros
        assert fn(MIN_PLUS, 4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, None, 4, 4, None) == EINVAL    # null Y with rows
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 0, None) == EINVAL     # k < 1
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 3, DUMMY, 4, 4, None) == EINVAL     # ldx < k
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 3, 4, None) == EINVAL     # ldy < k
        assert fn(PLUS_TIMES, -1, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL
        assert fn(PLUS_TIMES, 4, 4, 4, None, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL  # null Ap
    for name in PATTERN:
        fn = getattr(lib, name)
        #       semiring  rows cols nnz Ap     Aj     X      ldx Y      ldy k  stream
        assert fn(5, 4, 4, 4, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, None, 4, DUMMY, 4, 4, None) == EINVAL             # null X with nonzeros
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, 4, None, 4, 4, None) == EINVAL             # null Y with rows
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 0, None) == EINVAL
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, 3, DUMMY, 4, 4, None) == EINVAL
        assert fn(OR_AND, 4, 4, 4, DUMMY, DUMMY, DUMMY, 4, DUMMY, 3, 4, None) == EINVAL
        assert fn(OR_AND, 4, 4, 4, DUMMY, None, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL             # null Aj with nonzeros
        assert fn(OR_AND, 4, 0, 4, DUMMY, DUMMY, DUMMY, 4, DUMMY, 4, 4, None) == EINVAL            # nonzeros but no columns


class _OnDevice:
    """A tensor that says it lives on the device: the dtype and shape checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_python_entry_points_refuse_what_the_library_would(sp):
    Ap = _OnDevice(torch.tensor([0, 1, 2], dtype=torch.int32))
    Aj = _OnDevice(torch.tensor([0, 1], dtype=torch.int32))
    X, Y = _OnDevice(torch.ones(2, 4)), _OnDevice(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.spmm_pattern("or_and", 2, 2, 2, Ap, Aj, torch.ones(2, 4), Y)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.MultiPlan(2, 2, 2, torch.tensor([0, 1, 2], dtype=torch.int32), Aj, torch.float32, 4, mat_dtype="pattern")
    with pytest.raises(TypeError, match="mixed precision"):
        sp.MultiPlan(2, 2, 2, Ap, Aj, torch.float64, 4, mat_dtype=torch.float32)
    with pytest.raises(KeyError):
        sp.MultiPlan(2, 2, 2, Ap, Aj, torch.float32, 4, semiring="times_plus")
    with pytest.raises(KeyError):
        sp.spmm_pattern("times_plus", 2, 2, 2, Ap, Aj, X, Y)
    with pytest.raises(TypeError, match="value type"):
        sp.spmm_pattern("or_and", 2, 2, 2, Ap, Aj, X, _OnDevice(torch.zeros(2, 4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="different numbers of vectors"):
        sp.spmm_pattern("or_and", 2, 2, 2, Ap, Aj, X, _OnDevice(torch.zeros(2, 3)))
    with pytest.raises(TypeError, match="float32 or float64 or int32"):      # no 16-bit values under a semiring
        sp.spmm(2, 2, 2, Ap, Aj, _OnDevice(torch.ones(2, dtype=torch.float16)), X, Y, semiring="min_plus")
    # execute of a valued plan refuses Ax=None; a pattern plan takes it (objects made without the library)
    plan = sp.MultiPlan.__new__(sp.MultiPlan)
    plan.n_rows, plan.n_cols, plan.nnz, plan.k_max, plan.val_dtype, plan.pattern, plan._h = 2, 2, 2, 4, torch.float32, False, C.c_void_p()
    with pytest.raises(TypeError, match="only a pattern plan"):
        plan.execute(None, X, Y)
    plan.pattern = True
    with pytest.raises(ValueError, match="2-D"):
        plan.execute(None, _OnDevice(torch.ones(8)), Y)
    with pytest.raises(ValueError, match="2-D"):        # an Ax that is given is ignored: neither its type nor its length is looked at
        plan.execute(torch.ones(1, dtype=torch.float64), _OnDevice(torch.ones(8)), Y)
