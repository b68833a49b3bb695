"""The heads of sparse attention in one call without a device (mi355_spmv_attention[_bwd]_reserve_heads / _get_heads_max /
_execute_heads): the names are declared, exported and bound with the header's signatures; every refusal comes before any
device call, on dummy pointers, with a text that names the argument; an object of a matrix without rows reserves and
executes without a device call; the Python rank and shape errors; and the coverage of tests/attention_heads_cases.py, which
the host simulations and the device files rely on.  (The backward object cannot be made without a device: its refusals run
through the same functions of csrc/attention_common.hpp, and tests/test_gpu_attention_bwd_heads.py asks them of a real
object.  The grid bound needs a structure no test can hold: tests/test_attention_heads_sim_cpu.py asks it of the check alone.)"""
import collections
import ctypes as C
import re

import pytest
import torch

import attention_heads_cases as hd
from test_attention_cpu import DUMMY, EINVAL, F32, F64, OFF_I32, OFF_I64, OK, _OnDevice, declared_arguments, header, refused

NAMES = ["mi355_spmv_attention%s_%s" % (b, n) for b in ("", "_bwd") for n in ("reserve_heads", "get_heads_max", "execute_heads")]


def test_the_names_are_declared_exported_and_bound(sp):
    text, lib = header(), sp.capi.lib()
    assert re.search(r"^#define MI355_SPMV_HAS_ATTENTION_HEADS 1\b", text, flags=re.M)
    for n in NAMES:
        assert hasattr(lib, n) and n in sp.capi.EXPORTS, n
        args, bound = declared_arguments(text, n), getattr(lib, n).argtypes
        assert len(args) == len(bound), (n, args)
    for b in ("", "_bwd"):
        # "then exactly the arguments of execute after m"
        assert declared_arguments(text, "mi355_spmv_attention%s_execute_heads" % b)[3:] == declared_arguments(text, "mi355_spmv_attention%s_execute" % b)[1:]
    for struct_name, bound in (("mi355_spmv_attention_head_strides", sp.capi.AttentionHeadStrides),
                               ("mi355_spmv_attention_bwd_head_strides", sp.capi.AttentionBackwardHeadStrides)):
        m = re.search(r"typedef struct %s \{\s*int64_t ([^;]*);\s*\} %s;" % (struct_name, struct_name), text)
        assert [f.strip() for f in m.group(1).split(",")] == [n for n, _ in bound._fields_]
        assert all(t is C.c_int64 for _, t in bound._fields_)
    assert text.count("heads in one call") == 1 and "Out of scope: heads" not in text      # struck from the four out-of-scope lists


def strides(sp, **kw):
    return sp.capi.AttentionHeadStrides(**dict(dict(q=8, k=8, v=8, bias=0, o=8, lse=0), **kw))


@pytest.mark.parametrize("off,val", [(OFF_I32, F32), (OFF_I64, F64)])
def test_an_object_without_rows_reserves_and_executes_without_a_device_and_refuses_bad_heads(sp, off, val):
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_attention_create(0, 7, 0, None, None, off, val, 40, 70, C.byref(h)) == OK
    n = C.c_int32(-1)
    assert lib.mi355_spmv_attention_get_heads_max(h, C.byref(n)) == OK and n.value == 1          # after create
    ex = lambda n_heads, hs, d=8, dv=8, ldq=64, ldo=64, lse=None: lib.mi355_spmv_attention_execute_heads(
        h, n_heads, hs, d, dv, DUMMY, ldq, DUMMY, 64, DUMMY, 64, None, DUMMY, ldo, lse, None)
    assert ex(1, None) == OK                                                                    # one head: no stride is read
    refused(lib, ex(2, C.byref(strides(sp))), EINVAL, "n_heads = 2", "n_heads_max = 1")
    refused(lib, lib.mi355_spmv_attention_reserve_heads(h, 0), EINVAL, "n_heads_max = 0")
    refused(lib, lib.mi355_spmv_attention_reserve_heads(None, 2), EINVAL, "object")
    refused(lib, lib.mi355_spmv_attention_get_heads_max(h, None), EINVAL, "null")
    assert lib.mi355_spmv_attention_reserve_heads(h, 5) == OK                                   # no rows: no device call
    assert lib.mi355_spmv_attention_get_heads_max(h, C.byref(n)) == OK and n.value == 5
    info = sp.capi.AttentionInfo()
    assert lib.mi355_spmv_attention_get_info(h, C.byref(info)) == OK and info.scratch_bytes == 0
    # every check of execute first, with execute's messages
    refused(lib, ex(5, C.byref(strides(sp)), d=0), EINVAL, "d = 0")
    refused(lib, ex(5, C.byref(strides(sp)), ldq=7), EINVAL, "ldq")
    refused(lib, lib.mi355_spmv_attention_execute_heads(None, 1, None, 8, 8, DUMMY, 8, DUMMY, 8, DUMMY, 8, None, DUMMY, 8, None, None), EINVAL, "object")
    # then n_heads, then the strides
    refused(lib, ex(0, C.byref(strides(sp))), EINVAL, "n_heads = 0")
    refused(lib, ex(-1, None), EINVAL, "n_heads = -1")
    refused(lib, ex(6, C.byref(strides(sp))), EINVAL, "n_heads = 6", "n_heads_max = 5")
    refused(lib, ex(2, None), EINVAL, "hs")
    for name in ("q", "k", "v", "bias", "o", "lse"):
        refused(lib, ex(3, C.byref(strides(sp, **{name: -1}))), EINVAL, "negative", "stride %s" % name)
    # (no rows: the outputs have no elements, nothing can overlap, nothing is launched)
    assert ex(5, C.byref(strides(sp, o=0))) == OK and ex(3, C.byref(strides(sp))) == OK
    assert lib.mi355_spmv_attention_reserve_heads(h, 2) == OK and lib.mi355_spmv_attention_get_heads_max(h, C.byref(n)) == OK and n.value == 2
    assert lib.mi355_spmv_attention_destroy(h) == OK


def test_null_backward_objects_are_refused(sp):
    lib = sp.capi.lib()
    refused(lib, lib.mi355_spmv_attention_bwd_reserve_heads(None, 2), EINVAL, "object")
    refused(lib, lib.mi355_spmv_attention_bwd_get_heads_max(None, None), EINVAL, "null")
    args = [None, 2, None, 8, 8] + [DUMMY, 8] * 3 + [None] + [DUMMY, 8] * 2 + [DUMMY] + [DUMMY, 8] * 3 + [None, None]
    refused(lib, lib.mi355_spmv_attention_bwd_execute_heads(*args), EINVAL, "object")


def test_python_rank_and_shape_errors(sp):
    Ap, Aj = _OnDevice(torch.zeros(1, dtype=torch.int32)), _OnDevice(torch.zeros(0, dtype=torch.int32))
    plan = sp.SparseAttentionPlan(0, 2, 0, Ap, Aj, torch.float32, 8, 8, n_heads_max=3)        # no rows: no device
    assert plan.n_heads_max == 3
    plan.reserve_heads(2)
    assert plan.n_heads_max == 2
    with pytest.raises(RuntimeError, match="n_heads_max = 0"):
        plan.reserve_heads(0)
    plan.n_rows = 3
    on = lambda *shape: _OnDevice(torch.ones(*shape))
    with pytest.raises(ValueError, match="mixed ranks"):
        plan.execute(on(3, 2, 8), on(2, 8), on(2, 2, 8))
    with pytest.raises(ValueError, match="mixed ranks"):
        plan.execute(on(3, 2, 8), on(2, 2, 8), on(2, 2, 8), out=on(3, 8))
    with pytest.raises(ValueError, match="differ in their heads"):
        plan.execute(on(3, 2, 8), on(2, 1, 8), on(2, 2, 8))
    with pytest.raises(ValueError, match="must be 2-D or 3-D"):
        plan.execute(on(24), on(16), on(16))
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(torch.ones(3, 2, 8), on(2, 2, 8), on(2, 2, 8))
    plan.destroy()
    for cls in (sp.SparseAttentionPlan, sp.SparseAttentionBackwardPlan, sp.SparseAttentionBackwardHalfPlan):
        assert callable(cls.reserve_heads) and isinstance(cls.n_heads_max, property) and callable(cls.with_heads)


def test_the_table_covers_what_it_says_and_fits_what_the_library_reserves(sp):
    # the table's widths and heads are what an object without rows accepts (the checks of execute_heads before any launch)
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_attention_create(0, 7, 0, None, None, OFF_I32, F32, hd.D_MAX, hd.DV_MAX, C.byref(h)) == OK
    assert lib.mi355_spmv_attention_reserve_heads(h, max(c.H_max for c in hd.forward_cases())) == OK
    for c in hd.forward_cases():
        lay, vs = hd.layout(c), hd.vector_strides(c)
        hs = sp.capi.AttentionHeadStrides(lay["Q"][1], lay["K"][1], lay["V"][1], vs["bias"], lay["O"][1], vs["lse"])
        assert lib.mi355_spmv_attention_execute_heads(h, c.H, C.byref(hs), c.d, c.dv, DUMMY, lay["Q"][0], DUMMY, lay["K"][0], DUMMY, lay["V"][0], None,
                                                      DUMMY, lay["O"][0], None, None) == OK, c.name
    assert lib.mi355_spmv_attention_destroy(h) == OK
    s = hd.structures()
    assert [hd.n_slices(s[n]) for n in ("one", "two", "five", "eight")] == [1, 2, 5, 8]
    cross = {n: hd.crossing(m) for n, m in s.items()}
    assert cross["five"][0] >= 1 and cross["five"][1] >= 1 and cross["five"][2] >= 1        # three slices, the workgroup edge, a slice inside a row
    assert cross["eight"][3] >= 1 and cross["two"][3] >= 1                                  # empty rows at a slice end
    assert max(len(m.lens) + sum(m.lens) for m in s.values()) <= 8 * hd.SLICE_LEN
    for cases in (hd.forward_cases(), hd.backward_cases()):
        assert len({c.name for c in cases}) == len(cases)
        multi = [c for c in cases if c.H > 1]
        assert {c.H for c in cases} == set(hd.HEADS)
        assert {(c.H, c.H_max > c.H) for c in cases} >= {(h, above) for h in hd.HEADS for above in (False, True)}
        assert {c.layout for c in multi} == set(hd.LAYOUTS) and {c.bias for c in multi} == set(hd.BIASES)
        assert {(c.off, c.val) for c in cases} == set(hd.TYPES)
        assert {(hd.n_slices(c.matrix), c.H > 1) for c in cases} >= {(n, True) for n in (1, 2, 5, 8)}
        for off, val in hd.TYPES:
            mine = [c for c in multi if c.val == val]
            assert {(c.d, c.dv) for c in mine} == set(hd.DIMS[val]), val
            assert any(c.dv > hd.WIDEST[val] for c in mine) and any(c.d % 4 for c in mine)    # two passes; a remainder of the loop over d
            # the heads take the element path under rows that the single-head execute takes 16 bytes at a time
            width_bytes = {"f32": 4, "f64": 8}.get(val, 2)
            assert any(c.layout == "odd" and c.shift == 0 and (c.d * width_bytes) % 16 == 0 and (c.dv * width_bytes) % 16 == 0 for c in mine), val
        assert any(c.bias == "per_head" and hd.n_slices(c.matrix) == 5 for c in multi)
    bwd = hd.backward_cases()
    assert {c.need for c in bwd} == set(hd.NEEDS) and {c.want_dbias for c in bwd if c.need[0]} == {True, False}
    assert any(hd.layout(c)["O"] != hd.layout(c)["dO"] for c in bwd if c.H > 1)                 # O and dO in different layouts
    assert collections.Counter(c.want_lse for c in hd.forward_cases())[False] >= 5
