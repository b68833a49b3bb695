"""Row softmax without a device (mi355_spmv_row_softmax_*, sp.RowSoftmaxPlan, sp.row_softmax): the names are declared,
exported and bound; every argument error is refused before any device call with a status and a text that names the
argument (on dummy pointers: nothing is dereferenced); an object of a matrix that stores nothing is made, reported,
executed and destroyed without a device call; the Python checks; and the table's own self-checks against numpy
(tests/row_softmax_cases.py: its references, its masks and its exact values, which both the host simulation and the device
file rely on)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import row_softmax_cases as rc
from conftest import ROOT

NAMES = (["mi355_spmv_row_softmax_" + n for n in ("create", "set_scale", "execute", "backward", "get_info", "destroy")]
         + ["mi355_spmv_row_softmax_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")])
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
    assert re.search(r"^#define MI355_SPMV_HAS_ROW_SOFTMAX 1\b", text, flags=re.M)
    assert re.search(r"^#define MI355_SPMV_VERSION 310\b", text, flags=re.M) and lib.mi355_spmv_version() == 310
    assert sp.RowSoftmaxPlan is sp.capi.RowSoftmaxPlan and sp.row_softmax is sp.capi.row_softmax
    assert "row_softmax.hip" in open(os.path.join(ROOT, "spmv-samples_amd", "csrc", "Makefile")).read()


def refused(lib, status, want, *words):
    assert status == want, (status, lib.mi355_spmv_last_error())
    text = lib.mi355_spmv_last_error().decode()
    for w in words:
        assert w in text, (w, text)


def test_create_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a: lib.mi355_spmv_row_softmax_create(C.byref(h), *a)
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
    refused(lib, create(OFF_I32, F32, 0, 4, 4, None, DUMMY), EINVAL, "n_rows")
    assert not h.value
    refused(lib, lib.mi355_spmv_row_softmax_create(None, OFF_I32, F32, 4, 4, 4, DUMMY, DUMMY), EINVAL, "out")


@pytest.mark.parametrize("off,val", [(OFF_I32, F32), (OFF_I64, F64)])
@pytest.mark.parametrize("n_rows", [0, 4, 5000])
def test_an_object_that_stores_nothing_needs_no_device(sp, off, val, n_rows):
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_row_softmax_create(C.byref(h), off, val, n_rows, 7, 0, DUMMY if n_rows else None, None) == OK
    info = sp.capi.RowSoftmaxInfo()
    assert lib.mi355_spmv_row_softmax_get_info(h, C.byref(info)) == OK
    assert (info.off_type, info.val_type) == (off, val)
    assert info.slice_len == 1024 and info.block_threads % 64 == 0
    assert info.n_slices == -(-n_rows // info.slice_len)
    assert info.grid_blocks == -(-info.n_slices // (info.block_threads // 64))
    assert info.scratch_bytes == 0
    assert info.main_kernel == b"row_softmax_slice_kernel"
    assert lib.mi355_spmv_row_softmax_get_info(h, None) == EINVAL and lib.mi355_spmv_row_softmax_get_info(None, C.byref(info)) == EINVAL
    assert lib.mi355_spmv_row_softmax_set_scale(h, 0.125) == OK
    # nothing stored: nothing launched, also with every operand null
    assert lib.mi355_spmv_row_softmax_execute(h, None, None, None) == OK
    assert lib.mi355_spmv_row_softmax_backward(h, None, None, None, None) == OK
    assert lib.mi355_spmv_row_softmax_destroy(h) == OK


def test_execute_backward_and_the_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    refused(lib, lib.mi355_spmv_row_softmax_execute(None, DUMMY, DUMMY, None), EINVAL, "object")
    refused(lib, lib.mi355_spmv_row_softmax_backward(None, DUMMY, DUMMY, DUMMY, None), EINVAL, "object")
    refused(lib, lib.mi355_spmv_row_softmax_set_scale(None, 1.0), EINVAL, "object")
    assert lib.mi355_spmv_row_softmax_destroy(None) == OK
    for o in ("i32", "i64"):
        for v in ("f32", "f64"):
            f = getattr(lib, "mi355_spmv_row_softmax_%s_%s" % (o, v))
            refused(lib, f(4, 4, 4, None, DUMMY, DUMMY, DUMMY, 1.0, None), EINVAL, "Ap")
            refused(lib, f(4, 4, 4, DUMMY, None, DUMMY, DUMMY, 1.0, None), EINVAL, "Aj")
            refused(lib, f(4, 4, -1, DUMMY, DUMMY, DUMMY, DUMMY, 1.0, None), EINVAL, "nnz")
            refused(lib, f(-1, 4, 4, DUMMY, DUMMY, DUMMY, DUMMY, 1.0, None), EINVAL, "n_rows")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, None, DUMMY, 1.0, None), EINVAL, "null x")
            refused(lib, f(4, 4, 4, DUMMY, DUMMY, DUMMY, None, 1.0, None), EINVAL, "null out")
            # nothing stored: nothing to launch, no device call, OK — also with every pointer null
            assert f(0, 4, 0, None, None, None, None, 1.0, None) == OK
            assert f(4, 4, 0, DUMMY, None, None, None, 0.5, None) == OK


class _OnDevice:
    """A tensor that says it lives on the device: the other checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_python_checks(sp):
    Ap = torch.zeros(4, dtype=torch.int32)
    Aj = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.RowSoftmaxPlan(3, 2, 0, Ap, Aj, torch.float32)
    dAp, dAj = _OnDevice(Ap), _OnDevice(Aj)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.RowSoftmaxPlan(3, 2, 0, dAp, _OnDevice(Aj.long()), torch.float32)
    for dt in (torch.int32, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32 or float64"):
            sp.RowSoftmaxPlan(3, 2, 0, dAp, dAj, dt)
    # the object of a matrix that stores nothing is made without a device; its operand checks are those of any plan
    plan = sp.RowSoftmaxPlan(3, 2, 0, dAp, dAj, torch.float32)
    plan.nnz = 3        # (the checks below compare against the Python object's sizes; nothing reaches the library)
    info = plan.info()
    assert info["n_slices"] == 1 and info["slice_len"] == 1024 and info["main_kernel"] == "row_softmax_slice_kernel"
    assert info["scratch_bytes"] == 0
    plan.set_scale(0.5)
    x, out = _OnDevice(torch.ones(3)), _OnDevice(torch.zeros(3))
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(torch.ones(3), out)
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(x, torch.zeros(3))
    with pytest.raises(RuntimeError, match="contiguous"):
        plan.execute(_OnDevice(torch.ones(6)[::2]), out)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(_OnDevice(torch.ones(3, dtype=torch.float64)), out)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(x, _OnDevice(torch.zeros(3, dtype=torch.float16)))
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(_OnDevice(torch.ones(2)), out)
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(x, _OnDevice(torch.zeros(2)))
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(_OnDevice(torch.ones(3, 1)), out)          # not 1-D
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.backward(x, torch.ones(3), out)
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.backward(x, _OnDevice(torch.ones(3, dtype=torch.float64)), out)
    with pytest.raises(ValueError, match="shorter than"):
        plan.backward(_OnDevice(torch.ones(2)), x, out)
    with pytest.raises(ValueError, match="shorter than"):
        plan.backward(x, x, _OnDevice(torch.zeros(1)))
    plan.destroy()
    plan.destroy()
    # the one-shot
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.row_softmax(3, 2, 3, Ap, Aj, x)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.row_softmax(3, 2, 3, dAp, dAj, torch.ones(3))
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.row_softmax(3, 2, 3, dAp, _OnDevice(Aj.long()), x)
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.row_softmax(3, 2, 3, dAp, dAj, _OnDevice(torch.ones(3, dtype=torch.float16)))
    with pytest.raises(TypeError, match="differs from the plan's"):
        sp.row_softmax(3, 2, 3, dAp, dAj, x, _OnDevice(torch.zeros(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="shorter than"):
        sp.row_softmax(3, 2, 4, dAp, dAj, x)


# ---- the table's own self-checks ---------------------------------------------------------------------------------------
def serial_softmax(x, scale, lens):
    """Row by row, in fp64, the plain way."""
    out, n = np.zeros(len(x)), 0
    for length in lens:
        v = scale * x[n:n + length].astype(np.float64)
        if length and np.isfinite(v.max()):
            e = np.exp(v - v.max())
            out[n:n + length] = e / e.sum()
        n += length
    return out


def test_the_table_has_names_of_its_own_and_covers_what_it_says():
    table = rc.table()
    assert len({c.name for c in table}) == len(table) > 800
    assert max(sum(c.matrix.lens) for c in table) == 30000 + 50
    for fam in rc.FAMILIES[:8]:
        cases = rc.family(fam)
        assert {c.val for c in cases} == {"f32", "f64"} and {c.off for c in cases} == {"i32", "i64"}, fam
        assert {(c.mode, c.kind) for c in cases} == {("fwd", "const"), ("fwd", "masked"), ("fwd", "real"), ("bwd", "const"), ("bwd", "real")}
        assert {c.scale for c in cases if c.kind == "real"} == set(rc.SCALES)
    assert {c.shift for c in table} == set(rc.SHIFTS)
    hub = [c.name for c in table if c.matrix.name == "hub_row_30000" and (c.off, c.val) == ("i32", "f32")]
    assert "const" in hub[0] and any("real" in n for n in hub[1:])      # other values on the hub row's plan, behind its first execute
    assert len(rc.slices(rc.structures("hub")[0].lens)) >= 30


def test_the_references_agree_with_a_serial_softmax_and_its_jacobian():
    for fam in ("row_ends", "slice_edges", "ragged", "pow2"):
        m = rc.structures(fam)[0]
        c = rc._case(m, "i32", "f64", "fwd", "real", 1, -2.0)
        x, _ = rc.operands(c)
        want, v, vmax, spread = rc.forward_ref(x, c.scale, m)
        assert np.allclose(want, serial_softmax(x, c.scale, m.lens), rtol=1e-13, atol=0)
        assert spread.max() <= 20.0 and vmax.max() <= 71.0
        sums = np.bincount(rc.rows_of(m), weights=want, minlength=len(m.lens))
        assert np.allclose(sums[np.asarray(m.lens) > 0], 1.0, rtol=1e-12)
        # backward = the Jacobian of the forward applied to dp: a central difference of the serial softmax along a direction
        rng = np.random.RandomState(5)
        dp = rng.rand(len(x)) * 2 - 1
        dx, t, tabs = rc.backward_ref(want, dp, c.scale, m)
        d = rng.rand(len(x)) - 0.5
        h = 1e-6
        fd = (serial_softmax(x + h * d, c.scale, m.lens) - serial_softmax(x - h * d, c.scale, m.lens)) / (2 * h)
        assert abs(np.dot(dx, d) - np.dot(dp.astype(np.float64), fd)) <= 1e-6 * (np.abs(dx * d).sum() + 1e-12)


def test_the_masks_reach_every_place_the_issue_names():
    for fam in ("slice_edges", "ragged", "hub", "pow2"):
        for m in rc.structures(fam):
            lens = np.asarray(m.lens)
            Ap = np.concatenate(([0], np.cumsum(lens)))
            nnz = int(Ap[-1])
            if nnz == 0:
                continue
            both = [rc.mask(m, v) for v in (0, 1)]
            for mk in both:
                assert 0 < mk.sum() < nnz or nnz < 8
                for r0, r1, n0, nn in rc.slices(m.lens):
                    for e in range(n0, n0 + nn + 1, rc.STEP):       # both sides of every group and slice edge
                        assert (e == 0 or mk[e - 1]) and (e >= nnz or e >= n0 + nn or mk[e])
            either = both[0] | both[1]
            rows = [r for r in range(len(lens)) if lens[r] > 1]
            assert len(rows) < 8 or (any(both[0][Ap[r]] for r in rows) and any(both[0][Ap[r + 1] - 1] for r in rows))   # first, last of a row
            whole = [r for r in range(len(lens)) if lens[r] and either[Ap[r]:Ap[r + 1]].all()]
            assert whole or len(rows) < 8, m.name
    # a whole piece of a crossing row, head and tail, and the rest of that row left live
    m = rc.structures("hub")[0]
    sl = rc.slices(m.lens)
    hub_begin, hub_end = 3, 30003
    mid = [(n0, nn) for r0, r1, n0, nn in sl if n0 > hub_begin and n0 + nn < hub_end]
    for v in (0, 1):
        mk = rc.mask(m, v)
        assert any(mk[n0:n0 + nn].all() for n0, nn in mid) and not mk[hub_begin:hub_end].all()


def test_the_exact_values_are_what_numpy_gives_in_fp64():
    """const and masked rows: the fp64 reference rounds to the exact value the table asks for, bit for bit."""
    for fam in ("open_row", "pow2"):
        m = rc.structures(fam)[1 if fam == "open_row" else 0]
        for val in ("f32", "f64"):
            for kind, variant in (("const", 0), ("masked", 0), ("masked", 1)):
                c = rc._case(m, "i32", val, "fwd", kind, variant, 1.0)
                x, _ = rc.operands(c)
                want = rc.forward_ref(x, 1.0, m)[0].astype(rc.NP[val])
                rc.check(c, want)
                if kind == "masked":
                    bad = want.copy()
                    bad[np.nonzero(np.isneginf(x))[0][0]] = -0.0        # a masked entry must be +0, not -0
                    with pytest.raises(AssertionError):
                        rc.check(c, bad)
            b = rc._case(m, "i32", val, "bwd", "const", 0, -2.0)
            p, dp = rc.operands(b)
            rc.check(b, rc.backward_ref(p, dp, -2.0, m)[0].astype(rc.NP[val]))
            off = rc.backward_ref(p, dp, -2.0, m)[0].astype(rc.NP[val])
            off[0] = np.nextafter(off[0], rc.NP[val](9))
            with pytest.raises(AssertionError):
                rc.check(b, off)
