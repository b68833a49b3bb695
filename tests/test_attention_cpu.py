"""Fused sparse attention without a device (mi355_spmv_attention_*, sp.SparseAttentionPlan, sp.sparse_attention): the
names are declared with the header's signatures, exported and bound; every argument error is refused before any device
call with a status and a text that names the argument (on dummy pointers: nothing is dereferenced); an object of a matrix
without rows is made, reported, executed and destroyed without a device call; the Python checks; and the table's own
self-checks against numpy (tests/attention_cases.py: its reference, its exact values and its coverage, which both the
host simulation and the device file rely on)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import attention_cases as ac
from conftest import ROOT

NAMES = (["mi355_spmv_attention_" + n for n in ("create", "set_scale", "execute", "get_info", "destroy")]
         + ["mi355_spmv_attention_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")])
OK, EINVAL, ENOTSUP = 0, 1, 2
OFF_I32, OFF_I64 = 0, 1
F32, F64, I32, PATTERN, F16, BF16 = 0, 1, 2, 3, 4, 5
DUMMY = C.c_void_p(256)


def header():
    return open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()


def declared_arguments(text, name):
    """The C types of a declaration's arguments, names and spaces dropped."""
    m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        words = arg.replace("*", " * ").split()
        out.append(" ".join(w for w in words[:-1]).replace(" *", "*"))
    return out


C_OF = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}


def test_the_names_are_declared_with_the_headers_signatures_exported_and_bound(sp):
    text = header()
    lib = sp.capi.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in sp.capi.EXPORTS, n
        args = declared_arguments(text, n)
        bound = getattr(lib, n).argtypes
        assert bound is not None and len(bound) == len(args), (n, args)
        for a, b in zip(args, bound):
            if a.endswith("**"):
                assert b is C.POINTER(C.c_void_p) or b is C.c_void_p, (n, a, b)
            elif a.endswith("*"):
                assert b is C.c_void_p or (a.endswith("_info*") and b is C.POINTER(sp.capi.AttentionInfo)), (n, a, b)
            else:
                assert b is C_OF[a], (n, a, b)
    assert re.search(r"^#define MI355_SPMV_HAS_ATTENTION 1\b", text, flags=re.M)
    assert sp.SparseAttentionPlan is sp.capi.SparseAttentionPlan and sp.sparse_attention is sp.capi.sparse_attention
    assert "attention.hip" in open(os.path.join(ROOT, "spmv-samples_amd", "csrc", "Makefile")).read()


def test_the_info_struct_is_the_headers(sp):
    m = re.search(r"typedef struct mi355_spmv_attention_info \{(.*?)\} mi355_spmv_attention_info;", header(), flags=re.S)
    fields = []
    for line in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        words = line.split()
        if not words:
            continue
        for name in " ".join(words[1:]).split(","):
            name = name.strip()
            k = re.match(r"(\w+)\[(\d+)\]", name)
            fields.append((k.group(1), C.c_char * int(k.group(2))) if k else (name, C_OF[words[0]]))
    assert [(n, t) for n, t in sp.capi.AttentionInfo._fields_] == fields


def refused(lib, status, want, *words):
    assert status == want, (status, lib.mi355_spmv_last_error())
    text = lib.mi355_spmv_last_error().decode()
    for w in words:
        assert w in text, (w, text)


def test_create_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda n_rows, n_cols, nnz, Ap, Aj, off, val, d_max=8, dv_max=8: lib.mi355_spmv_attention_create(
        n_rows, n_cols, nnz, Ap, Aj, off, val, d_max, dv_max, C.byref(h))
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, 5, F32), EINVAL, "off_type")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, I32), ENOTSUP, "val_type", "I32")
    for vt in (PATTERN, F16, BF16, 9, -1):
        refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, vt), EINVAL, "val_type")
    refused(lib, create(-1, 4, 4, DUMMY, DUMMY, OFF_I32, F32), EINVAL, "n_rows")
    refused(lib, create(4, -1, 4, DUMMY, DUMMY, OFF_I32, F32), EINVAL, "n_cols")
    refused(lib, create(4, 4, -1, DUMMY, DUMMY, OFF_I32, F32), EINVAL, "nnz")
    refused(lib, create(4, 4, 2 ** 31, DUMMY, DUMMY, OFF_I32, F64), EINVAL, "nnz", "32-bit")
    refused(lib, create(4, 4, 4, None, DUMMY, OFF_I32, F32), EINVAL, "Ap")
    refused(lib, create(4, 4, 4, DUMMY, None, OFF_I64, F32), EINVAL, "Aj")
    refused(lib, create(4, 0, 4, DUMMY, DUMMY, OFF_I32, F32), EINVAL, "n_cols")
    refused(lib, create(0, 4, 4, None, DUMMY, OFF_I32, F32), EINVAL, "n_rows")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, F32, 0, 8), EINVAL, "d_max")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, F32, 8, 0), EINVAL, "dv_max")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, F32, -3, 8), EINVAL, "d_max")
    assert not h.value
    refused(lib, lib.mi355_spmv_attention_create(4, 4, 4, DUMMY, DUMMY, OFF_I32, F32, 8, 8, None), EINVAL, "out")


@pytest.mark.parametrize("off,val", [(OFF_I32, F32), (OFF_I64, F64)])
def test_an_object_without_rows_needs_no_device_and_refuses_bad_operands(sp, off, val):
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert lib.mi355_spmv_attention_create(0, 7, 0, None, None, off, val, 40, 70, C.byref(h)) == OK
    info = sp.capi.AttentionInfo()
    assert lib.mi355_spmv_attention_get_info(h, C.byref(info)) == OK
    assert (info.off_type, info.val_type, info.d_max, info.dv_max) == (off, val, 40, 70)
    assert info.slice_len == 1024 and info.block_threads % 64 == 0
    assert info.widest_tile == (32, 16)[val] and info.passes == -(-70 // info.widest_tile) and info.lanes_per_slot == 8
    assert info.n_slices == 0 and info.grid_blocks == 0 and info.scratch_bytes == 0
    assert info.main_kernel == b"attention_slice_kernel"
    assert lib.mi355_spmv_attention_get_info(h, None) == EINVAL and lib.mi355_spmv_attention_get_info(None, C.byref(info)) == EINVAL
    assert lib.mi355_spmv_attention_set_scale(h, 0.125) == OK
    ex = lambda d=8, dv=8, Q=DUMMY, ldq=8, K=DUMMY, ldk=8, V=DUMMY, ldv=8, bias=None, O=DUMMY, ldo=8, lse=None: lib.mi355_spmv_attention_execute(
        h, d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse, None)
    refused(lib, ex(d=0), EINVAL, "d = 0")
    refused(lib, ex(dv=0), EINVAL, "dv = 0")
    refused(lib, ex(d=-2), EINVAL, "d = -2")
    refused(lib, ex(d=41, ldq=64, ldk=64), EINVAL, "d = 41", "d_max = 40")
    refused(lib, ex(dv=71, ldv=80, ldo=80), EINVAL, "dv = 71", "dv_max = 70")
    refused(lib, ex(ldq=7), EINVAL, "ldq")
    refused(lib, ex(ldk=7), EINVAL, "ldk")
    refused(lib, ex(ldv=7), EINVAL, "ldv")
    refused(lib, ex(ldo=7), EINVAL, "ldo")
    # no rows: nothing launched, no device call, also with every operand null
    assert ex(Q=None, K=None, V=None, O=None) == OK
    assert ex(d=40, dv=70, ldq=40, ldk=41, ldv=70, ldo=99) == OK
    assert lib.mi355_spmv_attention_destroy(h) == OK


def test_execute_and_the_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    refused(lib, lib.mi355_spmv_attention_execute(None, 8, 8, DUMMY, 8, DUMMY, 8, DUMMY, 8, None, DUMMY, 8, None, None), EINVAL, "object")
    refused(lib, lib.mi355_spmv_attention_set_scale(None, 1.0), EINVAL, "object")
    assert lib.mi355_spmv_attention_destroy(None) == OK
    for o in ("i32", "i64"):
        for v in ("f32", "f64"):
            f = getattr(lib, "mi355_spmv_attention_%s_%s" % (o, v))
            call = lambda n_rows=4, n_cols=4, nnz=4, Ap=DUMMY, Aj=DUMMY, d=8, dv=8, Q=DUMMY, ldq=8, K=DUMMY, ldk=8, V=DUMMY, ldv=8, bias=None, O=DUMMY, ldo=8: f(
                n_rows, n_cols, nnz, Ap, Aj, d, dv, Q, ldq, K, ldk, V, ldv, bias, 1.0, O, ldo, None, None)
            refused(lib, call(Ap=None), EINVAL, "Ap")
            refused(lib, call(Aj=None), EINVAL, "Aj")
            refused(lib, call(nnz=-1), EINVAL, "nnz")
            refused(lib, call(n_rows=-1), EINVAL, "n_rows")
            refused(lib, call(d=0), EINVAL, "d = 0")
            refused(lib, call(dv=0), EINVAL, "dv = 0")
            refused(lib, call(ldq=7), EINVAL, "ldq")
            refused(lib, call(ldk=3), EINVAL, "ldk")
            refused(lib, call(ldv=7), EINVAL, "ldv")
            refused(lib, call(ldo=1), EINVAL, "ldo")
            refused(lib, call(Q=None), EINVAL, "null Q")
            refused(lib, call(K=None), EINVAL, "null K")
            refused(lib, call(V=None), EINVAL, "null V")
            refused(lib, call(O=None), EINVAL, "null O")
            # no rows: nothing to launch, no device call, OK — also with every pointer null
            assert call(n_rows=0, nnz=0, Ap=None, Aj=None, Q=None, K=None, V=None, O=None) == OK


class _OnDevice:
    """A tensor that says it lives on the device: the other checks come after the device checks."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_python_checks(sp):
    Ap = torch.zeros(1, dtype=torch.int32)
    Aj = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.SparseAttentionPlan(0, 2, 0, Ap, Aj, torch.float32, 8, 8)
    dAp, dAj = _OnDevice(Ap), _OnDevice(Aj)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.SparseAttentionPlan(0, 2, 0, dAp, _OnDevice(Aj.long()), torch.float32, 8, 8)
    for dt in (torch.int32, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32 or float64"):
            sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, dt, 8, 8)
    with pytest.raises(RuntimeError, match="d_max"):
        sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, torch.float32, 0, 8)
    # the object of a matrix without rows is made without a device; its operand checks are those of any plan
    plan = sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, torch.float32, 8, 40)
    plan.n_rows = 3     # (the checks below compare against the Python object's sizes; nothing reaches the library)
    info = plan.info()
    assert info["n_slices"] == 0 and info["passes"] == 2 and info["main_kernel"] == "attention_slice_kernel" and "reserved" not in info
    plan.set_scale(0.5)
    Q, K, V = _OnDevice(torch.ones(3, 8)), _OnDevice(torch.ones(2, 8)), _OnDevice(torch.ones(2, 5))
    out = _OnDevice(torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(torch.ones(3, 8), K, V, out)
    with pytest.raises(RuntimeError, match="device tensors only"):
        plan.execute(Q, K, V, torch.zeros(3, 5))
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(_OnDevice(torch.ones(3, 8, dtype=torch.float64)), K, V, out)
    with pytest.raises(ValueError, match="2-D"):
        plan.execute(_OnDevice(torch.ones(24)), K, V, out)
    with pytest.raises(ValueError, match="row-major"):
        plan.execute(_OnDevice(torch.ones(8, 3).t()), K, V, out)
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(_OnDevice(torch.ones(2, 8)), K, V, out)
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(Q, K, _OnDevice(torch.ones(1, 5)), out)
    with pytest.raises(ValueError, match="Q and K differ"):
        plan.execute(Q, _OnDevice(torch.ones(2, 7)), V, out)
    with pytest.raises(ValueError, match="above the plan's"):
        plan.execute(_OnDevice(torch.ones(3, 9)), _OnDevice(torch.ones(2, 9)), V, out)
    with pytest.raises(ValueError, match="above the plan's"):
        plan.execute(Q, K, _OnDevice(torch.ones(2, 41)), None)
    with pytest.raises(ValueError, match="out has 4 columns"):
        plan.execute(Q, K, V, _OnDevice(torch.zeros(3, 4)))
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(Q, K, V, out, lse=_OnDevice(torch.zeros(2)))
    with pytest.raises(TypeError, match="differs from the plan's"):
        plan.execute(Q, K, V, out, lse=_OnDevice(torch.zeros(3, dtype=torch.float64)))
    plan.nnz = 4
    with pytest.raises(ValueError, match="shorter than"):
        plan.execute(Q, K, V, out, bias=_OnDevice(torch.zeros(3)))
    plan.destroy()
    plan.destroy()
    # the one-shot
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.sparse_attention(3, 2, 3, Ap, Aj, Q, K, V)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.sparse_attention(3, 2, 3, dAp, dAj, torch.ones(3, 8), K, V)
    with pytest.raises(TypeError, match="Aj must be int32"):
        sp.sparse_attention(3, 2, 3, dAp, _OnDevice(Aj.long()), Q, K, V)
    with pytest.raises(TypeError, match="float32 or float64"):
        sp.sparse_attention(3, 2, 3, dAp, dAj, _OnDevice(torch.ones(3, 8, dtype=torch.float16)), K, V)
    with pytest.raises(ValueError, match="Q and K differ"):
        sp.sparse_attention(3, 2, 3, dAp, dAj, Q, _OnDevice(torch.ones(2, 7)), V)


# ---- the table's own self-checks ---------------------------------------------------------------------------------------
def serial_attention(c):
    """Row by row, in fp64, the plain way: (O, lse)."""
    m = c.matrix
    Ap, Aj = ac.csr(m, c.off)
    Q, K, V, bias = ac.operands(c)
    n_rows = len(m.lens)
    O, lse = np.zeros((n_rows, c.dv)), np.full(n_rows, -np.inf)
    scale = float(ac.NP[c.val](c.scale))
    for r in range(n_rows):
        a, b = int(Ap[r]), int(Ap[r + 1])
        cols = Aj[a:b]
        v = scale * (K[cols, c.c0:c.c0 + c.d].astype(np.float64) @ Q[r, c.c0:c.c0 + c.d].astype(np.float64))
        if bias is not None:
            v = v + bias[a:b].astype(np.float64)
        live = np.isfinite(v)
        v, cols = v[live], cols[live]
        if v.size:
            e = np.exp(v - v.max())
            O[r] = (e[:, None] * V[cols, c.cv0:c.cv0 + c.dv].astype(np.float64)).sum(0) / e.sum()
            lse[r] = v.max() + np.log(e.sum())
    return O, lse


def test_the_table_has_names_of_its_own_and_covers_what_it_says():
    table = ac.table()
    assert len({c.name for c in table}) == len(table) > 600
    assert max(sum(c.matrix.lens) for c in table) == 30000 + 50
    assert any(c.matrix.n_cols == 1 for c in table)
    for fam in ac.STRUCTURE_FAMILIES:
        cases = ac.family(fam)
        assert {c.val for c in cases} == {"f32", "f64"} and {c.off for c in cases} == {"i32", "i64"}, fam
        assert {c.kind for c in cases} == {"const", "masked", "real"}, fam
        assert {c.scale for c in cases if c.kind == "real"} == set(ac.SCALES), fam
    assert {c.shift for c in table} >= set(ac.SHIFTS)
    assert {(c.ldq - c.d, c.ldk - c.d, c.ldv - c.dv, c.ldo - c.dv) for c in table} == set(ac.PADS)
    assert {c.want_lse for c in table} == {True, False}
    for val in ("f32", "f64"):
        mine = [c for c in table if c.val == val]
        assert {c.dv for c in mine} >= set(ac.DV_ALL[val]) and {c.d for c in mine} >= set(ac.D_ALL[val])
        # every C, widths that are no multiple of a lane's columns, the widest tile, two and three passes
        assert {ac.lanes_per_slot(min(c.dv, ac.TILE[val]), val) for c in mine} == set(ac.LANES_PER_SLOT)
        assert {-(-c.dv // ac.TILE[val]) for c in mine} == {1, 2, 3}
        assert any(c.dv % ac.VEC[val] for c in mine) and any(c.dv == ac.TILE[val] for c in mine)
        # the tile loop over d: one round, two rounds, more, and a last round that is not whole
        rounds = {(-(-c.d // (ac.lanes_per_slot(min(c.dv, ac.TILE[val]), val) * ac.VEC[val])),
                   c.d % (ac.lanes_per_slot(min(c.dv, ac.TILE[val]), val) * ac.VEC[val]) != 0) for c in mine}
        assert {r for r, _ in rounds} >= {1, 2} and max(r for r, _ in rounds) > 2 and {(1, True), (2, True), (2, False), (1, False)} <= rounds
    seq = [c for c in ac.hub_sequence() if (c.off, c.val) == ("i32", "f32")]
    assert seq[0].kind == "const" and any(c.kind == "real" for c in seq[1:])        # other operands behind the first execute
    assert [c.dv for c in seq].index(3) > [c.dv for c in seq].index(65)             # a narrow dv after a wide one
    assert len(ac.slices(ac.structures("hub")[0].lens)) >= 30


def test_the_reference_agrees_with_a_serial_attention():
    for fam, i in (("row_ends", 0), ("slice_edges", 0), ("ragged", 0), ("one_col", 0)):
        m = ac.structures(fam)[i]
        for kind, variant, scale, d, dv in (("real", 0, 0.125, 13, 5), ("real", 2, -2.0, 4, 9), ("masked", 1, 0.125, 3, 4)):
            c = ac._case(m, "i32", "f64", kind, variant, scale, d, dv)
            ex = ac.expected(c)
            O, lse = serial_attention(c)
            assert np.allclose(ex["want"], O, rtol=1e-12, atol=1e-14), (fam, kind)      # (integer sums that cancel)
            assert np.array_equal(np.isneginf(ex["lse"]), np.isneginf(lse)), (fam, kind)
            ok = ~np.isneginf(lse)
            assert np.allclose(ex["lse"][ok], lse[ok], rtol=1e-12), (fam, kind)
            if kind == "real":
                assert ex["spread"].max() <= 20.0 and np.all(ex["bound"] > 0)


def test_the_exact_values_are_what_numpy_gives_in_fp64_and_a_wrong_one_is_caught():
    m = ac.structures("pow2")[0]
    for val in ("f32", "f64"):
        for kind, variant in (("const", 0), ("const", 1), ("masked", 0), ("masked", 1)):
            c = ac._case(m, "i32", val, kind, variant, 1.0, 3, 5)
            ex = ac.expected(c)
            T = ac.NP[val]
            O = (np.rint(ex["want"] * np.maximum(ex["live"], 1)[:, None]).astype(T) / np.maximum(ex["live"], 1).astype(T)[:, None]).astype(T)
            lse = ex["lse"].astype(T)
            ac.check(c, O, lse)
            bad = O.copy()
            r = int(np.nonzero(ex["live"] > 2)[0][0])
            bad[r, 0] = np.nextafter(bad[r, 0], T(9))
            with pytest.raises(AssertionError):
                ac.check(c, bad, lse)
            dead = np.nonzero(ex["live"] == 0)[0]
            assert dead.size
            bad = O.copy()
            bad[dead[0], 1] = -0.0          # a row without a live entry must be +0, not -0
            with pytest.raises(AssertionError):
                ac.check(c, bad, lse)
            bad = lse.copy()
            bad[dead[0]] = 0.0
            with pytest.raises(AssertionError):
                ac.check(c, O, bad)
    # real data: the fp64 value passes, a value twice the bound away does not
    c = ac._case(ac.structures("ragged")[0], "i64", "f32", "real", 1, 0.125, 17, 9)
    ex = ac.expected(c)
    O, lse = ex["want"].astype(np.float32), ex["lse"].astype(np.float32)
    ratios = []
    ac.check(c, O, lse, ratios)
    assert len(ratios) == 1 and ratios[0] < 1
    bad = O.copy()
    r = int(np.argmax(ex["bound"][:, 0]))
    bad[r, 0] += np.float32(4 * ex["bound"][r, 0])
    with pytest.raises(AssertionError):
        ac.check(c, bad, lse)
