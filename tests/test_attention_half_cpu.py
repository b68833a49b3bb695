"""Fused sparse attention with 16-bit Q, K, V and O without a device (mi355_spmv_attention_create_half / _get_types /
_half_*, sp.SparseAttentionPlan(vec_dtype=), sp.sparse_attention_half): the names are declared with the header's signatures,
exported and bound; every argument error is refused before any device call with a status and a text that names the argument
(on dummy pointers: nothing is dereferenced); an object of a matrix without rows is made, reported, executed and destroyed
without a device call; the Python checks; the self-checks of the table (tests/attention_half_cases.py); and a serial
emulation of the contract — fp32 on the widened values, row by row in plain order, ONE narrowing at the end — which must
stay inside the derived bound on every real case and reproduce the const and masked expectations bit for bit: the proof
that a correct implementation can meet what the host simulation and the device file hold the library to."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import attention_half_cases as hc
from test_attention_cpu import C_OF, DUMMY, _OnDevice, declared_arguments, header, refused

NAMES = (["mi355_spmv_attention_create_half", "mi355_spmv_attention_get_types"]
         + ["mi355_spmv_attention_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")])
OK, EINVAL, ENOTSUP = 0, 1, 2
OFF_I32, OFF_I64 = 0, 1
F32, F64, I32, PATTERN, F16, BF16 = 0, 1, 2, 3, 4, 5


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
                assert b is C.POINTER(C.c_void_p), (n, a, b)
            elif a == "int*":
                assert b is C.POINTER(C.c_int), (n, a, b)
            elif a.endswith("*"):
                assert b is C.c_void_p, (n, a, b)
            else:
                assert b is C_OF[a], (n, a, b)
    assert re.search(r"^#define MI355_SPMV_HAS_ATTENTION_HALF 1\b", text, flags=re.M)
    assert sp.sparse_attention_half is sp.capi.sparse_attention_half


def create_half(lib, h, n_rows, n_cols, nnz, Ap, Aj, off, vec, d_max=8, dv_max=8):
    return lib.mi355_spmv_attention_create_half(C.byref(h), off, vec, n_rows, n_cols, nnz, Ap, Aj, d_max, dv_max)


def test_create_half_refuses_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    h = C.c_void_p()
    create = lambda *a, **k: create_half(lib, h, *a, **k)
    for vt in (F32, F64, I32, PATTERN, 9, -1):
        refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, vt), EINVAL, "vec_type")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, 5, F16), EINVAL, "off_type")
    refused(lib, create(-1, 4, 4, DUMMY, DUMMY, OFF_I32, F16), EINVAL, "n_rows")
    refused(lib, create(4, -1, 4, DUMMY, DUMMY, OFF_I32, BF16), EINVAL, "n_cols")
    refused(lib, create(4, 4, -1, DUMMY, DUMMY, OFF_I32, F16), EINVAL, "nnz")
    refused(lib, create(4, 4, 2 ** 31, DUMMY, DUMMY, OFF_I32, BF16), EINVAL, "nnz", "32-bit")
    refused(lib, create(4, 4, 4, None, DUMMY, OFF_I32, F16), EINVAL, "Ap")
    refused(lib, create(4, 4, 4, DUMMY, None, OFF_I64, BF16), EINVAL, "Aj")
    refused(lib, create(4, 0, 4, DUMMY, DUMMY, OFF_I32, F16), EINVAL, "n_cols")
    refused(lib, create(0, 4, 4, None, DUMMY, OFF_I32, F16), EINVAL, "n_rows")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, F16, 0, 8), EINVAL, "d_max")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, BF16, 8, 0), EINVAL, "dv_max")
    refused(lib, create(4, 4, 4, DUMMY, DUMMY, OFF_I32, F16, -3, 8), EINVAL, "d_max")
    assert not h.value
    refused(lib, lib.mi355_spmv_attention_create_half(None, OFF_I32, F16, 4, 4, 4, DUMMY, DUMMY, 8, 8), EINVAL, "out")
    # the fp32 / fp64 create keeps refusing the 16-bit types as a val_type
    for vt in (F16, BF16):
        refused(lib, lib.mi355_spmv_attention_create(4, 4, 4, DUMMY, DUMMY, OFF_I32, vt, 8, 8, C.byref(h)), EINVAL, "val_type", "16-bit")
    assert not h.value


def types_of(lib, h):
    val, vec = C.c_int(-1), C.c_int(-1)
    assert lib.mi355_spmv_attention_get_types(h, C.byref(val), C.byref(vec)) == OK
    return val.value, vec.value


@pytest.mark.parametrize("off,vec", [(OFF_I32, F16), (OFF_I64, BF16)])
def test_an_object_without_rows_needs_no_device_reports_its_types_and_refuses_bad_operands(sp, off, vec):
    lib = sp.capi.lib()
    h = C.c_void_p()
    assert create_half(lib, h, 0, 7, 0, None, None, off, vec, 40, 130) == OK
    info = sp.capi.AttentionInfo()
    assert lib.mi355_spmv_attention_get_info(h, C.byref(info)) == OK
    assert (info.off_type, info.val_type, info.d_max, info.dv_max) == (off, F32, 40, 130)
    assert info.slice_len == 1024 and info.block_threads % 64 == 0
    assert info.widest_tile == 64 and info.passes == 3 and info.lanes_per_slot == 8
    assert info.n_slices == 0 and info.grid_blocks == 0 and info.scratch_bytes == 0
    assert info.main_kernel == b"attention_half_slice_kernel"
    assert types_of(lib, h) == (F32, vec)
    val = C.c_int()
    refused(lib, lib.mi355_spmv_attention_get_types(None, C.byref(val), C.byref(val)), EINVAL, "get_types")
    refused(lib, lib.mi355_spmv_attention_get_types(h, None, C.byref(val)), EINVAL, "get_types")
    refused(lib, lib.mi355_spmv_attention_get_types(h, C.byref(val), None), EINVAL, "get_types")
    assert lib.mi355_spmv_attention_set_scale(h, 0.125) == OK
    ex = lambda d=8, dv=8, Q=DUMMY, ldq=8, K=DUMMY, ldk=8, V=DUMMY, ldv=8, bias=None, O=DUMMY, ldo=8, lse=None: lib.mi355_spmv_attention_execute(
        h, d, dv, Q, ldq, K, ldk, V, ldv, bias, O, ldo, lse, None)
    refused(lib, ex(d=0), EINVAL, "d = 0")
    refused(lib, ex(dv=0), EINVAL, "dv = 0")
    refused(lib, ex(d=41, ldq=64, ldk=64), EINVAL, "d = 41", "d_max = 40")
    refused(lib, ex(dv=131, ldv=136, ldo=136), EINVAL, "dv = 131", "dv_max = 130")
    refused(lib, ex(ldq=7), EINVAL, "ldq")
    refused(lib, ex(ldk=7), EINVAL, "ldk")
    refused(lib, ex(ldv=7), EINVAL, "ldv")
    refused(lib, ex(ldo=7), EINVAL, "ldo")
    assert ex(Q=None, K=None, V=None, O=None) == OK       # no rows: nothing launched, also with every operand null
    assert ex(d=40, dv=130, ldq=40, ldk=41, ldv=130, ldo=199) == OK
    assert lib.mi355_spmv_attention_destroy(h) == OK
    # one tile, and a narrow one
    for dv_max, passes, lanes in ((64, 1, 8), (65, 2, 8), (33, 1, 8), (32, 1, 4), (9, 1, 2), (8, 1, 1)):
        assert create_half(lib, h, 0, 7, 0, None, None, off, vec, 16, dv_max) == OK
        assert lib.mi355_spmv_attention_get_info(h, C.byref(info)) == OK
        assert (info.passes, info.lanes_per_slot, info.widest_tile) == (passes, lanes, 64), dv_max
        assert lib.mi355_spmv_attention_destroy(h) == OK


def test_get_types_of_an_fp32_and_an_fp64_object_gives_the_type_twice(sp):
    lib = sp.capi.lib()
    for val in (F32, F64):
        h = C.c_void_p()
        assert lib.mi355_spmv_attention_create(0, 7, 0, None, None, OFF_I32, val, 8, 8, C.byref(h)) == OK
        assert types_of(lib, h) == (val, val)
        assert lib.mi355_spmv_attention_destroy(h) == OK


def test_the_one_shots_refuse_bad_arguments_before_any_device_call(sp):
    lib = sp.capi.lib()
    for o in ("i32", "i64"):
        for v in ("f16", "bf16"):
            f = getattr(lib, "mi355_spmv_attention_half_%s_%s" % (o, v))
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
            assert call(n_rows=0, nnz=0, Ap=None, Aj=None, Q=None, K=None, V=None, O=None) == OK


def test_python_checks(sp):
    Ap = torch.zeros(1, dtype=torch.int32)
    Aj = torch.zeros(0, dtype=torch.int32)
    dAp, dAj = _OnDevice(Ap), _OnDevice(Aj)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sp.SparseAttentionPlan(0, 2, 0, Ap, Aj, torch.float32, 8, 8, vec_dtype=torch.float16)
    with pytest.raises(TypeError, match="vec_dtype needs val_dtype float32"):
        sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, torch.float64, 8, 8, vec_dtype=torch.bfloat16)
    for dt in (torch.float32, torch.float64, torch.int32):
        with pytest.raises(TypeError, match="vec_dtype must be float16 or bfloat16"):
            sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, torch.float32, 8, 8, vec_dtype=dt)
    for dt in (torch.float16, torch.bfloat16):      # as a val_dtype they stay refused, with the message of before
        with pytest.raises(TypeError, match="float32 or float64"):
            sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, dt, 8, 8)
    assert sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, torch.float64, 8, 8).vec_dtype is torch.float64       # vec_dtype=None: as before
    for T in (torch.float16, torch.bfloat16):
        plan = sp.SparseAttentionPlan(0, 2, 0, dAp, dAj, torch.float32, 8, 70, vec_dtype=T)
        assert plan.vec_dtype is T and plan.val_dtype is torch.float32
        plan.n_rows = 3     # (the checks below compare against the Python object's sizes; nothing reaches the library)
        info = plan.info()
        assert info["n_slices"] == 0 and info["passes"] == 2 and info["widest_tile"] == 64 and info["main_kernel"] == "attention_half_slice_kernel"
        hc.assert_geometry(info)
        Q, K, V = _OnDevice(torch.ones(3, 8, dtype=T)), _OnDevice(torch.ones(2, 8, dtype=T)), _OnDevice(torch.ones(2, 5, dtype=T))
        out = _OnDevice(torch.zeros(3, 5, dtype=T))
        other = torch.float16 if T is torch.bfloat16 else torch.bfloat16
        for wrong in (torch.float32, other):
            with pytest.raises(TypeError, match="differs from the plan's"):
                plan.execute(_OnDevice(torch.ones(3, 8, dtype=wrong)), K, V, out)
            with pytest.raises(TypeError, match="differs from the plan's"):
                plan.execute(Q, _OnDevice(torch.ones(2, 8, dtype=wrong)), V, out)
            with pytest.raises(TypeError, match="differs from the plan's"):
                plan.execute(Q, K, _OnDevice(torch.ones(2, 5, dtype=wrong)), out)
            with pytest.raises(TypeError, match="differs from the plan's"):
                plan.execute(Q, K, V, _OnDevice(torch.zeros(3, 5, dtype=wrong)))
        for wrong in (T, torch.float64):            # bias and lse are float32
            with pytest.raises(TypeError, match="differs from the plan's"):
                plan.execute(Q, K, V, out, lse=_OnDevice(torch.zeros(3, dtype=wrong)))
            plan.nnz = 4
            with pytest.raises(TypeError, match="differs from the plan's"):
                plan.execute(Q, K, V, out, bias=_OnDevice(torch.zeros(4, dtype=wrong)))
            plan.nnz = 0
        with pytest.raises(ValueError, match="Q and K differ"):
            plan.execute(Q, _OnDevice(torch.ones(2, 7, dtype=T)), V, out)
        with pytest.raises(ValueError, match="above the plan's"):
            plan.execute(Q, K, _OnDevice(torch.ones(2, 71, dtype=T)), None)
        with pytest.raises(ValueError, match="out has 4 columns"):
            plan.execute(Q, K, V, _OnDevice(torch.zeros(3, 4, dtype=T)))
        plan.destroy()
        plan.destroy()
        # the one-shot
        with pytest.raises(RuntimeError, match="device tensors only"):
            sp.sparse_attention_half(3, 2, 3, dAp, dAj, torch.ones(3, 8, dtype=T), K, V)
        with pytest.raises(TypeError, match="Aj must be int32"):
            sp.sparse_attention_half(3, 2, 3, dAp, _OnDevice(Aj.long()), Q, K, V)
        with pytest.raises(ValueError, match="Q and K differ"):
            sp.sparse_attention_half(3, 2, 3, dAp, dAj, Q, _OnDevice(torch.ones(2, 7, dtype=T)), V)
        with pytest.raises(TypeError, match="differs from the plan's"):
            sp.sparse_attention_half(3, 2, 3, dAp, dAj, Q, K, V, out=out, lse=_OnDevice(torch.zeros(3, dtype=T)))
        with pytest.raises(TypeError, match="float32 or float64"):      # the fp32 / fp64 one-shot keeps refusing 16-bit Q
            sp.sparse_attention(3, 2, 3, dAp, dAj, Q, K, V)
    for T in (torch.float32, torch.float64):
        with pytest.raises(TypeError, match="float16 or bfloat16"):
            sp.sparse_attention_half(3, 2, 3, dAp, dAj, _OnDevice(torch.ones(3, 8, dtype=T)), _OnDevice(torch.ones(2, 8, dtype=T)),
                                     _OnDevice(torch.ones(2, 5, dtype=T)))


# ---- the table's own self-checks ---------------------------------------------------------------------------------------
def test_the_table_has_names_of_its_own_and_covers_what_it_says():
    table = hc.table()
    assert 300 < len({c.name for c in table}) == len(table) < 700
    assert (hc.VEC, hc.TILE, hc.SLICE_LEN, hc.STEP, tuple(hc.LANES_PER_SLOT)) == (8, 64, 1024, 64, (1, 2, 4, 8))
    assert max(sum(c.matrix.lens) for c in table) == 30000 + 50
    assert any(c.matrix.n_cols == 1 for c in table)
    assert len(hc.PAIRS) == 11 and max(d for d, _ in hc.PAIRS) <= hc.KF - 4 and max(dv for _, dv in hc.PAIRS) <= hc.KV
    for fam in hc.STRUCTURE_FAMILIES:
        cases = hc.family(fam)
        assert cases, fam
        assert {c.kind for c in cases} == {"const", "masked", "real"}, fam
        assert {c.scale for c in cases if c.kind == "real"} == set(hc.SCALES), fam
        assert len({(c.off, c.vec) for c in cases}) >= 2, fam
    for fam in hc.FAMILIES:
        assert hc.family(fam), fam
    assert {(c.off, c.vec) for c in table} == set(hc.TYPES)
    for vec in hc.VECS:
        mine = [c for c in table if c.vec == vec]
        assert {(c.d, c.dv) for c in mine} >= set(hc.PAIRS), vec
        assert {c.off for c in mine} == set(hc.OFFS) and {c.kind for c in mine} == {"const", "masked", "real"}
        assert {hc.lanes_per_slot(min(c.dv, hc.TILE)) for c in mine} == set(hc.LANES_PER_SLOT)
        assert {-(-c.dv // hc.TILE) for c in mine} == {1, 2, 3}
    assert {c.shift for c in table} >= set(hc.SHIFTS)
    assert {(c.ldq - c.d, c.ldk - c.d, c.ldv - c.dv, c.ldo - c.dv) for c in table} == set(hc.PADS)
    assert any(c.ldv > c.dv and c.ldv % hc.VEC == 0 and c.dv % hc.VEC == 0 for c in table)      # padded rows that stay aligned
    assert {c.want_lse for c in table} == {True, False}
    ragged = [c for c in hc.family("widths")]
    for kind in ("const", "real"):
        assert {c.dv for c in ragged if c.kind == kind} >= set(range(1, 10)) | {63, 64, 65}
    # the tile loop over d: one round, two rounds with a remainder, a long loop on one lane
    rounds = {(-(-c.d // (hc.lanes_per_slot(min(c.dv, hc.TILE)) * hc.VEC)), c.d % (hc.lanes_per_slot(min(c.dv, hc.TILE)) * hc.VEC) != 0) for c in table}
    assert {(1, True), (1, False), (2, False), (2, True)} <= rounds and max(r for r, _ in rounds) >= 13
    seq = [c for c in hc.hub_sequence() if c.off == "i32"]
    assert seq[0].kind == "const" and any(c.kind == "real" for c in seq[1:])        # other operands behind the first execute
    assert [c.dv for c in seq].index(3) > [c.dv for c in seq].index(129)            # a narrow dv after a wide one
    assert len(hc.slices(hc.structures("hub")[0].lens)) >= 30
    pairs = hc.fp32_pairs()
    assert pairs and all(c.dv <= 4 and c.kind == "real" for c in pairs) and {c.vec for c in pairs} == set(hc.VECS)


def test_the_operands_hold_only_values_of_their_type_and_the_rows_do_not_spread():
    for c in hc.table():
        Q, K, V, bias = hc.operands(c)
        for a in (Q, K, V):
            assert a.dtype == np.float32 and np.array_equal(hc.from_bits(hc.to_bits(a, c.vec), c.vec).reshape(a.shape), a), c.name
        assert bias is None or bias.dtype == np.float32
        assert np.abs(Q).max(initial=0.0) < hc.F16_MAX
        if c.kind == "real":
            ex = hc.expected(c)
            assert ex["spread"].max() <= 20.0 and np.all(hc.o_bound(c) > 0), c.name
            assert np.abs(ex["want"]).max(initial=0.0) <= 1.0       # a convex combination of values in [-1, 1] (a draw may round to 1)


def serial_emulation(c):
    """The contract, the plain way: fp32 on the widened values (numpy's float32 operations round once each), every row's
    entries in their stored order, one narrowing of acc / l at the end.  (O bits, lse)."""
    m = c.matrix
    Ap, Aj = hc.csr(m, c.off)
    Q, K, V, bias = hc.operands(c)
    n_rows, rows = len(m.lens), hc.rows_of(m)
    f = np.float32
    q, k = Q[:, c.c0:c.c0 + c.d][rows], K[:, c.c0:c.c0 + c.d][Aj]
    dot = np.zeros(len(Aj), dtype=f)
    for j in range(c.d):
        dot = dot + q[:, j] * k[:, j]          # (the product of two 16-bit values is exact in fp32: one rounding, as an fma)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = f(c.scale) * dot
        if bias is not None:
            v = v + bias
        top = np.full(n_rows, -np.inf, dtype=f)
        np.maximum.at(top, rows, v)
        live = ~np.isneginf(v)
        diff = np.where(live, v - top[rows], f(0))
        e = np.where(live, np.where(diff == 0, f(1), np.exp(diff, dtype=f)), f(0)).astype(f)
        l = np.zeros(n_rows, dtype=f)
        np.add.at(l, rows, e)
        acc = np.zeros((n_rows, c.dv), dtype=f)
        np.add.at(acc, rows, e[:, None] * np.where(live[:, None], V[:, c.cv0:c.cv0 + c.dv][Aj], f(0)))
        assert e.dtype == f and l.dtype == f and acc.dtype == f and v.dtype == f
        O = np.where(l[:, None] > 0, acc / np.where(l > 0, l, f(1))[:, None], f(0)).astype(f)
        lse = np.where(l > 0, top + np.log(np.where(l > 0, l, f(1)), dtype=f), f(-np.inf)).astype(f)
    return hc.to_bits(O, c.vec).reshape(n_rows, c.dv), lse


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_a_serial_emulation_of_the_contract_meets_every_check_of_the_table(family):
    ratios = []
    for c in hc.family(family):
        O, lse = serial_emulation(c)
        hc.check(c, O, lse if c.want_lse else None, ratios)
    if any(c.kind == "real" for c in hc.family(family)):
        assert ratios and max(ratios) < 1


def test_a_wrong_value_is_caught():
    m = hc.structures("pow2")[0]
    for vec in hc.VECS:
        c = hc._case(m, "i32", vec, "masked", 0, 1.0, 3, 5)
        O, lse = serial_emulation(c)
        hc.check(c, O, lse)
        ex = hc.expected(c)
        r = int(np.nonzero(ex["live"] > 2)[0][0])
        bad = O.copy()
        bad[r, 0] += 1                      # the next 16-bit value
        with pytest.raises(AssertionError):
            hc.check(c, bad, lse)
        dead = np.nonzero(ex["live"] == 0)[0]
        assert dead.size
        bad = O.copy()
        bad[dead[0], 1] = 0x8000            # a row without a live entry must be +0, not -0
        with pytest.raises(AssertionError):
            hc.check(c, bad, lse)
        # the fp64 quotient rounded straight to 16 bits is NOT the expectation where it differs from the fp32 one
        c = hc._case(hc.structures("ragged")[0], "i64", vec, "real", 1, 0.125, 17, 9)
        O, lse = serial_emulation(c)
        hc.check(c, O, lse)
        bad = hc.from_bits(O, vec).reshape(O.shape).copy()
        r, j = np.unravel_index(np.argmax(hc.o_bound(c)), O.shape)
        bad[r, j] += np.float32(4 * hc.o_bound(c)[r, j] + 2 * hc.U16[vec])
        with pytest.raises(AssertionError):
            hc.check(c, hc.to_bits(bad, vec).reshape(O.shape), lse)
