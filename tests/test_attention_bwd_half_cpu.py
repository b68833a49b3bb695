"""The fused attention backward with 16-bit operands without a device: the exported names and header lines, get_types, every
argument refusal of mi355_spmv_attention_bwd_create_half and of the four 16-bit one-shots on dummy pointers (each comes
before any device call and names its argument), the Python layer's dtype refusals, the pairing refusals of
sp.sparse_attention_function, the self-checks of tests/attention_bwd_half_cases.py against the kernel's constants, an exact
case that is exact with a mutated result that is caught, and a serial fp32 emulation of one real case that shows the derived
bound is attainable and not vacuous."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import attention_bwd_half_cases as bh
import sim_runner as sr

EINVAL, ENOTSUP = 1, 2
F16, BF16 = 4, 5


@pytest.fixture(scope="module")
def L(sp):
    return sp.capi.lib()


def last_error(L):
    return L.mi355_spmv_last_error().decode()


def test_exported_names_and_header_lines(sp, L):
    names = ["mi355_spmv_attention_bwd_create_half", "mi355_spmv_attention_bwd_get_types"]
    names += ["mi355_spmv_attention_bwd_half_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f16", "bf16")]
    header = open(sr.ROOT + "/include/mi355_spmv.h").read()
    assert "#define MI355_SPMV_HAS_ATTENTION_BACKWARD_HALF 1" in header
    for n in names:
        assert n in sp.capi.EXPORTS and hasattr(L, n), n
        assert "int %s(" % n in header, n
    assert "the 16-bit object has no backward" not in header
    assert issubclass(sp.SparseAttentionBackwardHalfPlan, sp.SparseAttentionBackwardPlan)
    assert list(inspect.signature(sp.SparseAttentionBackwardHalfPlan.__init__).parameters) == [
        "self", "n_rows", "n_cols", "nnz", "Ap", "Aj", "vec_dtype", "d_max", "dv_max", "stream"]
    for n in ("execute", "set_scale", "info", "destroy"):
        assert getattr(sp.SparseAttentionBackwardHalfPlan, n) is getattr(sp.SparseAttentionBackwardPlan, n)
    assert list(inspect.signature(sp.sparse_attention_backward_half).parameters) == list(inspect.signature(sp.sparse_attention_backward).parameters)
    # the info struct is the fp32 object's, unchanged
    assert C.sizeof(sp.capi.AttentionBackwardInfo) == 8 * 4 + 6 * 4 + 6 * 8 + 64


def test_get_types_refuses_null_arguments(L):
    a, b = C.c_int(), C.c_int()
    assert L.mi355_spmv_attention_bwd_get_types(None, C.byref(a), C.byref(b)) == EINVAL and "null argument" in last_error(L)


def test_the_table_agrees_with_the_kernels_constants():
    unit, cut, common, cols = sr.source("attention_bwd.hip"), sr.source("slice_cut.hpp"), sr.source("common.hpp"), sr.source("half_cols.hpp")
    assert sr.kernel_constant(unit, "kAttentionBwdSlice") == sr.kernel_constant(cut, "kSliceLen") == bh.SLICE_LEN
    assert sr.kernel_constant(unit, "kAttentionBwdGroupsMax") == sr.kernel_constant(cut, "kSliceGroupsMax") == max(bh.LANES_PER_SLOT)
    assert sr.kernel_constant(cols, "kHalfV") == bh.VEC and bh.VEC * max(bh.LANES_PER_SLOT) == bh.TILE
    assert sr.kernel_constant(common, "kWave") == bh.STEP
    half = sr.source("attention_bwd_half_kernel.hpp")
    assert '#include "attention_bwd_slice_walk.inc"' in half and '#include "attention_bwd_slice_walk.inc"' in unit


def test_the_table_covers_what_it_says():
    table = bh.table()
    names = [c.name for c in table]
    assert len(set(names)) == len(names)
    assert {(c.off, c.vec) for c in table} == set(bh.TYPES)
    for vec in bh.VECS:
        cs = [c for c in table if c.vec == vec]
        assert {c.side for c in cs} == {"A", "T"} and {c.off for c in cs} == {"i32", "i64"}
        assert {c.kind for c in cs} == {"exact", "masked", "single", "real"}
        for widths in ({c.d for c in cs}, {c.dv for c in cs}):
            assert {1, bh.TILE, 65, 129} <= widths and any(1 < w < bh.VEC for w in widths)      # (below a lane)
            assert {bh.lanes_per_slot(w) for w in widths} == set(bh.LANES_PER_SLOT)
            assert {-(-w // bh.TILE) for w in widths} == {1, 2, 3}
        assert any((c.d, c.dv) == (100, 3) for c in cs) and any((c.d, c.dv) == (3, 100) for c in cs)
        assert any(c.want_dbias for c in cs) and any(not c.want_dbias and c.need[0] for c in cs)
        assert any(c.shift for c in cs) and any(c.pad == bh.PADS[-1] for c in cs)
        assert max(c.d for c in cs) <= bh.D_MAX and max(c.dv for c in cs) <= bh.DV_MAX
    ragged = [c for c in bh.family("widths")]
    assert set(bh.RAGGED) <= {c.d for c in ragged} and set(bh.RAGGED) <= {c.dv for c in ragged}
    # exact variant 2 (a score that is -inf on its own) is bf16's alone
    assert {c.vec for c in table if c.kind == "exact" and c.variant == 2} == {"bf16"}
    for fam in bh.STRUCTURE_FAMILIES:
        assert {c.side for c in bh.family(fam)} == {"A", "T"}, fam
    assert all(p[0] % 8 == 0 and p[1] % 8 == 0 for p in bh.ALIGN_PAIRS) and all(x % 8 == 0 for x in bh.PADS[-1])


def test_the_operands_are_16_bit_values_and_nan_rows_hold_the_types_nan_bits():
    c = next(c for c in bh.family("ragged") + bh.family("hub") if c.kind == "masked" and np.isnan(bh.operands(c)["K"]).any())
    ops = bh.operands(c)
    for name in bh.ORDER:
        a = ops[name]
        back = bh.from_bits(bh.to_bits(a, c.vec), c.vec).reshape(a.shape)
        assert np.array_equal(back, a, equal_nan=True), name
    nan = np.isnan(ops["K"])
    assert nan.any() and np.all(bh.to_bits(ops["K"], c.vec).reshape(nan.shape)[nan] == bh.NAN_BITS[c.vec])
    assert ops["lse"].dtype == np.float32 and ops["bias"].dtype == np.float32


def test_an_exact_case_is_exact_and_a_mutated_result_is_caught():
    for vec in bh.VECS:
        c = next(c for c in bh.family("hub") if c.kind == "masked" and c.vec == vec and c.want_dbias)
        ex = bh.expected(c)
        good = [bh.to_bits(ex[n].astype(np.float32), vec).reshape(ex[n].shape) for n in ("dQ", "dK", "dV")] + [ex["dbias"].astype(np.float32)]
        bh.check(c, *good)
        line = np.nonzero(ex["live_cols"])[0][0]
        bad = [g.copy() for g in good]
        bad[2][line, 0] = bh.to_bits(np.float32(ex["dV"][line, 0] + 1), vec).reshape(-1)[0]
        with pytest.raises(AssertionError):
            bh.check(c, *bad)
        # a value narrowed TWICE (through the other 16-bit type first) or a line without a live entry as -0 is caught too
        none = np.nonzero(ex["live_cols"] == 0)[0]
        if none.size:
            bad = [g.copy() for g in good]
            bad[1][none[0], 0] = 0x8000
            with pytest.raises(AssertionError):
                bh.check(c, *bad)


def test_a_serial_fp32_emulation_of_a_real_case_lies_inside_the_bound_and_uses_it():
    """The formulas in plain float32, one entry after the other, every line summed serially and narrowed once: inside the
    derived bound (it is attainable), and its largest error / bound is not tiny (the bound is not vacuous)."""
    c = next(c for c in bh.family("ragged") if c.kind == "real" and c.variant == 1 and c.side == "A" and c.d <= 64 and c.dv <= 64)
    n_rows, n_cols, Ap, Aj, _ = bh.csr(c)
    ops = bh.operands(c)
    f = np.float32
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))

    def dot(a, b):
        s = np.zeros(a.shape[0], dtype=f)
        for j in range(a.shape[1]):
            s = s + a[:, j] * b[:, j]       # (float32 throughout)
        return s

    v = f(c.scale) * dot(ops["Q"][rows], ops["K"][Aj]) + ops["bias"]
    p = np.exp(v - ops["lse"][rows]).astype(f)
    ds = p * (dot(ops["dO"][rows], ops["V"][Aj]) - dot(ops["dO"], ops["O"])[rows])
    assert ds.dtype == f

    def lines(index, n, coef, x):
        out = np.zeros((n, x.shape[1]), dtype=f)
        np.add.at(out, index, (coef[:, None] * x).astype(f))       # unbuffered: one entry after the other, in float32
        return bh.to_bits(out, c.vec).reshape(out.shape)

    got = (lines(rows, n_rows, f(c.scale) * ds, ops["K"][Aj]), lines(Aj, n_cols, f(c.scale) * ds, ops["Q"][rows]), lines(Aj, n_cols, p, ops["dO"][rows]),
           ds if c.want_dbias else None)
    ratios = []
    bh.check(c, *got, ratios=ratios)
    print("%s: serial fp32 emulation, largest error / bound %.3f" % (c.name, max(ratios)))
    assert 0.05 <= max(ratios) <= 1.0


# ---- refusals: dummy pointers, no device call ------------------------------------------------------------------------------
def create_half(L, off_type=0, vec_type=BF16, n_rows=4, n_cols=4, nnz=8, Ap=0x1000, Aj=0x2000, d_max=8, dv_max=8, out=True):
    h = C.c_void_p()
    st = L.mi355_spmv_attention_bwd_create_half(C.byref(h) if out else None, off_type, vec_type, n_rows, n_cols, nnz, C.c_void_p(Ap), C.c_void_p(Aj),
                                                d_max, dv_max, None)
    assert not h
    return st, last_error(L)


@pytest.mark.parametrize("kw,status,word", [
    (dict(out=False), EINVAL, "out"), (dict(vec_type=0), EINVAL, "vec_type"), (dict(vec_type=1), EINVAL, "vec_type"), (dict(vec_type=2), EINVAL, "vec_type"),
    (dict(vec_type=99), EINVAL, "vec_type"), (dict(off_type=7), EINVAL, "off_type"), (dict(d_max=0), EINVAL, "d_max"), (dict(dv_max=0), EINVAL, "dv_max"),
    (dict(n_rows=-1), EINVAL, "n_rows"), (dict(n_cols=-1), EINVAL, "n_cols"), (dict(nnz=-1), EINVAL, "nnz"), (dict(Ap=0), EINVAL, "Ap"),
    (dict(Aj=0), EINVAL, "Aj"), (dict(off_type=1, nnz=2 ** 32), ENOTSUP, "2^32")])
def test_create_half_refusals(L, kw, status, word):
    for vec_type in (F16, BF16):
        st, text = create_half(L, **dict(dict(vec_type=vec_type), **kw))
        assert st == status and word in text, (st, text)


def test_the_fp32_create_still_refuses_16_bit_value_types_and_points_to_create_half(L):
    for val_type in (F16, BF16):
        h = C.c_void_p()
        st = L.mi355_spmv_attention_bwd_create(C.byref(h), 0, val_type, 4, 4, 8, C.c_void_p(0x1000), C.c_void_p(0x2000), 8, 8, None)
        assert st == EINVAL and not h and "val_type" in last_error(L) and "create_half" in last_error(L)


ONE_SHOT = dict(n_rows=4, n_cols=4, nnz=8, Ap=0x1000, Aj=0x2000, d=8, dv=6, Q=0x3000, ldq=8, K=0x4000, ldk=8, V=0x5000, ldv=6, bias=0, scale=1.0,
                O=0x6000, ldo=6, dO=0x7000, lddo=6, lse=0x8000, dQ=0x9000, lddq=8, dK=0xa000, lddk=8, dV=0xb000, lddv=6, dbias=0)


def one_shot(L, name, **kw):
    a = dict(ONE_SHOT, **kw)
    p = lambda k: C.c_void_p(a[k]) if a[k] else None
    st = getattr(L, name)(a["n_rows"], a["n_cols"], a["nnz"], p("Ap"), p("Aj"), a["d"], a["dv"], p("Q"), a["ldq"], p("K"), a["ldk"], p("V"), a["ldv"],
                          p("bias"), a["scale"], p("O"), a["ldo"], p("dO"), a["lddo"], p("lse"), p("dQ"), a["lddq"], p("dK"), a["lddk"], p("dV"),
                          a["lddv"], p("dbias"), None)
    return st, last_error(L)


@pytest.mark.parametrize("kw,word", [
    (dict(d=0), "d ="), (dict(dv=0), "dv ="), (dict(ldq=7), "ldq"), (dict(ldk=7), "ldk"), (dict(ldv=5), "ldv"), (dict(ldo=5), "ldo"),
    (dict(lddo=5), "lddo"), (dict(lddq=7), "lddq"), (dict(lddk=7), "lddk"), (dict(lddv=5), "lddv"), (dict(Q=0), "Q"), (dict(K=0), "K"),
    (dict(V=0), "V"), (dict(O=0), "null O"), (dict(dO=0), "dO"), (dict(lse=0), "lse"), (dict(dQ=0, dK=0, dV=0), "all null"),
    (dict(dQ=0, dbias=0xc000), "dbias without dQ"), (dict(Ap=0), "Ap"), (dict(Aj=0), "Aj"), (dict(n_rows=-1), "n_rows")])
def test_one_shot_refusals_on_every_type(L, kw, word):
    for o in ("i32", "i64"):
        for v in ("f16", "bf16"):
            st, text = one_shot(L, "mi355_spmv_attention_bwd_half_%s_%s" % (o, v), **kw)
            assert st == EINVAL and word in text, (o, v, st, text)


def test_the_python_layer_names_the_argument_of_a_wrong_dtype(sp):
    import torch
    T = torch.bfloat16
    mk = lambda rows, cols, dtype=T: torch.zeros(rows, cols, dtype=dtype)
    good = dict(Q=mk(3, 4), K=mk(2, 4), V=mk(2, 5), O=mk(3, 5), dO=mk(3, 5), dQ=None, dK=None, dV=None)
    for name in good:
        for wrong in (torch.float16, torch.float32):
            a = dict(good)
            a[name] = torch.zeros_like(good[name], dtype=wrong) if good[name] is not None else mk(*{"dQ": (3, 4), "dK": (2, 4), "dV": (2, 5)}[name], wrong)
            with pytest.raises(TypeError, match=r"\b%s is" % name):
                sp.capi._attention_backward_operands(3, 2, 6, torch.float32, a["Q"], a["K"], a["V"], a["O"], a["dO"], torch.zeros(3), None, a["dQ"],
                                                     a["dK"], a["dV"], None, (True, True, True), vec_dtype=T)
    with pytest.raises(TypeError):
        sp.SparseAttentionBackwardHalfPlan(1, 1, 0, torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.float32, 4, 4)
    with pytest.raises(RuntimeError):       # a device is needed: the CPU tensors are refused before the library is called
        sp.SparseAttentionBackwardHalfPlan(1, 1, 0, torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), T, 4, 4)


def test_sparse_attention_function_pairs_plans_of_one_vector_type(sp):
    import torch
    plan = lambda val, vec: types.SimpleNamespace(n_rows=3, n_cols=2, nnz=4, val_dtype=val, vec_dtype=vec)
    f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
    for fwd, bwd in ((plan(f32, f16), plan(f32, bf16)), (plan(f32, f32), plan(f32, bf16)), (plan(f32, f16), plan(f32, f32))):
        with pytest.raises(TypeError):
            sp.sparse_attention_function(fwd, bwd)
    for vec in (f32, f16, bf16):
        assert callable(sp.sparse_attention_function(plan(f32, vec), plan(f32, vec)))
    with pytest.raises(ValueError):
        sp.sparse_attention_function(plan(f32, bf16), types.SimpleNamespace(n_rows=3, n_cols=2, nnz=5, val_dtype=f32, vec_dtype=bf16))
