"""The fused attention backward without a device: the exported names and signatures, the info struct, every argument
refusal of mi355_spmv_attention_bwd_* on dummy pointers (each comes before any device call and names its argument), and the
self-checks of tests/attention_bwd_cases.py against the kernel's constants."""
import ctypes as C
import inspect

import numpy as np
import pytest

import attention_bwd_cases as bc
import sim_runner as sr

EINVAL, ENOTSUP = 1, 2


@pytest.fixture(scope="module")
def L(sp):
    return sp.capi.lib()


def last_error(L):
    return L.mi355_spmv_last_error().decode()


def test_exported_names_and_signatures(sp, L):
    names = ["mi355_spmv_attention_bwd_" + n for n in ("create", "set_scale", "execute", "get_info", "destroy")]
    names += ["mi355_spmv_attention_bwd_%s_%s" % (o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
    for n in names:
        assert n in sp.capi.EXPORTS and hasattr(L, n), n
    header = open(sr.ROOT + "/include/mi355_spmv.h").read()
    assert "#define MI355_SPMV_HAS_ATTENTION_BACKWARD 1" in header
    for n in names:
        assert "int %s(" % n in header, n
    assert list(inspect.signature(sp.SparseAttentionBackwardPlan.__init__).parameters) == [
        "self", "n_rows", "n_cols", "nnz", "Ap", "Aj", "dtype", "d_max", "dv_max", "stream"]
    assert list(inspect.signature(sp.SparseAttentionBackwardPlan.execute).parameters) == [
        "self", "Q", "K", "V", "O", "dO", "lse", "bias", "dQ", "dK", "dV", "dbias", "need", "stream"]
    for n in ("set_scale", "info", "destroy"):
        assert callable(getattr(sp.SparseAttentionBackwardPlan, n))
    assert callable(sp.sparse_attention_backward) and callable(sp.sparse_attention_function)
    assert sp.autograd.sparse_attention_function is sp.sparse_attention_function


def test_info_struct_matches_the_header(sp):
    fields = [n for n, _ in sp.capi.AttentionBackwardInfo._fields_]
    header = open(sr.ROOT + "/include/mi355_spmv.h").read()
    body = header[header.index("typedef struct mi355_spmv_attention_bwd_info {"):header.index("} mi355_spmv_attention_bwd_info;")]
    at = [body.index(n) for n in fields]
    assert at == sorted(at), "the fields are declared in the order capi.py reads them"
    assert C.sizeof(sp.capi.AttentionBackwardInfo) == 8 * 4 + 6 * 4 + 6 * 8 + 64


def test_the_table_agrees_with_the_kernels_constants():
    unit, cut, common = sr.source("attention_bwd.hip"), sr.source("slice_cut.hpp"), sr.source("common.hpp")
    assert sr.kernel_constant(unit, "kAttentionBwdSlice") == sr.kernel_constant(cut, "kSliceLen") == bc.SLICE_LEN
    assert sr.kernel_constant(unit, "kAttentionBwdGroupsMax") == sr.kernel_constant(cut, "kSliceGroupsMax") == max(bc.LANES_PER_SLOT)
    assert sr.kernel_constant(common, "kWave") == bc.STEP
    assert sr.kernel_constant(common, "kBlock") % bc.STEP == 0


def test_the_table_covers_what_it_says():
    table = bc.table()
    names = [c.name for c in table]
    assert len(set(names)) == len(names)
    for val in ("f32", "f64"):
        cs = [c for c in table if c.val == val]
        assert {c.side for c in cs} == {"A", "T"} and {c.off for c in cs} == {"i32", "i64"}
        assert {c.kind for c in cs} == {"exact", "masked", "single", "real"}
        tile = bc.TILE[val]
        for widths in ({c.d for c in cs}, {c.dv for c in cs}):
            assert 1 in widths and tile in widths and any(w > 2 * tile for w in widths) and any(tile < w <= 2 * tile for w in widths)
            assert {bc.lanes_per_slot(w, val) for w in widths} == set(bc.LANES_PER_SLOT)
        assert any(c.d > c.dv for c in cs) and any(c.d < c.dv for c in cs)
        assert max(c.d for c in cs) <= bc.D_MAX[val] and max(c.dv for c in cs) <= bc.DV_MAX[val]
    for fam in bc.STRUCTURE_FAMILIES:
        assert {c.side for c in bc.family(fam)} == {"A", "T"}, fam
    # the transpose of the table is the library's: inside a column, ascending source slot
    Ap, Aj = np.array([0, 2, 2, 5], dtype=np.int32), np.array([1, 0, 1, 1, 0], dtype=np.int32)
    Apt, Ajt, perm = bc.transpose(3, 2, Ap, Aj)
    assert Apt.tolist() == [0, 2, 5] and Ajt.tolist() == [0, 2, 0, 2, 2] and perm.tolist() == [1, 4, 0, 2, 3]


def test_an_exact_case_is_exact_and_a_mutated_result_is_caught():
    c = next(c for c in bc.family("ragged") if c.kind == "masked" and c.val == "f32")
    ex = bc.expected(c)
    T = bc.NP[c.val]
    good = [ex[n].astype(T) for n in ("dQ", "dK", "dV", "dbias")]
    if not c.want_dbias:
        good[3] = None
    bc.check(c, *good)
    bad = [None if g is None else g.copy() for g in good]
    bad[2][np.nonzero(ex["live_cols"])[0][0], 0] += 1
    with pytest.raises(AssertionError):
        bc.check(c, *bad)


# ---- refusals: dummy pointers, no device call ------------------------------------------------------------------------------
def create(L, off_type=0, val_type=0, n_rows=4, n_cols=4, nnz=8, Ap=0x1000, Aj=0x2000, d_max=8, dv_max=8, out=True):
    h = C.c_void_p()
    st = L.mi355_spmv_attention_bwd_create(C.byref(h) if out else None, off_type, val_type, n_rows, n_cols, nnz, C.c_void_p(Ap), C.c_void_p(Aj),
                                           d_max, dv_max, None)
    assert not h
    return st, last_error(L)


@pytest.mark.parametrize("kw,status,word", [
    (dict(out=False), EINVAL, "out"), (dict(off_type=7), EINVAL, "off_type"), (dict(val_type=2), ENOTSUP, "val_type"),
    (dict(val_type=3), EINVAL, "val_type"), (dict(val_type=4), EINVAL, "val_type"), (dict(val_type=5), EINVAL, "val_type"),
    (dict(val_type=99), EINVAL, "val_type"), (dict(d_max=0), EINVAL, "d_max"), (dict(dv_max=0), EINVAL, "dv_max"),
    (dict(n_rows=-1), EINVAL, "n_rows"), (dict(n_cols=-1), EINVAL, "n_cols"), (dict(nnz=-1), EINVAL, "nnz"), (dict(Ap=0), EINVAL, "Ap"),
    (dict(Aj=0), EINVAL, "Aj"), (dict(off_type=1, nnz=2 ** 32), ENOTSUP, "2^32")])
def test_create_refusals(L, kw, status, word):
    st, text = create(L, **kw)
    assert st == status and word in text, (st, text)


ONE_SHOT = dict(n_rows=4, n_cols=4, nnz=8, Ap=0x1000, Aj=0x2000, d=8, dv=6, Q=0x3000, ldq=8, K=0x4000, ldk=8, V=0x5000, ldv=6, bias=0, scale=1.0,
                O=0x6000, ldo=6, dO=0x7000, lddo=6, lse=0x8000, dQ=0x9000, lddq=8, dK=0xa000, lddk=8, dV=0xb000, lddv=6, dbias=0)


def one_shot(L, name="mi355_spmv_attention_bwd_i32_f32", **kw):
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
        for v in ("f32", "f64"):
            st, text = one_shot(L, "mi355_spmv_attention_bwd_%s_%s" % (o, v), **kw)
            assert st == EINVAL and word in text, (o, v, st, text)


def test_null_objects_are_refused(sp, L):
    assert L.mi355_spmv_attention_bwd_set_scale(None, 1.0) == EINVAL and "null object" in last_error(L)
    assert L.mi355_spmv_attention_bwd_execute(None, 1, 1, None, 1, None, 1, None, 1, None, None, 1, None, 1, None, None, 1, None, 1, None, 1, None,
                                              None) == EINVAL and "null object" in last_error(L)
    info = sp.capi.AttentionBackwardInfo()
    assert L.mi355_spmv_attention_bwd_get_info(None, C.byref(info)) == EINVAL
    assert L.mi355_spmv_attention_bwd_destroy(None) == 0


def test_the_python_layer_refuses_before_the_library(sp):
    import torch
    with pytest.raises(RuntimeError):
        sp.SparseAttentionBackwardPlan(1, 1, 0, torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.float32, 4, 4)
