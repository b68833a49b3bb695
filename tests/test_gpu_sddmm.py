"""SDDMM on the GPU (sp.SddmmPlan / sp.sddmm, csrc/sddmm.hip): the table of tests/sddmm_cases.py — the cases that
tests/test_sddmm_sim_cpu.py executes on the host — on the device, each out against numpy's fp64 value within the
dot-product bound of that module (integer data bit for bit); padding columns of U and V hold NaN, out starts as NaN
where beta = 0, and a canary behind out[nnz - 1] must survive.  Then what only a device shows: two executes give the
same bits, a side stream, one graph capture replayed on new U / V, the one-shots, a padded view, and the adjoint
identity that makes SDDMM the gradient of sp.spmm."""
import ctypes as C

import numpy as np
import pytest
import torch

import sddmm_cases as sc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TAIL = 5            # canary elements behind out


def on_device(flat, shift, tail=0, fill=0.0):
    """1-D device copy of `flat` whose base lies `shift` elements past a 16-byte boundary, `tail` elements of `fill`
    behind it (returns the view of flat.size + tail elements; an empty one has no base)."""
    t = torch.from_numpy(np.ascontiguousarray(flat))
    es = t.element_size()
    buf = torch.full((t.numel() + tail + 16 // es + 1,), fill, dtype=t.dtype, device=DEV)
    base = ((16 - buf.data_ptr() % 16) % 16) // es + shift
    v = buf[base:base + t.numel() + tail]
    v[:t.numel()].copy_(t)
    assert v.numel() == 0 or v.data_ptr() % 16 == shift * es
    return v


def execute_case(sp, plan, c, dAx):
    """One case of the table on `plan`; returns out as numpy (the canary checked)."""
    Ap, Aj, Ax, O0, U, V = sc.arrays(c.matrix, c.off, c.val, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    uh = np.full((n_rows, c.ldu), np.nan, dtype=U.dtype)
    uh[:, :c.k] = U[:, c.c0:c.c0 + c.k]
    vh = np.full((n_cols, c.ldv), np.nan, dtype=V.dtype)
    vh[:, :c.k] = V[:, c.c0:c.c0 + c.k]
    uf, vf = on_device(uh.ravel(), c.shift[3]), on_device(vh.ravel(), c.shift[4])
    of = on_device(O0 if c.beta != 0.0 else np.full(nnz, np.nan, dtype=O0.dtype), c.shift[5], TAIL, sc.CANARY)
    plan.set_alpha_beta(c.alpha, c.beta)
    got = plan.execute(dAx if c.valued else None, torch.as_strided(uf, (n_rows, c.k), (c.ldu, 1)),
                       torch.as_strided(vf, (n_cols, c.k), (c.ldv, 1)), of[:nnz])
    assert nnz == 0 or got.data_ptr() == of.data_ptr()
    oh = of.cpu().numpy()       # (the copy synchronises)
    assert np.all(oh[nnz:] == sc.NP[c.val](sc.CANARY)), "%s: the canary behind out was written" % c.name
    return oh[:nnz]


@pytest.fixture(scope="module")
def table(sp):
    """Every case of the table, run once: {case name: out}.  Plans are made per (structure, types, matrix offsets) and
    reused over k, alpha / beta, leading dimensions and the offsets of U, V and out.  No case is skipped."""
    results = {}
    key, plan, dAx = None, None, None
    try:
        for c in sorted(sc.table(), key=sc.plan_key):
            if sc.plan_key(c) != key:
                if plan is not None:
                    plan.destroy()
                    plan = None
                key = sc.plan_key(c)
                Ap, Aj, Ax = sc.arrays(c.matrix, c.off, c.val, c.integer)[:3]
                dAp, dAj, dAx = on_device(Ap, c.shift[0]), on_device(Aj, c.shift[1]), on_device(Ax, c.shift[2])
                plan = sp.SddmmPlan(len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1]), dAp, dAj, dAx.dtype)
                sc.assert_geometry(plan.info())
                assert plan.info()["n_slices"] == -(-(len(c.matrix.lens) + int(Ap[-1])) // sc.SLICE_LEN)
            results[c.name] = execute_case(sp, plan, c, dAx)
    finally:
        if plan is not None:
            plan.destroy()
    return results


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_table(table, family):
    cases = sc.family(family)
    assert cases
    for c in cases:
        sc.check(c, table[c.name])


def test_alignment_changes_no_bit(table):
    for a, b in sc.alignment_pairs():
        assert np.array_equal(table[a.name].view(np.uint8), table[b.name].view(np.uint8)), a.name


def test_equal_rows_of_u_and_v_give_equal_bits_wherever_the_entry_lies(table):
    for a, b, ia, ib in sc.position_checks():
        oa, ob = table[a.name], table[b.name]
        assert ia.size > 100
        bad = np.nonzero(oa[ia].view(np.uint8).reshape(ia.size, -1) != ob[ib].view(np.uint8).reshape(ib.size, -1))[0]
        assert bad.size == 0, "%s vs %s: entries %s / %s differ" % (a.name, b.name, ia[bad[:8]], ib[bad[:8]])


# ---- what only a device shows ---------------------------------------------------------------------------------------------
def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ragged_real(off="i32", val="f32", k=13):
    """The ragged structure with real data as a case of its own (valued, alpha / beta = 2.5 / 0, no padding)."""
    return sc._case(sc.ragged_structure(), off, val, k, (2.5, 0.0), (0, 0), sc.ALIGNED, True, "-device")


def test_repeat_side_stream_and_graph(sp):
    c = ragged_real()
    Ap, Aj, Ax, O0, U, V = sc.arrays(c.matrix, c.off, c.val, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    plan = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32)
    plan.set_alpha_beta(c.alpha, c.beta)
    dU, dV = d(U[:, c.c0:c.c0 + c.k]), d(V[:, c.c0:c.c0 + c.k])
    out = torch.full((nnz,), float("nan"), device=DEV)
    plan.execute(dAx, dU, dV, out)
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    sc.check(c, first)
    out.fill_(float("nan"))
    plan.execute(dAx, dU, dV, out)              # two executes: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(first.view(np.uint32), out.cpu().numpy().view(np.uint32))
    # out=None makes the result
    made = plan.execute(dAx, dU, dV)
    assert made.shape == (nnz,) and np.array_equal(first.view(np.uint32), made.cpu().numpy().view(np.uint32))
    # a side stream
    s = torch.cuda.Stream()
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        plan.execute(dAx, dU, dV, out)
    s.synchronize()
    assert np.array_equal(first.view(np.uint32), out.cpu().numpy().view(np.uint32))
    # one capture, replayed on new U / V: the case of other columns of the full operands
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute(dAx, dU, dV, out)
    c2 = c._replace(c0=c.c0 + 40, name=c.name + "-replayed")
    dU.copy_(d(U[:, c2.c0:c2.c0 + c.k]))
    dV.copy_(d(V[:, c2.c0:c2.c0 + c.k]))
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    sc.check(c2, got)
    assert not np.array_equal(got, first)
    del g
    plan.destroy()


@pytest.mark.parametrize("off,val", [("i32", "f32"), ("i32", "f64"), ("i64", "f32"), ("i64", "f64")])
def test_one_shots_equal_the_plan(sp, off, val):
    c = ragged_real(off, val, 9)
    Ap, Aj, Ax, O0, U, V = sc.arrays(c.matrix, c.off, c.val, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    dU, dV = d(U[:, c.c0:c.c0 + c.k]), d(V[:, c.c0:c.c0 + c.k])
    plan = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, dAx.dtype)
    for ax in (dAx, None):
        want = plan.execute(ax, dU, dV)
        got = sp.sddmm(n_rows, n_cols, nnz, dAp, dAj, ax, dU, dV)
        torch.cuda.synchronize()                    # (neither synchronises)
        assert torch.equal(got, want)
        sc.check(c._replace(alpha=1.0, valued=ax is not None), got.cpu().numpy())
        # the C entry point itself, into a given out
        out = torch.full((nnz,), float("nan"), dtype=dAx.dtype, device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        f = getattr(sp.capi.lib(), "mi355_spmv_sddmm_%s_%s" % (off, val))
        assert f(n_rows, n_cols, nnz, ptr(dAp), ptr(dAj), ptr(ax), ptr(dU), c.k, ptr(dV), c.k, ptr(out), c.k,
                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    plan.destroy()


def test_a_padded_view_and_k_below_the_columns_held(sp):
    c = ragged_real(k=11)
    Ap, Aj, Ax, O0, U, V = sc.arrays(c.matrix, c.off, c.val, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    plan = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32)
    plan.set_alpha_beta(c.alpha, c.beta)
    dUfull, dVfull = d(U), d(V)                                # KF columns each
    uview = dUfull[:, c.c0:c.c0 + c.k]                         # non-contiguous: stride(0) = KF
    assert not uview.is_contiguous() and uview.stride() == (sc.KF, 1)
    dense = plan.execute(dAx, uview.contiguous(), dVfull[:, c.c0:c.c0 + c.k].contiguous())
    got = plan.execute(dAx, uview, dVfull[:, c.c0:c.c0 + c.k])
    torch.cuda.synchronize()
    sc.check(c, got.cpu().numpy())
    assert torch.equal(got, dense)                             # the leading dimension changes no bit
    # k given: the first k columns of wider operands
    c0 = c._replace(c0=0, k=7, name=c.name + "-k7")
    got = plan.execute(dAx, dUfull, dVfull, k=7)
    sc.check(c0, got.cpu().numpy())
    plan.destroy()


def test_nothing_stored_launches_nothing(sp):
    for n_rows in (0, 2500):
        Ap = torch.zeros(n_rows + 1, dtype=torch.int32, device=DEV)
        Aj = torch.zeros(0, dtype=torch.int32, device=DEV)
        plan = sp.SddmmPlan(n_rows, 5, 0, Ap, Aj, torch.float32)
        out = plan.execute(None, torch.ones(max(n_rows, 1), 4, device=DEV)[:n_rows], torch.ones(5, 4, device=DEV))
        torch.cuda.synchronize()
        assert out.numel() == 0 and plan.info()["n_slices"] == -(-n_rows // 1024)
        plan.destroy()


@pytest.mark.parametrize("n_rows,nnz", [(0, 0), (1, 0), (23, 1000), (1, 1023), (1025, 0), (96, 4000), (4096, 1)])
def test_the_multi_object_and_the_sddmm_object_cut_alike(sp, n_rows, nnz):
    """No rows, one item, and n_rows + nnz = 1 023, 1 024, 1 025, 4 096, 4 097: both objects report one slice length, one
    slice count and one grid (a create reads nothing of Ap / Aj; the multi object's needs the device for its carries)."""
    lib = sp.capi.lib()
    dummy = C.c_void_p(256)
    hm, hs = C.c_void_p(), C.c_void_p()
    assert lib.mi355_spmv_multi_create(C.byref(hm), 1, 0, n_rows, 7, nnz, dummy, dummy, 4) == 0
    assert lib.mi355_spmv_sddmm_create(C.byref(hs), 1, 0, n_rows, 7, nnz, dummy, dummy) == 0
    mi, si = sp.capi.MultiInfo(), sp.capi.SddmmInfo()
    assert lib.mi355_spmv_multi_get_info(hm, C.byref(mi)) == 0 and lib.mi355_spmv_sddmm_get_info(hs, C.byref(si)) == 0
    assert lib.mi355_spmv_multi_destroy(hm) == 0 and lib.mi355_spmv_sddmm_destroy(hs) == 0
    assert (mi.slice_len, mi.n_slices, mi.grid_blocks) == (si.slice_len, si.n_slices, si.grid_blocks)
    assert si.slice_len == sc.SLICE_LEN and si.n_slices == -(-(n_rows + nnz) // sc.SLICE_LEN)
    assert si.grid_blocks == -(-si.n_slices // (si.block_threads // sc.STEP))


@pytest.mark.parametrize("val", ["f32", "f64"])
def test_sddmm_is_the_adjoint_of_spmm_in_ax(sp, val):
    """For integer dY, X, Ax: sum(out * Ax) == sum(dY * spmm(A, X)) exactly, out = SDDMM(dY, X) on the pattern — the
    identity <dY, d(A X)/dAx . Ax> that makes SDDMM the gradient of sp.spmm with respect to Ax."""
    m = sc.ragged_structure()
    Ap, Aj, Ax, O0, U, V = sc.arrays(m, "i32", val, True)
    n_rows, n_cols, nnz, k = len(m.lens), m.n_cols, int(Ap[-1]), 12
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    dY, X = d(U[:, :k]), d(V[:, :k])
    out = sp.sddmm(n_rows, n_cols, nnz, dAp, dAj, None, dY, X)
    Y = torch.full((n_rows, k), float("nan"), dtype=dAx.dtype, device=DEV)
    sp.spmm(n_rows, n_cols, nnz, dAp, dAj, dAx, X, Y)
    torch.cuda.synchronize()
    lhs = (out.double() * dAx.double()).sum().item()
    rhs = (dY.double() * Y.double()).sum().item()
    assert lhs == rhs and lhs != 0.0 and float(lhs).is_integer()
