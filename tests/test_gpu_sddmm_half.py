"""SDDMM with 16-bit U and V on the GPU (sp.SddmmPlan(..., vec_dtype=) / sp.sddmm_half, csrc/sddmm_half_kernel.hpp): the
table of tests/sddmm_half_cases.py — the cases that tests/test_sddmm_half_sim_cpu.py executes on the host — on the
device, each out against numpy's fp64 value on the widened operands within the dot-product bound of that module (integer
data bit for bit); padding columns of U and V hold NaN, out starts as NaN where beta = 0, and a canary behind
out[nnz - 1] must survive.  Every case is also run through the fp32 SddmmPlan on the widened operands: on integer data
the two outs are equal bit for bit, on real data they lie within twice the bound (each lies within it of the fp64 value).
Then what only a device shows: two executes give the same bits, a side stream, one graph capture replayed on new U / V,
the one-shots, a padded view, Ax = None, k below the columns held, and the adjoint identity that makes SDDMM the gradient
of sp.spmm."""
import ctypes as C

import numpy as np
import pytest
import torch

import sddmm_half_cases as hc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TAIL = 5            # canary elements behind out
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}


def on_device(flat, shift, tail=0, fill=0.0, dtype=None):
    """1-D device copy of `flat` whose base lies `shift` elements past a 16-byte boundary, `tail` elements of `fill`
    behind it (returns the view of flat.size + tail elements; an empty one has no base).  dtype: the 16-bit type that a
    uint16 array of bit patterns stands for."""
    flat = np.ascontiguousarray(flat)
    t = torch.from_numpy(flat.view(np.int16)).view(dtype) if dtype is not None else torch.from_numpy(flat)
    es = t.element_size()
    buf = torch.full((t.numel() + tail + 16 // es + 1,), fill, dtype=t.dtype, device=DEV)
    base = ((16 - buf.data_ptr() % 16) % 16) // es + shift
    v = buf[base:base + t.numel() + tail]
    v[:t.numel()].copy_(t)
    assert v.numel() == 0 or v.data_ptr() % 16 == shift * es
    return v


def half(a, vec):
    """A device tensor of the 16-bit type holding the (exactly representable) values of the fp32 array a."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return torch.from_numpy(hc.to_bits(a, vec).view(np.int16)).view(TORCH[vec]).reshape(a.shape).to(DEV)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def execute_case(plan, wide, c, dAx):
    """One case of the table on `plan`, and on the fp32 plan `wide` with the widened operands; returns both outs as
    numpy (the canary checked)."""
    Ap, Aj, Ax, O0, U, V = hc.arrays(c.matrix, c.off, c.vec, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    nan = np.uint16(hc.NAN_BITS[c.vec])
    uh = np.full((n_rows, c.ldu), nan, dtype=np.uint16)
    uh[:, :c.k] = hc.to_bits(U[:, c.c0:c.c0 + c.k], c.vec)
    vh = np.full((n_cols, c.ldv), nan, dtype=np.uint16)
    vh[:, :c.k] = hc.to_bits(V[:, c.c0:c.c0 + c.k], c.vec)
    uf, vf = on_device(uh.ravel(), c.shift[3], dtype=TORCH[c.vec]), on_device(vh.ravel(), c.shift[4], dtype=TORCH[c.vec])
    of = on_device(O0 if c.beta != 0.0 else np.full(nnz, np.nan, dtype=np.float32), c.shift[5], TAIL, hc.CANARY)
    o32 = of[:nnz].clone()
    uv, vv = torch.as_strided(uf, (n_rows, c.k), (c.ldu, 1)), torch.as_strided(vf, (n_cols, c.k), (c.ldv, 1))
    for p in (plan, wide):
        p.set_alpha_beta(c.alpha, c.beta)
    got = plan.execute(dAx if c.valued else None, uv, vv, of[:nnz])
    assert nnz == 0 or got.data_ptr() == of.data_ptr()
    wide.execute(dAx if c.valued else None, uv.float(), vv.float(), o32)
    oh = of.cpu().numpy()       # (the copy synchronises)
    assert np.all(oh[nnz:] == np.float32(hc.CANARY)), "%s: the canary behind out was written" % c.name
    return oh[:nnz], o32.cpu().numpy()


@pytest.fixture(scope="module")
def table(sp):
    """Every case of the table, run once: {case name: (out, the fp32 plan's out)}.  Plans are made per (structure, types,
    matrix offsets) and reused over k, alpha / beta, leading dimensions and the offsets of U, V and out.  No case is
    skipped."""
    results = {}
    key, plan, wide, dAx = None, None, None, None
    try:
        for c in sorted(hc.table(), key=hc.plan_key):
            if hc.plan_key(c) != key:
                for p in (plan, wide):
                    if p is not None:
                        p.destroy()
                plan = wide = None
                key = hc.plan_key(c)
                Ap, Aj, Ax = hc.arrays(c.matrix, c.off, c.vec, c.integer)[:3]
                n_rows, nnz = len(c.matrix.lens), int(Ap[-1])
                dAp, dAj, dAx = on_device(Ap, c.shift[0]), on_device(Aj, c.shift[1]), on_device(Ax, c.shift[2])
                plan = sp.SddmmPlan(n_rows, c.matrix.n_cols, nnz, dAp, dAj, torch.float32, vec_dtype=TORCH[c.vec])
                wide = sp.SddmmPlan(n_rows, c.matrix.n_cols, nnz, dAp, dAj, torch.float32)
                assert plan.vec_dtype is TORCH[c.vec] and plan.val_dtype is torch.float32
                hc.assert_geometry(plan.info())
                assert plan.info()["n_slices"] == wide.info()["n_slices"] == -(-(n_rows + nnz) // hc.SLICE_LEN)
            results[c.name] = execute_case(plan, wide, c, dAx)
    finally:
        for p in (plan, wide):
            if p is not None:
                p.destroy()
    return results


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_table(table, family):
    cases = hc.family(family)
    assert cases
    for c in cases:
        hc.check(c, table[c.name][0])


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_agreement_with_the_fp32_plan_on_the_widened_operands(table, family):
    for c in hc.family(family):
        got, wide = table[c.name]
        if c.integer:
            assert np.array_equal(got.view(np.uint32), wide.view(np.uint32)), c.name
        else:
            hc.check(c, wide)                   # the fp32 plan's own out lies within the bound of the fp64 value ...
            bound = hc.expected(c)[1]
            err = np.abs(got.astype(np.float64) - wide.astype(np.float64))
            bad = np.nonzero(err > 2 * bound)[0]        # ... so the two lie within twice the bound of each other
            assert bad.size == 0, "%s: entries %s (excess %s)" % (c.name, bad[:8], (err - 2 * bound)[bad[:8]])


def test_alignment_changes_no_bit(table):
    for a, b in hc.alignment_pairs():
        assert np.array_equal(table[a.name][0].view(np.uint8), table[b.name][0].view(np.uint8)), a.name


def test_equal_rows_of_u_and_v_give_equal_bits_wherever_the_entry_lies(table):
    for a, b, ia, ib in hc.position_checks():
        oa, ob = table[a.name][0], table[b.name][0]
        assert ia.size > 100
        bad = np.nonzero(oa[ia].view(np.uint8).reshape(ia.size, -1) != ob[ib].view(np.uint8).reshape(ib.size, -1))[0]
        assert bad.size == 0, "%s vs %s: entries %s / %s differ" % (a.name, b.name, ia[bad[:8]], ib[bad[:8]])


# ---- what only a device shows ---------------------------------------------------------------------------------------------
def ragged_real(off="i32", vec="bf16", k=13):
    """The ragged structure with real data as a case of its own (valued, alpha / beta = 2.5 / 0, no padding)."""
    return hc._case(hc.ragged_structure(), off, vec, k, (2.5, 0.0), (0, 0), hc.ALIGNED, True, "-device")


@pytest.mark.parametrize("vec", hc.VECS)
def test_repeat_side_stream_and_graph(sp, vec):
    c = ragged_real(vec=vec, k=21)
    Ap, Aj, Ax, O0, U, V = hc.arrays(c.matrix, c.off, c.vec, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    plan = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, vec_dtype=TORCH[vec])
    plan.set_alpha_beta(c.alpha, c.beta)
    dU, dV = half(U[:, c.c0:c.c0 + c.k], vec), half(V[:, c.c0:c.c0 + c.k], vec)
    out = torch.full((nnz,), float("nan"), device=DEV)
    plan.execute(dAx, dU, dV, out)
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    hc.check(c, first)
    out.fill_(float("nan"))
    plan.execute(dAx, dU, dV, out)              # two executes: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(first.view(np.uint32), out.cpu().numpy().view(np.uint32))
    # out=None makes the result, in fp32
    made = plan.execute(dAx, dU, dV)
    assert made.shape == (nnz,) and made.dtype == torch.float32
    assert np.array_equal(first.view(np.uint32), made.cpu().numpy().view(np.uint32))
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
    dU.copy_(half(U[:, c2.c0:c2.c0 + c.k], vec))
    dV.copy_(half(V[:, c2.c0:c2.c0 + c.k], vec))
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    hc.check(c2, got)
    assert not np.array_equal(got, first)
    del g
    plan.destroy()


@pytest.mark.parametrize("off,vec", [("i32", "f16"), ("i32", "bf16"), ("i64", "f16"), ("i64", "bf16")])
def test_one_shots_equal_the_plan(sp, off, vec):
    c = ragged_real(off, vec, 9)
    Ap, Aj, Ax, O0, U, V = hc.arrays(c.matrix, c.off, c.vec, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    dU, dV = half(U[:, c.c0:c.c0 + c.k], vec), half(V[:, c.c0:c.c0 + c.k], vec)
    plan = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, vec_dtype=TORCH[vec])
    for ax in (dAx, None):
        want = plan.execute(ax, dU, dV)
        got = sp.sddmm_half(n_rows, n_cols, nnz, dAp, dAj, ax, dU, dV)
        torch.cuda.synchronize()                    # (neither synchronises)
        assert got.dtype == torch.float32 and torch.equal(got, want)
        hc.check(c._replace(alpha=1.0, valued=ax is not None), got.cpu().numpy())
        # the C entry point itself, into a given out
        out = torch.full((nnz,), float("nan"), device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        f = getattr(sp.capi.lib(), "mi355_spmv_sddmm_half_%s_%s" % (off, vec))
        assert f(n_rows, n_cols, nnz, ptr(dAp), ptr(dAj), ptr(ax), ptr(dU), c.k, ptr(dV), c.k, ptr(out), c.k,
                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    plan.destroy()


@pytest.mark.parametrize("vec", hc.VECS)
def test_a_padded_view_and_k_below_the_columns_held(sp, vec):
    c = ragged_real(vec=vec, k=19)
    Ap, Aj, Ax, O0, U, V = hc.arrays(c.matrix, c.off, c.vec, c.integer)
    n_rows, n_cols, nnz = len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1])
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    plan = sp.SddmmPlan(n_rows, n_cols, nnz, dAp, dAj, torch.float32, vec_dtype=TORCH[vec])
    plan.set_alpha_beta(c.alpha, c.beta)
    dUfull, dVfull = half(U, vec), half(V, vec)                # KF columns each
    uview = dUfull[:, c.c0:c.c0 + c.k]                         # non-contiguous: stride(0) = KF
    assert not uview.is_contiguous() and uview.stride() == (hc.KF, 1)
    dense = plan.execute(dAx, uview.contiguous(), dVfull[:, c.c0:c.c0 + c.k].contiguous())
    got = plan.execute(dAx, uview, dVfull[:, c.c0:c.c0 + c.k])
    torch.cuda.synchronize()
    hc.check(c, got.cpu().numpy())
    assert torch.equal(got, dense)                             # the leading dimension changes no bit
    # k given: the first k columns of wider operands, and no values
    c0 = c._replace(c0=0, k=7, valued=False, name=c.name + "-k7")
    got = plan.execute(None, dUfull, dVfull, k=7)
    hc.check(c0, got.cpu().numpy())
    plan.destroy()


def test_nothing_stored_launches_nothing(sp):
    for n_rows in (0, 2500):
        Ap = torch.zeros(n_rows + 1, dtype=torch.int32, device=DEV)
        Aj = torch.zeros(0, dtype=torch.int32, device=DEV)
        plan = sp.SddmmPlan(n_rows, 5, 0, Ap, Aj, torch.float32, vec_dtype=torch.bfloat16)
        out = plan.execute(None, torch.ones(max(n_rows, 1), 4, dtype=torch.bfloat16, device=DEV)[:n_rows],
                           torch.ones(5, 4, dtype=torch.bfloat16, device=DEV))
        torch.cuda.synchronize()
        assert out.numel() == 0 and out.dtype == torch.float32 and plan.info()["n_slices"] == -(-n_rows // 1024)
        plan.destroy()


@pytest.mark.parametrize("vec", hc.VECS)
def test_sddmm_half_is_the_adjoint_of_spmm_in_ax(sp, vec):
    """For integer dY, X, Ax: sum(out * Ax) == sum(dY * spmm(A, X)) exactly, out = SDDMM(dY, X) on the pattern with dY and
    X in 16 bits, spmm from the fp32 multi-vector kind on the widened X."""
    m = hc.ragged_structure()
    Ap, Aj, Ax, O0, U, V = hc.arrays(m, "i32", vec, True)
    n_rows, n_cols, nnz, k = len(m.lens), m.n_cols, int(Ap[-1]), 12
    dAp, dAj, dAx = d(Ap), d(Aj), d(Ax)
    dY, X = half(U[:, :k], vec), half(V[:, :k], vec)
    out = sp.sddmm_half(n_rows, n_cols, nnz, dAp, dAj, None, dY, X)
    Y = torch.full((n_rows, k), float("nan"), device=DEV)
    sp.spmm(n_rows, n_cols, nnz, dAp, dAj, dAx, X.float(), Y)
    torch.cuda.synchronize()
    lhs = (out.double() * dAx.double()).sum().item()
    rhs = (dY.double() * Y.double()).sum().item()
    assert lhs == rhs and lhs != 0.0 and float(lhs).is_integer()
