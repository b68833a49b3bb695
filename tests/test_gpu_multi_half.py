"""Multi-vector SpMV with 16-bit vectors on the GPU (sp.MultiPlan(..., torch.float16 | torch.bfloat16, k_max,
mat_dtype=), sp.spmm on 16-bit operands; csrc/multi_half_kernels.hpp): the table of tests/multi_half_cases.py that
tests/test_multi_half_sim_cpu.py executes on the host, the ragged matrix through the one-shot, graph capture and
replay, a side stream, two executes with the same bits, k_max wider than k, and one comparison against the fp32
MultiPlan on widened operands.  Y is poisoned before every call with beta = 0; the padding columns of X hold NaN and
those of Y a canary that must survive."""
import numpy as np
import pytest
import torch

import multi_cases as mc
import multi_half_cases as hc
import sim_runner as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(flat, shift, dtype=None):
    """1-D device copy of `flat` whose base lies `shift` elements past a 16-byte boundary (an empty one has no base);
    16-bit patterns (uint16) are carried as int16 and viewed as `dtype`."""
    a = np.ascontiguousarray(flat)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    es = t.element_size()
    buf = torch.empty(t.numel() + 16 // es + 1, dtype=t.dtype, device=DEV)
    base = ((16 - buf.data_ptr() % 16) % 16) // es + shift
    v = buf[base:base + t.numel()]
    v.copy_(t)
    assert t.numel() == 0 or v.data_ptr() % 16 == shift * es
    return v if dtype is None or dtype == t.dtype else v.view(dtype)


def bits_of(t):
    """A 16-bit device tensor's patterns as a numpy uint16 array (the copy synchronises)."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def half_operand(a, t):
    """An fp32 array of exactly representable values as a device tensor of type t."""
    if t == "f32":
        return d(np.ascontiguousarray(a, dtype=np.float32))
    return d(hc.to_bits(a, t).view(np.int16)).view(TORCH[t])


# ---- the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["row_ends", "open_row", "slice_edges", "ragged"])
def test_table(sp, family):
    """Every case on the structures of the family, the sequences on one object among them: objects are made per
    (structure, types, data, matrix offsets, k_max) and reused over k, alpha / beta, leading dimensions and the offsets
    of X and Y.  No case is skipped."""
    groups = [g for g in sr.consecutive_runs(hc.table(), hc.plan_key) if g[0].matrix.family == family]
    assert groups
    for g in groups:
        c = g[0]
        Ap, Aj, Ax, X, Y0 = hc.arrays(c.matrix, c.off, c.vec, c.mat, c.integer)
        n_rows, n_cols = len(c.matrix.lens), c.matrix.n_cols
        mt = hc.mat_type(c)
        dAp, dAj = on_device(Ap, c.shift[0]), on_device(Aj, c.shift[1])
        dAx = on_device(hc.stored(Ax, mt), c.shift[2], TORCH[mt])
        plan = sp.MultiPlan(n_rows, n_cols, int(Ap[-1]), dAp, dAj, TORCH[c.vec], c.k_max, mat_dtype=TORCH[mt])
        try:
            info = plan.info()
            assert info["slice_len"] == mc.SLICE_LEN and info["widest_tile"] == hc.TILE == max(mc.LANES_PER_SLOT) * hc.VEC
            assert info["val_type"] == hc.VAL_TYPE[c.vec] and info["passes"] == -(-c.k_max // hc.TILE)
            carry_ld = -(-c.k_max // hc.TILE) * hc.TILE
            assert info["scratch_bytes"] == info["n_slices"] * (4 + 2 * carry_ld * 4)
            assert plan.types() == {"mat_type": hc.VAL_TYPE[mt], "vec_type": hc.VAL_TYPE[c.vec], "semiring": 0}
            xbits, y0bits = hc.to_bits(X, c.vec), hc.to_bits(Y0, c.vec)
            canary = hc.to_bits(np.float32(hc.CANARY), c.vec)[0]
            for c in g:
                xh = np.full((n_cols, c.ldx), hc.NAN_BITS[c.vec], dtype=np.uint16)
                xh[:, :c.k] = xbits[:, c.c0:c.c0 + c.k]
                yh = np.full((n_rows, c.ldy), canary, dtype=np.uint16)
                yh[:, :c.k] = y0bits[:, c.c0:c.c0 + c.k] if c.beta != 0.0 else hc.NAN_BITS[c.vec]
                xf = on_device(xh.ravel(), c.shift[3], TORCH[c.vec])
                yf = on_device(yh.ravel(), c.shift[4], TORCH[c.vec])
                plan.set_alpha_beta(c.alpha, c.beta)
                plan.execute(dAx, torch.as_strided(xf, (n_cols, c.k), (c.ldx, 1)), torch.as_strided(yf, (n_rows, c.k), (c.ldy, 1)))
                hc.check(c, bits_of(yf))        # (the copy synchronises)
        finally:
            plan.destroy()


# ---- the ragged matrix: one-shot, life cycle, the fp32 plan ---------------------------------------------------------------
def ragged(vec, integer):
    m = mc.ragged_structure()
    Ap, Aj, Ax, X, Y0 = hc.arrays(m, "i32", vec, "same", integer)
    return m, Ap, Aj, Ax, X, Y0


def ragged_case(vec, k, integer, alpha=1.0, beta=0.0, c0=0, k_max=None):
    m = mc.ragged_structure()
    return hc.Case("ragged-%s-k%d" % (vec, k), m, "i32", vec, "same", integer, k, k_max or k, c0, k, k, alpha, beta, mc.ALIGNED)


@pytest.mark.parametrize("vec", hc.VECS)
@pytest.mark.parametrize("off", hc.OFFS)
def test_spmm_calls_the_one_shot(sp, vec, off):
    for k, integer in ((13, True), (70, False)):
        m, Ap, Aj, Ax, X, Y0 = ragged(vec, integer)
        c = ragged_case(vec, k, integer)._replace(ldy=k + 2)
        ybuf = torch.full((len(m.lens), k + 2), hc.CANARY, dtype=TORCH[vec], device=DEV)
        dY = ybuf[:, :k]
        dY.fill_(float("nan"))
        out = sp.spmm(len(m.lens), m.n_cols, int(Ap[-1]), d(Ap.astype(mc.NP[off])), d(Aj), half_operand(Ax, vec),
                      half_operand(X[:, :k], vec), dY)        # (the one-shot synchronises)
        assert out is dY
        hc.check(c, bits_of(ybuf))


@pytest.mark.parametrize("vec", hc.VECS)
def test_repeat_side_stream_graph_and_k_max_wider_than_k(sp, vec):
    k = 40
    m, Ap, Aj, Ax, X, Y0 = ragged(vec, True)
    n_rows, nnz = len(m.lens), int(Ap[-1])
    dAp, dAj, dAx, dX = d(Ap), d(Aj), half_operand(Ax, vec), half_operand(X[:, :k], vec)
    c = ragged_case(vec, k, True, k_max=129)
    p = sp.MultiPlan(n_rows, m.n_cols, nnz, dAp, dAj, TORCH[vec], 129)      # k_max wider than k: three tiles of scratch
    assert p.info()["passes"] == 3 and p.info()["n_kernels"] == 4
    Y = torch.full((n_rows, k), float("nan"), dtype=TORCH[vec], device=DEV)
    p.execute(dAx, dX, Y)
    torch.cuda.synchronize()
    first = bits_of(Y)
    hc.check(c, first)
    Y.fill_(float("nan"))
    p.execute(dAx, dX, Y)                      # two executes: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(first, bits_of(Y))
    s = torch.cuda.Stream()                     # a side stream
    Y.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        p.execute(dAx, dX, Y)
    s.synchronize()
    assert np.array_equal(first, bits_of(Y))
    g = torch.cuda.CUDAGraph()                  # one capture, replayed twice
    with torch.cuda.graph(g):
        p.execute(dAx, dX, Y)
    for _ in range(2):
        Y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(first, bits_of(Y))
    del g
    with pytest.raises(RuntimeError, match="not supported"):
        p.set_semiring("min_plus")
    p.destroy()
    # an object of k_max = k gives the same bits: the width of the scratch is no part of the result
    q = sp.MultiPlan(n_rows, m.n_cols, nnz, dAp, dAj, TORCH[vec], k)
    Y.fill_(float("nan"))
    q.execute(dAx, dX, Y)
    torch.cuda.synchronize()
    assert np.array_equal(first, bits_of(Y))
    q.destroy()


@pytest.mark.parametrize("vec", hc.VECS)
def test_against_the_fp32_plan_on_widened_operands(sp, vec):
    """The fp32 MultiPlan on the widened Ax, X and Y0 computes the same sums in fp32 (in its own order) and does not
    round: the 16-bit result lies within the table's bound of the fp64 reference, and within one 16-bit rounding plus
    the two fp32 bounds of the fp32 plan's result."""
    k, alpha, beta = 33, -0.75, 3.0
    m, Ap, Aj, Ax, X, Y0 = ragged(vec, False)
    n_rows, nnz = len(m.lens), int(Ap[-1])
    dAp, dAj = d(Ap), d(Aj)
    half = sp.MultiPlan(n_rows, m.n_cols, nnz, dAp, dAj, TORCH[vec], k)
    wide = sp.MultiPlan(n_rows, m.n_cols, nnz, dAp, dAj, torch.float32, k)
    half.set_alpha_beta(alpha, beta)
    wide.set_alpha_beta(alpha, beta)
    Yh = half_operand(Y0[:, :k], vec)
    Yw = d(Y0[:, :k])
    half.execute(half_operand(Ax, vec), half_operand(X[:, :k], vec), Yh)
    wide.execute(d(Ax), d(X[:, :k]), Yw)
    torch.cuda.synchronize()
    got = bits_of(Yh)
    hc.check(ragged_case(vec, k, False, alpha, beta), got)
    y64, yabs = (a[:, :k] for a in hc.reference(m, vec, "same", False))
    y0 = Y0[:, :k].astype(np.float64)
    lens = np.asarray(m.lens, dtype=np.int64)[:, None]
    fp32_bound = (lens + 3) * 2.0 ** -24 * (abs(alpha) * yabs + np.abs(beta * y0)) + 1e-300
    w = Yw.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(w - (alpha * y64 + beta * y0)) <= fp32_bound)
    rounding = 2.0 ** -11 * np.abs(w) + 2.0 ** -25 if vec == "f16" else 2.0 ** -8 * np.abs(w)
    assert np.all(np.abs(hc.from_bits(got, vec).astype(np.float64) - w) <= 2 * fp32_bound + rounding)
    half.destroy()
    wide.destroy()
