"""GPU suite: COO -> CSR on the device (mi355_spmv_coo_to_csr, sp.coo_to_csr) against the reference's ToCsr
ordering — Ap from the row counts, entries of a row in input order, duplicates kept — checked bit for bit against a
stable argsort of the rows (numpy for the fixtures, torch.argsort(stable=True) on the GPU for the large cases).
Shapes cover every radix pass count (1 row: none; 255 / 256 / 257 rows: one or two; 65 536 / 65 537: two or three;
2^24: three), one row holding every entry (all lanes of a step share the digit), and more than 2^31 entries."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import __graft_entry__
from conftest import GOLD

pytestmark = pytest.mark.gpu
sp = __graft_entry__.load_package()
DEV = "cuda:0"
OFFS = {"i32": torch.int32, "i64": torch.int64}
VALS = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "none": None}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64}


def bits(t):
    return t.view(BITS[t.dtype])


def expected(n_rows, rows, cols, vals, off_dtype):
    """ToCsr by a stable sort on the row (the oracle: torch on the device)."""
    order = torch.argsort(rows.long(), stable=True)
    Ap = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    if rows.numel():
        torch.cumsum(torch.bincount(rows.long(), minlength=n_rows), 0, out=Ap[1:])
    return Ap.to(off_dtype), cols[order], (vals[order] if vals is not None else None), order


def check(n_rows, n_cols, rows, cols, vals=None, off="i32"):
    csr, perm = sp.coo_to_csr(n_rows, n_cols, rows, cols, vals, OFFS[off], return_perm=True)
    Ap, Aj, Ax, order = expected(n_rows, rows, cols, vals, OFFS[off])
    assert (csr.n_rows, csr.n_cols, csr.nnz) == (n_rows, n_cols, rows.numel())
    assert csr.Ap.dtype == OFFS[off] and torch.equal(csr.Ap, Ap)
    assert torch.equal(csr.Aj, Aj)
    assert torch.equal(perm, order)
    if vals is None:
        assert csr.Ax is None
    else:
        assert csr.Ax.dtype == vals.dtype and torch.equal(bits(csr.Ax), bits(Ax))
    return csr, perm


def make_coo(n_rows, nnz, order, seed, n_cols=None):
    """Rows with empty runs at the start, in the middle and at the end, duplicate (row, col) pairs, and the entries
    in one of four orders: shuffled, row-sorted, reverse-sorted or column-major."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    n_cols = n_cols or max(n_rows, 64)
    gap = max(1, n_rows // 16)
    lo, hi = (gap, n_rows - gap) if n_rows >= 16 else (0, n_rows)
    rows = torch.randint(lo, hi, (nnz,), generator=g, device=DEV)
    if n_rows >= 16:   # an empty run in the middle
        mid = (n_rows // 2 - gap // 2, n_rows // 2 + gap // 2)
        rows = torch.where((rows >= mid[0]) & (rows < mid[1]), rows - gap, rows)
    cols = torch.randint(0, min(n_cols, 8), (nnz,), generator=g, device=DEV)   # few columns: many duplicates
    cols = torch.where(torch.rand(nnz, generator=g, device=DEV) < 0.5, cols,
                       torch.randint(0, n_cols, (nnz,), generator=g, device=DEV))
    if order == "row-sorted":
        p = torch.argsort(rows, stable=True)
    elif order == "reverse-sorted":
        p = torch.argsort(-rows, stable=True)
    elif order == "column-major":
        p = torch.argsort(cols * n_rows + rows, stable=True)
    else:
        p = torch.randperm(nnz, generator=g, device=DEV)
    return rows[p].int().contiguous(), cols[p].int().contiguous(), n_cols


def values(nnz, kind, seed):
    if VALS[kind] is None:
        return None
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    if kind == "i32":
        return torch.randint(-2 ** 31, 2 ** 31 - 1, (nnz,), generator=g, device=DEV, dtype=torch.int32)
    return torch.randn(nnz, generator=g, device=DEV, dtype=VALS[kind])


def test_empty_matrix():
    e = torch.empty(0, dtype=torch.int32, device=DEV)
    for off in OFFS:
        csr = check(0, 0, e, e, None, off)[0]
        assert csr.Ap.tolist() == [0]
        csr = check(5, 3, e, e, torch.empty(0, device=DEV), off)[0]
        assert csr.Ap.tolist() == [0] * 6


def test_one_row_holds_every_entry():
    """100 000 entries of row 0 (no radix pass), and the same entries as the only non-empty row of 256 and of 2^17 rows,
    where every lane of every step shares one digit."""
    nnz = 100000
    cols = torch.randperm(nnz, device=DEV).int() % 977
    vals = values(nnz, "f64", 3)
    for n_rows, row in ((1, 0), (256, 255), (1 << 17, 70000)):
        rows = torch.full((nnz,), row, dtype=torch.int32, device=DEV)
        csr, perm = check(n_rows, 977, rows, cols, vals, "i64")
        assert torch.equal(perm, torch.arange(nnz, device=DEV))


@pytest.mark.parametrize("order", ["shuffled", "row-sorted", "reverse-sorted", "column-major"])
@pytest.mark.parametrize("n_rows,nnz", [(255, 40000), (256, 40000), (257, 40000), (65536, 300000), (65537, 300000),
                                        (1 << 24, 3 << 23)])
def test_shapes_and_orders(n_rows, nnz, order):
    rows, cols, n_cols = make_coo(n_rows, nnz, order, seed=n_rows + nnz)
    check(n_rows, n_cols, rows, cols, values(nnz, "f32", 1), "i32")


@pytest.mark.parametrize("off", list(OFFS))
@pytest.mark.parametrize("val", list(VALS))
def test_types(off, val):
    for n_rows, nnz in ((257, 5000), (65537, 123457)):   # one / two and two / three passes
        rows, cols, n_cols = make_coo(n_rows, nnz, "shuffled", seed=nnz)
        check(n_rows, n_cols, rows, cols, values(nnz, val, 2), off)


@pytest.mark.parametrize("off,val", [(o, v) for o in ("i32", "i64") for v in ("f32", "f64")])
def test_golden_fixtures_through_load_mtx_coo(oracle, off, val):
    tv = {"f32": torch.float32, "f64": torch.float64}[val]
    for path in sorted(glob.glob(os.path.join(GOLD, "*.mtx"))):
        coo = sp.load.load_mtx_coo(path, OFFS[off], tv, DEV)
        csr = sp.coo_to_csr(coo.n_rows, coo.n_cols, coo.rows, coo.cols, coo.vals, OFFS[off])
        n_rows, n_cols, Ap, Aj, Ax = oracle.load_mtx(path, off, val)
        assert (csr.n_rows, csr.n_cols) == (n_rows, n_cols), path
        assert np.array_equal(csr.Ap.cpu().numpy(), Ap), path
        assert np.array_equal(csr.Aj.cpu().numpy(), Aj), path
        assert np.array_equal(csr.Ax.cpu().numpy().view(np.uint8), Ax.view(np.uint8)), path


def test_c5_rmat24_edges_give_the_workloads_csr():
    """The edge list of synth.rmat (scale 24, edge factor 16, seed 5), regenerated here: 2^28 entries, hub rows."""
    scale, E = 24, 16 << 24
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    a, b, c = 0.57, 0.19, 0.19
    rows = torch.zeros(E, dtype=torch.int32, device=DEV)
    cols = torch.zeros(E, dtype=torch.int32, device=DEV)
    for _bit in range(scale):
        r = torch.rand(E, generator=g, device=DEV, dtype=torch.float32)
        rows.mul_(2).add_((r >= a + b).int())
        cols.mul_(2).add_((((r >= a) & (r < a + b)) | (r >= a + b + c)).int())
        del r
    csr = sp.coo_to_csr(1 << scale, 1 << scale, rows, cols)
    del rows, cols
    ref = sp.synth.workload("c5-rmat24", device=DEV)
    assert torch.equal(csr.Ap, ref.Ap)
    assert torch.equal(csr.Aj, ref.Aj)
    del csr, ref
    torch.cuda.empty_cache()


def test_more_than_2_31_entries():
    """nnz = 2^31 + 2^21 with row = k mod 2^20 and col = k >> 20: row r holds k = r + j * 2^20 for j = 0 .. 2049, in
    that order, so Ap[r] = 2050 r and Aj[2050 r + j] = j."""
    n_rows, per_row = 1 << 20, 2050
    nnz = n_rows * per_row
    assert nnz == 2 ** 31 + 2 ** 21
    rows = torch.empty(nnz, dtype=torch.int32, device=DEV)
    cols = torch.empty(nnz, dtype=torch.int32, device=DEV)
    step = 1 << 28
    for s in range(0, nnz, step):
        k = torch.arange(s, min(nnz, s + step), device=DEV, dtype=torch.int64)
        rows[s:s + k.numel()] = (k & (n_rows - 1)).int()
        cols[s:s + k.numel()] = (k >> 20).int()
        del k
    csr = sp.coo_to_csr(n_rows, per_row, rows, cols, None, torch.int64)
    del rows, cols
    torch.cuda.empty_cache()
    assert torch.equal(csr.Ap, torch.arange(n_rows + 1, device=DEV, dtype=torch.int64) * per_row)
    want = torch.arange(per_row, device=DEV, dtype=torch.int32)
    Aj = csr.Aj.view(n_rows, per_row)
    for r0 in range(0, n_rows, 1 << 16):
        assert torch.equal(Aj[r0:r0 + (1 << 16)], want.expand(1 << 16, per_row)), r0
    del csr, Aj
    torch.cuda.empty_cache()


def test_bad_index_is_rejected_and_nothing_is_written():
    """A row of -1, a row equal to n_rows and a column equal to n_cols: EINVAL, a message that names the first bad
    entry, and every output buffer and the guard bytes around it as they were."""
    L = sp.capi.lib()
    n_rows, n_cols, nnz, guard = 1000, 500, 70000, 4096
    rows0, cols0, _ = make_coo(n_rows, nnz, "shuffled", seed=9, n_cols=n_cols)
    vals = values(nnz, "f64", 9)
    ws_bytes = sp.capi.coo_to_csr_workspace_bytes(n_rows, nnz, torch.int64, torch.float64)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def guarded(nbytes):
        t = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
        return t, C.c_void_p(t.data_ptr() + guard)

    for where, bad_row, bad_col in ((4321, -1, None), (60000, n_rows, None), (123, None, n_cols)):
        rows, cols = rows0.clone(), cols0.clone()
        if bad_row is not None:
            rows[where] = bad_row
        if bad_col is not None:
            cols[where] = bad_col
        rows[where + 7] = n_rows + 5            # a later bad entry: the message names the first one
        bufs = [guarded(8 * (n_rows + 1)), guarded(4 * nnz), guarded(8 * nnz), guarded(8 * nnz)]
        size = C.c_size_t(ws_bytes)
        st = L.mi355_spmv_coo_to_csr(1, 1, n_rows, n_cols, nnz, C.c_void_p(rows.data_ptr()),
                                     C.c_void_p(cols.data_ptr()), C.c_void_p(vals.data_ptr()), bufs[0][1], bufs[1][1],
                                     bufs[2][1], bufs[3][1], C.c_void_p(ws.data_ptr()), C.byref(size),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = L.mi355_spmv_last_error().decode()
        assert st == 1, msg
        r, c = int(rows[where]), int(cols[where])
        assert "entry %d is (row %d, col %d)" % (where, r, c) in msg, msg
        for t, _ in bufs:
            assert bool((t == 0xA5).all())


def test_outputs_stay_inside_their_buffers():
    """A successful call writes exactly its outputs: guard bytes on both sides of each stay as they were."""
    L = sp.capi.lib()
    n_rows, nnz, guard = 70001, 250001, 4096
    rows, cols, n_cols = make_coo(n_rows, nnz, "column-major", seed=4)
    vals = values(nnz, "f32", 4)
    ws_bytes = sp.capi.coo_to_csr_workspace_bytes(n_rows, nnz, torch.int32, torch.float32)
    ws = torch.full((ws_bytes + 2 * guard,), 0x5A, dtype=torch.uint8, device=DEV)
    sizes = [4 * (n_rows + 1), 4 * nnz, 4 * nnz, 8 * nnz]
    bufs = [torch.full((n + 2 * guard,), 0x5A, dtype=torch.uint8, device=DEV) for n in sizes]
    p = [C.c_void_p(t.data_ptr() + guard) for t in bufs]
    size = C.c_size_t(ws_bytes)
    st = L.mi355_spmv_coo_to_csr(0, 0, n_rows, n_cols, nnz, C.c_void_p(rows.data_ptr()), C.c_void_p(cols.data_ptr()),
                                 C.c_void_p(vals.data_ptr()), p[0], p[1], p[2], p[3],
                                 C.c_void_p(ws.data_ptr() + guard), C.byref(size),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, L.mi355_spmv_last_error()
    for t, n in zip(bufs + [ws], sizes + [ws_bytes]):
        assert bool((t[:guard] == 0x5A).all()) and bool((t[guard + n:] == 0x5A).all())
    Ap, Aj, Ax, order = expected(n_rows, rows, cols, vals, torch.int32)
    out = lambda i, dt, n: bufs[i][guard:guard + sizes[i]].view(dt)[:n]
    assert torch.equal(out(0, torch.int32, n_rows + 1), Ap)
    assert torch.equal(out(1, torch.int32, nnz), Aj)
    assert torch.equal(out(2, torch.int32, nnz), bits(Ax))
    assert torch.equal(out(3, torch.int64, nnz), order)


def test_two_runs_are_bitwise_equal():
    rows, cols, n_cols = make_coo(1 << 20, 3 << 20, "shuffled", seed=12)
    rows[: 1 << 20] = 777                     # a hub row
    vals = values(rows.numel(), "f64", 12)
    a, pa = sp.coo_to_csr(1 << 20, n_cols, rows, cols, vals, torch.int64, return_perm=True)
    b, pb = sp.coo_to_csr(1 << 20, n_cols, rows, cols, vals, torch.int64, return_perm=True)
    assert torch.equal(a.Ap, b.Ap) and torch.equal(a.Aj, b.Aj) and torch.equal(bits(a.Ax), bits(b.Ax))
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("kind", ["vector", "merge", "light"])
def test_plan_on_device_made_csr_gives_the_same_y_as_on_the_host_made_one(tmp_path, kind):
    """A Matrix Market file through the host loader (LoadCoo + ToCsr) and through load_mtx_coo + coo_to_csr: a plan
    on either set of arrays gives y with the same bits."""
    rng = np.random.RandomState(21)
    n, nnz = 30000, 400000
    r = rng.randint(0, n, nnz)
    r[r % 97 == 3] = 5                         # a long row
    c = rng.randint(0, n, nnz)
    v = rng.uniform(-1, 1, nnz)
    path = tmp_path / "m.mtx"
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, nnz))
        np.savetxt(f, np.stack([r + 1, c + 1, v], 1), fmt="%d %d %.17g")
    host = sp.load.load_mtx(str(path), torch.int32, torch.float32, DEV)
    coo = sp.load.load_mtx_coo(str(path), torch.int32, torch.float32, DEV)
    dev = sp.coo_to_csr(coo.n_rows, coo.n_cols, coo.rows, coo.cols, coo.vals, torch.int32)
    assert torch.equal(dev.Ap, host.Ap) and torch.equal(dev.Aj, host.Aj) and torch.equal(bits(dev.Ax), bits(host.Ax))
    x = sp.synth.dense_vector(n, torch.float32, 21, DEV)
    ys = []
    for m in (host, dev):
        p = sp.Plan(kind, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32)
        y = torch.full((n,), float("nan"), device=DEV)
        p.execute(m.Ax, x, y)
        torch.cuda.synchronize()
        p.destroy()
        ys.append(y)
    assert torch.equal(bits(ys[0]), bits(ys[1]))
