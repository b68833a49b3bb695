"""GPU suite: the stored entries of a symmetric matrix -> CSR on the device (mi355_spmv_coo_to_csr_symmetric,
sp.coo_to_csr(..., symmetric=True), sp.load.load_mtx_device).  The expected arrays are always numpy: LoadCoo's
expansion rule (reference include/load.hpp:362-403: entry, then its mirror if it is off the diagonal), then a stable
argsort of the rows and a bincount, which is ToCsr.  Everything is compared bit for bit: Ap, Aj, the bits of Ax, perm
(the index of the STORED entry behind each CSR slot)."""
import ctypes as C
import glob
import json
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
NP_BITS = {4: np.uint32, 8: np.uint64}


def np_bits(a):
    return a.view(NP_BITS[a.dtype.itemsize])


def expected(n_rows, rows, cols, vals, off_dtype):
    """numpy: the expansion rule, then ToCsr by a stable sort on the row.  Returns Ap, Aj, Ax, perm."""
    reps = 1 + (rows != cols)
    src = np.repeat(np.arange(len(rows), dtype=np.int64), reps)
    mirror = np.zeros(len(src), dtype=bool)
    mirror[np.cumsum(reps)[reps == 2] - 1] = True
    er = np.where(mirror, cols[src], rows[src])
    ec = np.where(mirror, rows[src], cols[src])
    order = np.argsort(er, kind="stable")
    Ap = np.zeros(n_rows + 1, dtype=np.int64)
    if len(er):
        np.cumsum(np.bincount(er, minlength=n_rows), out=Ap[1:])
    np_off = np.int64 if off_dtype == torch.int64 else np.int32
    return Ap.astype(np_off), ec[order].astype(np.int32), (vals[src][order] if vals is not None else None), src[order]


def check(n, rows, cols, vals=None, off="i32", n_cols=None):
    """rows / cols / vals: numpy, the stored entries.  Runs the device call and compares with expected()."""
    n_cols = n if n_cols is None else n_cols
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None
    d_rows, d_cols, d_vals = t(rows.astype(np.int32)), t(cols.astype(np.int32)), t(vals)
    Ap, Aj, Ax, perm = expected(n, rows, cols, vals, OFFS[off])
    assert sp.coo_symmetric_nnz(d_rows, d_cols) == len(Aj)
    csr, d_perm = sp.coo_to_csr(n, n_cols, d_rows, d_cols, d_vals, OFFS[off], return_perm=True, symmetric=True)
    assert (csr.n_rows, csr.n_cols, csr.nnz) == (n, n_cols, len(Aj))
    assert csr.Ap.dtype == OFFS[off] and np.array_equal(csr.Ap.cpu().numpy(), Ap)
    assert np.array_equal(csr.Aj.cpu().numpy(), Aj)
    assert d_perm.dtype == torch.int64 and np.array_equal(d_perm.cpu().numpy(), perm)
    if vals is None:
        assert csr.Ax is None
    else:
        assert csr.Ax.dtype == d_vals.dtype and np.array_equal(np_bits(csr.Ax.cpu().numpy()), np_bits(Ax))
    return csr, d_perm


def make_stored(n, nnz, order, seed, diag="some"):
    """Stored entries of a symmetric n x n matrix: mostly the lower triangle, with empty rows and columns at both ends,
    repeated (row, col) pairs, and some entries stored in both triangles; diag = "some" | "none" | "only"."""
    rng = np.random.RandomState(seed)
    gap = max(1, n // 16) if n >= 16 else 0
    a = rng.randint(gap, n - gap, nnz)
    b = np.where(rng.rand(nnz) < 0.5, rng.randint(gap, min(n - gap, gap + 8), nnz), rng.randint(gap, n - gap, nnz))
    rows, cols = np.maximum(a, b), np.minimum(a, b)
    if diag == "only":
        cols = rows.copy()
    elif diag == "none":
        keep = rows != cols
        rows, cols = rows[keep], cols[keep]
    else:
        flip = rng.rand(len(rows)) < 0.05                   # some entries from the other triangle
        rows, cols = np.where(flip, cols, rows), np.where(flip, rows, cols)
    if order == "row-sorted":
        p = np.argsort(rows, kind="stable")
    elif order == "column-major":
        p = np.argsort(cols.astype(np.int64) * n + rows, kind="stable")
    else:
        p = rng.permutation(len(rows))
    return rows[p].astype(np.int32), cols[p].astype(np.int32)


def values(nnz, kind, seed):
    rng = np.random.RandomState(seed)
    if VALS[kind] is None:
        return None
    if kind == "i32":
        return rng.randint(-2 ** 31, 2 ** 31 - 1, nnz).astype(np.int32)
    return rng.standard_normal(nnz).astype(np.float32 if kind == "f32" else np.float64)


def test_no_entries():
    e = np.empty(0, dtype=np.int32)
    for off in OFFS:
        assert check(0, e, e, None, off)[0].Ap.tolist() == [0]
        assert check(5, e, e, np.empty(0, dtype=np.float32), off)[0].Ap.tolist() == [0] * 6


def test_only_diagonal_entries_and_no_diagonal_entries():
    for diag in ("only", "none"):
        rows, cols = make_stored(3000, 50000, "shuffled", 5, diag)
        csr, perm = check(3000, rows, cols, values(len(rows), "f64", 5), "i64")
        assert csr.nnz == (len(rows) if diag == "only" else 2 * len(rows))


def test_one_row():
    """A 1 x 1 matrix holds diagonal entries only: no radix pass, the identity permutation."""
    z = np.zeros(10000, dtype=np.int32)
    csr, perm = check(1, z, z, values(10000, "f32", 1), "i32")
    assert torch.equal(perm, torch.arange(10000, device=DEV))


def test_an_entry_stored_in_both_triangles_gives_four_and_repeats_are_kept():
    rows = np.array([2, 0, 1, 2, 2, 1], dtype=np.int32)       # (2,0) (0,2) (1,1) (2,0) again (2,1) (1,1) again
    cols = np.array([0, 2, 1, 0, 1, 1], dtype=np.int32)
    vals = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    csr, perm = check(3, rows, cols, vals, "i64")
    assert csr.Ap.tolist() == [0, 3, 6, 10]
    assert csr.Aj.tolist() == [2, 2, 2, 1, 2, 1, 0, 0, 0, 1]
    assert csr.Ax.tolist() == [1.0, 2.0, 4.0, 3.0, 5.0, 6.0, 1.0, 2.0, 4.0, 5.0]
    assert perm.tolist() == [0, 1, 3, 2, 4, 5, 0, 1, 3, 4]


@pytest.mark.parametrize("order", ["shuffled", "row-sorted", "column-major"])
@pytest.mark.parametrize("n,nnz", [(255, 30000), (256, 30000), (257, 30000), (65536, 200000), (65537, 200000)])
def test_pass_count_edges_and_stored_orders(n, nnz, order):
    rows, cols = make_stored(n, nnz, order, seed=n + nnz)
    check(n, rows, cols, values(len(rows), "f32", 1), "i32")


@pytest.mark.parametrize("off", list(OFFS))
@pytest.mark.parametrize("val", list(VALS))
def test_types(off, val):
    for n, nnz in ((257, 5000), (65537, 123457)):
        rows, cols = make_stored(n, nnz, "shuffled", seed=nnz)
        check(n, rows, cols, values(len(rows), val, 2), off)


def test_rectangular_matrix_with_entries_inside_the_square():
    """n_rows != n_cols is allowed as long as every entry and its mirror fit (the loader's rule)."""
    rows, cols = make_stored(300, 20000, "shuffled", 8)
    check(300, rows, cols, values(len(rows), "f64", 8), "i64", n_cols=1000)
    check(1000, rows, cols, values(len(rows), "f64", 8), "i32", n_cols=300)


@pytest.mark.parametrize("off,val", [(o, v) for o in ("i32", "i64") for v in ("f32", "f64")])
def test_symmetric_golden_fixtures_through_load_mtx_stored(oracle, off, val):
    gold = json.load(open(os.path.join(GOLD, "golden.json")))
    tv = {"f32": torch.float32, "f64": torch.float64}[val]
    for name in ("sym4_real.mtx", "c1_1138_bus_standin.mtx"):
        path = os.path.join(GOLD, name)
        st = sp.load.load_mtx_stored(path, OFFS[off], tv, DEV)
        assert st.symmetric
        csr = sp.coo_to_csr(st.n_rows, st.n_cols, st.rows, st.cols, st.vals, OFFS[off], symmetric=True)
        g = gold[name]["struct"]
        assert (csr.n_rows, csr.n_cols, csr.nnz) == (g["n_rows"], g["n_cols"], g["nnz"]) and csr.nnz == st.nnz_expanded
        assert csr.Ap.tolist() == g["Ap"] and csr.Aj.tolist() == g["Aj"], name
        n_rows, n_cols, Ap, Aj, Ax = oracle.load_mtx(path, off, val)
        assert np.array_equal(csr.Ap.cpu().numpy(), Ap) and np.array_equal(csr.Aj.cpu().numpy(), Aj), name
        assert np.array_equal(csr.Ax.cpu().numpy().view(np.uint8), Ax.view(np.uint8)), name


@pytest.mark.parametrize("off,val", [(o, v) for o in ("i32", "i64") for v in ("f32", "f64")])
def test_load_mtx_device_equals_load_mtx_for_every_golden_file(off, val):
    tv = {"f32": torch.float32, "f64": torch.float64}[val]
    files = sorted(glob.glob(os.path.join(GOLD, "*.mtx")))
    assert len(files) >= 9
    for path in files:
        host = sp.load.load_mtx(path, OFFS[off], tv)
        dev = sp.load.load_mtx_device(path, OFFS[off], tv, DEV)
        assert (dev.n_rows, dev.n_cols, dev.nnz) == (host.n_rows, host.n_cols, host.nnz), path
        assert dev.Ap.dtype == host.Ap.dtype and dev.Ax.dtype == host.Ax.dtype
        assert torch.equal(dev.Ap.cpu(), host.Ap) and torch.equal(dev.Aj.cpu(), host.Aj), path
        assert np.array_equal(dev.Ax.cpu().numpy().view(np.uint8), host.Ax.numpy().view(np.uint8)), path


def test_perm_names_the_stored_entry_behind_every_slot():
    n = 70000
    rows, cols = make_stored(n, 400000, "column-major", 6)
    vals = values(len(rows), "f64", 6)
    csr, perm = check(n, rows, cols, vals, "i64")
    p = perm.cpu().numpy()
    assert np.array_equal(np_bits(vals[p]), np_bits(csr.Ax.cpu().numpy()))           # Ax = vals[perm]
    slot_row = np.repeat(np.arange(n), np.diff(csr.Ap.cpu().numpy()))
    slot_col = csr.Aj.cpu().numpy()
    direct = (rows[p] == slot_row) & (cols[p] == slot_col)
    mirrored = (rows[p] == slot_col) & (cols[p] == slot_row)
    assert bool((direct | mirrored).all())
    # every off-diagonal stored entry is behind exactly two slots, every diagonal one behind one
    assert np.array_equal(np.bincount(p, minlength=len(rows)), 1 + (rows != cols))


def test_lower_triangle_of_the_c4_stencil_in_column_major_order():
    """The C4 stand-in (27-point stencil on 203^3 points, 224 M entries, int64 offsets, fp64 values; its pattern is
    symmetric): its lower triangle with the diagonal, stored column-major, against the host expansion + ToCsr in numpy.
    Inside a row the entries come in the order of the expanded sequence, not by column, so the result is not the
    stencil's own CSR: numpy's expansion + stable sort says what it is."""
    m = sp.synth.workload("c4-nlpkkt", device=DEV)
    n = m.n_rows
    lens = (m.Ap[1:] - m.Ap[:-1]).long()
    csr_row = torch.repeat_interleave(torch.arange(n, device=DEV, dtype=torch.int32), lens)
    # column-major COO of a symmetric pattern: (row, col) = (Aj[k], CSR row of k); keep row >= col.  The values are
    # those of the upper-triangle slots: any values do, the call moves bits.
    keep = m.Aj >= csr_row
    d_rows, d_cols, d_vals = m.Aj[keep].contiguous(), csr_row[keep].contiguous(), m.Ax[keep].contiguous()
    del m, lens, csr_row, keep
    torch.cuda.empty_cache()
    rows, cols, vals = d_rows.cpu().numpy(), d_cols.cpu().numpy(), d_vals.cpu().numpy()
    assert bool((np.diff(cols.astype(np.int64) * n + rows) > 0).all())                # column-major, no repeats
    csr, perm = sp.coo_to_csr(n, n, d_rows, d_cols, d_vals, torch.int64, return_perm=True, symmetric=True)
    del d_rows, d_cols, d_vals
    got = [t.cpu().numpy() for t in (csr.Ap, csr.Aj, csr.Ax, perm)]
    del csr, perm
    torch.cuda.empty_cache()
    Ap, Aj, Ax, p = expected(n, rows, cols, vals, torch.int64)
    assert len(Aj) == 2 * len(rows) - n                                               # a full diagonal
    assert np.array_equal(got[0], Ap)
    assert np.array_equal(got[1], Aj)
    assert np.array_equal(np_bits(got[2]), np_bits(Ax))
    assert np.array_equal(got[3], p)


def _guarded(nbytes, guard, fill):
    t = torch.full((nbytes + 2 * guard,), fill, dtype=torch.uint8, device=DEV)
    return t, C.c_void_p(t.data_ptr() + guard)


def test_bad_arguments_are_refused_and_nothing_is_written():
    """A stored entry whose mirror falls outside a rectangular matrix, a negative index, and an nnz_expanded one too
    small and one too large: EINVAL, a message with the entry or the two counts, every output buffer (NaN-patterned
    bytes) and the guard bytes around it as they were.  Bad arguments, refused cleanly."""
    L = sp.capi.lib()
    n_rows, n_cols, guard, fill = 1000, 600, 4096, 0xFF          # 0xFF bytes: NaN as fp64, -1 as integers
    rows0, cols0 = make_stored(n_cols, 70000, "shuffled", 9)      # every index < 600: valid for 1000 x 600
    nnz = len(rows0)
    true_expanded = nnz + int((rows0 != cols0).sum())
    vals = torch.from_numpy(values(nnz, "f64", 9)).to(DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(rows, cols, expanded):
        ws_bytes = sp.capi.coo_to_csr_symmetric_workspace_bytes(n_rows, nnz, expanded, torch.int64, torch.float64)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        d_rows, d_cols = torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)
        bufs = [_guarded(8 * (n_rows + 1), guard, fill), _guarded(4 * expanded, guard, fill),
                _guarded(8 * expanded, guard, fill), _guarded(8 * expanded, guard, fill)]
        size = C.c_size_t(ws_bytes)
        st = L.mi355_spmv_coo_to_csr_symmetric(1, 1, n_rows, n_cols, nnz, expanded, C.c_void_p(d_rows.data_ptr()),
                                               C.c_void_p(d_cols.data_ptr()), C.c_void_p(vals.data_ptr()), bufs[0][1],
                                               bufs[1][1], bufs[2][1], bufs[3][1], C.c_void_p(ws.data_ptr()),
                                               C.byref(size), stream)
        msg = L.mi355_spmv_last_error().decode()
        torch.cuda.synchronize()
        untouched = all(bool((t == fill).all()) for t, _ in bufs)
        return st, msg, untouched

    st, msg, untouched = call(rows0, cols0, true_expanded)        # the valid call, for contrast: it does write
    assert st == 0 and not untouched, msg
    # (row 700, col 3) is inside 1000 x 600, its mirror (3, 700) is not; (5, 800) is outside by itself
    for where, r, c in ((4321, 700, 3), (60000, -1, 3), (123, 5, 800), (9, 3, -7)):
        rows, cols = rows0.copy(), cols0.copy()
        rows[where], cols[where] = r, c
        rows[where + 7] = n_rows + 5                               # a later bad entry: the message names the first one
        st, msg, untouched = call(rows, cols, true_expanded)
        assert st == 1, msg
        assert "entry %d is (row %d, col %d)" % (where, r, c) in msg, msg
        assert untouched
    for wrong in (true_expanded - 1, true_expanded + 1):
        st, msg, untouched = call(rows0, cols0, wrong)
        assert st == 1, msg
        assert str(wrong) in msg and str(true_expanded) in msg, msg
        assert untouched


def test_outputs_stay_inside_their_buffers():
    """A successful call writes exactly its outputs: guard bytes on both sides of each, and of the workspace, stay."""
    L = sp.capi.lib()
    n, guard = 70001, 4096
    rows, cols = make_stored(n, 250001, "column-major", 4)
    vals = values(len(rows), "f32", 4)
    Ap, Aj, Ax, perm = expected(n, rows, cols, vals, torch.int32)
    nnz, expanded = len(rows), len(Aj)
    ws_bytes = sp.capi.coo_to_csr_symmetric_workspace_bytes(n, nnz, expanded, torch.int32, torch.float32)
    sizes = [4 * (n + 1), 4 * expanded, 4 * expanded, 8 * expanded, ws_bytes]
    bufs = [torch.full((b + 2 * guard,), 0x5A, dtype=torch.uint8, device=DEV) for b in sizes]
    p = [C.c_void_p(t.data_ptr() + guard) for t in bufs]
    d = [torch.from_numpy(a).to(DEV) for a in (rows, cols, vals)]
    size = C.c_size_t(ws_bytes)
    st = L.mi355_spmv_coo_to_csr_symmetric(0, 0, n, n, nnz, expanded, C.c_void_p(d[0].data_ptr()),
                                           C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()), p[0], p[1], p[2],
                                           p[3], p[4], C.byref(size), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, L.mi355_spmv_last_error()
    for t, b in zip(bufs, sizes):
        assert bool((t[:guard] == 0x5A).all()) and bool((t[guard + b:] == 0x5A).all())
    out = lambda i, dt: bufs[i][guard:guard + sizes[i]].cpu().numpy().view(dt)
    assert np.array_equal(out(0, np.int32), Ap) and np.array_equal(out(1, np.int32), Aj)
    assert np.array_equal(out(2, np.uint32), np_bits(Ax)) and np.array_equal(out(3, np.int64), perm)


def test_two_runs_are_bitwise_equal():
    n = 1 << 20
    rows, cols = make_stored(n, 3 << 20, "shuffled", 12)
    cols[: 1 << 19] = 777                                         # a hub column: its mirrors make a hub row
    rows[: 1 << 19] = np.maximum(rows[: 1 << 19], 778)
    t = lambda a: torch.from_numpy(a).to(DEV)
    d_rows, d_cols, d_vals = t(rows), t(cols), t(values(len(rows), "f64", 12))
    a, pa = sp.coo_to_csr(n, n, d_rows, d_cols, d_vals, torch.int64, return_perm=True, symmetric=True)
    b, pb = sp.coo_to_csr(n, n, d_rows, d_cols, d_vals, torch.int64, return_perm=True, symmetric=True)
    assert torch.equal(a.Ap, b.Ap) and torch.equal(a.Aj, b.Aj) and torch.equal(pa, pb)
    assert torch.equal(a.Ax.view(torch.int64), b.Ax.view(torch.int64))


@pytest.mark.parametrize("kind", ["vector", "merge", "light"])
def test_plan_on_device_made_csr_gives_the_same_y_as_on_the_host_made_one(tmp_path, kind):
    """A symmetric Matrix Market file through the host loader (LoadCoo + ToCsr) and through load_mtx_device: a plan on
    either set of arrays gives y with the same bits."""
    rng = np.random.RandomState(21)
    n, nnz = 30000, 250000
    a, b = rng.randint(0, n, nnz), rng.randint(0, n, nnz)
    b[a % 97 == 3] = 5                                            # a long column, hence a long row
    r, c = np.maximum(a, b), np.minimum(a, b)
    v = rng.uniform(-1, 1, nnz)
    path = tmp_path / "m.mtx"
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real symmetric\n%d %d %d\n" % (n, n, nnz))
        np.savetxt(f, np.stack([r + 1, c + 1, v], 1), fmt="%d %d %.17g")
    host = sp.load.load_mtx(str(path), torch.int32, torch.float32, DEV)
    dev = sp.load.load_mtx_device(str(path), torch.int32, torch.float32, DEV)
    assert dev.nnz == host.nnz > nnz
    assert torch.equal(dev.Ap, host.Ap) and torch.equal(dev.Aj, host.Aj)
    assert torch.equal(dev.Ax.view(torch.int32), host.Ax.view(torch.int32))
    x = sp.synth.dense_vector(n, torch.float32, 21, DEV)
    ys = []
    for m in (host, dev):
        p = sp.Plan(kind, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32)
        y = torch.full((n,), float("nan"), device=DEV)
        p.execute(m.Ax, x, y)
        torch.cuda.synchronize()
        p.destroy()
        ys.append(y)
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))
