"""GPU suite: the structure of A^T on the device (mi355_spmv_csr_transpose, sp.csr_transpose) against numpy, exactly:
perm == argsort(Aj, kind="stable"), Ajt == rows[perm], Apt == cumsum(bincount(Aj, minlength=n_cols)).  Shapes: the
structures of tests/golden/*.mtx, a hub COLUMN (30 000 entries of one column spread over 30 000 rows), duplicate entries,
2 x 6 and 6 x 2, empty columns at both ends, every radix pass count of the column (1, 256 / 257, 65 537 columns), no rows,
no nonzeros, both offset widths."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import __graft_entry__
from conftest import GOLD, random_csr

pytestmark = pytest.mark.gpu
sp = __graft_entry__.load_package()
DEV = "cuda:0"
OFFS = {"i32": torch.int32, "i64": torch.int64}
NP_OFF = {"i32": np.int32, "i64": np.int64}


def expected(n_rows, n_cols, Ap, Aj):
    perm = np.argsort(Aj, kind="stable")
    rows = np.repeat(np.arange(n_rows, dtype=np.int32), np.diff(Ap.astype(np.int64)))
    Apt = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(Aj, minlength=n_cols), out=Apt[1:])
    return Apt.astype(Ap.dtype), rows[perm].astype(np.int32), perm.astype(np.int32)


def transpose(n_rows, n_cols, Ap, Aj):
    return sp.csr_transpose(n_rows, n_cols, torch.from_numpy(Ap).to(DEV), torch.from_numpy(Aj).to(DEV))


def check(n_rows, n_cols, Ap, Aj):
    """Two calls, both equal to numpy's stable sort by column; returns the device outputs."""
    want = expected(n_rows, n_cols, Ap, Aj)
    first = transpose(n_rows, n_cols, Ap, Aj)
    second = transpose(n_rows, n_cols, Ap, Aj)
    for name, w, a, b in zip(("Apt", "Ajt", "perm"), want, first, second):
        assert a.dtype == torch.from_numpy(w).dtype and np.array_equal(a.cpu().numpy(), w), name
        assert torch.equal(a, b), name + " differs between two calls"
    return first


def shapes():
    rng = np.random.RandomState(5)
    out = {}
    out["rect2x6"] = (2, 6, np.array([0, 4, 7]), np.array([5, 0, 3, 0, 1, 5, 2], dtype=np.int32))
    out["rect6x2"] = (6, 2, np.array([0, 1, 1, 3, 4, 4, 7]), np.array([1, 0, 1, 0, 1, 1, 0], dtype=np.int32))
    # one column holds an entry of every one of 30 000 rows, between ragged others
    n = 30000
    lens = rng.randint(0, 3, size=n) + 1
    Ap = np.concatenate(([0], np.cumsum(lens)))
    Aj = rng.randint(0, 500, size=int(Ap[-1])).astype(np.int32)
    Aj[Ap[:-1] + rng.randint(0, 1 << 30, size=n) % lens] = 77
    out["hub_column"] = (n, 500, Ap, Aj)
    Ap, Aj, _ = random_csr(rng, 400, 9, 12)                   # few columns: duplicate (row, column) pairs, unsorted rows
    out["duplicates"] = (400, 9, Ap, Aj)
    Ap, Aj, _ = random_csr(rng, 700, 300, 9)                  # columns 0 .. 19 and 280 .. 299 stay empty
    out["empty_columns_at_both_ends"] = (700, 300, Ap, (Aj % 260 + 20).astype(np.int32))
    for n_cols in (1, 256, 257, 65537):                       # 0, 1, 2 and 3 radix passes
        Ap, Aj, _ = random_csr(rng, 900, n_cols, 20, long_row=3000)
        out["cols_%d" % n_cols] = (900, n_cols, Ap, Aj)
    out["no_rows"] = (0, 7, np.array([0]), np.zeros(0, dtype=np.int32))
    out["no_nonzeros"] = (5, 3, np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32))
    out["no_columns"] = (4, 0, np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.int32))
    return out


SHAPES = shapes()


@pytest.mark.parametrize("off", list(OFFS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_against_a_stable_sort_by_column(name, off):
    n_rows, n_cols, Ap, Aj = SHAPES[name]
    assert np.bincount(Aj, minlength=1).max() >= 30000 or name != "hub_column"
    check(n_rows, n_cols, Ap.astype(NP_OFF[off]), Aj)


@pytest.mark.parametrize("off", list(OFFS))
def test_golden_fixture_structures(off):
    paths = sorted(glob.glob(os.path.join(GOLD, "*.mtx")))
    assert paths
    for path in paths:
        coo = sp.load.load_mtx_coo(path, OFFS[off], torch.float32, DEV)
        m = sp.coo_to_csr(coo.n_rows, coo.n_cols, coo.rows, coo.cols, coo.vals, OFFS[off])
        check(m.n_rows, m.n_cols, m.Ap.cpu().numpy(), m.Aj.cpu().numpy())


def test_the_workspace_query_touches_no_device():
    for n_cols, nnz in ((1, 10), (300, 0), (300, 100000), (70000, 5)):
        assert sp.capi.csr_transpose_workspace_bytes(n_cols, nnz) == sp.capi.coo_to_csr_workspace_bytes(n_cols, nnz) >= 256
    ws = C.c_size_t(0)      # sizes are refused in the query too
    assert sp.capi.lib().mi355_spmv_csr_transpose(0, 4, 4, 2 ** 31, None, None, None, None, None, None, C.byref(ws), None) == 1
    assert sp.capi.lib().mi355_spmv_csr_transpose(1, 4, 4, 2 ** 32, None, None, None, None, None, None, C.byref(ws), None) == 2


def call_with_canaries(n_rows, n_cols, Ap, Aj):
    Apt = torch.full((n_cols + 1,), -7, dtype=Ap.dtype, device=DEV)
    Ajt = torch.full((Aj.numel(),), -7, dtype=torch.int32, device=DEV)
    perm = torch.full((Aj.numel(),), -7, dtype=torch.int32, device=DEV)
    nbytes = sp.capi.csr_transpose_workspace_bytes(n_cols, Aj.numel(), Ap.dtype)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    size = C.c_size_t(nbytes)
    st = sp.capi.lib().mi355_spmv_csr_transpose(sp.capi.OFF_TYPES[Ap.dtype][0], n_rows, n_cols, Aj.numel(), C.c_void_p(Ap.data_ptr()),
                                                C.c_void_p(Aj.data_ptr()), C.c_void_p(Apt.data_ptr()), C.c_void_p(Ajt.data_ptr()),
                                                C.c_void_p(perm.data_ptr()), C.c_void_p(ws.data_ptr()), C.byref(size), None)
    torch.cuda.synchronize()
    untouched = all(bool((t == -7).all()) for t in (Apt, Ajt, perm))
    return st, sp.capi.lib().mi355_spmv_last_error().decode(), untouched


@pytest.mark.parametrize("off", list(OFFS))
def test_a_bad_column_or_offset_is_refused_and_nothing_is_written(off):
    n_rows, n_cols, Ap, Aj = SHAPES["duplicates"]
    Ap = torch.from_numpy(Ap.astype(NP_OFF[off])).to(DEV)
    Aj = torch.from_numpy(Aj).to(DEV)
    for where, col in ((600, n_cols), (77, -1)):
        bad = Aj.clone()
        bad[where], bad[where + 500] = col, n_cols + 3      # the first offender is the one named
        st, text, untouched = call_with_canaries(n_rows, n_cols, Ap, bad)
        assert st == 1 and untouched, text
        assert "entry %d of Aj is column %d" % (where, col) in text, text
    for where in (0, 200, n_rows):
        bad = Ap.clone()
        bad[where] = bad[where] + 1 if where in (0, n_rows) else bad[where - 1] - 1
        st, text, untouched = call_with_canaries(n_rows, n_cols, bad, Aj)
        assert st == 1 and untouched, text
        assert "Ap[%d]" % where in text, text
    st, text, untouched = call_with_canaries(n_rows, n_cols, Ap, Aj)
    assert st == 0 and not untouched, text


@pytest.mark.parametrize("off", list(OFFS))
def test_transposing_twice_returns_the_matrix(off):
    """Sorted, duplicate-free rows: (A^T)^T is A, slot for slot, and the two slot maps compose to the identity."""
    rng = np.random.RandomState(31)
    n_rows, n_cols = 500, 260
    cols = [np.sort(rng.choice(n_cols, size=rng.randint(0, 40), replace=False)) for _ in range(n_rows)]
    Ap = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(NP_OFF[off])
    Aj = np.concatenate(cols).astype(np.int32)
    Apt, Ajt, perm = check(n_rows, n_cols, Ap, Aj)
    Ap2, Aj2, perm2 = sp.csr_transpose(n_cols, n_rows, Apt, Ajt)
    assert np.array_equal(Ap2.cpu().numpy(), Ap) and np.array_equal(Aj2.cpu().numpy(), Aj)
    assert torch.equal(perm[perm2.long()], torch.arange(len(Aj), dtype=torch.int32, device=DEV))
