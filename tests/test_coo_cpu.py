"""CPU suite: the COO entry points of the Matrix Market loader (mi355_load_mtx_coo) and the device COO -> CSR call's
size query and argument checks, none of which needs a GPU.  A stable sort of the loaded COO by row is the CSR the
reference's ToCsr makes (tests/golden/golden.json, oracle.load_mtx, mi355_load_mtx)."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

FIXTURES = sorted(glob.glob(os.path.join(GOLD, "*.mtx")))
TYPES = [(o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
TORCH = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "f64": torch.float64}


@pytest.mark.parametrize("off,val", TYPES)
@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_load_mtx_coo_then_stable_row_sort_is_the_loaders_csr(sp, oracle, path, off, val):
    gold = json.load(open(os.path.join(GOLD, "golden.json")))
    coo = sp.load.load_mtx_coo(path, TORCH[off], TORCH[val])
    rows, cols, vals = coo.rows.numpy(), coo.cols.numpy(), coo.vals.numpy()
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.dtype(val.replace("f", "float"))
    assert len(rows) == len(cols) == len(vals) == coo.nnz
    order = np.argsort(rows, kind="stable")
    Ap = np.zeros(coo.n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=coo.n_rows), out=Ap[1:])
    Aj, Ax = cols[order], vals[order]

    n_rows, n_cols, oAp, oAj, oAx = oracle.load_mtx(path, off, val)
    assert (coo.n_rows, coo.n_cols) == (n_rows, n_cols)
    assert np.array_equal(Ap, oAp) and np.array_equal(Aj, oAj) and np.array_equal(Ax, oAx)
    m = sp.load.load_mtx(path, TORCH[off], TORCH[val])
    assert (m.n_rows, m.n_cols, m.nnz) == (coo.n_rows, coo.n_cols, coo.nnz)
    assert np.array_equal(m.Ap.numpy(), Ap) and np.array_equal(m.Aj.numpy(), Aj) and np.array_equal(m.Ax.numpy(), Ax)
    case = gold.get(os.path.basename(path))
    if case is not None:
        st = case["struct"]
        assert (coo.n_rows, coo.n_cols, coo.nnz) == (st["n_rows"], st["n_cols"], st["nnz"])
        assert Ap.tolist() == st["Ap"] and Aj.tolist() == st["Aj"]


def test_load_mtx_coo_keeps_file_order_and_mirrors_after_the_entry(sp, tmp_path):
    p = tmp_path / "sym.mtx"
    p.write_text("%%MatrixMarket matrix coordinate real symmetric\n3 3 3\n3 1 2.5\n2 2 1\n3 2 4\n")
    coo = sp.load.load_mtx_coo(str(p), val_dtype=torch.float64)
    assert coo.rows.tolist() == [2, 0, 1, 2, 1]
    assert coo.cols.tolist() == [0, 2, 1, 1, 2]
    assert coo.vals.tolist() == [2.5, 2.5, 1.0, 4.0, 4.0]


def test_load_mtx_coo_errors_are_those_of_load_mtx(sp, tmp_path):
    L = sp.load.lib()
    h = C.c_void_p()
    assert L.mi355_load_mtx_coo(None, 0, 0, C.byref(h)) == 1
    assert L.mi355_load_mtx_coo(b"/nonexistent/none.mtx", 0, 0, C.byref(h)) == 2
    assert L.mi355_load_mtx_coo(FIXTURES[0].encode(), 0, 7, C.byref(h)) == 1
    bad = tmp_path / "bad.mtx"
    bad.write_text("%%MatrixMarket matrix coordinate real general\n2 2 1\n3 1 1.0\n")
    assert L.mi355_load_mtx_coo(str(bad).encode(), 0, 0, C.byref(h)) == 3
    assert b"beyond" in L.mi355_load_last_error()
    with pytest.raises(RuntimeError, match="could not be opened"):
        sp.load.load_mtx_coo("/nonexistent/none.mtx")


def test_coo_to_csr_size_query_needs_no_device(sp):
    """workspace == NULL: the byte count, and OK, with nothing on the device (this box has none)."""
    L = sp.capi.lib()
    size = lambda n_rows, nnz, off=1: _query(L, off, 0, n_rows, 4, nnz)
    assert size(0, 0) == size(1, 10 ** 6) == size(5, 0) > 0                  # no pass: the validation word only
    one, two, three = size(256, 10 ** 6), size(257, 10 ** 6), size(1 << 24, 10 ** 6)
    assert 8 * 10 ** 6 < one < two == three                                   # one key / payload buffer pair, then two
    assert size(1 << 24, 2 * 10 ** 6) > three
    assert sp.capi.coo_to_csr_workspace_bytes(1 << 20, 3 * 10 ** 6, torch.int64) == size(1 << 20, 3 * 10 ** 6)


def _query(L, off, val, n_rows, n_cols, nnz):
    ws = C.c_size_t(0)
    st = L.mi355_spmv_coo_to_csr(off, val, n_rows, n_cols, nnz, None, None, None, None, None, None, None, None,
                                 C.byref(ws), None)
    assert st == 0, L.mi355_spmv_last_error()
    return ws.value


def test_coo_to_csr_rejects_bad_arguments_without_touching_the_device(sp):
    L = sp.capi.lib()
    d = C.c_void_p(256)          # never dereferenced: every case fails before anything is enqueued
    big = C.c_size_t(1 << 40)

    def call(off=1, val=0, n_rows=4, n_cols=4, nnz=4, rows=d, cols=d, vals=d, Ap=d, Aj=d, Ax=d, ws=d, ws_bytes=big):
        return L.mi355_spmv_coo_to_csr(off, val, n_rows, n_cols, nnz, rows, cols, vals, Ap, Aj, Ax, None, ws,
                                       C.byref(ws_bytes) if ws_bytes is not None else None, None)

    assert call(off=2) == 1 and call(val=3) == 1
    assert call(n_rows=-1) == 1 and call(n_cols=-1) == 1 and call(nnz=-1) == 1
    assert call(rows=None) == 1 and call(cols=None) == 1 and call(Aj=None) == 1 and call(Ap=None) == 1
    assert call(ws_bytes=None) == 1
    assert call(vals=None) == 1 and b"Ax" in L.mi355_spmv_last_error()          # Ax given, vals NULL
    assert call(Ax=None) == 1                                                   # vals given, Ax NULL
    assert call(ws_bytes=C.c_size_t(16)) == 1 and b"workspace" in L.mi355_spmv_last_error()
    assert call(off=0, nnz=2 ** 31) == 1 and b"32-bit offsets" in L.mi355_spmv_last_error()
    assert call(off=0, nnz=2 ** 31, ws=None) == 1                               # the size query checks sizes too
    assert call(off=1, nnz=2 ** 32) == 2 and call(off=1, nnz=2 ** 32, ws=None) == 2
    assert call(off=1, nnz=2 ** 32 - 1, ws=None) == 0


def test_coo_to_csr_binding_refuses_host_tensors(sp):
    r = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        sp.coo_to_csr(4, 4, r, r)
