"""CPU suite: the file as stored (mi355_load_mtx_stored, sp.load.load_mtx_stored) and the size query and argument
checks of the symmetric device COO -> CSR call (mi355_spmv_coo_to_csr_symmetric), none of which needs a GPU.
Expanding the stored entries by LoadCoo's rule (reference include/load.hpp:362-403: entry, then its mirror if it is off
the diagonal) must give load_mtx_coo's arrays entry for entry."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

FIXTURES = sorted(glob.glob(os.path.join(GOLD, "*.mtx")))
TYPES = [(o, v) for o in ("i32", "i64") for v in ("f32", "f64")]
TORCH = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "f64": torch.float64}


def banner_symmetry(path):
    return open(path).readline().split()[4].lower()


def expand(rows, cols, vals):
    """LoadCoo's expansion of the stored entries of a symmetric file, in numpy."""
    reps = 1 + (rows != cols)
    src = np.repeat(np.arange(len(rows)), reps)
    mirror = np.zeros(len(src), dtype=bool)
    mirror[np.cumsum(reps)[reps == 2] - 1] = True
    return np.where(mirror, cols[src], rows[src]), np.where(mirror, rows[src], cols[src]), vals[src]


def test_expand_helper_on_a_hand_made_case():
    r, c, v = expand(np.array([2, 1, 2]), np.array([0, 1, 1]), np.array([2.5, 1.0, 4.0]))
    assert r.tolist() == [2, 0, 1, 2, 1] and c.tolist() == [0, 2, 1, 1, 2] and v.tolist() == [2.5, 2.5, 1.0, 4.0, 4.0]


@pytest.mark.parametrize("off,val", TYPES)
@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_load_mtx_stored_then_the_expansion_rule_is_load_mtx_coo(sp, path, off, val):
    st = sp.load.load_mtx_stored(path, TORCH[off], TORCH[val])
    coo = sp.load.load_mtx_coo(path, TORCH[off], TORCH[val])
    rows, cols, vals = st.rows.numpy(), st.cols.numpy(), st.vals.numpy()
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.dtype(val.replace("f", "float"))
    assert len(rows) == len(cols) == len(vals) == st.nnz
    assert (st.n_rows, st.n_cols) == (coo.n_rows, coo.n_cols)
    assert st.symmetric == (banner_symmetry(path) == "symmetric")
    assert st.nnz_expanded == coo.nnz
    if st.symmetric:
        assert st.nnz_expanded == st.nnz + int((rows != cols).sum())
        rows, cols, vals = expand(rows, cols, vals)
    else:
        assert st.nnz_expanded == st.nnz
    assert np.array_equal(rows, coo.rows.numpy()) and np.array_equal(cols, coo.cols.numpy())
    assert np.array_equal(vals.view(np.uint8), coo.vals.numpy().view(np.uint8))


def test_symmetric_fixtures_are_expanded_and_the_skew_one_is_not(sp):
    sym = sp.load.load_mtx_stored(os.path.join(GOLD, "sym4_real.mtx"))
    assert sym.symmetric and (sym.nnz, sym.nnz_expanded) == (5, 8)       # two of the five are diagonal (golden.json: nnz 8)
    bus = sp.load.load_mtx_stored(os.path.join(GOLD, "c1_1138_bus_standin.mtx"))
    assert bus.symmetric and bus.nnz < bus.nnz_expanded == 4054
    skew = sp.load.load_mtx_stored(os.path.join(GOLD, "skew3_not_expanded.mtx"))
    assert banner_symmetry(os.path.join(GOLD, "skew3_not_expanded.mtx")) == "skew-symmetric"
    assert not skew.symmetric and skew.nnz == skew.nnz_expanded == 2
    assert bool((skew.rows != skew.cols).all())                         # off-diagonal entries, and still not counted


def test_load_mtx_stored_keeps_file_order_and_pattern_values(sp, tmp_path):
    p = tmp_path / "sym.mtx"
    p.write_text("%%MatrixMarket matrix coordinate pattern symmetric\n3 3 4\n3 1\n2 2\n3 2\n3 1\n")
    st = sp.load.load_mtx_stored(str(p), val_dtype=torch.float64)
    assert st.rows.tolist() == [2, 1, 2, 2] and st.cols.tolist() == [0, 1, 1, 0] and st.vals.tolist() == [1.0] * 4
    assert st.symmetric and (st.nnz, st.nnz_expanded) == (4, 7)
    h = tmp_path / "herm.mtx"
    h.write_text("%%MatrixMarket matrix coordinate real hermitian\n2 2 2\n2 1 3\n1 1 1\n")
    st = sp.load.load_mtx_stored(str(h))
    assert not st.symmetric and (st.nnz, st.nnz_expanded) == (2, 2)


def test_load_mtx_stored_errors_are_those_of_the_other_entry_points(sp, tmp_path):
    L = sp.load.lib()
    h, sym, n = C.c_void_p(), C.c_int(), C.c_int64()
    call = lambda path, off=0, val=0, out=C.byref(h), s=C.byref(sym), e=C.byref(n): \
        L.mi355_load_mtx_stored(path, off, val, out, s, e)
    assert call(None) == 1 and call(FIXTURES[0].encode(), val=7) == 1 and call(FIXTURES[0].encode(), off=2) == 1
    assert call(FIXTURES[0].encode(), s=None) == 1 and call(FIXTURES[0].encode(), e=None) == 1
    assert call(b"/nonexistent/none.mtx") == 2
    bad = tmp_path / "bad.mtx"
    bad.write_text("%%MatrixMarket matrix coordinate real general\n2 2 1\n3 1 1.0\n")
    assert call(str(bad).encode()) == 3 and b"beyond" in L.mi355_load_last_error()
    # a symmetric file whose mirror would fall outside a rectangular matrix: refused as by load_mtx_coo
    rect = tmp_path / "rect.mtx"
    rect.write_text("%%MatrixMarket matrix coordinate real symmetric\n2 4 1\n1 3 1.0\n")
    assert call(str(rect).encode()) == 3
    hc = C.c_void_p()
    assert L.mi355_load_mtx_coo(str(rect).encode(), 0, 0, C.byref(hc)) == 3
    with pytest.raises(RuntimeError, match="could not be opened"):
        sp.load.load_mtx_stored("/nonexistent/none.mtx")


def _query(L, off, val, n_rows, nnz_stored, nnz_expanded):
    ws = C.c_size_t(0)
    st = L.mi355_spmv_coo_to_csr_symmetric(off, val, n_rows, 4, nnz_stored, nnz_expanded, None, None, None, None,
                                           None, None, None, None, C.byref(ws), None)
    assert st == 0, L.mi355_spmv_last_error()
    return ws.value


def test_symmetric_size_query_needs_no_device(sp):
    """workspace == NULL: the byte count, and OK, with nothing on the device (this box has none)."""
    L = sp.capi.lib()
    size = lambda n_rows, stored, expanded: _query(L, 1, 0, n_rows, stored, expanded)
    s = 10 ** 6
    assert size(0, 0, 0) > 0
    prev = 0
    for e in (s, s + 1, s + 4096, 3 * s // 2, 2 * s):                  # monotone in nnz_expanded
        now = size(1 << 20, s, e)
        assert now >= prev and now > 8 * e                              # a key and a payload per expanded entry, at least
        prev = now
    assert size(1 << 20, s, 2 * s) > size(1 << 20, s, s)
    # equal across n_rows that need the same number of radix passes
    assert size(2, s, 2 * s) == size(256, s, 2 * s)                     # one
    assert size(257, s, 2 * s) == size(65536, s, 2 * s)                 # two
    assert size(65537, s, 2 * s) == size(1 << 24, s, 2 * s)             # three
    assert size(1, s, s) < size(2, s, s)                                # one row: no pass, no sort buffers
    assert sp.capi.coo_to_csr_symmetric_workspace_bytes(1 << 20, s, 2 * s, torch.int64) == size(1 << 20, s, 2 * s)


def test_plain_size_query_is_what_it_was(sp):
    """mi355_spmv_coo_to_csr's workspace for the shapes tests/test_coo_cpu.py names, by its documented layout: the
    256-byte validation word, one or two key / payload pairs, 256 counts per 4 096-entry tile, the scan's sums."""
    up = lambda v: (v + 255) // 256 * 256
    for n_rows, nnz, passes in ((1, 10 ** 6, 0), (256, 10 ** 6, 1), (257, 10 ** 6, 2), (1 << 24, 2 * 10 ** 6, 3)):
        want = 256
        if passes:
            tiles = (nnz + 4095) // 4096
            want += (4 if passes > 1 else 2) * up(4 * nnz) + up(4 * 256 * tiles) + up(4 * ((256 * tiles + 4095) // 4096))
        assert sp.capi.coo_to_csr_workspace_bytes(n_rows, nnz, torch.int64) == want


def test_symmetric_call_rejects_bad_arguments_without_touching_the_device(sp):
    L = sp.capi.lib()
    d = C.c_void_p(256)          # never dereferenced: every case fails before anything is enqueued
    big = C.c_size_t(1 << 40)

    def call(off=1, val=0, n_rows=4, n_cols=4, stored=4, expanded=6, rows=d, cols=d, vals=d, Ap=d, Aj=d, Ax=d, ws=d,
             ws_bytes=big):
        return L.mi355_spmv_coo_to_csr_symmetric(off, val, n_rows, n_cols, stored, expanded, rows, cols, vals, Ap, Aj,
                                                 Ax, None, ws, C.byref(ws_bytes) if ws_bytes is not None else None, None)

    err = L.mi355_spmv_last_error
    assert call(off=2) == 1 and call(val=3) == 1                                   # bad enums
    assert call(n_rows=-1) == 1 and call(n_cols=-1) == 1                           # negative sizes
    assert call(stored=-1, expanded=0) == 1 and call(stored=4, expanded=-1) == 1
    assert call(stored=4, expanded=3) == 1 and b"nnz_expanded" in err()            # fewer than stored
    assert call(stored=4, expanded=9) == 1 and b"nnz_expanded" in err()            # more than twice the stored
    assert call(stored=0, expanded=1) == 1
    assert call(stored=4, expanded=3, ws=None) == 1                                # the size query checks sizes too
    assert call(rows=None) == 1 and call(cols=None) == 1 and call(Aj=None) == 1 and call(Ap=None) == 1
    assert call(ws_bytes=None) == 1
    assert call(vals=None) == 1 and b"Ax" in err()                                 # Ax given, vals NULL
    assert call(Ax=None) == 1 and b"Ax" in err()                                   # vals given, Ax NULL
    assert call(ws_bytes=C.c_size_t(16)) == 1 and b"workspace" in err()
    assert call(off=0, stored=2 ** 30, expanded=2 ** 31) == 1 and b"32-bit offsets" in err()
    assert call(off=0, stored=2 ** 30, expanded=2 ** 31, ws=None) == 1
    assert call(off=0, stored=2 ** 30, expanded=2 ** 31 - 1, ws=None) == 0
    assert call(off=1, stored=2 ** 31, expanded=2 ** 32) == 2 and b"2^32" in err()  # the sort's counters are 32-bit
    assert call(off=1, stored=2 ** 31, expanded=2 ** 32, ws=None) == 2
    assert call(off=1, stored=2 ** 31, expanded=2 ** 31, ws=None) == 2 and b"stored" in err()
    assert call(off=1, stored=2 ** 31 - 1, expanded=2 ** 32 - 2, ws=None) == 0
    out = C.c_int64(-1)
    assert L.mi355_spmv_coo_symmetric_nnz(-1, d, d, None, C.byref(out)) == 1
    assert L.mi355_spmv_coo_symmetric_nnz(4, None, d, None, C.byref(out)) == 1
    assert L.mi355_spmv_coo_symmetric_nnz(4, d, d, None, None) == 1
    assert L.mi355_spmv_coo_symmetric_nnz(0, None, None, None, C.byref(out)) == 0 and out.value == 0   # nothing to count


def test_bindings_refuse_host_tensors(sp):
    r = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        sp.coo_to_csr(4, 4, r, r, symmetric=True)
    with pytest.raises(RuntimeError, match="device tensors"):
        sp.coo_symmetric_nnz(r, r)
    with pytest.raises(RuntimeError, match="device tensors"):
        sp.load.load_mtx_device(os.path.join(GOLD, "sym4_real.mtx"), device="cpu")
