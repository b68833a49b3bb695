"""ctypes binding of libmi355load.so (include/mi355_load.h): Matrix Market file -> CSR, through the product loader
(host/load.hpp: the reference's LoadCoo + ToCsr, include/load.hpp:268-474, main.cu:32-39), or -> the COO before
ToCsr (load_mtx_coo), or -> the entries as the file stores them (load_mtx_stored).  Host code only, except
load_mtx_device, which hands the stored entries to the device COO -> CSR of capi.py."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from .synth import Csr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355_LOAD_LIB") or os.path.join(_HERE, "lib", "libmi355load.so")
EXPORTS = ["mi355_load_mtx", "mi355_csr_host_dims", "mi355_csr_host_Ap", "mi355_csr_host_Aj", "mi355_csr_host_Ax",
           "mi355_csr_host_free", "mi355_load_last_error",
           "mi355_load_mtx_coo", "mi355_load_coo_dims", "mi355_load_coo_rows", "mi355_load_coo_cols",
           "mi355_load_coo_vals", "mi355_load_coo_free", "mi355_load_mtx_stored"]
STATUS = {1: "invalid argument", 2: "not a usable Matrix Market coordinate file", 3: "malformed entry",
          4: "does not fit the index / offset types"}
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: build it (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.mi355_load_mtx.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.mi355_csr_host_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        for f in (L.mi355_csr_host_Ap, L.mi355_csr_host_Aj, L.mi355_csr_host_Ax):
            f.argtypes = [C.c_void_p]
            f.restype = C.c_void_p
        L.mi355_csr_host_free.argtypes = [C.c_void_p]
        L.mi355_csr_host_free.restype = None
        L.mi355_load_last_error.restype = C.c_char_p
        L.mi355_load_mtx_coo.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.mi355_load_coo_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        for f in (L.mi355_load_coo_rows, L.mi355_load_coo_cols, L.mi355_load_coo_vals):
            f.argtypes = [C.c_void_p]
            f.restype = C.c_void_p
        L.mi355_load_coo_free.argtypes = [C.c_void_p]
        L.mi355_load_coo_free.restype = None
        L.mi355_load_mtx_stored.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int64)]
        _lib = L
    return _lib


def _view(ptr, count, dt):
    """A copy of `count` elements of dtype `dt` at host address `ptr`."""
    if count == 0 or not ptr:
        return np.zeros(count, dtype=dt)
    buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dt, count=count).copy()


@dataclass
class Coo:
    """A Matrix Market file as LoadCoo leaves it: entries in file order (`symmetric` expanded entry-then-mirror)."""
    n_rows: int
    n_cols: int
    nnz: int
    rows: torch.Tensor   # int32
    cols: torch.Tensor   # int32
    vals: torch.Tensor   # float32 or float64


def _take_coo(L, h, val_dtype):
    """(n_rows, n_cols, nnz, rows, cols, vals) of a mi355_coo_host as numpy copies."""
    nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
    L.mi355_load_coo_dims(h, C.byref(nr), C.byref(nc), C.byref(nnz))
    n = nnz.value
    rows = _view(L.mi355_load_coo_rows(h), n, np.int32)
    cols = _view(L.mi355_load_coo_cols(h), n, np.int32)
    vals = _view(L.mi355_load_coo_vals(h), n, np.float64 if val_dtype == torch.float64 else np.float32)
    return nr.value, nc.value, n, rows, cols, vals


def load_mtx_coo(path, off_dtype=torch.int32, val_dtype=torch.float32, device="cpu"):
    """The file as the reference's LoadCoo gives it, before ToCsr (mi355_load_mtx_coo), as a Coo on `device`;
    sp.coo_to_csr then builds the CSR on the GPU.  off_dtype only decides which sizes fit, as for load_mtx."""
    L = lib()
    h = C.c_void_p()
    st = L.mi355_load_mtx_coo(os.fsencode(path), 1 if off_dtype == torch.int64 else 0,
                              1 if val_dtype == torch.float64 else 0, C.byref(h))
    if st != 0:
        raise RuntimeError("mi355_load_mtx_coo(%s): %s (%s)" % (path, STATUS.get(st, st),
                                                                L.mi355_load_last_error().decode()))
    try:
        n_rows, n_cols, n, rows, cols, vals = _take_coo(L, h, val_dtype)
    finally:
        L.mi355_load_coo_free(h)
    t = lambda a: torch.from_numpy(a).to(device)
    return Coo(n_rows, n_cols, n, t(rows), t(cols), t(vals))


@dataclass
class StoredCoo(Coo):
    """A Matrix Market file as it is stored: entries in file order, a `symmetric` file's entries not mirrored."""
    symmetric: bool = False      # the banner says `symmetric` (skew-symmetric / hermitian: False, not expanded)
    nnz_expanded: int = 0        # entries LoadCoo makes of it: nnz + the off-diagonal ones if symmetric, else nnz


def load_mtx_stored(path, off_dtype=torch.int32, val_dtype=torch.float32, device="cpu"):
    """The file as stored (mi355_load_mtx_stored), as a StoredCoo on `device`: what
    sp.coo_to_csr(..., symmetric=stored.symmetric) turns into the loader's CSR on the GPU."""
    L = lib()
    h = C.c_void_p()
    sym, expanded = C.c_int(0), C.c_int64(0)
    st = L.mi355_load_mtx_stored(os.fsencode(path), 1 if off_dtype == torch.int64 else 0,
                                 1 if val_dtype == torch.float64 else 0, C.byref(h), C.byref(sym), C.byref(expanded))
    if st != 0:
        raise RuntimeError("mi355_load_mtx_stored(%s): %s (%s)" % (path, STATUS.get(st, st),
                                                                   L.mi355_load_last_error().decode()))
    try:
        n_rows, n_cols, n, rows, cols, vals = _take_coo(L, h, val_dtype)
    finally:
        L.mi355_load_coo_free(h)
    t = lambda a: torch.from_numpy(a).to(device)
    return StoredCoo(n_rows, n_cols, n, t(rows), t(cols), t(vals), bool(sym.value), expanded.value)


def load_mtx_device(path, off_dtype=torch.int32, val_dtype=torch.float32, device="cuda:0"):
    """load_mtx with the CSR built on the GPU: the file is parsed on the host, its STORED entries are uploaded and
    mi355_spmv_coo_to_csr (or, for a symmetric file, mi355_spmv_coo_to_csr_symmetric) makes the arrays — element for
    element those of load_mtx(path, ...).  `device` must be a GPU: there is no host path here."""
    from . import capi
    if torch.device(device).type != "cuda":
        raise RuntimeError("mi355 spmv takes device tensors only (no CPU path exists)")
    coo = load_mtx_stored(path, off_dtype, val_dtype, device)
    csr = capi.coo_to_csr(coo.n_rows, coo.n_cols, coo.rows, coo.cols, coo.vals, off_dtype, symmetric=coo.symmetric)
    if csr.nnz != coo.nnz_expanded:
        raise RuntimeError("load_mtx_device(%s): the device expanded to %d entries, the loader counted %d"
                           % (path, csr.nnz, coo.nnz_expanded))
    return Csr(csr.n_rows, csr.n_cols, csr.nnz, csr.Ap, csr.Aj, csr.Ax, os.path.basename(path),
               {"synthetic": False, "path": str(path)})


def load_mtx(path, off_dtype=torch.int32, val_dtype=torch.float32, device="cpu"):
    """The file as the reference's harness would hold it after LoadCoo + ToCsr, as a synth.Csr on `device`."""
    L = lib()
    h = C.c_void_p()
    st = L.mi355_load_mtx(os.fsencode(path), 1 if off_dtype == torch.int64 else 0, 1 if val_dtype == torch.float64 else 0,
                          C.byref(h))
    if st != 0:
        raise RuntimeError("mi355_load_mtx(%s): %s (%s)" % (path, STATUS.get(st, st), L.mi355_load_last_error().decode()))
    try:
        nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        L.mi355_csr_host_dims(h, C.byref(nr), C.byref(nc), C.byref(nnz))
        n_rows, n_cols, n = nr.value, nc.value, nnz.value
        np_off = np.int64 if off_dtype == torch.int64 else np.int32
        np_val = np.float64 if val_dtype == torch.float64 else np.float32

        def view(ptr, count, dt):
            if count == 0 or not ptr:
                return np.zeros(count, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt, count=count).copy()
        Ap = view(L.mi355_csr_host_Ap(h), n_rows + 1, np_off)
        Aj = view(L.mi355_csr_host_Aj(h), n, np.int32)
        Ax = view(L.mi355_csr_host_Ax(h), n, np_val)
    finally:
        L.mi355_csr_host_free(h)
    t = lambda a: torch.from_numpy(a).to(device)
    return Csr(n_rows, n_cols, n, t(Ap), t(Aj), t(Ax), os.path.basename(path), {"synthetic": False, "path": str(path)})
