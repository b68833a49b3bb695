import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLD = os.path.join(ROOT, "tests", "golden")

# The product runs a SMALL regular matrix (VECTOR kind, up to 4.1 M nonzeros) on its plain one-pass kernel (capi.hip,
# small_plain).  Most matrices of this suite are small on purpose — empty rows, one long row, ragged lengths — and are
# there to put the CHUNKED kernels through those cases, so the suite switches that choice off for itself;
# tests/test_gpu_small.py runs the same kinds of matrices through the product's default, and the forced-code-path
# matrix (scripts/gpu_env_matrix.sh) has a MI355_SPMV_SMALL=1 pass over the whole parity file.
os.environ.setdefault("MI355_SPMV_SMALL", "0")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def sp():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="session")
def oracle():
    from oracle.oracle import Oracle
    return Oracle()


REF_RECORDING = os.path.join(GOLD, "ref_outputs.npz")


def _ref_key(method, args):
    """Digest of one call's inputs: arrays by dtype, shape and bytes, scalars by value (a file: its contents)."""
    h = hashlib.sha256(method.encode())
    for a in args:
        if isinstance(a, np.ndarray):
            h.update(("|%s%s|" % (a.dtype.str, a.shape)).encode())
            h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(("|%r|" % (a,)).encode())
    return h.hexdigest()[:32]


class RecordedRef:
    """The reference build's answers to the suite's own inputs, as oracle/_ref/libspmv_ref.so gave them
    (tests/golden/ref_outputs.npz): the `ref` tests hold where the reference tree is not there to build it.
    record=<live Ref>: pass every call through and keep its answer; save() writes the file."""

    def __init__(self, record=None):
        self.live, self.new = record, {}
        self.stored = {} if record is not None else dict(np.load(REF_RECORDING))

    def _call(self, method, *args):
        key_args = args
        if method == "load_mtx":                     # a file by its contents, not by its (temporary) path
            with open(args[0], "rb") as f:
                key_args = (f.read(),) + args[1:]
        key = _ref_key(method, key_args)
        if self.live is not None:
            out = getattr(self.live, method)(*args)
            for i, a in enumerate(out if isinstance(out, tuple) else (out,)):
                self.new["%s/%d" % (key, i)] = np.asarray(a)
            return out
        if key + "/0" not in self.stored:
            raise KeyError("no recorded reference answer for this %s call: re-record %s with MI355_REF_RECORD=1 "
                           "(see tests/conftest.py)" % (method, os.path.relpath(REF_RECORDING, ROOT)))
        if method == "load_mtx":
            return tuple([int(self.stored["%s/%d" % (key, i)]) for i in (0, 1)] +
                         [self.stored["%s/%d" % (key, i)] for i in (2, 3, 4)])
        return self.stored[key + "/0"]

    def save(self):
        np.savez_compressed(REF_RECORDING, **self.new)

    def load_mtx(self, path, off="i32", val="f32"):
        return self._call("load_mtx", path, off, val)

    def spmv_cpu(self, n_cols, Ap, Aj, Ax, x):
        return self._call("spmv_cpu", n_cols, Ap, Aj, Ax, x)

    def spmv_genl_cpu(self, semiring, n_cols, Ap, Aj, Ax, x):
        return self._call("spmv_genl_cpu", semiring, n_cols, Ap, Aj, Ax, x)

    def spmv_cpu_mixed(self, n_cols, Ap, Aj, Ax, x):
        return self._call("spmv_cpu_mixed", n_cols, Ap, Aj, Ax, x)


@pytest.fixture(scope="session")
def ref():
    """The reference's own loader + serial SpMV: oracle/_ref/libspmv_ref.so where oracle/Makefile could compile it
    from the reference's headers, else that library's answers recorded in tests/golden/ref_outputs.npz.
    To re-record after changing a `ref` test's inputs (every user of this fixture is in test_oracle.py), with the
    library built:  MI355_REF_RECORD=1 python -m pytest tests/test_oracle.py"""
    from oracle.oracle import Ref
    if os.environ.get("MI355_REF_RECORD"):
        if not Ref.available():
            pytest.fail("MI355_REF_RECORD needs oracle/_ref/libspmv_ref.so")
        rec = RecordedRef(record=Ref())
        yield rec
        rec.save()
        return
    yield Ref() if Ref.available() else RecordedRef()


@pytest.fixture(scope="session")
def golden():
    with open(os.path.join(GOLD, "golden.json")) as f:
        return json.load(f)


def unhex(lst, dtype):
    return np.array([float.fromhex(v) for v in lst], dtype=dtype)


def seeded_x(n, dtype):
    """The non-trivial x of oracle/make_golden.py."""
    i = np.arange(n, dtype=np.int64)
    return (((7 * i + 3) % 11 - 5) / 4.0).astype(dtype)


def random_csr(rng, n_rows, n_cols, max_len, off_dtype=np.int32, val_dtype=np.float32,
               empty_frac=0.2, long_row=None, integer_values=False):
    """Ragged CSR with empty rows, duplicates and unsorted columns."""
    lens = rng.randint(0, max_len + 1, size=n_rows)
    lens[rng.rand(n_rows) < empty_frac] = 0
    if long_row is not None and n_rows > 0:
        lens[rng.randint(0, n_rows)] = long_row
    Ap = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    Aj = rng.randint(0, max(n_cols, 1), size=nnz).astype(np.int32)
    if integer_values:
        Ax = rng.randint(-3, 4, size=nnz).astype(val_dtype)
    else:
        Ax = (rng.rand(nnz) * 2 - 1).astype(val_dtype)
    return Ap.astype(off_dtype), Aj, Ax


def parity_bound(oracle, Ap, Aj, Ax, x, n_threads=1):
    """Per-row bound of SURVEY.md §8(c): (len+2) * eps * sum|a*x| around the fp64 serial sum.
    n_threads splits the rows of the oracle pass over host threads (same values)."""
    y64, yabs = oracle.spmv_ref64(Ap, Aj, Ax, x, n_threads)
    eps = 2.0 ** -24 if Ax.dtype == np.float32 else 2.0 ** -53
    lens = np.diff(Ap.astype(np.int64))
    return y64, (lens + 2) * eps * yabs
