"""The table of permuted multi-vector SpMV cases (mi355_spmv_multi_create_permuted, csrc/multi_perm.hip and the permuted
walk of csrc/multi_slice_walk.inc) that tests/test_multi_perm_sim_cpu.py executes on the host and
tests/test_gpu_multi_transposed.py on the device: the same structures, permutations and operands for both.

Structures: those of tests/multi_cases.py (row ends, open rows, slice edges at SLICE_LEN merge items, the ragged matrix)
and four of this file's: a hub row of 30 000 entries, runs of empty rows around short ones, n_cols = 1, and no rows.
Each gets every permutation family:
    identity     perm[n] = n
    reversal     perm[n] = nnz - 1 - n
    random       a seeded random permutation
    shared       a non-injective map into n_values = nnz // 2 values, every value used at least twice (nnz >= 4)
    sparse       an injective map into n_values = 2 nnz + 3 values (most values unused)
k comes from multi_cases.K_REDUCED: one below a tile, the widest tile, and one of two passes (33 / 17).  The offset width,
the width of perm, alpha / beta and the padding of X and Y rotate over the cases; both value types run everywhere.

The bar, in both files: bit for bit the result of the plain object on the same structure with Ax[perm] materialised —
the same walk on the same values.  Data is integer-valued ({-3 .. 3}), so the result is also the exact dense product,
which check() holds it to (the sign of a zero apart)."""
import collections
import struct

import numpy as np

import multi_cases as mc

PERMS = ("identity", "reversal", "random", "shared", "sparse")
K = {"f32": (3, 32, 33), "f64": (3, 16, 17)}
AB = ((1.0, 0.0), (-2.0, 3.0))
OFF_TYPE = {"i32": 0, "i64": 1}
assert all(k in mc.K_REDUCED[v] for v in K for k in K[v]) and all(K[v][1] == mc.TILE[v] for v in K)

Case = collections.namedtuple("Case", "name matrix perm off val poff k k_max ldx ldy alpha beta")


def own_structures():
    rng = np.random.RandomState(99)
    short = rng.randint(1, 6, size=40).tolist()
    return [mc.Matrix("hub_row_30000", "own", (3, 30000, 0, 0, 7), 53, 500),
            mc.Matrix("empty_row_runs", "own", tuple([0] * 70 + short[:20] + [0] * 1100 + short[20:] + [0] * 65), 29, 501),
            mc.Matrix("one_column", "own", tuple(int(v) for v in rng.randint(0, 9, size=300)), 1, 502),
            mc.Matrix("no_rows", "own", (), 5, 503)]


def structures():
    return mc.row_end_structures() + mc.open_row_structures() + mc.slice_edge_structures() + [mc.ragged_structure()] + own_structures()


_csr = {}


def csr(m):
    """(Ap as int64, Aj) of a structure: made once and left unchanged."""
    if m.name not in _csr:
        rng = np.random.RandomState(m.seed)
        Ap = np.zeros(len(m.lens) + 1, dtype=np.int64)
        np.cumsum(m.lens, out=Ap[1:])
        _csr[m.name] = (Ap, rng.randint(0, m.n_cols, size=int(Ap[-1])).astype(np.int32))
    return _csr[m.name]


def permutation(m, kind):
    """(perm as int64, n_values)."""
    nnz = int(csr(m)[0][-1])
    rng = np.random.RandomState(m.seed + 7)
    if kind == "identity":
        return np.arange(nnz, dtype=np.int64), nnz
    if kind == "reversal":
        return np.arange(nnz, dtype=np.int64)[::-1].copy(), nnz
    if kind == "random":
        return rng.permutation(nnz).astype(np.int64), nnz
    if kind == "shared":
        if nnz < 4:
            return np.zeros(nnz, dtype=np.int64), max(nnz, 1)
        nv = nnz // 2
        p = np.concatenate((np.arange(nv), np.arange(nv), rng.randint(0, nv, size=nnz - 2 * nv))).astype(np.int64)
        return rng.permutation(p), nv
    if kind == "sparse":
        nv = 2 * nnz + 3
        return rng.permutation(nv)[:nnz].astype(np.int64), nv
    raise KeyError(kind)


_operands = {}


def operands(c):
    """(Ap, Aj, perm, n_values, Ax[n_values], X[n_cols, k], Y0[n_rows, k]) in the case's types."""
    draw = lambda rng, *shape: rng.randint(-3, 4, size=shape).astype(mc.NP[c.val])
    key = (c.matrix.name, c.perm, c.val)        # the values go with the permutation, not with k: cases of a plan share them
    if key not in _operands:
        perm, nv = permutation(c.matrix, c.perm)
        _operands[key] = (perm, nv, draw(np.random.RandomState(c.matrix.seed + 13 * PERMS.index(c.perm)), nv))
    perm, nv, Ax = _operands[key]
    key = (c.matrix.name, c.val, c.k)
    if key not in _operands:
        rng = np.random.RandomState(c.matrix.seed + 1000 + c.k)
        _operands[key] = (draw(rng, c.matrix.n_cols, c.k), draw(rng, len(c.matrix.lens), c.k))
    X, Y0 = _operands[key]
    Ap, Aj = csr(c.matrix)
    return Ap.astype(mc.NP[c.off]), Aj, perm.astype(mc.NP[c.poff]), nv, Ax, X, Y0


def expected(c):
    """alpha * A X + beta * Y0 with A's values Ax[perm], exact: every operand is a small integer."""
    Ap, Aj, perm, nv, Ax, X, Y0 = operands(c)
    n_rows = len(c.matrix.lens)
    rows = np.repeat(np.arange(n_rows), np.diff(Ap))
    want = np.zeros((n_rows, c.k), dtype=np.float64)
    np.add.at(want, rows, Ax[perm].astype(np.float64)[:, None] * X[Aj].astype(np.float64))
    return (c.alpha * want + (c.beta * Y0.astype(np.float64) if c.beta != 0.0 else 0.0)).astype(mc.NP[c.val])


def check(c, ybuf, yplain):
    """ybuf / yplain: what the permuted and the plain execute left of Y, (n_rows - 1) * ldy + k elements each."""
    n_rows = len(c.matrix.lens)
    assert np.array_equal(np.asarray(ybuf).view(np.uint8), np.asarray(yplain).view(np.uint8)), \
        "%s: the permuted object differs from the plain one on Ax[perm]" % c.name
    if n_rows == 0:
        assert len(ybuf) == 0
        return
    full = np.full(n_rows * c.ldy, mc.CANARY, dtype=mc.NP[c.val])
    full[:len(ybuf)] = ybuf
    full = full.reshape(n_rows, c.ldy)
    assert np.all(full[:, c.k:] == mc.NP[c.val](mc.CANARY)), "%s: a padding column of Y was written" % c.name
    got = full[:, :c.k]
    assert not np.any(np.isnan(got)), "%s: NaN in Y" % c.name
    assert np.array_equal(mc.bits(got), mc.bits(expected(c))), "%s: differs from the dense product" % c.name


def table():
    out, n = [], 0
    for m in structures():
        for perm in PERMS:
            for val in ("f32", "f64"):
                for k in K[val]:
                    off, poff = ("i32", "i64")[n % 2], ("i32", "i64")[(n // 2) % 2]
                    (alpha, beta), pad = AB[(n // 3) % 2], (0, 1, 0, 3)[n % 4]
                    name = "%s-%s-%s-%s-p%s-k%d-a%g-b%g-pad%d" % (m.name, perm, off, val, poff, k, alpha, beta, pad)
                    out.append(Case(name, m, perm, off, val, poff, k, mc.K_MAX[val], k + pad, k + (pad + 2 if pad else 0), alpha, beta))
                    n += 1
    return out


def plan_key(c):
    return (c.matrix.name, c.off, c.val, c.perm, c.poff)


def weight(g):
    return sum((len(c.matrix.lens) + sum(c.matrix.lens) + 2000) * (c.k + 8) for c in g)


# bad indices, on the ragged structure under the random permutation: (where, the value there, the width of perm)
def bad_cases():
    nv = permutation(mc.ragged_structure(), "random")[1]
    return [("n_values_i32", 17, nv, "i32"), ("n_values_i64", 4000, nv, "i64"), ("minus_one_i64", 0, -1, "i64"), ("minus_one_i32", 5, -1, "i32")]


# ---- the host program's batch file (tests/cpp/multi_perm_sim.cpp, whose header comment has the records) -------------------
def write_batch(path, cases, bad=()):
    """Cases in plan order, then (if asked) the bad-index records on the last matrix and perm written; returns the cases."""
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    last_m = last_p = None
    with open(path, "wb") as f:
        for c in cases:
            Ap, Aj, perm, nv, Ax, X, Y0 = operands(c)
            if (c.matrix.name, c.off, c.val) != last_m:
                last_m, last_p = (c.matrix.name, c.off, c.val), None
                f.write(words(1, OFF_TYPE[c.off], mc.VAL_TYPE[c.val], len(c.matrix.lens), c.matrix.n_cols, len(Aj)))
                f.write(Ap.tobytes() + Aj.tobytes())
            if (c.perm, c.poff) != last_p:
                last_p = (c.perm, c.poff)
                f.write(words(2, OFF_TYPE[c.poff], nv))
                f.write(perm.tobytes() + Ax.tobytes())
            f.write(words(3, c.k, c.k_max, c.ldx, c.ldy) + struct.pack("<2d", c.alpha, c.beta))
            f.write(np.ascontiguousarray(X).tobytes() + np.ascontiguousarray(Y0).tobytes())
        for _, pos, value, _ in bad:
            f.write(words(4, pos, value))
        f.write(words(0))
    return list(cases)


def read_results(path, cases, n_bad=0):
    """[(status, Y of the permuted object, Y of the plain one)] per case, then [(status, made)] per bad record when asked."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            st, count = struct.unpack("<2q", f.read(16))
            n_rows = len(c.matrix.lens)
            assert count == ((n_rows - 1) * c.ldy + c.k if n_rows else 0), c.name
            size = count * np.dtype(mc.NP[c.val]).itemsize
            out.append((st, np.frombuffer(f.read(size), dtype=mc.NP[c.val]), np.frombuffer(f.read(size), dtype=mc.NP[c.val])))
        bad = [struct.unpack("<2q", f.read(16)) for _ in range(n_bad)]
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return (out, bad) if n_bad else out
