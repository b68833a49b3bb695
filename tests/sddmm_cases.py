"""The table of SDDMM cases (csrc/sddmm.hip) that tests/test_sddmm_sim_cpu.py executes on the host and
tests/test_gpu_sddmm.py on the device: the same structures, operands and expected results for both.

    out[n] = alpha * s[n] * sum_{j < k} U[r(n), j] * V[Aj[n], j] + beta * out[n],     s = Ax, or 1 without values

The structures are those of tests/multi_cases.py (imported, not copied: the kernel cuts its work exactly as the
multi-vector kind does, SLICE_LEN merge items per wave, STEP nonzeros per step, C in LANES_PER_SLOT lanes per slot), plus a
hub row of 30 000 nonzeros, runs of more than SLICE_LEN empty rows, and two structures for position independence.  Both
test files assert the geometry: the host file against the constants of csrc/sddmm.hip and csrc/common.hpp, the device
file against info() (assert_geometry).

Expected values come from numpy in fp64 from the CSR arrays (expected()).  Integer-valued data ({-3 .. 3}, integer
alpha / beta: exact in any order for k <= 100 in fp32) is compared bit for bit, the sign of a zero apart; real data in
(-1, 1) is held to the dot-product bound the project uses for rows, with len = k:
    |got - want| <= |alpha| (k + 3) eps |s| sum_j |u_j v_j| + 2 eps (|alpha d| + |beta out_old| + |want|),   d = s * dot
(the + 1 over the row bound is the multiplication by s; the last term is the two roundings of the scaling; eps = 2^-24 /
2^-53; nothing in it is measured).  Padding columns of U and V hold NaN; with beta = 0, out starts as NaN and no NaN may
remain; on the device a canary behind out[nnz - 1] must survive."""
import collections
import struct

import numpy as np

import multi_cases as mc
from multi_cases import (AB_REDUCED, LANES_PER_SLOT, NP, SLICE_LEN, STEP, VEC, TILE, bits, is_integer_pair, open_row_structures,  # noqa: F401
                         ragged_structure, row_end_structures, slice_edge_structures, slices)

CANARY = -777.25
KF = 104                            # columns of the full U / V of a matrix: a case takes columns c0 .. c0 + k
K_ALL = {"f32": tuple(range(1, 34)) + (64, 65, 100), "f64": tuple(range(1, 18)) + (32, 33, 50)}
# one k per C and per masked remainder class (k mod W), at both numbers of live column groups where C allows two, one k
# of two tiles (multi_cases.K_REDUCED), and one of more than three tiles
K_REDUCED = {"f32": mc.K_REDUCED["f32"] + (100,), "f64": mc.K_REDUCED["f64"] + (50,)}
K_HUB = {"f32": (1, 8, 17, 32, 100), "f64": (3, 16, 50)}
ALIGNED, SHIFTED = (0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 1)      # element offsets of Ap, Aj, Ax, U, V, out from an aligned base
SHIFTS = (ALIGNED, SHIFTED, ALIGNED, (0, 0, 0, 1, 0, 0), ALIGNED, (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1))
PADS = ((0, 0), (1, 3), (3, 0), (0, 2), (4, 4))                # (ldu - k, ldv - k)

Matrix = collections.namedtuple("Matrix", "name family lens n_cols seed")
Case = collections.namedtuple("Case", "name matrix off val integer k c0 ldu ldv alpha beta valued shift")


def assert_geometry(info):
    """info() of a plan agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    assert "sddmm_slice_kernel" in info["main_kernel"]


def lanes_per_slot(k, val):
    """C of an execute: from k alone, as the multi-vector kind chooses its tile."""
    groups = -(-k // VEC[val])
    return next((c for c in LANES_PER_SLOT if groups <= c), max(LANES_PER_SLOT))


# ---- structures --------------------------------------------------------------------------------------------------------
def hub_structure(L=SLICE_LEN):
    lens = [3, 0, 30000, 0, 0, 5, 41, 1]
    assert sum(1 for r0, r1, n0, nn in slices(lens, L) if nn == L and r1 == r0) >= 28
    return Matrix("hub_row_30000", "hub", tuple(lens), 211, 500)


def empty_run_structure(L=SLICE_LEN):
    lens = [4] + [0] * (L + 476) + [7, 70] + [0] * (2 * L + 552) + [2, 0, 0, 9] + [0] * (L + 76) + [1]
    assert sum(1 for r0, r1, n0, nn in slices(lens, L) if nn == 0 and r1 - r0 == L) >= 2
    return Matrix("empty_runs", "empty_runs", tuple(lens), 53, 501)


# Position independence.  `dup`: every row holds its column list twice ([c_0 .. c_{n-1}, c_0 .. c_{n-1}]), so equal
# (row, column) pairs lie n nonzeros apart: in other slots, steps and (rows longer than L / 2) slices.  `moved`: the rows
# of `base` behind a prefix of other rows (12 nonzeros and 3 row ends more in front of them, then a row that pushes them
# into later slices); its U is the prefix's rows followed by base's U, its V is base's V.
_DUP_HALF = (1, 2, 3, 5, 8, 13, 31, 32, 33, 64, 100, 0, 7, 600, 1, 1, 17)
_BASE_LENS = (3, 0, 17, 64, 1, 1, 130, 0, 0, 9, 700, 2, 63, 65, 5)
_MOVED_PREFIX = (5, 0, 7, 1500)


def position_structures():
    return [Matrix("dup", "position", tuple(2 * n for n in _DUP_HALF), 97, 510),
            Matrix("base", "position", _BASE_LENS, 89, 511),
            Matrix("moved", "position", _MOVED_PREFIX + _BASE_LENS, 89, 512)]


def pair_value(r, c, integer, val):
    """A value that depends on (row, column) alone: Ax of the position structures."""
    h = (np.asarray(r, dtype=np.int64) * 7919 + np.asarray(c, dtype=np.int64) * 104729) % 2001
    return (h % 7 - 3).astype(NP[val]) if integer else ((h - 1000) / 1000.5).astype(NP[val])


# ---- operands ----------------------------------------------------------------------------------------------------------
_arrays = {}


def arrays(m, off, val, integer):
    """(Ap, Aj, Ax, O0, U, V) of a matrix: U and V have KF columns, O0 is the nnz old values of out.  Made once and
    left unchanged."""
    key = (m.name, off, val, integer)
    if key in _arrays:
        return _arrays[key]
    rng = np.random.RandomState(m.seed)
    Ap = np.zeros(len(m.lens) + 1, dtype=NP[off])
    np.cumsum(m.lens, out=Ap[1:])
    nnz = int(Ap[-1])
    if integer:
        draw = lambda *shape: rng.randint(-3, 4, size=shape).astype(NP[val])
    else:
        draw = lambda *shape: (rng.rand(*shape) * 2 - 1).astype(NP[val])
    rows = np.repeat(np.arange(len(m.lens)), m.lens)
    if m.name == "dup":
        Aj = np.concatenate([np.tile(rng.randint(0, m.n_cols, size=n // 2), 2) for n in m.lens] + [np.zeros(0, int)]).astype(np.int32)
        Ax, O0, U, V = pair_value(rows, Aj, integer, val), draw(nnz), draw(len(m.lens), KF), draw(m.n_cols, KF)
    elif m.name == "moved":
        bAp, bAj, bAx, bO0, bU, bV = arrays(position_structures()[1], off, val, integer)
        pre = int(sum(_MOVED_PREFIX))
        Aj = np.concatenate([rng.randint(0, m.n_cols, size=pre).astype(np.int32), bAj])
        Ax, O0 = pair_value(rows - len(_MOVED_PREFIX), Aj, integer, val), np.concatenate([draw(pre), bO0])
        U, V = np.concatenate([draw(len(_MOVED_PREFIX), KF), bU]), bV
    else:
        Aj = rng.randint(0, m.n_cols, size=nnz).astype(np.int32)
        Ax = pair_value(rows, Aj, integer, val) if m.name == "base" else draw(nnz)
        O0, U, V = draw(nnz), draw(len(m.lens), KF), draw(m.n_cols, KF)
    _arrays[key] = (Ap, Aj, Ax, O0, U, V)
    return _arrays[key]


def expected(c):
    """(want, bound) of a case in fp64; bound is None for integer data (want is then exact)."""
    Ap, Aj, Ax, O0, U, V = arrays(c.matrix, c.off, c.val, c.integer)
    rows = np.repeat(np.arange(len(c.matrix.lens)), c.matrix.lens)
    u = U[:, c.c0:c.c0 + c.k].astype(np.float64)[rows]
    v = V[:, c.c0:c.c0 + c.k].astype(np.float64)[Aj]
    s = Ax.astype(np.float64) if c.valued else np.ones(len(Aj))
    dot, dabs = (u * v).sum(1), np.abs(u * v).sum(1)
    old = c.beta * O0.astype(np.float64) if c.beta != 0.0 else np.zeros(len(Aj))
    want = c.alpha * (s * dot) + old
    if c.integer:
        return want, None
    eps = 2.0 ** -24 if c.val == "f32" else 2.0 ** -53
    bound = abs(c.alpha) * (c.k + 3) * eps * np.abs(s) * dabs + 2 * eps * (np.abs(c.alpha * s * dot) + np.abs(old) + np.abs(want))
    return want, bound


def check(c, out):
    """out: the nnz values an execute left."""
    out = np.asarray(out)
    assert out.shape == (sum(c.matrix.lens),) and out.dtype == NP[c.val], c.name
    assert not np.any(np.isnan(out)), "%s: NaN in out (entries %s)" % (c.name, np.nonzero(np.isnan(out))[0][:8])
    want, bound = expected(c)
    if c.integer:
        bad = np.nonzero(bits(out) != bits(want.astype(NP[c.val])))[0]
        assert bad.size == 0, "%s: entries %s differ from the exact value (got %s, want %s)" % (c.name, bad[:8], out[bad[:8]], want[bad[:8]])
        return
    err = np.abs(out.astype(np.float64) - want)
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, "%s: entries %s outside the bound (excess %s)" % (c.name, bad[:8], (err - bound)[bad[:8]])


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, off, val, k, ab, pad, shift, valued, tag=""):
    alpha, beta = ab
    c0 = 0 if k > KF - 4 else (k % 5)
    name = "%s-%s-%s-k%d-a%g-b%g-pad%d.%d-%s-%s%s" % (m.name, off, val, k, alpha, beta, pad[0], pad[1], "".join(map(str, shift)),
                                                     "valued" if valued else "pattern", tag)
    return Case(name, m, off, val, is_integer_pair(alpha, beta), k, c0, k + pad[0], k + pad[1], alpha, beta, bool(valued), tuple(shift))


class _Rotation:
    """alpha / beta, padding, operand offsets, offset width and valued / pattern, rotating with periods 5, 5, 7, 2 and 4."""

    def __init__(self):
        self.n = 0

    def case(self, m, val, k, tag=""):
        n = self.n
        self.n += 1
        return _case(m, ("i32", "i64")[n % 2], val, k, AB_REDUCED[n % len(AB_REDUCED)], PADS[(n // 2) % len(PADS)],
                     SHIFTS[n % len(SHIFTS)], (n // 2) % 2 == 0, tag)


def reduced(ms):
    rot, out = _Rotation(), []
    for m in ms:
        for val in ("f32", "f64"):
            out += [rot.case(m, val, k) for k in K_REDUCED[val]]
    return out


def ragged_cross():
    """Every k x both offset widths x valued / pattern; alpha / beta, padding and operand offsets rotate."""
    m, out, n = ragged_structure(), [], 0
    for val in ("f32", "f64"):
        for k in K_ALL[val]:
            for off in ("i32", "i64"):
                for valued in (True, False):
                    out.append(_case(m, off, val, k, AB_REDUCED[n % len(AB_REDUCED)], PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)],
                                     valued, "-cross"))
                    n += 1
    return out


def alignment_pairs():
    """[(aligned case, the same case with every operand one element off a 16-byte boundary)]: equal bit for bit."""
    m, out = ragged_structure(), []
    for val in ("f32", "f64"):
        for i, k in enumerate(K_REDUCED[val]):
            off, ab = ("i32", "i64")[i % 2], ((-0.75, 3.0), (2.5, 0.0))[i % 2]
            out.append((_case(m, off, val, k, ab, (0, 0), ALIGNED, True, "-align"), _case(m, off, val, k, ab, (0, 0), SHIFTED, True, "-align")))
    return out


def hub_cases():
    rot, m = _Rotation(), hub_structure()
    return [rot.case(m, val, k) for val in ("f32", "f64") for k in K_HUB[val]]


K_POSITION = {"f32": (3, 8, 13, 32, 65), "f64": (1, 4, 7, 16, 33)}


def position_cases():
    """Real data, beta = 0, valued (Ax a function of (row, column)) and pattern; every structure under the same k, types
    and scaling, so that outputs can be compared across structures."""
    out = []
    for m in position_structures():
        for val in ("f32", "f64"):
            for i, k in enumerate(K_POSITION[val]):
                out.append(_case(m, ("i32", "i64")[i % 2], val, k, (2.5, 0.0), (0, 0), ALIGNED, i % 2 == 0, "-pos"))
    return out


def position_checks():
    """[(case a, case b, entries of a, entries of b)]: out_a[ia] == out_b[ib] bit for bit — equal (row of U, row of V,
    s, alpha, beta, k) at other positions."""
    cases = {c.name: c for c in position_cases()}
    out = []
    for c in cases.values():
        if c.matrix.name == "dup":
            Ap = np.concatenate(([0], np.cumsum(c.matrix.lens)))
            first = np.concatenate([np.arange(a, a + (b - a) // 2) for a, b in zip(Ap[:-1], Ap[1:])] + [np.zeros(0, int)]).astype(np.int64)
            second = first + np.repeat(np.asarray(c.matrix.lens) // 2, np.asarray(c.matrix.lens) // 2)
            out.append((c, c, first, second))
        elif c.matrix.name == "base":
            moved = cases[c.name.replace("base-", "moved-", 1)]
            n = np.arange(sum(_BASE_LENS), dtype=np.int64)
            out.append((c, moved, n, n + sum(_MOVED_PREFIX)))
    assert len(out) == 2 * sum(len(v) for v in K_POSITION.values())
    return out


FAMILIES = ("row_ends", "open_row", "slice_edges", "ragged_cross", "alignment", "hub", "empty_runs", "position")


def family(name):
    """The cases of one family, in plan order: consecutive cases of one (matrix, types, matrix offsets) share a plan."""
    if name == "row_ends":
        out = reduced(row_end_structures())
    elif name == "open_row":
        out = reduced(open_row_structures())
    elif name == "slice_edges":
        out = reduced(slice_edge_structures())
    elif name == "ragged_cross":
        out = ragged_cross()
    elif name == "alignment":
        out = [c for pair in alignment_pairs() for c in pair]
    elif name == "hub":
        out = hub_cases()
    elif name == "empty_runs":
        out = reduced([empty_run_structure()])
    elif name == "position":
        out = position_cases()
    else:
        raise KeyError(name)
    return sorted(out, key=plan_key)


def plan_key(c):
    return (c.matrix.name, c.off, c.val, c.integer, c.shift[:3])


def table():
    return [c for f in FAMILIES for c in family(f)]


# ---- the host program's batch file (tests/cpp/sddmm_sim.cpp, whose header comment has the records) ------------------------
NAN_BITS = {"f32": 0x7FC00000, "f64": 0x7FF8000000000000}


def batch_operands(c):
    """What write_batch asks of a case: its plan key, the MI355_VAL_* of U and V, (Ap, Aj, Ax, O0, U, V) as the program
    reads them, and the bit pattern of a NaN of U's and V's type."""
    return plan_key(c), ("f32", "f64").index(c.val), arrays(c.matrix, c.off, c.val, c.integer), NAN_BITS[c.val]


def write_batch(path, cases, operands=batch_operands):
    """Cases in plan order; returns them in the order their results come back."""
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    last = None
    with open(path, "wb") as f:
        for c in cases:
            key, type_word, (Ap, Aj, Ax, O0, U, V), nan_bits = operands(c)
            if key != last:
                last = key
                f.write(words(1, ("i32", "i64").index(c.off), type_word, len(c.matrix.lens), c.matrix.n_cols, int(Ap[-1]), *c.shift[:3]))
                for a in (Ap, Aj, Ax, O0):
                    f.write(a.tobytes())
                f.write(words(2, U.shape[1]))
                f.write(np.ascontiguousarray(U).tobytes())
                f.write(np.ascontiguousarray(V).tobytes())
            f.write(words(4, c.k, c.c0, c.ldu, c.ldv, c.shift[3], c.shift[4], c.shift[5], int(c.valued), int(c.beta == 0.0), nan_bits))
            f.write(struct.pack("<2d", c.alpha, c.beta))
        f.write(words(0))
    return list(cases)


def read_results(path, cases, dtype=lambda c: NP[c.val]):
    """[(status, out)] per case, out in dtype(c); raises if the file is not complete."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            st, count = struct.unpack("<2q", f.read(16))
            assert count == sum(c.matrix.lens), c.name
            out.append((st, np.frombuffer(f.read(count * np.dtype(dtype(c)).itemsize), dtype=dtype(c))))
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return out
