"""The table of multi-vector SpMV cases (csrc/multi.hip) that tests/test_multi_sim_cpu.py executes on the host and
tests/test_gpu_multi.py on the device: the same structures, operands and expected results for both.

Geometry the structures are built from (never from literals): a slice is L = SLICE_LEN merge items (row ends and
nonzeros; the nonzeros of row r come before its end, so nonzero n of row r is item n + r and the end of row r is item
Ap[r + 1] + r); a wave walks the nonzeros of its slice STEP = 64 at a time, counted from the slice's first nonzero; a
tile has C in LANES_PER_SLOT lanes per nonzero slot, so S = STEP / C slots.  Every structure of the row-end and
open-row families is ONE slice (fewer than L items), so that its nonzero numbers are the kernel's step positions.

Data: integer-valued ({-3 .. 3}, exact in any summation order) where alpha and beta are integers — compared bit for
bit with the serial oracle (the sign of a zero apart, which follows the summation order) — and real values in (-1, 1) otherwise, compared within the per-row parity bound of
tests/test_gpu_multi.py::run_case.  Padding columns of X hold NaN, those of Y a canary that must survive; with
beta = 0, Y0 is NaN."""
import collections
import struct

import numpy as np

# The kernel's geometry.  Both test files assert it: the host file against the constants of csrc/multi.hip and
# csrc/common.hpp (kMultiSlice, kWave, kMultiGroupsMax; multi.hip asserts them equal to slice_cut.hpp's kSliceLen and
# kSliceGroupsMax, which the kernels use), the device file against info() (assert_geometry).
SLICE_LEN = 1024                    # merge items per slice = info()["slice_len"]
STEP = 64                           # nonzeros per step = the wave width
LANES_PER_SLOT = (1, 2, 4, 8)       # up to kSliceGroupsMax 16-byte column groups: widest_tile = 8 * VEC
SLOTS = tuple(STEP // c for c in LANES_PER_SLOT)
CANARY = -777.25
KF = 72                             # columns of the full X / Y0 of a matrix: a case takes columns c0 .. c0 + k
NP = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
VEC = {"f32": 4, "f64": 2}          # columns per 16-byte group
TILE = {"f32": 32, "f64": 16}       # widest tile
AB = ((1.0, 0.0), (2.5, 0.0), (-0.75, 3.0), (0.0, 2.0))
AB_REDUCED = AB + ((2.0, -1.0),)
K_CROSS = {"f32": tuple(range(1, 34)) + (64, 65), "f64": tuple(range(1, 18)) + (32, 33)}
# one k per C and per masked remainder class (k mod V), at both numbers of live column groups where C allows two, and
# one k of two passes
K_REDUCED = {"f32": (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 14, 16, 17, 23, 26, 32, 33), "f64": (1, 2, 3, 4, 5, 8, 11, 16, 17)}
K_MAX = {"f32": 65, "f64": 33}
ALL_TYPES = (("i32", "f32"), ("i64", "f64"), ("i64", "f32"), ("i32", "f64"))
ALIGNED, SHIFTED = (0, 0, 0, 0, 0), (1, 1, 1, 1, 1)      # element offsets of Ap, Aj, Ax, X, Y from an aligned base



def assert_geometry(info, val):
    """info() of a plan of value type `val` agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["widest_tile"] == max(LANES_PER_SLOT) * VEC[val] == TILE[val]
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    assert info["passes"] == -(-info["k_max"] // TILE[val])


Matrix = collections.namedtuple("Matrix", "name family lens n_cols seed")
Case = collections.namedtuple("Case", "name matrix off val integer k k_max c0 ldx ldy alpha beta shift")


def is_integer_pair(alpha, beta):
    return float(alpha).is_integer() and float(beta).is_integer()


# ---- structures ------------------------------------------------------------------------------------------------------
class Rows:
    """Row lengths, with the merge item count kept so that a row end can be put on a chosen item."""

    def __init__(self, lens=()):
        self.lens = list(lens)

    @property
    def items(self):
        return sum(self.lens) + len(self.lens)

    def add(self, *lens):
        self.lens += list(lens)
        return self

    def end_at(self, item):
        """One more row whose row-end item is `item` (its last nonzero, if it has one, is item - 1)."""
        n = item - self.items
        assert n >= 0, (item, self.items)
        self.lens.append(n)
        return self


def slices(lens, L=SLICE_LEN):
    """(r0, r1, n0, nn) of every slice, as the kernel's two diagonal searches give them."""
    Ap = np.concatenate(([0], np.cumsum(np.asarray(lens, dtype=np.int64))))
    ends = Ap[1:] + np.arange(len(lens))
    items = len(lens) + int(Ap[-1])
    out = []
    for w in range(-(-items // L)):
        d0, d1 = w * L, min((w + 1) * L, items)
        r0, r1 = int(np.searchsorted(ends, d0, "left")), int(np.searchsorted(ends, d1, "left"))
        out.append((r0, r1, d0 - r0, (d1 - r1) - (d0 - r0)))
    return out


def row_end_structures(L=SLICE_LEN):
    out = []
    # the last nonzero of a row at position S - 1, S and S + 1 of a 64-step, one row end per step (S = 64: lanes 63, 0
    # and 1 of consecutive steps)
    r = Rows()
    nnz = 0
    for j, p in enumerate(sorted({S + e for S in SLOTS[1:] for e in (-1, 0, 1)}) + [STEP - 1]):
        end = STEP * j + p + 1
        r.add(end - nnz)
        nnz = end
    r.add(1, 1, 20)
    out.append(("ends_one_per_step", r.lens))
    # ... and all of them in ONE step, behind a row that runs into it
    lens, nnz = [], 0
    for p in sorted({S + e for S in SLOTS[1:] for e in (-1, 0, 1)}) + [STEP - 1, STEP, STEP + 1]:
        end = STEP + p + 1
        lens.append(end - nnz)
        nnz = end
    out.append(("ends_in_one_step", lens + [13]))
    # a last partial step of `left` nonzeros that holds a row end, a row's start and the slice's end
    for left in sorted({1, STEP - 1} | {S + e for S in SLOTS[1:] for e in (-1, 0, 1)}):
        a = (left + 1) // 2
        out.append(("left_%d" % left, [50, STEP - 50 + a, left - a]))
    out.append(("left_1_of_one_row", [STEP + 1]))
    out.append(("left_63_of_one_row", [2 * STEP - 1]))
    for name, lens in out:
        assert len(lens) + sum(lens) < L, name
    return [Matrix(n, "row_ends", tuple(l), 37, 100 + i) for i, (n, l) in enumerate(out)]


def open_row_structures(L=SLICE_LEN):
    whole = [S for S in SLOTS[::-1] for _ in range(STEP // S)] + [2 * STEP, 3 * STEP, STEP]
    out = [
        # ends mid-step; then a row through two whole steps that ends mid-step; an empty row; again
        ("open_through_whole_steps", [20, (STEP - 20) + 2 * STEP + 30, 5, 0, (STEP - 35) + STEP + 1, STEP, 3]),
        # rows of exactly S nonzeros on slot boundaries, of exactly one step, of 64 n
        ("whole_slots_and_steps", whole),
        ("whole_slots_and_steps_shifted", [3] + whole),
        # single-nonzero rows filling whole steps (every slot a head and a tail), behind a whole-step row and a short one
        ("single_nonzero_rows", [STEP] + [1] * (2 * STEP) + [5] + [1] * (STEP + 6)),
    ]
    for name, lens in out:
        assert len(lens) + sum(lens) < L, name
    return [Matrix(n, "open_row", tuple(l), 41, 200 + i) for i, (n, l) in enumerate(out)]


def slice_edge_structures(L=SLICE_LEN):
    out = []
    # a row end on every item within 2 of a slice end, empty rows behind it: d = 0 is a row end that is the slice's
    # last item, d = 1 a last nonzero that is, with its row end the next slice's first, d = 2 a carried row whose
    # final slice holds only its last nonzero
    r = Rows([3, 0, 2])
    for i, d in enumerate((-2, -1, 0, 1, 2)):
        r.end_at((i + 1) * L - 1 + d).add(0, 0, 0, 5)
    r.add(17, 0, 0)
    out.append(("edge_within_2", r.lens))
    # runs of empty rows before, across and after a slice end
    r = Rows([4]).end_at(L - 8).add(*[0] * 6).add(4).end_at(2 * L - 4).add(*[0] * 6).end_at(3 * L - 1).add(*[0] * 6).add(2)
    out.append(("edge_empty_runs", r.lens))
    out.append(("slice_of_row_ends_only", [5] + [0] * (2 * L + 10) + [3]))
    out.append(("slices_inside_one_row", [10, 3 * L + 100, 10]))
    out.append(("two_carried_rows", [100, L, L, 50]))
    out.append(("last_nonzero_alone", Rows([7]).end_at(L + 1).add(3).lens))
    rng = np.random.RandomState(77)
    for total in (L - 1, L, L + 1, 2 * L):
        r = Rows(rng.randint(0, 13, size=60).tolist())
        out.append(("items_%d" % total, r.end_at(total - 1).lens))
        assert r.items == total
    out.append(("one_row", [2 * L + 37]))
    out.append(("one_short_row", [5]))
    out.append(("no_nonzeros", [0] * (2 * L + 3)))
    out.append(("first_and_last_rows_empty", [0, 0, L - 300, 9, 0, 400, 0, 0]))
    by = dict(out)
    s = slices(by["edge_within_2"], L)
    assert len(s) == 6
    assert any(nn == 0 and r1 - r0 == L for r0, r1, n0, nn in slices(by["slice_of_row_ends_only"], L))
    assert any(nn == L and r1 == r0 for r0, r1, n0, nn in slices(by["slices_inside_one_row"], L))
    assert [r1 for r0, r1, n0, nn in slices(by["two_carried_rows"], L)][:2] == [1, 2]
    assert slices(by["last_nonzero_alone"], L)[1][:2] == (1, 3) and slices(by["last_nonzero_alone"], L)[1][3] == 1 + 3
    return [Matrix(n, "slice_edges", tuple(l), 43, 300 + i) for i, (n, l) in enumerate(out)]


def ragged_structure(L=SLICE_LEN):
    rng = np.random.RandomState(4242)
    lens = rng.randint(0, 41, size=600)
    lens[rng.rand(600) < 0.2] = 0
    lens[300] = 3 * L
    return Matrix("ragged", "ragged", tuple(int(v) for v in lens), 97, 400)


# ---- operands and expected results -------------------------------------------------------------------------------------
_arrays = {}


def arrays(m, off, val, integer):
    """(Ap, Aj, Ax, X, Y0) of a matrix: X and Y0 have KF columns.  Made once and left unchanged."""
    key = (m.name, off, val, integer)
    if key not in _arrays:
        rng = np.random.RandomState(m.seed)
        Ap = np.zeros(len(m.lens) + 1, dtype=NP[off])
        np.cumsum(m.lens, out=Ap[1:])
        nnz = int(Ap[-1])
        Aj = rng.randint(0, m.n_cols, size=nnz).astype(np.int32)
        if integer:
            draw = lambda *shape: rng.randint(-3, 4, size=shape).astype(NP[val])
        else:
            draw = lambda *shape: (rng.rand(*shape) * 2 - 1).astype(NP[val])
        _arrays[key] = (Ap, Aj, draw(nnz), draw(m.n_cols, KF), draw(len(m.lens), KF))
    return _arrays[key]


_refs = {}


def reference(orc, m, val, integer):
    """Per column of the full X: the serial sum in the value type (integer data) or (fp64 sum, sum |a x|)."""
    key = (m.name, val, integer)
    if key not in _refs:
        Ap, Aj, Ax, X, _ = arrays(m, "i32", val, integer)
        cols = [np.ascontiguousarray(X[:, j]) for j in range(KF)]
        if integer:
            _refs[key] = [orc.spmv_genl_serial(0, Ap, Aj, Ax, x) for x in cols]
        else:
            _refs[key] = [orc.spmv_ref64(Ap, Aj, Ax, x) for x in cols]
    return _refs[key]


def bits(a):
    """The bit patterns of a float array with -0 taken as +0: the sign of a zero sum follows the summation order (a lone
    product -0 is -0, the serial sum 0 + -0 is +0), every other value of integer data has one pattern."""
    a = np.ascontiguousarray(a) + a.dtype.type(0)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(orc, c, ybuf):
    """ybuf: what the execute left of Y, n_rows x ldy (padding included)."""
    m = c.matrix
    n_rows = len(m.lens)
    ybuf = np.asarray(ybuf).reshape(n_rows, c.ldy)
    got = ybuf[:, :c.k]
    assert np.all(ybuf[:, c.k:] == NP[c.val](CANARY)), "%s: a padding column of Y was written" % c.name
    assert not np.any(np.isnan(got)), "%s: NaN in Y (rows %s)" % (c.name, np.unique(np.nonzero(np.isnan(got))[0])[:8])
    ref = reference(orc, m, c.val, c.integer)
    Y0 = arrays(m, c.off, c.val, c.integer)[4][:, c.c0:c.c0 + c.k]
    V = NP[c.val]
    if c.integer:
        for j in range(c.k):
            want = V(c.alpha) * ref[c.c0 + j]
            if c.beta != 0.0:
                want = want + V(c.beta) * Y0[:, j]
            bad = np.nonzero(bits(got[:, j]) != bits(want))[0]
            assert bad.size == 0, "%s: column %d differs from the serial sum in rows %s (got %s, want %s)" % (
                c.name, j, bad[:8], got[bad[:8], j], want[bad[:8]])
        return
    eps = 2.0 ** -24 if c.val == "f32" else 2.0 ** -53
    lens = np.asarray(m.lens, dtype=np.int64)
    extra = 2 if (c.alpha, c.beta) == (1.0, 0.0) else 3
    for j in range(c.k):
        y64, yabs = ref[c.c0 + j]
        y0 = Y0[:, j].astype(np.float64) if c.beta != 0.0 else np.zeros(n_rows)
        want = c.alpha * y64 + c.beta * y0
        bound = (lens + extra) * eps * (abs(c.alpha) * yabs + np.abs(c.beta * y0)) + 1e-300
        err = np.abs(got[:, j].astype(np.float64) - want)
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, "%s: column %d outside the bound in rows %s (excess %s)" % (c.name, j, bad[:8], (err - bound)[bad[:8]])


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, off, val, k, ab, pad, shift, k_max=None, c0=0, tag=""):
    alpha, beta = ab
    integer = is_integer_pair(alpha, beta)
    name = "%s-%s-%s-k%d-a%g-b%g-pad%d-%s%s" % (m.name, off, val, k, alpha, beta, pad, "".join(map(str, shift)), tag)
    return Case(name, m, off, val, integer, k, k_max or K_MAX[val], c0, k + pad, k + (pad + 2 if pad else 0), alpha, beta,
                tuple(shift))


def reduced(m):
    """One k per C and masked remainder class; alpha / beta, the padding and the operand offsets rotate over the cases
    (with X alone and Y alone off the boundary among them: x_vec and y_vec are separate decisions)."""
    out = []
    shifts = (ALIGNED, SHIFTED, ALIGNED, (0, 0, 0, 1, 0), ALIGNED, (0, 0, 0, 0, 1))
    pads = (0, 1, 0, 3)
    n = 0
    for off, val in ALL_TYPES:
        for k in K_REDUCED[val]:
            out.append(_case(m, off, val, k, AB_REDUCED[n % len(AB_REDUCED)], pads[n % len(pads)], shifts[n % len(shifts)]))
            n += 1
    return out


def cross(m, val):
    """Every k of the type x both offset widths x alpha / beta x padding x operand offsets."""
    out = []
    for k in K_CROSS[val]:
        for off in ("i32", "i64"):
            for ab in AB:
                for pad in (0, 1 if k % 2 == 0 else 3):
                    for shift in (ALIGNED, SHIFTED):
                        out.append(_case(m, off, val, k, ab, pad, shift, tag="-cross"))
    return out


def stale_carries(m, val="f32"):
    """A plan of k_max = 33 executed at k = 33 and then at k = 5 on other vectors."""
    return [_case(m, "i32", val, 33, (1.0, 0.0), 0, ALIGNED, k_max=33, tag="-stale"),
            _case(m, "i32", val, 5, (1.0, 0.0), 1, ALIGNED, k_max=33, c0=40, tag="-stale"),
            _case(m, "i32", val, 33, (2.5, 0.0), 0, ALIGNED, k_max=33, tag="-stale"),
            _case(m, "i32", val, 5, (-0.75, 3.0), 3, (0, 0, 0, 1, 1), k_max=33, c0=40, tag="-stale")]


FAMILIES = ("row_ends", "open_row", "slice_edges", "stale_carries", "ragged_cross_f32", "ragged_cross_f64",
            "edge_cross_f32", "edge_cross_f64")


def family(name, L=SLICE_LEN):
    """The cases of one family, in plan order: consecutive cases of one (matrix, types, matrix offsets, k_max) share a plan."""
    edge = slice_edge_structures(L)
    if name == "row_ends":
        ms = row_end_structures(L)
    elif name == "open_row":
        ms = open_row_structures(L)
    elif name == "slice_edges":
        ms = edge
    elif name == "stale_carries":
        out = stale_carries(ragged_structure(L)) + stale_carries(edge[0], "f64")
        return sorted(out, key=plan_key)
    elif name.startswith("ragged_cross_"):
        return sorted(cross(ragged_structure(L), name[-3:]), key=plan_key)
    elif name.startswith("edge_cross_"):
        return sorted(cross(edge[0], name[-3:]), key=plan_key)
    else:
        raise KeyError(name)
    out = []
    for m in ms:
        out += reduced(m)
    return sorted(out, key=plan_key)


def plan_key(c):
    return (c.matrix.name, c.off, c.val, c.integer, c.shift[:3], c.k_max)


def table(L=SLICE_LEN):
    return [c for f in FAMILIES for c in family(f, L)]


def weight(g):
    """Of a plan group, to deal the groups of any multi-vector table to batches: merge items x columns."""
    return sum((len(c.matrix.lens) + sum(c.matrix.lens) + 2000) * (c.k + 8) for c in g)


# ---- the host program's batch file (tests/cpp/multi_sim.cpp, whose header comment has the records) ------------------------
VAL_TYPE = {"f32": 0, "f64": 1, "i32": 2, "f16": 4, "bf16": 5}      # MI355_VAL_*
CREATE, CREATE_TYPED, CREATE_HALF = 0, 1, 2                         # the plan record's `how`
# What write_batch asks of a case.  matrix_key: cases of one key share a matrix record; plan = (k_max, how, pattern): the
# plan record, made anew where it changes; the MI355_VAL_* of X / Y and of Ax as stored; Ap, Aj, Ax, Xs (the variants of
# X a run chooses from by x_kind) and Y0 as the program reads them; semiring = its number, or -1 for no set_semiring
# call; x_pad, y_poison, canary: the bit patterns of what the padding of X, a poisoned Y and the padding of Y hold.
Operands = collections.namedtuple("Operands", "matrix_key plan vec_type mat_type Ap Aj Ax Xs Y0 semiring x_kind x_pad y_poison canary")


def word_of(value, dtype):
    """The bit pattern of a value of dtype as an int64 word (its low bytes)."""
    return int.from_bytes(np.asarray(value, dtype=dtype).tobytes().ljust(8, b"\0"), "little", signed=True)


def batch_operands(c):
    Ap, Aj, Ax, X, Y0 = arrays(c.matrix, c.off, c.val, c.integer)
    nan = word_of(float("nan"), NP[c.val])
    return Operands(plan_key(c)[:5], (c.k_max, CREATE, 0), VAL_TYPE[c.val], VAL_TYPE[c.val], Ap, Aj, Ax, (X,), Y0, -1, 0, nan, nan,
                    word_of(CANARY, NP[c.val]))


def write_batch(path, cases, operands=batch_operands):
    """Cases in plan order; returns them in the order their results come back."""
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    last_m = last_p = None
    with open(path, "wb") as f:
        for c in cases:
            o = operands(c)
            if o.matrix_key != last_m:
                last_m, last_p = o.matrix_key, None
                f.write(words(1, ("i32", "i64").index(c.off), o.vec_type, o.mat_type, len(c.matrix.lens), c.matrix.n_cols,
                              int(o.Ap[-1]), *c.shift[:3]))
                for a in (o.Ap, o.Aj, o.Ax):
                    f.write(a.tobytes())
                f.write(words(2, o.Y0.shape[1], len(o.Xs)))
                for a in o.Xs + (o.Y0,):
                    f.write(np.ascontiguousarray(a).tobytes())
            if o.plan != last_p:
                last_p = o.plan
                f.write(words(3, *o.plan))
            f.write(words(4, c.k, c.c0, c.ldx, c.ldy, c.shift[3], c.shift[4], int(c.beta == 0.0), o.semiring, o.x_kind, o.x_pad,
                          o.y_poison, o.canary))
            f.write(struct.pack("<2d", c.alpha, c.beta))
        f.write(words(0))
    return list(cases)


def read_results(path, cases, dtype=lambda c: NP[c.val]):
    """[(status, Y buffer as n_rows x ldy)] per case, Y in dtype(c); raises if the file is not complete."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            st, count = struct.unpack("<2q", f.read(16))
            assert count == len(c.matrix.lens) * c.ldy, c.name
            out.append((st, np.frombuffer(f.read(count * np.dtype(dtype(c)).itemsize), dtype=dtype(c))))
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return out
