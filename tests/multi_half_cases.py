"""The table of multi-vector SpMV cases with 16-bit vectors (csrc/multi_half_kernels.hpp, mi355_spmv_multi_create_half)
that tests/test_multi_half_sim_cpu.py executes on the host and tests/test_gpu_multi_half.py on the device: the same
structures, operands and expected results for both.

The structures are those of tests/multi_cases.py, imported: row ends on every slot and step boundary, the open-row
state machine, items within 2 of a slice end, slices of row ends only and of one row only, carried rows, the ragged
matrix.  Over them: {f16, bf16} vectors x {the matrix in the vectors' type, in fp32} x {i32, i64} offsets, k in K (every
tile width 8 / 16 / 32 / 64, every masked-remainder class k mod 8, two and three passes), the alpha / beta pairs of
multi_cases.AB_REDUCED, padded ldx / ldy, operands one element off a 16-byte boundary, and a narrow execute after a
wide one on one object: the full cross on the ragged matrix, a rotation elsewhere.

The contract that check() holds Y to: every stored 16-bit value is widened exactly to fp32, products and sums are fp32,
out = alpha * S (+ beta * float(Y0) when beta != 0), and Y is out rounded to the 16-bit type ONCE (nearest even).

Data.  Integer-valued (draws in -3 .. 3, as multi_cases.arrays makes them) where alpha and beta are integers: every fp32
sum is exact, so the expected value is alpha * S in fp32, + beta * Y0, rounded once, compared BIT FOR BIT (the sign of a
zero apart, which follows the summation order).  The rows that cross a slice end have one-signed matrix values, and the
odd columns of X are one-signed, so that a hub row's sums in those columns lie far above 256 — the point past which
bf16 does not hold every integer: a kernel that rounds a carried row twice (a rounded partial plus rounded carries)
fails.  Real-valued data in [-1, 1] (rounded to the stored types first) otherwise: the per-row bound of
multi_cases.check in fp32, (len + extra) * 2^-24 * (|alpha| * sum|a x| + |beta * y0|), plus one 16-bit rounding of the
result: 2^-11 * |want| for fp16 (11 significand bits), 2^-8 * |want| for bf16 (8), plus 2^-25 absolute for fp16's
subnormal spacing (2^-24).  Padding columns of X hold NaN, those of Y a canary that must survive; with beta = 0, Y0 is
NaN."""
import collections
import functools

import numpy as np

import multi_cases as mc

VECS = ("f16", "bf16")
MATS = ("same", "f32")                  # the matrix in the vectors' type, or in fp32
OFFS = ("i32", "i64")
VAL_TYPE = {"f32": 0, "f16": 4, "bf16": 5}      # MI355_VAL_*
VEC = 8                                 # columns per 16-byte group
TILE = 64                               # widest tile = max(mc.LANES_PER_SLOT) * VEC
K = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129)
K_MAX = 129
KF = 136                                # columns of the full X / Y0 of a matrix: a case takes columns c0 .. c0 + k
CANARY = -776.0                         # exact in binary16 and in bfloat16
NAN_BITS = {"f16": 0x7E00, "bf16": 0x7FC0}
HUB = 256                               # bf16 holds every integer up to here

Case = collections.namedtuple("Case", "name matrix off vec mat integer k k_max c0 ldx ldy alpha beta shift")


# ---- the 16-bit formats, from integer operations ---------------------------------------------------------------------
def bf16_bits(a):
    """fp32 -> bfloat16 bit patterns: nearest, ties to even; overflow carries into inf; NaN stays NaN."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def to_bits(a, t):
    """fp32 -> the bit patterns of the 16-bit type t, rounded once."""
    if t == "bf16":
        return bf16_bits(a)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def from_bits(b, t):
    """The exact fp32 value of 16-bit patterns."""
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if t == "bf16":
        return (b.astype(np.uint32) << 16).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def mat_type(c):
    return c.vec if c.mat == "same" else "f32"


def tile_lanes(k):
    """Lanes per slot C of the narrowest tile that serves the last pass of k columns (launch_multi_half)."""
    groups = -(-(k % TILE or TILE) // VEC)
    return 1 if groups <= 1 else 2 if groups <= 2 else 4 if groups <= 4 else 8


def structures():
    return mc.row_end_structures() + mc.open_row_structures() + mc.slice_edge_structures() + [mc.ragged_structure()]


def carried_rows(lens, L=mc.SLICE_LEN):
    """Rows whose nonzeros lie in more than one slice (nonzero n of row r is merge item n + r)."""
    lens = np.asarray(lens, dtype=np.int64)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    r = np.arange(len(lens))
    first, last = Ap[:-1] + r, Ap[1:] - 1 + r
    return np.nonzero((lens > 0) & (first // L != last // L))[0]


# ---- operands and expected results -----------------------------------------------------------------------------------
_arrays = {}


def arrays(m, off, vec, mat, integer):
    """(Ap, Aj, Ax, X, Y0) as fp32 arrays whose every value the stored type holds exactly (Ax: vec or fp32; X, Y0: vec);
    X and Y0 have KF columns.  Made once and left unchanged."""
    key = (m.name, off, vec, mat, integer)
    if key not in _arrays:
        rng = np.random.RandomState(m.seed)
        Ap = np.zeros(len(m.lens) + 1, dtype=mc.NP[off])
        np.cumsum(m.lens, out=Ap[1:])
        nnz = int(Ap[-1])
        Aj = rng.randint(0, m.n_cols, size=nnz).astype(np.int32)
        if integer:
            draw = lambda *shape: rng.randint(-3, 4, size=shape).astype(np.float32)
        else:
            draw = lambda *shape: (rng.rand(*shape) * 2 - 1).astype(np.float32)
        Ax, X, Y0 = draw(nnz), draw(m.n_cols, KF), draw(len(m.lens), KF)
        if integer:
            for r in carried_rows(m.lens):
                Ax[Ap[r]:Ap[r + 1]] = np.abs(Ax[Ap[r]:Ap[r + 1]])
            X[:, 1::2] = np.abs(X[:, 1::2])
        else:
            if mat == "same":
                Ax = from_bits(to_bits(Ax, vec), vec)
            X, Y0 = from_bits(to_bits(X, vec), vec), from_bits(to_bits(Y0, vec), vec)
        _arrays[key] = (Ap, Aj, Ax, X, Y0)
    return _arrays[key]


def stored(a, t):
    """An fp32 array of exactly representable values as the bytes the library reads: uint16 patterns, or fp32."""
    return np.ascontiguousarray(a, dtype=np.float32) if t == "f32" else to_bits(a, t)


_refs = {}


def reference(m, vec, mat, integer):
    """Over all KF columns: the exact row sums as fp32 (integer data; they are integers below 2^24), or the pair
    (fp64 row sums, row sums of |a x|)."""
    key = (m.name, vec, mat, integer)
    if key not in _refs:
        Ap, Aj, Ax, X, _ = arrays(m, "i32", vec, mat, integer)
        Ap = Ap.astype(np.int64)
        rows = np.nonzero(np.diff(Ap))[0]

        def row_sums(P):
            out = np.zeros((len(m.lens), KF), dtype=P.dtype)
            if rows.size:
                out[rows] = np.add.reduceat(P, Ap[rows], axis=0)
            return out

        if integer:
            S = row_sums(Ax.astype(np.int64)[:, None] * X[Aj].astype(np.int64))
            assert np.abs(S).max(initial=0) < 2 ** 24
            _refs[key] = S.astype(np.float32)
        else:
            P = Ax.astype(np.float64)[:, None] * X[Aj].astype(np.float64)
            _refs[key] = (row_sums(P), row_sums(np.abs(P)))
    return _refs[key]


def _nonzero_bits(b):
    """16-bit patterns with -0 taken as +0."""
    return np.where((b & 0x7FFF) == 0, 0, b)


def is_nan_bits(b, t):
    b = np.asarray(b, dtype=np.uint16) & 0x7FFF
    return b > (0x7C00 if t == "f16" else 0x7F80)


def check(c, ybits):
    """ybits: what the execute left of Y as uint16 patterns, n_rows x ldy (padding included)."""
    m = c.matrix
    n_rows = len(m.lens)
    ybits = np.asarray(ybits, dtype=np.uint16).reshape(n_rows, c.ldy)
    got = ybits[:, :c.k]
    assert np.all(ybits[:, c.k:] == to_bits(np.float32(CANARY), c.vec)), "%s: a padding column of Y was written" % c.name
    nan = is_nan_bits(got, c.vec)
    assert not nan.any(), "%s: NaN in Y (rows %s)" % (c.name, np.unique(np.nonzero(nan)[0])[:8])
    ref = reference(m, c.vec, c.mat, c.integer)
    Y0 = arrays(m, c.off, c.vec, c.mat, c.integer)[4][:, c.c0:c.c0 + c.k]
    if c.integer:
        want = np.float32(c.alpha) * ref[:, c.c0:c.c0 + c.k]
        if c.beta != 0.0:
            want = want + np.float32(c.beta) * Y0
        assert want.dtype == np.float32
        wbits = to_bits(want, c.vec)
        bad = np.nonzero(_nonzero_bits(got) != _nonzero_bits(wbits))
        assert bad[0].size == 0, "%s: rows %s columns %s differ from the sum rounded once (got %s, want %s)" % (
            c.name, bad[0][:8], bad[1][:8], from_bits(got[bad][:8], c.vec), from_bits(wbits[bad][:8], c.vec))
        return
    y64, yabs = (a[:, c.c0:c.c0 + c.k] for a in ref)
    lens = np.asarray(m.lens, dtype=np.int64)[:, None]
    extra = 2 if (c.alpha, c.beta) == (1.0, 0.0) else 3
    y0 = Y0.astype(np.float64) if c.beta != 0.0 else np.zeros((n_rows, c.k))
    want = c.alpha * y64 + c.beta * y0
    bound = (lens + extra) * 2.0 ** -24 * (abs(c.alpha) * yabs + np.abs(c.beta * y0)) + 1e-300
    bound = bound + (2.0 ** -11 * np.abs(want) + 2.0 ** -25 if c.vec == "f16" else 2.0 ** -8 * np.abs(want))
    err = np.abs(from_bits(got, c.vec).astype(np.float64) - want)
    bad = np.nonzero(err > bound)
    assert bad[0].size == 0, "%s: rows %s columns %s outside the bound (excess %s)" % (
        c.name, bad[0][:8], bad[1][:8], (err - bound)[bad][:8])


def hub_sums(c):
    """|alpha * S + beta * Y0| of an integer case on the rows that cross a slice end (empty where there are none)."""
    rows = carried_rows(c.matrix.lens)
    S = reference(c.matrix, c.vec, c.mat, True)[rows, c.c0:c.c0 + c.k]
    Y0 = arrays(c.matrix, c.off, c.vec, c.mat, True)[4][rows, c.c0:c.c0 + c.k]
    return np.abs(np.float32(c.alpha) * S + np.float32(c.beta) * Y0)


# ---- the table ---------------------------------------------------------------------------------------------------------
SHIFTS = (mc.ALIGNED, mc.SHIFTED, mc.ALIGNED, (0, 0, 0, 1, 0), mc.ALIGNED, (0, 0, 0, 0, 1))
PADS = (0, 1, 0, 3)
COMBOS = tuple((v, t, o) for v in VECS for t in MATS for o in OFFS)


def _case(m, off, vec, mat, k, ab, pad, shift, k_max=K_MAX, c0=0, tag=""):
    alpha, beta = ab
    integer = mc.is_integer_pair(alpha, beta)
    name = "%s-%s-%s-%s-k%d-a%g-b%g-pad%d-%s%s" % (m.name, off, vec, mat, k, alpha, beta, pad, "".join(map(str, shift)), tag)
    return Case(name, m, off, vec, mat, integer, k, k_max, c0, k + pad, k + (pad + 2 if pad else 0), alpha, beta, tuple(shift))


def _sweep():
    """Per structure every k of K once; the (vector type, matrix type, offset width) combinations, alpha / beta, the
    padding and the operand offsets rotate on counters that run over the whole table, so that every combination meets
    every tile width (test: every combination occurs)."""
    out = []
    n = 0
    for m in structures()[:-1]:
        for k in K:
            vec, mat, off = COMBOS[(n + n // len(COMBOS)) % len(COMBOS)]
            out.append(_case(m, off, vec, mat, k, mc.AB_REDUCED[(n // 2) % len(mc.AB_REDUCED)], PADS[n % len(PADS)],
                             SHIFTS[n % len(SHIFTS)]))
            n += 1
    return out


def _cross(m):
    """The ragged matrix: every k x vector type x matrix type x offset width x alpha / beta; padding and operand
    offsets rotate."""
    out = []
    n = 0
    for vec, mat, off in COMBOS:
        for k in K:
            for ab in mc.AB_REDUCED:
                out.append(_case(m, off, vec, mat, k, ab, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], tag="-cross"))
                n += 1
    return out


def _stale(m, vec, mat):
    """An object of k_max = 129 executed at k = 129 and then at k = 5 on other vectors, and again with carries of
    another width: the tails and carries of the wide execute must not reach the narrow one's rows.  A sequence is
    consecutive cases of one plan key, run in table order."""
    return [_case(m, "i32", vec, mat, 129, (1.0, 0.0), 0, mc.ALIGNED, c0=0, tag="-stale0"),
            _case(m, "i32", vec, mat, 5, (1.0, 0.0), 1, mc.ALIGNED, c0=130, tag="-stale1"),
            _case(m, "i32", vec, mat, 65, (2.0, -1.0), 0, mc.ALIGNED, c0=7, tag="-stale2"),
            _case(m, "i32", vec, mat, 17, (0.0, 2.0), 3, mc.ALIGNED, c0=100, tag="-stale3")]


def plan_key(c):
    """Cases that share an object: one (structure, types, data, matrix offsets, k_max)."""
    return (c.matrix.name, c.off, c.vec, c.mat, c.integer, c.shift[:3], c.k_max)


_table = []


def table():
    """Every case, in plan order (a stable sort: the cases of a sequence keep their order)."""
    if not _table:
        ragged, edge = mc.ragged_structure(), mc.slice_edge_structures()
        by = {m.name: m for m in edge}
        seq = []
        for vec in VECS:
            seq += _stale(ragged, vec, "same") + _stale(by["slices_inside_one_row"], vec, "f32")
        _table.extend(sorted(_sweep() + _cross(ragged), key=plan_key) + seq)
    return list(_table)


def self_test():
    """What the table promises: names of their own, every combination, and carried hub rows with sums above 256."""
    t = table()
    assert len({c.name for c in t}) == len(t)
    assert 1200 <= len(t) <= 4000, len(t)
    seen = {(c.vec, c.mat, tile_lanes(c.k)) for c in t}
    assert seen == {(v, m, lanes) for v in VECS for m in MATS for lanes in mc.LANES_PER_SLOT}
    assert {(c.vec, c.mat, c.off) for c in t} == set(COMBOS)
    assert {(c.vec, c.mat, c.k) for c in t if c.matrix.family == "ragged"} >= {(v, m, k) for v in VECS for m in MATS for k in K}
    assert {c.k % VEC for c in t} == set(range(VEC)) and {-(-c.k // TILE) for c in t} == {1, 2, 3}
    assert {(c.alpha, c.beta) for c in t} == set(mc.AB_REDUCED)
    assert {c.matrix.name for c in t} == {m.name for m in structures()}
    assert {c.shift for c in t} == set(map(tuple, SHIFTS)) and {c.ldx - c.k for c in t} == set(PADS)
    assert {(c.vec, c.integer) for c in t} == {(v, i) for v in VECS for i in (False, True)}
    # carried rows far above 256 under every vector and matrix type, in slices the kernel carries through and ends in
    hubs = collections.Counter()
    for c in t:
        if c.integer and c.alpha != 0.0 and carried_rows(c.matrix.lens).size:
            h = hub_sums(c)
            if h.size and h.max() > 4 * HUB:
                hubs[(c.vec, c.mat)] += 1
    assert all(hubs[(v, m)] >= 10 for v in VECS for m in MATS), hubs
    for name in ("ragged", "slices_inside_one_row", "two_carried_rows", "one_row"):
        assert any(c.matrix.name == name and c.integer and c.alpha != 0.0 and hub_sums(c).max() > 4 * HUB for c in t), name
    return t


# ---- the host program's batch file: multi_cases' records, with X, Y0 and Y as 16-bit patterns, through create_half -------
@functools.lru_cache(maxsize=1)     # cases come in plan order: the conversion is made once per matrix record
def _stored_arrays(m, off, vec, mat, integer):
    """arrays() as the program reads them: Ax in the matrix type, X (its one variant) and Y0 as 16-bit patterns."""
    Ap, Aj, Ax, X, Y0 = arrays(m, off, vec, mat, integer)
    return Ap, Aj, stored(Ax, vec if mat == "same" else "f32"), (to_bits(X, vec),), to_bits(Y0, vec)


def batch_operands(c):
    nan = NAN_BITS[c.vec]
    return mc.Operands(plan_key(c)[:6], (c.k_max, mc.CREATE_HALF, 0), VAL_TYPE[c.vec], VAL_TYPE[mat_type(c)],
                       *_stored_arrays(c.matrix, c.off, c.vec, c.mat, c.integer), -1, 0, nan, nan,
                       int(to_bits(np.float32(CANARY), c.vec).ravel()[0]))


def write_batch(path, cases):
    return mc.write_batch(path, cases, batch_operands)


def read_results(path, cases):
    return mc.read_results(path, cases, lambda c: np.uint16)
