"""The table of multi-vector SpMV cases over semirings, int32 values and pattern matrices (csrc/multi_kernels.hpp) that
tests/test_multi_semiring_sim_cpu.py executes on the host and tests/test_gpu_multi_semiring.py on the device: the same
structures, operands and expected results for both.

The structures are those of tests/multi_cases.py (row ends on every slot and step boundary, the open-row state machine,
items within 2 of a slice end, slices of row ends only and of one row only, carried rows, the ragged matrix).  Over
them: semiring x {f32, f64, i32} x {valued, pattern}, one k per tile width and masked-remainder class plus one k of
two passes (K), with the (semiring, valued / pattern) pairs, the offset widths, padded ldx / ldy, operands one element
off a 16-byte boundary and — (+, *) on the float types only — alpha / beta rotating over the cases.

Data: integer-valued in {-3 .. 3} (zeros included: (or, and) sees both outcomes) or real-valued in (-1, 1); int32 is
always integer-valued.  Under (min, +) on floats a tenth of X is +inf, under (max, +) -inf (unreached vertices); no
infinities under the two x semirings, no NaN.  The reference is Oracle.spmv_genl_serial per column, with Ax = ones of
the vector type for a pattern case.  Integer-valued data: bit for bit (-0 taken as +0, multi_cases.bits).
Real-valued data under (min, +), (max, *), (max, +), (or, and): bit for bit as well — a product is one rounding and
min / max do not round.  Real-valued (+, *): the per-row bound of multi_cases.check.  Padding columns of X hold NaN
(int32: a large value), those of Y a canary that must survive; Y is poisoned before every call (NaN; int32: a value
that would win the semiring's reduce), which under a semiring other than (+, *) also proves that Y is not read."""
import collections

import numpy as np

import multi_cases as mc

SEMIRINGS = ("plus_times", "min_plus", "max_times", "max_plus", "or_and")      # MI355_SEMIRING_* in order
VALS = ("f32", "f64", "i32")
VAL_TYPE = {"f32": 0, "f64": 1, "i32": 2}       # MI355_VAL_*
VAL_PATTERN = 3
VEC = {"f32": 4, "f64": 2, "i32": 4}            # columns per 16-byte group
TILE = {"f32": 32, "f64": 16, "i32": 32}        # widest tile
# one k per lanes-per-slot C in (1, 2, 4, 8) and per masked remainder class (k mod VEC), and one k of two passes
K = {"f32": mc.K_REDUCED["f32"], "f64": mc.K_REDUCED["f64"], "i32": mc.K_REDUCED["f32"]}
K_MAX = {"f32": 65, "f64": 33, "i32": 65}
KF = mc.KF
CANARY = mc.CANARY
X_PAD_I32 = 1515870810                          # what a padding column of an int32 X holds
Y_POISON_I32 = {"plus_times": 1515870810, "min_plus": -2000000000, "max_times": 2000000000, "max_plus": 2000000000,
                "or_and": 7}
PAIRS = tuple((s, p) for s in SEMIRINGS for p in (False, True))     # (semiring, pattern)

Case = collections.namedtuple("Case", "name matrix off val integer k k_max c0 ldx ldy alpha beta shift semiring pattern")


def tile_lanes(val, k):
    """Lanes per slot C of the narrowest tile that serves the last pass of k columns (launch_multi)."""
    cols = k % TILE[val] or TILE[val]
    groups = -(-cols // VEC[val])
    return 1 if groups <= 1 else 2 if groups <= 2 else 4 if groups <= 4 else 8


def structures():
    return mc.row_end_structures() + mc.open_row_structures() + mc.slice_edge_structures() + [mc.ragged_structure()]


# ---- operands ------------------------------------------------------------------------------------------------------------
_x = {}


def x_kind(c):
    """0 = X as drawn; 1 = a tenth of it +inf ((min, +) on floats); 2 = -inf ((max, +) on floats)."""
    if c.val == "i32":
        return 0
    return {"min_plus": 1, "max_plus": 2}.get(c.semiring, 0)


def x_variants(m, off, val, integer):
    """(X, X with +inf, X with -inf): KF columns each, the infinities in the same tenth of the entries."""
    key = (m.name, val, integer)
    if key not in _x:
        X = mc.arrays(m, off, val, integer)[3]
        if val == "i32":
            _x[key] = (X, X, X)
        else:
            mask = np.random.RandomState(m.seed + 9000).rand(*X.shape) < 0.1
            _x[key] = (X, np.where(mask, mc.NP[val](np.inf), X), np.where(mask, mc.NP[val](-np.inf), X))
    return _x[key]


def operands(c):
    """(Ap, Aj, Ax, X of the case's semiring, Y0): X and Y0 have KF columns.  Made once and left unchanged."""
    Ap, Aj, Ax, _, Y0 = mc.arrays(c.matrix, c.off, c.val, c.integer)
    return Ap, Aj, Ax, x_variants(c.matrix, c.off, c.val, c.integer)[x_kind(c)], Y0


def y_poison(c):
    return float("nan") if c.val != "i32" else Y_POISON_I32[c.semiring]


def x_pad(c):
    return float("nan") if c.val != "i32" else X_PAD_I32


# ---- expected results ------------------------------------------------------------------------------------------------------
_refs = {}


def reference(orc, c, col):
    """Column `col` of the full X through the serial oracle: the semiring's result in the value type, or for real-valued
    (+, *) the pair (fp64 sum, sum |a x|)."""
    real_sum = c.semiring == "plus_times" and not c.integer
    key = (c.matrix.name, c.val, c.integer, c.semiring, c.pattern, col)
    if key not in _refs:
        Ap, Aj, Ax, X, _ = operands(c._replace(off="i32"))
        if c.pattern:
            Ax = np.ones_like(Ax)
        x = np.ascontiguousarray(X[:, col])
        _refs[key] = orc.spmv_ref64(Ap, Aj, Ax, x) if real_sum else orc.spmv_genl_serial(SEMIRINGS.index(c.semiring), Ap, Aj, Ax, x)
    return _refs[key]


def bits(a):
    """multi_cases.bits; int32 values as they are."""
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.int32 else mc.bits(a)


def check(orc, c, ybuf):
    """ybuf: what the execute left of Y, n_rows x ldy (padding included)."""
    m = c.matrix
    n_rows = len(m.lens)
    V = mc.NP[c.val]
    ybuf = np.asarray(ybuf).reshape(n_rows, c.ldy)
    got = ybuf[:, :c.k]
    assert np.all(ybuf[:, c.k:] == V(CANARY)), "%s: a padding column of Y was written" % c.name
    if c.val != "i32":
        assert not np.any(np.isnan(got)), "%s: NaN in Y (rows %s)" % (c.name, np.unique(np.nonzero(np.isnan(got))[0])[:8])
    Y0 = mc.arrays(m, c.off, c.val, c.integer)[4][:, c.c0:c.c0 + c.k]
    if c.semiring != "plus_times" or c.integer:
        for j in range(c.k):
            want = reference(orc, c, c.c0 + j)
            if c.semiring == "plus_times" and (c.alpha, c.beta) != (1.0, 0.0):
                want = V(c.alpha) * want
                if c.beta != 0.0:
                    want = want + V(c.beta) * Y0[:, j]
            bad = np.nonzero(bits(got[:, j]) != bits(want))[0]
            assert bad.size == 0, "%s: column %d differs from the serial oracle in rows %s (got %s, want %s)" % (
                c.name, j, bad[:8], got[bad[:8], j], want[bad[:8]])
        return
    eps = 2.0 ** -24 if c.val == "f32" else 2.0 ** -53
    lens = np.asarray(m.lens, dtype=np.int64)
    extra = 2 if (c.alpha, c.beta) == (1.0, 0.0) else 3
    for j in range(c.k):
        y64, yabs = reference(orc, c, c.c0 + j)
        y0 = Y0[:, j].astype(np.float64) if c.beta != 0.0 else np.zeros(n_rows)
        want = c.alpha * y64 + c.beta * y0
        bound = (lens + extra) * eps * (abs(c.alpha) * yabs + np.abs(c.beta * y0)) + 1e-300
        err = np.abs(got[:, j].astype(np.float64) - want)
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, "%s: column %d outside the bound in rows %s (excess %s)" % (c.name, j, bad[:8], (err - bound)[bad[:8]])


# ---- the table -------------------------------------------------------------------------------------------------------------
SHIFTS = (mc.ALIGNED, mc.SHIFTED, mc.ALIGNED, (0, 0, 0, 1, 0), mc.ALIGNED, (0, 0, 0, 0, 1))
PADS = (0, 1, 0, 3)
OFFS = ("i32", "i64")


def _case(m, off, val, semiring, pattern, integer, k, ab, pad, shift, k_max=None, c0=0, tag=""):
    alpha, beta = ab
    name = "%s-%s-%s-%s-%s-%s-k%d-a%g-b%g-pad%d-%s%s" % (m.name, off, val, semiring, "pat" if pattern else "val",
                                                        "int" if integer else "real", k, alpha, beta, pad,
                                                        "".join(map(str, shift)), tag)
    return Case(name, m, off, val, integer, k, k_max or K_MAX[val], c0, k + pad, k + (pad + 2 if pad else 0), alpha, beta,
                tuple(shift), semiring, pattern)


def _sweep():
    """Per structure and value type, every k of K under two (semiring, valued / pattern) pairs; the pairs, offset
    widths, padding, operand offsets, integer / real data and alpha / beta rotate on counters that run over the whole
    table, so that every pair meets every tile width of every value type (test: every combination occurs)."""
    out = []
    n = 0
    for m in structures():
        for val in VALS:
            for k in K[val]:
                for _ in range(2):
                    semiring, pattern = PAIRS[(n + n // len(PAIRS)) % len(PAIRS)]
                    ab = (1.0, 0.0)
                    integer = val == "i32" or (n // 3) % 2 == 0
                    if semiring == "plus_times" and val != "i32":
                        ab = mc.AB_REDUCED[(n // 2) % len(mc.AB_REDUCED)]
                        integer = mc.is_integer_pair(*ab) and (n // 7) % 2 == 0
                    out.append(_case(m, OFFS[(n // 5) % 2], val, semiring, pattern, integer, k, ab, PADS[n % len(PADS)],
                                     SHIFTS[n % len(SHIFTS)]))
                    n += 1
    return out


def _sequences():
    """On one object: a narrow execute after a wide one (other vectors: no stale carries of the columns beyond k), and a
    set_semiring between two executes (no stale carries across semirings).  A sequence is consecutive cases of one
    plan key, run in table order."""
    ragged, edge = mc.ragged_structure(), mc.slice_edge_structures()[0]
    out = []
    for m, val, pattern in ((ragged, "f32", False), (edge, "f64", True), (ragged, "i32", True), (edge, "i32", False)):
        for seq, (s1, s2) in enumerate((("min_plus", "min_plus"), ("max_plus", "or_and"), ("plus_times", "min_plus"),
                                        ("or_and", "max_times"))):
            tag = "-seq%d" % seq
            out += [_case(m, "i32", val, s1, pattern, True, 33, (1.0, 0.0), 0, mc.ALIGNED, k_max=33, tag=tag + "a"),
                    _case(m, "i32", val, s2, pattern, True, 5, (1.0, 0.0), 1, mc.ALIGNED, k_max=33, c0=40, tag=tag + "b"),
                    _case(m, "i32", val, s1, pattern, val == "i32", 33, (1.0, 0.0), 0, mc.ALIGNED, k_max=33, tag=tag + "c"),
                    _case(m, "i32", val, s2, pattern, val == "i32", 17, (1.0, 0.0), 3, (0, 0, 0, 1, 1), k_max=33, c0=40, tag=tag + "d")]
    return out


def plan_key(c):
    """Cases that share an object: one (structure, types, valued / pattern, data, matrix offsets, k_max)."""
    return (c.matrix.name, c.off, c.val, c.integer, c.shift[:3], c.pattern, c.k_max)


_table = []


def table():
    """Every case, in plan order (a stable sort: the cases of a sequence keep their order)."""
    if not _table:
        _table.extend(sorted(_sweep(), key=plan_key) + _sequences())
    return list(_table)


# ---- the host program's batch file: multi_cases' records, through create_typed and set_semiring -------------------------
def batch_operands(c):
    Ap, Aj, Ax, _, Y0 = operands(c)
    V = mc.NP[c.val]        # (the canary of an int32 Y is V(CANARY) = -777, as check() has it)
    return mc.Operands((c.matrix.name, c.off, c.val, c.integer, c.shift[:3]), (c.k_max, mc.CREATE_TYPED, int(c.pattern)),
                       VAL_TYPE[c.val], VAL_TYPE[c.val], Ap, Aj, Ax, x_variants(c.matrix, c.off, c.val, c.integer), Y0,
                       SEMIRINGS.index(c.semiring), x_kind(c), mc.word_of(x_pad(c), V), mc.word_of(y_poison(c), V), mc.word_of(CANARY, V))


def write_batch(path, cases):
    return mc.write_batch(path, cases, batch_operands)


read_results = mc.read_results
