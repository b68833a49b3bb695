"""The table of SDDMM cases with 16-bit U and V (csrc/sddmm_half_kernel.hpp, mi355_spmv_sddmm_create_half) that
tests/test_sddmm_half_sim_cpu.py executes on the host and tests/test_gpu_sddmm_half.py on the device: the same
structures, operands and expected results for both.

    out[n] = alpha * s[n] * sum_{j < k} float(U[r(n), j]) * float(V[Aj[n], j]) + beta * out[n],   s = Ax, or 1 without values

U and V are binary16 or bfloat16; Ax, out and the arithmetic are fp32.  The structures are those of tests/sddmm_cases.py,
imported: row ends on every slot and step boundary, the open-row state machine, items within 2 of a slice end, the ragged
matrix, the hub row of 30 000 nonzeros, runs of more than SLICE_LEN empty rows, dup / base / moved.  A lane's 16 bytes are
VEC = 8 columns, so C in LANES_PER_SLOT lanes per slot give tiles of 8 / 16 / 32 / 64 columns; both test files assert
that geometry (the host file against the sources, the device file against info()).

k: every k of 1 .. 65 and 128, 129, 200 on the ragged matrix (every C, every k mod 8, the tile boundary at 64 / 65, four
tiles) x both offset widths x both 16-bit types x valued / pattern; elsewhere K_REDUCED: one k per C and per remainder
class, one of two tiles, one of four.

Operands are drawn in fp32 and U and V are rounded to the 16-bit type FIRST (multi_half_cases' conversions): what the
library reads is what expected() widens.  Expected values are fp64 on the widened values.  Integer data ({-3 .. 3},
integer alpha / beta: every value is exact in both 16-bit types, and every partial sum, product and scaling in fp32 for
k <= 200 — nothing exceeds 2 * 3 * (200 * 9) + 2 * 3, far below 2^24) is compared bit for bit, the sign of a zero apart.  Real data in (-1, 1) is
held to sddmm_cases' bound with eps = 2^-24:
    |got - want| <= |alpha| (k + 3) eps |s| sum_j |u_j v_j| + 2 eps (|alpha d| + |beta out_old| + |want|),   d = s * dot
derived, not measured: the product of two 16-bit values (at most 11 significand bits each) is exact in fp32, so an fma
per column rounds once per column as the fp32 kernel's does, and the tree, the multiplication by s and the scaling are
what the bound already counts.  Padding columns of U and V hold NaN; with beta = 0, out starts as NaN and no NaN may
remain; on the device a canary behind out[nnz - 1] must survive."""
import collections

import numpy as np

import sddmm_cases as sc
from multi_half_cases import NAN_BITS, VAL_TYPE, from_bits, to_bits  # noqa: F401
from sddmm_cases import (AB_REDUCED, ALIGNED, CANARY, LANES_PER_SLOT, NP, SHIFTED, SLICE_LEN, STEP, bits,  # noqa: F401
                         is_integer_pair, ragged_structure)

VECS = ("f16", "bf16")
OFFS = ("i32", "i64")
VEC = 8                             # columns per 16-byte group
TILE = 64                           # widest tile = max(LANES_PER_SLOT) * VEC
KF = 204                            # columns of the full U / V of a matrix: a case takes columns c0 .. c0 + k
K_ALL = tuple(range(1, 66)) + (128, 129, 200)
# one k per C and per masked remainder class (k mod 8) — 1 .. 8 under C = 1, and each remainder again under some C > 1 with
# both numbers of live column groups where C allows two — one k of two tiles (65) and one of four (200)
K_REDUCED = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 22, 27, 32, 33, 39, 45, 52, 58, 63, 64, 65, 200)
K_HUB = (1, 8, 13, 16, 30, 64, 65, 200)
K_POSITION = (3, 8, 13, 16, 29, 64, 65, 129)
# element offsets of Ap, Aj, Ax, U, V, out from a 16-byte boundary: sddmm_cases' (all, U alone, V alone, out alone) and Ax
# alone; an element of U and V is 2 bytes.  Nine of them: coprime to the rotations of type, width and valued / pattern
SHIFTS = sc.SHIFTS + ((0, 0, 1, 0, 0, 0), ALIGNED)
PADS = sc.PADS + ((8, 16),)         # (ldu - k, ldv - k); the last keeps rows of k % 8 == 0 aligned under padding

Case = collections.namedtuple("Case", "name matrix off vec integer k c0 ldu ldv alpha beta valued shift")


def assert_geometry(info):
    """info() of a 16-bit plan agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    assert info["main_kernel"] == "sddmm_half_slice_kernel"
    assert info["val_type"] == VAL_TYPE["f32"]


def lanes_per_slot(k):
    """C of an execute: from ceil(k / 8) alone."""
    groups = -(-k // VEC)
    return next((c for c in LANES_PER_SLOT if groups <= c), max(LANES_PER_SLOT))


# ---- operands ----------------------------------------------------------------------------------------------------------
_arrays = {}


def arrays(m, off, vec, integer):
    """(Ap, Aj, Ax, O0, U, V) of a matrix, all values fp32: Ax and O0 (nnz each) as the library reads them, U and V (KF
    columns) holding only values the 16-bit type `vec` has.  Made once and left unchanged.  The position structures
    are made as tests/sddmm_cases.py makes them: Ax a function of (row, column), `moved` = a prefix in front of `base`."""
    key = (m.name, off, vec, integer)
    if key in _arrays:
        return _arrays[key]
    rng = np.random.RandomState(m.seed)
    Ap = np.zeros(len(m.lens) + 1, dtype=NP[off])
    np.cumsum(m.lens, out=Ap[1:])
    nnz = int(Ap[-1])
    if integer:
        draw = lambda *shape: rng.randint(-3, 4, size=shape).astype(np.float32)
        held = draw
    else:
        draw = lambda *shape: (rng.rand(*shape) * 2 - 1).astype(np.float32)
        held = lambda *shape: from_bits(to_bits(draw(*shape), vec), vec)     # rounded to the stored type first
    rows = np.repeat(np.arange(len(m.lens)), m.lens)
    if m.name == "dup":
        Aj = np.concatenate([np.tile(rng.randint(0, m.n_cols, size=n // 2), 2) for n in m.lens] + [np.zeros(0, int)]).astype(np.int32)
        Ax, O0, U, V = sc.pair_value(rows, Aj, integer, "f32"), draw(nnz), held(len(m.lens), KF), held(m.n_cols, KF)
    elif m.name == "moved":
        bAp, bAj, bAx, bO0, bU, bV = arrays(sc.position_structures()[1], off, vec, integer)
        pre = int(sum(sc._MOVED_PREFIX))
        Aj = np.concatenate([rng.randint(0, m.n_cols, size=pre).astype(np.int32), bAj])
        Ax, O0 = sc.pair_value(rows - len(sc._MOVED_PREFIX), Aj, integer, "f32"), np.concatenate([draw(pre), bO0])
        U, V = np.concatenate([held(len(sc._MOVED_PREFIX), KF), bU]), bV
    else:
        Aj = rng.randint(0, m.n_cols, size=nnz).astype(np.int32)
        Ax = sc.pair_value(rows, Aj, integer, "f32") if m.name == "base" else draw(nnz)
        O0, U, V = draw(nnz), held(len(m.lens), KF), held(m.n_cols, KF)
    for a in (Ax, O0, U, V):
        assert a.dtype == np.float32
    assert np.array_equal(from_bits(to_bits(U, vec), vec), U) and np.array_equal(from_bits(to_bits(V, vec), vec), V)
    _arrays[key] = (Ap, Aj, Ax, O0, U, V)
    return _arrays[key]


def expected(c):
    """(want, bound) of a case in fp64 on the widened values; bound is None for integer data (want is then exact)."""
    Ap, Aj, Ax, O0, U, V = arrays(c.matrix, c.off, c.vec, c.integer)
    rows = np.repeat(np.arange(len(c.matrix.lens)), c.matrix.lens)
    u = U[:, c.c0:c.c0 + c.k].astype(np.float64)[rows]
    v = V[:, c.c0:c.c0 + c.k].astype(np.float64)[Aj]
    s = Ax.astype(np.float64) if c.valued else np.ones(len(Aj))
    dot, dabs = (u * v).sum(1), np.abs(u * v).sum(1)
    old = c.beta * O0.astype(np.float64) if c.beta != 0.0 else np.zeros(len(Aj))
    want = c.alpha * (s * dot) + old
    if c.integer:
        return want, None
    eps = 2.0 ** -24
    bound = abs(c.alpha) * (c.k + 3) * eps * np.abs(s) * dabs + 2 * eps * (np.abs(c.alpha * s * dot) + np.abs(old) + np.abs(want))
    return want, bound


def check(c, out, slack=1):
    """out: the nnz fp32 values an execute left.  slack multiplies the bound of real data (2: a value that another
    execute within the bound computed is compared, tests/test_gpu_sddmm_half.py)."""
    out = np.asarray(out)
    assert out.shape == (sum(c.matrix.lens),) and out.dtype == np.float32, c.name
    assert not np.any(np.isnan(out)), "%s: NaN in out (entries %s)" % (c.name, np.nonzero(np.isnan(out))[0][:8])
    want, bound = expected(c)
    if c.integer:
        bad = np.nonzero(bits(out) != bits(want.astype(np.float32)))[0]
        assert bad.size == 0, "%s: entries %s differ from the exact value (got %s, want %s)" % (c.name, bad[:8], out[bad[:8]], want[bad[:8]])
        return
    err = np.abs(out.astype(np.float64) - want)
    bad = np.nonzero(err > slack * bound)[0]
    assert bad.size == 0, "%s: entries %s outside the bound (excess %s)" % (c.name, bad[:8], (err - slack * bound)[bad[:8]])


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, off, vec, k, ab, pad, shift, valued, tag=""):
    alpha, beta = ab
    c0 = 0 if k > KF - 4 else (k % 5)
    name = "%s-%s-%s-k%d-a%g-b%g-pad%d.%d-%s-%s%s" % (m.name, off, vec, k, alpha, beta, pad[0], pad[1], "".join(map(str, shift)),
                                                     "valued" if valued else "pattern", tag)
    return Case(name, m, off, vec, is_integer_pair(alpha, beta), k, c0, k + pad[0], k + pad[1], alpha, beta, bool(valued), tuple(shift))


class _Rotation:
    """alpha / beta, padding, operand offsets, offset width, valued / pattern and the 16-bit type, rotating with periods
    5, 12, 9, 2, 4 and 8: every combination of (type, width, valued) comes round every 8 cases."""

    def __init__(self):
        self.n = 0

    def case(self, m, k, tag=""):
        n = self.n
        self.n += 1
        return _case(m, OFFS[n % 2], VECS[(n // 4) % 2], k, AB_REDUCED[n % len(AB_REDUCED)], PADS[(n // 2) % len(PADS)],
                     SHIFTS[n % len(SHIFTS)], (n // 2) % 2 == 0, tag)


def reduced(ms):
    rot = _Rotation()
    return [rot.case(m, k) for m in ms for k in K_REDUCED]


def ragged_cross():
    """Every k x both offset widths x both 16-bit types x valued / pattern; alpha / beta, padding and operand offsets rotate."""
    m, out, n = ragged_structure(), [], 0
    for vec in VECS:
        for k in K_ALL:
            for off in OFFS:
                for valued in (True, False):
                    out.append(_case(m, off, vec, k, AB_REDUCED[n % len(AB_REDUCED)], PADS[(n // 4) % len(PADS)],
                                     SHIFTS[n % len(SHIFTS)], valued, "-cross"))
                    n += 1
    return out


def alignment_pairs():
    """[(aligned case, the same case with every operand one ELEMENT off a 16-byte boundary)]: equal bit for bit."""
    m, out = ragged_structure(), []
    for vec in VECS:
        for i, k in enumerate(K_REDUCED):
            off, ab = OFFS[i % 2], ((-0.75, 3.0), (2.5, 0.0))[i % 2]
            out.append((_case(m, off, vec, k, ab, (0, 0), ALIGNED, True, "-align"), _case(m, off, vec, k, ab, (0, 0), SHIFTED, True, "-align")))
    return out


def hub_cases():
    rot, m = _Rotation(), sc.hub_structure()
    return [rot.case(m, k) for k in K_HUB + K_HUB[::-1]]        # (twice: each k under both 16-bit types)


def position_cases():
    """Real data, beta = 0, valued (Ax a function of (row, column)) and pattern; every structure under the same k, types
    and scaling, so that outputs can be compared across structures."""
    out = []
    for m in sc.position_structures():
        for vec in VECS:
            for i, k in enumerate(K_POSITION):
                out.append(_case(m, OFFS[i % 2], vec, k, (2.5, 0.0), (0, 0), ALIGNED, i % 2 == 0, "-pos"))
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
            n = np.arange(sum(sc._BASE_LENS), dtype=np.int64)
            out.append((c, moved, n, n + sum(sc._MOVED_PREFIX)))
    assert len(out) == 2 * len(VECS) * len(K_POSITION)
    return out


FAMILIES = sc.FAMILIES


def family(name):
    """The cases of one family, in plan order: consecutive cases of one (matrix, types, data, matrix offsets) share a plan."""
    if name == "row_ends":
        out = reduced(sc.row_end_structures())
    elif name == "open_row":
        out = reduced(sc.open_row_structures())
    elif name == "slice_edges":
        out = reduced(sc.slice_edge_structures())
    elif name == "ragged_cross":
        out = ragged_cross()
    elif name == "alignment":
        out = [c for pair in alignment_pairs() for c in pair]
    elif name == "hub":
        out = hub_cases()
    elif name == "empty_runs":
        out = reduced([sc.empty_run_structure()])
    elif name == "position":
        out = position_cases()
    else:
        raise KeyError(name)
    return sorted(out, key=plan_key)


def plan_key(c):
    return (c.matrix.name, c.off, c.vec, c.integer, c.shift[:3])


_table = []


def table():
    if not _table:
        _table.extend(c for f in FAMILIES for c in family(f))
    return list(_table)


def self_test():
    """What the table promises."""
    t = table()
    assert len({c.name for c in t}) == len(t) > 1000
    assert max(sum(c.matrix.lens) for c in t) < 60000
    ragged = [c for c in t if c.name.endswith("-cross")]
    for vec in VECS:
        for k in K_ALL:
            assert {(c.off, c.valued) for c in ragged if c.vec == vec and c.k == k} == {(o, v) for o in OFFS for v in (True, False)}
    assert K_ALL[:65] == tuple(range(1, 66)) and set(K_ALL[65:]) == {128, 129, 200}
    assert {(lanes_per_slot(k), k % VEC) for k in K_REDUCED if k <= TILE} >= {(1, r % VEC) for r in range(1, 9)}
    assert {k % VEC for k in K_REDUCED if k > VEC} == set(range(VEC))
    assert {lanes_per_slot(k) for k in K_REDUCED} == set(LANES_PER_SLOT)
    assert {-(-k // TILE) for k in K_REDUCED} >= {1, 2, 4} and {-(-k // TILE) for k in K_ALL} >= {1, 2, 3, 4}
    for name in {c.matrix.name for c in t}:
        sub = [c for c in t if c.matrix.name == name]
        assert {(c.vec, c.off) for c in sub} == {(v, o) for v in VECS for o in OFFS}, name
        assert {c.valued for c in sub} == {True, False}, name
    assert {(c.alpha, c.beta) for c in t} >= set(AB_REDUCED)
    assert {c.shift for c in t} == set(SHIFTS) >= {SHIFTED, (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1)}
    for sh in set(SHIFTS):
        assert {(c.vec, c.valued) for c in t if c.shift == sh} == {(v, w) for v in VECS for w in (True, False)}, sh
    assert any(c.ldu % VEC and c.ldu > c.k for c in t) and any(c.ldv % VEC and c.ldv > c.k for c in t)
    assert any(c.ldu % VEC == 0 and c.ldu > c.k for c in t) and any(c.ldv % VEC == 0 and c.ldv > c.k for c in t)
    assert {(c.vec, c.integer) for c in t} == {(v, i) for v in VECS for i in (False, True)}
    return t


# ---- the host program's batch file: sddmm_cases' records, with U and V as 16-bit patterns and fp32 results ---------------
def batch_operands(c):
    Ap, Aj, Ax, O0, U, V = arrays(c.matrix, c.off, c.vec, c.integer)
    return plan_key(c), VAL_TYPE[c.vec], (Ap, Aj, Ax, O0, to_bits(U, c.vec), to_bits(V, c.vec)), NAN_BITS[c.vec]


def write_batch(path, cases):
    return sc.write_batch(path, cases, batch_operands)


def read_results(path, cases):
    return sc.read_results(path, cases, lambda c: np.float32)
