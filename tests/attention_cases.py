"""The table of fused sparse-attention cases (csrc/attention.hip) that tests/test_attention_sim_cpu.py executes on the host
and tests/test_gpu_attention.py on the device: the same structures, operands and expected results for both.

    v[n] = scale * dot(Q[r, :d], K[c, :d]) + bias[n];  m_r = max_row v;  l_r = sum_row exp(v - m_r)
    O[r, :dv] = (sum_row exp(v[n] - m_r) V[c, :dv]) / l_r;  lse[r] = m_r + log(l_r)

The structures are those of tests/multi_cases.py, tests/sddmm_cases.py and tests/row_softmax_cases.py (imported, not copied:
the kernel cuts its work exactly as the multi-vector kind does, SLICE_LEN merge items per wave, STEP nonzeros per group, C in
LANES_PER_SLOT lanes per slot), plus one of a single column.  Both test files assert the geometry: the host file against the
constants of csrc/attention.hip and csrc/common.hpp, the device file against info() (assert_geometry).

Expected values come from numpy in fp64 on the row-wise formulation above (expected()).  Kinds of data:
  const    Q = 0, V small integers ({-3 .. 3}), bias = c_r for every entry of row r, c_r spread over +-1e4 (variant 0; a
           kernel that forgets the max overflows), or no bias at all (variant 1).  Every v of a row is equal, so every exp
           is exp(0) = 1 — in the steps, in the folds of the open row and in every merge of the fix-up — every l is a count
           and every acc a sum of small integers: O[r] must be val(sum_row V[c]) / val(len_r), correctly rounded, whatever
           the order (bit for bit, the sign of a zero apart), and lse[r] = c_r + log(len_r) within
               eps (|lse| + 2 (E_LOG + 1) log(len_r))        (the log's E_LOG ulps and the rounding of the sum)
           exactly c_r on a row of one entry.
  masked   const variant 0 with bias = -inf at the entries of row_softmax_cases.mask(): the first and last entry of rows,
           both sides of every group and slice edge, whole pieces of crossing rows, whole rows.  Expected: the same row
           with those entries deleted — (sum over the live entries of V[c]) / val(live), and +0 (that bit pattern) and
           lse = -inf on a row without a live entry, as on an empty row.
  real     Q uniform in (-0.3, 0.3) / |scale|, K and V uniform in (-1, 1), bias = b_r + (0, 4) with b_r in (-50, 50)
           (variants 0, 1) or none (variant 2), scale in SCALES; the row spread D_r of v stays <= 20 (asserted), so
           nothing underflows.  The bound is composed of the bounds the project already states, eps the unit roundoff:
             score    dv_n = |scale| (d + 3) eps sum_j |q_j k_j| + 2 eps |v_n|                  (tests/sddmm_cases.py; the
                      + 3 holds the rounding of scale * dot, the last term the rounding of + bias)
             exp      v_n and m_r carry errors of at most Dv_r = max_row dv, but the kernel uses ONE computed m_r in the
                      numerator and in l_r, so it cancels: p_n = exp(v_n) / sum_k exp(v_k), and an error of at most Dv_r in
                      every v moves p_n by at most the relative 2 Dv_r — twice the score error, absolute, as a relative
                      error of p                                                (first order; Dv_r is ~1e-5 at most)
             softmax  p_n = exp(v_n - m_r) / l_r computed from those v: relative eps (2 len_r + 2 E + 2 (max_row |v| + D_r) + 4),
                      E = 3                                                         (tests/row_softmax_cases.py; the count
                      holds the rescales of the merges and the divide, wherever in the row they are applied)
             sum      sum_row p_n V[c, j] in any order: (len_r + 2) eps sum_row p_n |V[c, j]|   (the multi-vector kind's
                      row bound)
           together, with rho_r = 2 Dv_r + eps (2 len_r + 2 E + 2 (max_row |v| + D_r) + 4):
               |O[r, j] - want| <= (rho_r + (len_r + 2) eps) sum_row p_n |V[c, j]|  +  the smallest normal
               |lse[r] - want|  <= Dv_r + rho_r + eps (2 E_LOG |log l_r| + 2 |lse[r]|)
           (lse: the error of m_r; the relative error of l_r under that m_r, which rho_r holds; the log's ulps; the rounding of the sum).  Nothing in it
           is measured; E_LOG = 3 is the OpenCL full-profile bound for log, as E is for exp.
In EVERY case a row of one live entry must give O[r] = V[c] bit for bit.  Padding columns of Q, K and V hold NaN; O starts
as a canary that must survive in its padding columns (and, on the device, behind every operand); lse starts as NaN."""
import collections
import struct

import numpy as np

import multi_cases as mc
import row_softmax_cases as rc
import sddmm_cases as sc
from multi_cases import LANES_PER_SLOT, NP, SLICE_LEN, STEP, TILE, VEC, bits, slices  # noqa: F401

CANARY = -777.25
E_EXP, E_LOG = 3, 3
SCALES = (1.0, 0.125, -2.0)
KF = 104                            # columns of the full Q / K of a data set: a case takes columns c0 .. c0 + d
KV = 72                             # columns of the full V: a case takes columns cv0 .. cv0 + dv
ALL_TYPES = mc.ALL_TYPES
EPS, TINY = rc.EPS, rc.TINY
# dv: below a tile, every C, a non-tile width, the widest tile, two and three passes
DV_ALL = {"f32": (1, 3, 4, 8, 16, 23, 32, 33, 65), "f64": (1, 2, 4, 8, 11, 16, 17, 33)}
# d: 1, below a tile, a tile, one and two rounds of the tile loop (and more under a narrow dv), a non-multiple
D_ALL = {"f32": (1, 3, 4, 8, 32, 64, 45, 100), "f64": (1, 2, 4, 16, 32, 23, 50)}
# the (d, dv) pairs that every structure rotates through: every C with one round, two rounds and a remainder of the loop
PAIRS = {"f32": ((1, 1), (8, 4), (3, 8), (32, 16), (64, 32), (45, 23), (16, 33), (100, 3), (4, 65), (33, 32)),
         "f64": ((1, 1), (4, 2), (2, 4), (16, 8), (32, 16), (23, 11), (8, 17), (50, 2), (2, 33), (17, 16))}
# element offsets of Ap, Aj, Q, K, V, bias, O, lse from an aligned base
ALIGNED, SHIFTED = (0,) * 8, (1,) * 8
SHIFTS = (ALIGNED, SHIFTED, (0, 0, 1, 0, 0, 0, 0, 0), (0, 0, 0, 1, 0, 0, 0, 0), (0, 0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 0, 0, 1, 1, 0),
          (0, 0, 0, 0, 0, 0, 1, 1))
PADS = ((0, 0, 0, 0), (1, 3, 2, 1), (3, 0, 0, 4), (0, 2, 1, 0), (4, 4, 4, 4))     # (ldq - d, ldk - d, ldv - dv, ldo - dv)

Matrix = sc.Matrix
# kind: "const" | "masked" | "real"; variant: the bias's, the mask's or the draw's; ld*: leading dimensions
Case = collections.namedtuple("Case", "name matrix off val kind variant scale d dv c0 cv0 ldq ldk ldv ldo want_lse shift")


def assert_geometry(info, val):
    """info() of a plan of value type `val` agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["widest_tile"] == max(LANES_PER_SLOT) * VEC[val] == TILE[val]
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    assert info["passes"] == -(-info["dv_max"] // TILE[val])
    assert info["lanes_per_slot"] == lanes_per_slot(min(info["dv_max"], TILE[val]), val)
    assert info["main_kernel"] == "attention_slice_kernel"


def lanes_per_slot(dv, val):
    """C of a pass over a tile of dv columns: as the multi-vector kind chooses its tile."""
    groups = -(-dv // VEC[val])
    return next((c for c in LANES_PER_SLOT if groups <= c), max(LANES_PER_SLOT))


# ---- structures --------------------------------------------------------------------------------------------------------
def one_column_structure():
    """n_cols = 1: every entry gathers the one row of K and V."""
    return Matrix("one_col", "one_col", (3, 0, 70, 1, 1300, 0, 2), 1, 700)


def structures(family):
    if family == "one_col":
        return [one_column_structure()]
    return rc.structures(family)


STRUCTURE_FAMILIES = ("row_ends", "open_row", "slice_edges", "ragged", "hub", "empty_runs", "position", "pow2", "one_col")


def rows_of(m):
    return np.repeat(np.arange(len(m.lens)), m.lens)


_csr = {}


def csr(m, off):
    """(Ap, Aj): random columns (the position structures: those of tests/sddmm_cases.py)."""
    key = (m.name, off)
    if key not in _csr:
        if m.family == "position":
            Ap, Aj = sc.arrays(m, off, "f32", True)[:2]
        else:
            Ap = np.zeros(len(m.lens) + 1, dtype=NP[off])
            np.cumsum(m.lens, out=Ap[1:])
            Aj = np.random.RandomState(m.seed + 3).randint(0, max(m.n_cols, 1), size=int(Ap[-1])).astype(np.int32)
        _csr[key] = (Ap, Aj)
    return _csr[key]


# ---- operands and expected results -------------------------------------------------------------------------------------
_operands = {}


def data_key(c):
    return (c.matrix.name, c.val, c.kind, c.variant, c.scale if c.kind == "real" else 0.0)


def operands(c):
    """(Q, K, V, bias) of a case's data set in its value type: Q is n_rows x KF, K n_cols x KF, V n_cols x KV, bias nnz
    values or None.  Made once and left unchanged."""
    key = data_key(c)
    if key in _operands:
        return _operands[key]
    m, T = c.matrix, NP[c.val]
    n_rows, nnz, rows = len(m.lens), sum(m.lens), rows_of(m)
    rng = np.random.RandomState(m.seed * 37 + c.variant * 11 + ("const", "masked", "real").index(c.kind) + 2000)
    K = (rng.rand(m.n_cols, KF) * 2 - 1).astype(T)
    if c.kind in ("const", "masked"):
        Q = np.zeros((n_rows, KF), dtype=T)
        V = rng.randint(-3, 4, size=(m.n_cols, KV)).astype(T)
        bias = rc.row_constants(m)[rows].astype(T) if (c.kind == "masked" or c.variant == 0) else None
        if c.kind == "masked":
            bias[rc.mask(m, c.variant)] = -np.inf
    else:
        Q = ((rng.rand(n_rows, KF) * 2 - 1) * (0.3 / abs(c.scale))).astype(T)
        V = (rng.rand(m.n_cols, KV) * 2 - 1).astype(T)
        bias = (rng.uniform(-50, 50, size=n_rows)[rows] + rng.rand(nnz) * 4).astype(T) if c.variant != 2 else None
    _operands[key] = (Q, K, V, bias)
    return _operands[key]


_expected = {}


def expected(c):
    """In fp64 from the operands as stored: dict of want (n_rows x dv), lse, live (unmasked entries per row), and for real
    data the bounds on O and lse.  Computed once per (data set, widths)."""
    key = data_key(c) + (c.off, c.d, c.dv, c.c0, c.cv0, c.scale)
    if key in _expected:
        return _expected[key]
    m = c.matrix
    Ap, Aj = csr(m, c.off)
    Q, K, V, bias = operands(c)
    n_rows, rows, lens = len(m.lens), rows_of(m), np.asarray(m.lens, dtype=np.int64)
    eps = EPS[c.val]
    scale = float(NP[c.val](c.scale))
    q = Q[:, c.c0:c.c0 + c.d].astype(np.float64)[rows]
    k = K[:, c.c0:c.c0 + c.d].astype(np.float64)[Aj]
    x = V[:, c.cv0:c.cv0 + c.dv].astype(np.float64)[Aj]
    dot, dabs = (q * k).sum(1), np.abs(q * k).sum(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = scale * dot + (bias.astype(np.float64) if bias is not None else 0.0)
        masked = np.isneginf(v)
        top = np.full(n_rows, -np.inf)
        np.maximum.at(top, rows, v)
        e = np.where(masked, 0.0, np.exp(v - np.where(np.isneginf(top), 0.0, top)[rows]))
        l = np.bincount(rows, weights=e, minlength=n_rows)
        p = e / np.where(l > 0, l, 1.0)[rows]
        live = np.bincount(rows, weights=~masked, minlength=n_rows).astype(np.int64)
        want, pabs = np.zeros((n_rows, c.dv)), np.zeros((n_rows, c.dv))
        for j in range(c.dv):
            want[:, j] = np.bincount(rows, weights=p * np.where(masked, 0.0, x[:, j]), minlength=n_rows)
            pabs[:, j] = np.bincount(rows, weights=p * np.where(masked, 0.0, np.abs(x[:, j])), minlength=n_rows)
        lse = np.where(l > 0, top + np.log(np.where(l > 0, l, 1.0)), -np.inf)
        res = dict(want=want, lse=lse, live=live, l=l)
        if c.kind == "real":
            fin = np.where(masked, np.nan, v)
            lo, hi = np.full(n_rows, np.inf), np.full(n_rows, -np.inf)
            np.fmin.at(lo, rows, fin)
            np.fmax.at(hi, rows, fin)
            vmax = np.where(hi >= lo, np.maximum(np.abs(lo), np.abs(hi)), 0.0)
            spread = np.where(hi >= lo, hi - lo, 0.0)
            dv_n = abs(scale) * (c.d + 3) * eps * dabs + 2 * eps * np.abs(v)
            Dv = np.zeros(n_rows)
            np.maximum.at(Dv, rows, dv_n)
            rho = 2 * Dv + eps * (2 * lens + 2 * E_EXP + 2 * (vmax + spread) + 4)
            res.update(spread=spread, bound=(rho + (lens + 2) * eps)[:, None] * pabs + TINY[c.val],
                       lse_bound=Dv + rho + eps * (2 * E_LOG * np.abs(np.log(np.where(l > 0, l, 1.0))) + 2 * np.abs(np.where(l > 0, lse, 0.0))))
    _expected[key] = res
    return res


def exact_bits(a):
    """The bit patterns as they are (the +0 of a row without a live entry must be +0)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(c, O, lse, ratios=None):
    """O: the n_rows x dv values an execute left; lse: its n_rows values, or None where the case asks for none.  ratios: a
    list that takes the largest error / bound of a real case (the device file records it)."""
    m, T = c.matrix, NP[c.val]
    n_rows, lens = len(m.lens), np.asarray(m.lens, dtype=np.int64)
    O = np.asarray(O)
    assert O.shape == (n_rows, c.dv) and O.dtype == T, c.name
    assert not np.any(np.isnan(O)), "%s: NaN in O (rows %s)" % (c.name, np.nonzero(np.isnan(O).any(1))[0][:8])
    assert (lse is not None) == bool(c.want_lse), c.name
    ex = expected(c)
    Ap, Aj = csr(m, c.off)
    Vc = operands(c)[2][:, c.cv0:c.cv0 + c.dv]
    dead = ex["live"] == 0
    assert np.all(exact_bits(O[dead]) == 0), "%s: a row without a live entry is not +0 (rows %s)" % (c.name, np.nonzero(dead)[0][:8])
    # a row of one live entry: V[c] bit for bit
    one = np.nonzero((lens == 1) & (ex["live"] == 1))[0]
    if one.size:
        assert np.array_equal(exact_bits(O[one]), exact_bits(Vc[Aj[Ap[one].astype(np.int64)]])), "%s: a row of one entry is not V[c]" % c.name
    if lse is not None:
        lse = np.asarray(lse)
        assert lse.shape == (n_rows,) and lse.dtype == T and not np.any(np.isnan(lse)), c.name
        assert np.all(np.isneginf(lse[dead])) and not np.any(np.isinf(lse[~dead])), "%s: lse of the rows without a live entry" % c.name
    eps = EPS[c.val]
    if c.kind in ("const", "masked"):
        # the fp64 sum is exact; the divide in the value type is the correctly rounded quotient
        total = np.rint(ex["want"] * np.maximum(ex["live"], 1)[:, None])
        exact = total.astype(T) / np.maximum(ex["live"], 1).astype(T)[:, None]
        bad = np.nonzero((bits(O) != bits(exact)).any(1))[0]
        assert bad.size == 0, "%s: rows %s differ from the exact value (got %s, want %s)" % (c.name, bad[:8], O[bad[:4]], exact[bad[:4]])
        if lse is not None:
            ok = ~dead
            bound = eps * (np.abs(ex["lse"][ok]) + 2 * (E_LOG + 1) * np.log(ex["live"][ok]))
            err = np.abs(lse[ok].astype(np.float64) - ex["lse"][ok])
            assert np.all(err <= bound), "%s: lse outside the bound (rows %s)" % (c.name, np.nonzero(ok)[0][np.nonzero(err > bound)[0][:8]])
            single = ok & (ex["live"] == 1)
            assert np.all(lse[single].astype(np.float64) == ex["lse"][single]), "%s: lse of a row of one live entry is not v" % c.name
        return
    assert ex["spread"].max() <= 20.0, c.name
    err = np.abs(O.astype(np.float64) - ex["want"])
    ratio = float((err / ex["bound"]).max()) if err.size else 0.0
    bad = np.nonzero((err > ex["bound"]).any(1))[0]
    assert bad.size == 0, "%s: rows %s outside the bound (largest error / bound %g)" % (c.name, bad[:8], ratio)
    if lse is not None:
        ok = ~dead
        lerr = np.abs(lse[ok].astype(np.float64) - ex["lse"][ok])
        lratio = float((lerr / ex["lse_bound"][ok]).max()) if lerr.size else 0.0
        assert np.all(lerr <= ex["lse_bound"][ok]), "%s: lse outside the bound (largest error / bound %g)" % (c.name, lratio)
        ratio = max(ratio, lratio)
    if ratios is not None:
        ratios.append(ratio)


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, off, val, kind, variant, scale, d, dv, pad=PADS[0], shift=ALIGNED, want_lse=True, tag=""):
    c0 = 0 if d > KF - 4 else d % 5
    cv0 = 0 if dv > KV - 8 else dv % 7
    name = "%s-%s-%s-%s%d-s%g-d%d-dv%d-pad%s-%s-lse%d%s" % (m.name, off, val, kind, variant, scale, d, dv, ".".join(map(str, pad)),
                                                           "".join(map(str, shift)), int(want_lse), tag)
    return Case(name, m, off, val, kind, variant, float(scale), d, dv, c0, cv0, d + pad[0], d + pad[1], dv + pad[2], dv + pad[3],
                bool(want_lse), tuple(shift))


KINDS = (("const", 0, 1.0), ("const", 1, -2.0), ("masked", 0, 1.0), ("masked", 1, 0.125), ("real", 0, 1.0), ("real", 1, 0.125),
         ("real", 2, -2.0))


def structure_cases(m, types, n0=0):
    """What every structure is put through, per (offset width, value type) of `types`: both const data sets, both masks,
    real data under every scale; widths, padding and operand offsets rotate; every seventh case asks for no lse."""
    out, n = [], n0
    for off, val in types:
        for kind, variant, scale in KINDS:
            d, dv = PAIRS[val][n % len(PAIRS[val])]
            out.append(_case(m, off, val, kind, variant, scale, d, dv, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], n % 7 != 5))
            n += 1
    return out


def width_cases():
    """Every dv and every d on the ragged structure, const and real data."""
    m, out, n = structures("ragged")[0], [], 0
    for val in ("f32", "f64"):
        for i, dv in enumerate(DV_ALL[val]):
            d = D_ALL[val][i % len(D_ALL[val])]
            for kind, variant, scale in (("const", 0, 1.0), ("real", n % 3, SCALES[n % 3])):
                out.append(_case(m, ("i32", "i64")[n % 2], val, kind, variant, scale, d, dv, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], True, "-w"))
                n += 1
        for i, d in enumerate(D_ALL[val]):
            dv = DV_ALL[val][(i + 3) % len(DV_ALL[val])]
            out.append(_case(m, ("i32", "i64")[n % 2], val, "real", n % 3, SCALES[n % 3], d, dv, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], True, "-w"))
            n += 1
    return out


def alignment_pairs():
    """[(aligned case, the same case with every operand one element off a 16-byte boundary)]: equal bit for bit."""
    out = []
    for m in (structures("ragged")[0], structures("slice_edges")[4]):
        for val in ("f32", "f64"):
            for i, (d, dv) in enumerate(PAIRS[val][1::2]):
                off = ("i32", "i64")[i % 2]
                out.append((_case(m, off, val, "real", i % 3, SCALES[i % 3], d, dv, PADS[0], ALIGNED, True, "-align"),
                            _case(m, off, val, "real", i % 3, SCALES[i % 3], d, dv, PADS[0], SHIFTED, True, "-align")))
    return out


def repeat_pairs():
    """[(a case, the same case once more on the same plan)]: equal bit for bit."""
    out, n = [], 0
    for fam in ("ragged", "hub"):
        for m in structures(fam):
            for val in ("f32", "f64"):
                d, dv = PAIRS[val][6 if n % 2 else 4]
                off = ("i32", "i64")[n % 2]
                n += 1
                out.append((_case(m, off, val, "real", 0, 0.125, d, dv, PADS[1], ALIGNED, True, "-repeat"),
                            _case(m, off, val, "real", 0, 0.125, d, dv, PADS[1], ALIGNED, True, "-repeat-again")))
    return out


def hub_sequence():
    """On ONE plan of the hub row, in this order: const data (every merge of the 30-slice fix-up chain is exp(0)), other
    operands behind it, a wide dv of three passes, then a narrow one."""
    m, out = structures("hub")[0], []
    for off, val in (("i32", "f32"), ("i64", "f64")):
        wide, narrow = (65, 3) if val == "f32" else (33, 1)
        for kind, variant, scale, d, dv in (("const", 0, 1.0, 8, TILE[val]), ("real", 0, 1.0, 8, TILE[val]), ("masked", 1, 0.125, 5, wide),
                                            ("real", 1, 0.125, 40, wide), ("real", 2, -2.0, 40, narrow), ("const", 1, -2.0, 3, narrow)):
            out.append(_case(m, off, val, kind, variant, scale, d, dv, PADS[0], ALIGNED, True, "-seq"))
    return out


FAMILIES = STRUCTURE_FAMILIES + ("widths", "alignment", "repeat", "hub_sequence")


def two_types(i):
    return (ALL_TYPES[0], ALL_TYPES[1]) if i % 2 == 0 else (ALL_TYPES[2], ALL_TYPES[3])


def family(name):
    """The cases of one family, in plan order: cases of one (matrix, types, matrix offsets) share a plan, and keep the
    order they have here."""
    if name == "widths":
        return width_cases()
    if name == "alignment":
        return [c for pair in alignment_pairs() for c in pair]
    if name == "repeat":
        return [c for pair in repeat_pairs() for c in pair]
    if name == "hub_sequence":
        return hub_sequence()
    out = []
    for i, m in enumerate(structures(name)):
        out += structure_cases(m, ALL_TYPES if name in ("ragged", "hub", "pow2", "one_col") else two_types(i), 3 * i)
    return out


def plan_key(c):
    return (c.matrix.name, c.off, c.val, c.shift[:2])


def table():
    return [c for f in FAMILIES for c in family(f)]


def weight(g):
    """Of a plan group, to deal the groups to batches: merge items times the lanes' work per nonzero."""
    return sum((len(c.matrix.lens) + sum(c.matrix.lens)) * -(-c.dv // TILE[c.val]) * (2 + c.d // 16) + 3000 for c in g)


# ---- the host program's batch file (tests/cpp/attention_sim.cpp, whose header comment has the records) -------------------
NAN_BITS = {"f32": 0x7FC00000, "f64": 0x7FF8000000000000}
VAL_TYPE = mc.VAL_TYPE
# What write_batch and read_results ask of a case.  plan_key / data_key: cases of one key share a matrix / data record;
# feat_type: the MI355_VAL_* of Q, K, V and O; Ap, Aj; Q, K, V (kf, kf and kv columns) and bias (or None) as operands() has
# them, and to_bits, which makes the bytes of Q, K and V of them; dtype / side_dtype: an element of O / of lse as the
# program writes it; nan, canary, side_nan: the bit patterns that the padding of Q, K and V, all of O and lse start with.
Batch = collections.namedtuple("Batch", "plan_key data_key feat_type Ap Aj Q K V bias to_bits dtype side_dtype nan canary side_nan")


def batch_operands(c):
    T = NP[c.val]
    return Batch(plan_key(c), data_key(c), VAL_TYPE[c.val], *csr(c.matrix, c.off), *operands(c), np.ascontiguousarray, T, T, NAN_BITS[c.val],
                 mc.word_of(CANARY, T), NAN_BITS[c.val])


def write_batch(path, cases, operands=batch_operands):
    """Cases in plan order; returns them in the order their results come back."""
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    last, last_data = None, None
    with open(path, "wb") as f:
        for c in cases:
            o = operands(c)
            if o.plan_key != last:
                last, last_data = o.plan_key, None
                f.write(words(1, ("i32", "i64").index(c.off), o.feat_type, len(c.matrix.lens), c.matrix.n_cols, int(o.Ap[-1]), c.shift[0], c.shift[1],
                              o.Q.shape[1], o.V.shape[1]))
                f.write(o.Ap.tobytes())
                f.write(o.Aj.tobytes())
            if o.data_key != last_data:
                last_data = o.data_key
                f.write(words(2, o.Q.shape[1], o.V.shape[1], int(o.bias is not None)))
                for a in (o.Q, o.K, o.V):
                    f.write(o.to_bits(a).tobytes())
                if o.bias is not None:
                    assert o.bias.dtype == o.side_dtype
                    f.write(o.bias.tobytes())
            f.write(words(4, c.d, c.dv, c.c0, c.cv0, c.ldq, c.ldk, c.ldv, c.ldo, *c.shift[2:], int(c.want_lse), o.nan, o.canary, o.side_nan))
            f.write(struct.pack("<d", c.scale))
        f.write(words(0))
    return list(cases)


def read_results(path, cases, operands=batch_operands):
    """[(status, padding elements of O that lost their canary, O, lse or None)] per case; raises if the file is not complete."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            o = operands(c)
            st, bad, count = struct.unpack("<3q", f.read(24))
            n_rows = len(c.matrix.lens)
            assert count == n_rows * c.dv, c.name
            O = np.frombuffer(f.read(count * np.dtype(o.dtype).itemsize), dtype=o.dtype).reshape(n_rows, c.dv)
            lse = np.frombuffer(f.read(n_rows * np.dtype(o.side_dtype).itemsize), dtype=o.side_dtype)
            out.append((st, bad, O, lse if c.want_lse else None))
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return out
