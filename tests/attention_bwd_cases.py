"""The table of fused attention-backward cases (csrc/attention_bwd.hip) that tests/test_attention_bwd_sim_cpu.py executes on
the host and tests/test_gpu_attention_bwd.py on the device: the same structures, operands and expected results for both.

    v[n] = scale * dot(Q[r], K[c]) + bias[n];  p[n] = v[n] == -inf ? 0 : exp(v[n] - lse[r])
    delta[r] = dot(dO[r], O[r]);  dp[n] = dot(dO[r], V[c]);  ds[n] = p[n] (dp[n] - delta[r])
    dQ[r] = scale sum_row ds K[c];  dK[c] = scale sum_col ds Q[r];  dV[c] = sum_col p dO[r];  dbias[n] = ds[n]

The structures are those of tests/attention_cases.py (which imports those of the multi-vector, SDDMM and row-softmax tables),
each used on BOTH sides: side "A" takes the structure as A (the DQ walk meets its edges), side "T" takes A := the structure
transposed, so that A^T — what the DK and DV walks run on — is the structure itself, row lengths, slice and step edges and
all.  Both test files assert the geometry: the host file against the constants of csrc/attention_bwd.hip, the device file
against info() (assert_geometry).

Expected values come from numpy in fp64 on the formulas above (expected()), from the SAME O and lse the kernel is given.
Kinds of data:
  exact    variant 0: Q = 0, variant 1: K = 0 (then dQ = 0 and dK is the structural output); variant 2: variant 0 where every
           third row has Q[r, 0] = -(the largest finite value) against K[:, 0] = 2, a finite bias and lse = -inf: the score
           is -inf on its own, the entry counts as masked, and only the test on v keeps -inf - -inf from being formed.  bias[n] = lse[r] = a constant
           per row spread over +-1e4, so v = lse and p = exp(0) = 1 exactly.  The other operands are small integers (K or Q
           in {-2 .. 2}; V, O, dO in {-1, 0, 1}) and scale is a power of two, so dp, delta, ds and every partial sum are
           integers below 2^24 (130 * 2 * 30 000 on the hub row): all three outputs and dbias must EQUAL the reference
           whatever the order of addition (the sign of a zero apart).
  masked   exact variant 0 (mask variant 0) or 1 (mask variant 1: K = 0, so dK carries values under a mask) with bias = -inf at the entries of row_softmax_cases.mask() of the structure (carried to A's
           order on side T): the first and last entry of lines, both sides of every group and slice edge, whole pieces of
           crossing lines, whole lines.  Expected: the matrix with those entries deleted.  The rows of K and V that only
           masked entries touch hold NaN; a row of A masked whole has lse = -inf.  No NaN may come out, and a line without
           a live entry is +0 (that bit pattern).
  single   rows of at most one entry with the true O = V[c] and lse = v, on integers: p = 1, dp = delta, ds = 0, so
           dQ = dK = 0 and dV[c] = sum over the column of dO[r], exactly.
  real     Q uniform in (-0.3, 0.3) / |scale|, K, V and dO uniform in (-1, 1), bias = b_r + (0, 4) with b_r in (-50, 50)
           (variants 0, 1) or none (variant 2), scale in SCALES: the forward table's ranges, the row spread of v <= 20
           (asserted).  O and lse are the fp64 forward rounded to the value type.
In EVERY case a line of A (dQ) or of A^T (dK, dV) without a live entry must be +0.

The bound of a real case is composed of the bounds the project already states, u the unit roundoff, first order in u:
  score    dv_n = |scale| (d + 3) u sum_j |q_j k_j| + 2 u |v_n|                                   (tests/sddmm_cases.py)
  exp      the argument v_n - lse_r carries dv_n and the rounding of the subtraction, u |v_n - lse_r|; exp turns an absolute
           error of its argument into a relative error of p, and adds its own E = 3 ulps = 2 E u:
               rho_n = dv_n + u |v_n - lse_r| + 2 E u                          (E as tests/row_softmax_cases.py, OpenCL's)
  dots     dp_n and delta_r are dots over dv in fixed orders: e_dp_n = (dv + 2) u sum_j |dO_rj V_cj|,
           e_delta_r = (dv + 2) u sum_j |dO_rj O_rj|                            (the dot bound of tests/sddmm_cases.py)
  ds       ds = p (dp - delta): e_ds_n = p_n ((e_dp_n + e_delta_r) + (rho_n + 2 u) |dp_n - delta_r|)
           (the 2 u: the roundings of the subtraction and the product)
  sums     a line's sum of len terms coef_n x_nj in any order: (len + 2) u sum_n |coef_n x_nj|    (the multi-vector kind's
           row bound, which holds the rounding of each product), on top of the coefficients' own errors:
               |dQ[r, j] - want| <= sum_row |scale| (e_ds_n + u |ds_n|) |K[c, j]| + (len_r + 2) u sum_row |scale ds_n K[c, j]|
               |dK[c, j] - want| <= sum_col |scale| (e_ds_n + u |ds_n|) |Q[r, j]| + (len_c + 2) u sum_col |scale ds_n Q[r, j]|
               |dV[c, j] - want| <= sum_col p_n rho_n |dO[r, j]|                  + (len_c + 2) u sum_col p_n |dO[r, j]|
               |dbias[n] - want| <= e_ds_n
           (the u |ds_n|: the rounding of scale * ds), each plus (len + 2) times the smallest normal for products that
           leave the normal range.  Nothing in it is measured.
Padding columns of the inputs hold NaN; the outputs start as a canary that must survive in their padding columns (and, on
the device, behind every operand)."""
import collections
import struct

import numpy as np

import attention_cases as ac
import row_softmax_cases as rc
from multi_cases import LANES_PER_SLOT, NP, SLICE_LEN, STEP, TILE, VEC, bits, word_of  # noqa: F401

CANARY = -777.25
E_EXP = 3
SCALES = ac.SCALES
EPS, TINY = rc.EPS, rc.TINY
ALL_TYPES = ac.ALL_TYPES
# (d, dv): independent; 1, below a tile, every C, non-tile widths, the widest tile, two and three passes, d != dv both ways
# (the dot over the OTHER width then runs fewer and more rounds than the output tile has lanes)
PAIRS = {"f32": ((1, 1), (8, 4), (3, 8), (32, 16), (16, 32), (45, 23), (16, 33), (100, 3), (4, 65), (33, 32), (65, 5), (2, 40)),
         "f64": ((1, 1), (4, 2), (2, 4), (16, 8), (8, 16), (23, 11), (8, 17), (50, 2), (2, 33), (17, 16), (33, 3), (1, 20))}
PADS = ((0,) * 8, (1, 3, 2, 1, 2, 1, 3, 2), (3, 0, 0, 4, 0, 2, 0, 1), (4,) * 8)   # ld - width of Q, K, V, O, dO, dQ, dK, dV
NEED_ALL = (1, 1, 1)

Matrix = ac.Matrix
# side: "A" | "T"; kind: "exact" | "masked" | "single" | "real"; need: which of dQ, dK, dV; shift: every operand's element offset
Case = collections.namedtuple("Case", "name matrix side off val kind variant scale d dv pad shift need want_dbias")


def lanes_per_slot(width, val):
    return ac.lanes_per_slot(min(width, TILE[val]), val)


def assert_geometry(info, val):
    """info() of a plan of value type `val` agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["widest_tile"] == max(LANES_PER_SLOT) * VEC[val] == TILE[val]
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    widths = {"dq": info["d_max"], "dk": info["d_max"], "dv": info["dv_max"]}
    for role, w in widths.items():
        assert info["passes"][role] == -(-w // TILE[val])
        assert info["lanes_per_slot"][role] == lanes_per_slot(w, val)
    assert info["main_kernel"] == "attention_bwd_slice_kernel"


# ---- structures --------------------------------------------------------------------------------------------------------
def single_structure():
    """Rows of zero or one entry over seven columns: the columns are long lines that cross slices."""
    rng = np.random.RandomState(77)
    return Matrix("single", "single", tuple(int(x) for x in (rng.rand(2600) < 0.8)), 7, 977)


STRUCTURE_FAMILIES = ac.STRUCTURE_FAMILIES


def structures(family):
    return [single_structure()] if family == "single" else ac.structures(family)


def transpose(n_rows, n_cols, Ap, Aj):
    """(Apt, Ajt, perm) as mi355_spmv_csr_transpose defines them: inside a column, ascending source slot."""
    perm = np.argsort(Aj, kind="stable")
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))
    Apt = np.zeros(n_cols + 1, dtype=Ap.dtype)
    np.cumsum(np.bincount(Aj, minlength=n_cols), out=Apt[1:])
    return Apt, rows[perm].astype(np.int32), perm


_csr = {}


def csr(c):
    """(n_rows, n_cols, Ap, Aj, src): A of a case; src[n] = the structure's CSR slot behind A's slot n."""
    key = (c.matrix.name, c.side, c.off)
    if key not in _csr:
        m = c.matrix
        Ap, Aj = ac.csr(m, c.off)
        n_rows, n_cols = len(m.lens), m.n_cols
        if c.side == "T":
            Apt, Ajt, perm = transpose(n_rows, n_cols, Ap, Aj)
            _csr[key] = (n_cols, n_rows, Apt, Ajt, perm)
        else:
            _csr[key] = (n_rows, n_cols, Ap, Aj, np.arange(len(Aj)))
    return _csr[key]


# ---- operands and expected results -------------------------------------------------------------------------------------
_operands = {}


def data_key(c):
    return (c.matrix.name, c.side, c.off, c.val, c.kind, c.variant, c.scale, c.d, c.dv)


def operands(c):
    """dict of Q, K, V, O, dO (2-D, exactly d / dv columns), lse and bias (or None), in the case's value type.  Made once
    and left unchanged."""
    key = data_key(c)
    if key in _operands:
        return _operands[key]
    n_rows, n_cols, Ap, Aj, src = csr(c)
    T, nnz = NP[c.val], len(Aj)
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))
    rng = np.random.RandomState(c.matrix.seed * 41 + c.variant * 13 + c.d * 7 + c.dv + ("exact", "masked", "single", "real").index(c.kind) + 3000)
    ints = lambda lo, hi, shape: rng.randint(lo, hi + 1, size=shape).astype(T)
    if c.kind in ("exact", "masked"):
        Q = np.zeros((n_rows, c.d), dtype=T) if c.variant != 1 else ints(-2, 2, (n_rows, c.d))
        K = ints(-2, 2, (n_cols, c.d)) if c.variant != 1 else np.zeros((n_cols, c.d), dtype=T)
        V, O, dO = ints(-1, 1, (n_cols, c.dv)), ints(-1, 1, (n_rows, c.dv)), ints(-1, 1, (n_rows, c.dv))
        lse = (rng.randint(-40000, 40001, size=n_rows) * 0.25).astype(T)
        bias = lse[rows].copy()
        if c.kind == "exact" and c.variant == 2:
            # every third row with entries: the score itself reaches -inf in the value type under a finite bias
            gone = (np.arange(n_rows) % 3 == 1) & (np.diff(Ap.astype(np.int64)) > 0)
            Q[gone, 0], K[:, 0] = -np.finfo(T).max, 2
            bias[gone[rows]], lse[gone] = 0, -np.inf
        if c.kind == "masked":
            dead = rc.mask(c.matrix, c.variant)[src]
            bias[dead] = -np.inf
            live_rows = np.bincount(rows, weights=~dead, minlength=n_rows) > 0
            lse[~live_rows & (np.diff(Ap.astype(np.int64)) > 0)] = -np.inf
            live_cols = np.bincount(Aj, weights=~dead, minlength=n_cols) > 0
            K[~live_cols & (np.bincount(Aj, minlength=n_cols) > 0)] = np.nan
            V[~live_cols & (np.bincount(Aj, minlength=n_cols) > 0)] = np.nan
    elif c.kind == "single":
        assert np.diff(Ap.astype(np.int64)).max() <= 1
        Q, K = ints(-2, 2, (n_rows, c.d)), ints(-2, 2, (n_cols, c.d))
        V, dO = ints(-3, 3, (n_cols, c.dv)), ints(-3, 3, (n_rows, c.dv))
        bias = ints(-5, 5, (nnz,))
        v = float(T(c.scale)) * (Q.astype(np.float64)[rows] * K.astype(np.float64)[Aj]).sum(1) + bias
        O, lse = np.zeros((n_rows, c.dv), dtype=T), np.full(n_rows, -np.inf, dtype=T)
        O[rows], lse[rows] = V[Aj], v.astype(T)
    else:
        Q = ((rng.rand(n_rows, c.d) * 2 - 1) * (0.3 / abs(c.scale))).astype(T)
        K, V = (rng.rand(n_cols, c.d) * 2 - 1).astype(T), (rng.rand(n_cols, c.dv) * 2 - 1).astype(T)
        dO = (rng.rand(n_rows, c.dv) * 2 - 1).astype(T)
        bias = (rng.uniform(-50, 50, size=n_rows)[rows] + rng.rand(nnz) * 4).astype(T) if c.variant != 2 else None
        # the true forward in fp64 on the operands as stored, rounded to the value type
        v = float(T(c.scale)) * (Q.astype(np.float64)[rows] * K.astype(np.float64)[Aj]).sum(1) + (bias.astype(np.float64) if bias is not None else 0.0)
        top = np.full(n_rows, -np.inf)
        np.maximum.at(top, rows, v)
        e = np.exp(v - top[rows])
        l = np.bincount(rows, weights=e, minlength=n_rows)
        with np.errstate(divide="ignore", invalid="ignore"):
            lse = np.where(l > 0, top + np.log(np.where(l > 0, l, 1.0)), -np.inf).astype(T)
        O = np.zeros((n_rows, c.dv))
        pe = e / np.where(l > 0, l, 1.0)[rows]
        for j in range(c.dv):
            O[:, j] = np.bincount(rows, weights=pe * V[Aj, j].astype(np.float64), minlength=n_rows)
        O = O.astype(T)
    _operands[key] = dict(Q=Q, K=K, V=V, O=O, dO=dO, lse=lse, bias=bias)
    return _operands[key]


def _line_sums(index, n, weights):
    """sum of the rows of `weights` (nnz x width) per line index -> n x width"""
    out = np.zeros((n, weights.shape[1]))
    for j in range(weights.shape[1]):
        out[:, j] = np.bincount(index, weights=weights[:, j], minlength=n)
    return out


_expected = {}


def expected(c):
    """In fp64 from the operands as stored: dict of dQ, dK, dV, dbias, the live entries per row and per column, and for real
    data the bounds.  Computed once per data set."""
    key = data_key(c)
    if key in _expected:
        return _expected[key]
    n_rows, n_cols, Ap, Aj, _ = csr(c)
    ops = operands(c)
    f = lambda a: a.astype(np.float64)
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))
    u, tiny = EPS[c.val], TINY[c.val]
    scale = float(NP[c.val](c.scale))
    with np.errstate(invalid="ignore", over="ignore"):
        dead = np.isneginf(f(ops["bias"])) if ops["bias"] is not None else np.zeros(len(Aj), dtype=bool)
        z = lambda a: np.where(dead[:, None], 0.0, a)       # (a masked entry's rows are never loaded)
        q, k, x = z(f(ops["Q"])[rows]), z(f(ops["K"])[Aj]), z(f(ops["V"])[Aj])
        g = z(f(ops["dO"])[rows])
        dabs = np.abs(q * k).sum(1)
        top = float(np.finfo(NP[c.val]).max)
        # (the dot and scale * dot are values of the value type before + bias: beyond its range they are infinities)
        inf_beyond = lambda a: np.where(np.abs(a) > top, np.sign(a) * np.inf, a)
        sv = inf_beyond(scale * inf_beyond((q * k).sum(1)))
        v = np.where(dead, -np.inf, sv + (np.where(dead, 0.0, f(ops["bias"])) if ops["bias"] is not None else 0.0))
        dead = np.isneginf(v)               # masked by its bias, or a score that is -inf on its own
        lse = f(ops["lse"])[rows]
        p = np.where(dead, 0.0, np.exp(np.where(dead, 0.0, v - np.where(dead, 0.0, lse))))
        dp = (g * x).sum(1)
        delta = (f(ops["dO"]) * f(ops["O"])).sum(1)[rows]
        ds = np.where(dead, 0.0, p * (dp - np.where(dead, 0.0, delta)))
    res = dict(dQ=scale * _line_sums(rows, n_rows, ds[:, None] * k), dK=scale * _line_sums(Aj, n_cols, ds[:, None] * q),
               dV=_line_sums(Aj, n_cols, p[:, None] * g), dbias=ds,
               live_rows=np.bincount(rows, weights=~dead, minlength=n_rows).astype(np.int64),
               live_cols=np.bincount(Aj, weights=~dead, minlength=n_cols).astype(np.int64))
    if c.kind == "real":
        len_r, len_c = np.diff(Ap.astype(np.int64)), np.bincount(Aj, minlength=n_cols)
        lo, hi = np.full(n_rows, np.inf), np.full(n_rows, -np.inf)
        np.minimum.at(lo, rows, v)
        np.maximum.at(hi, rows, v)
        res["spread"] = np.where(hi >= lo, hi - lo, 0.0)
        dv_n = abs(scale) * (c.d + 3) * u * dabs + 2 * u * np.abs(v)
        rho = dv_n + u * np.abs(v - lse) + 2 * E_EXP * u
        e_dp = (c.dv + 2) * u * np.abs(g * x).sum(1)
        e_delta = ((c.dv + 2) * u * np.abs(f(ops["dO"]) * f(ops["O"])).sum(1))[rows]
        e_ds = p * ((e_dp + e_delta) + (rho + 2 * u) * np.abs(dp - delta))
        ce = abs(scale) * (e_ds + u * np.abs(ds))
        res["bound"] = dict(
            dQ=_line_sums(rows, n_rows, ce[:, None] * np.abs(k)) + ((len_r + 2) * u)[:, None] * _line_sums(rows, n_rows, np.abs(scale * ds)[:, None] * np.abs(k))
            + ((len_r + 2) * tiny)[:, None],
            dK=_line_sums(Aj, n_cols, ce[:, None] * np.abs(q)) + ((len_c + 2) * u)[:, None] * _line_sums(Aj, n_cols, np.abs(scale * ds)[:, None] * np.abs(q))
            + ((len_c + 2) * tiny)[:, None],
            dV=_line_sums(Aj, n_cols, (p * rho)[:, None] * np.abs(g)) + ((len_c + 2) * u)[:, None] * _line_sums(Aj, n_cols, p[:, None] * np.abs(g))
            + ((len_c + 2) * tiny)[:, None],
            dbias=e_ds + tiny)
    _expected[key] = res
    return res


def _lines(flags):
    return flags if flags.ndim == 1 else flags.any(1)


def exact_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(c, dQ, dK, dV, dbias, ratios=None):
    """The outputs an execute left (compact; None where the case does not ask for one).  ratios: a list that takes the
    largest error / bound of a real case (the device file records it)."""
    n_rows, n_cols, Ap, Aj, _ = csr(c)
    ex, T = expected(c), NP[c.val]
    got = dict(dQ=dQ, dK=dK, dV=dV, dbias=dbias)
    shapes = dict(dQ=(n_rows, c.d), dK=(n_cols, c.d), dV=(n_cols, c.dv), dbias=(len(Aj),))
    asked = dict(dQ=c.need[0], dK=c.need[1], dV=c.need[2], dbias=c.want_dbias)
    if c.kind == "real":
        assert ex["spread"].max() <= 20.0, c.name
    for name in ("dQ", "dK", "dV", "dbias"):
        a = got[name]
        assert (a is not None) == bool(asked[name]), "%s: %s" % (c.name, name)
        if a is None:
            continue
        a = np.asarray(a)
        assert a.shape == shapes[name] and a.dtype == T, "%s: %s" % (c.name, name)
        assert not np.any(np.isnan(a)), "%s: NaN in %s (lines %s)" % (c.name, name, np.nonzero(_lines(np.isnan(a)))[0][:8])
        if name != "dbias":
            none = (ex["live_rows"] if name == "dQ" else ex["live_cols"]) == 0
            assert np.all(exact_bits(a[none]) == 0), "%s: a line of %s without a live entry is not +0 (lines %s)" % (
                c.name, name, np.nonzero(none)[0][:8])
        if c.kind != "real":
            want = ex[name].astype(T)
            assert np.array_equal(want.astype(np.float64), ex[name]), "%s: the reference of %s is not exact in the value type" % (c.name, name)
            bad = np.nonzero(_lines(a != want))[0]
            assert bad.size == 0, "%s: lines %s of %s differ from the exact value (got %s, want %s)" % (c.name, bad[:8], name, a[bad[:3]], want[bad[:3]])
            continue
        err = np.abs(a.astype(np.float64) - ex[name])
        bound = ex["bound"][name]
        ratio = float((err / bound).max()) if err.size else 0.0
        assert np.all(err <= bound), "%s: %s outside the bound (largest error / bound %g)" % (c.name, name, ratio)
        if ratios is not None:
            ratios.append(ratio)


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, side, off, val, kind, variant, scale, d, dv, pad=PADS[0], shift=0, need=NEED_ALL, want_dbias=True, tag=""):
    name = "%s-%s-%s-%s-%s%d-s%g-d%d-dv%d-pad%s-sh%d-need%s-db%d%s" % (m.name, side, off, val, kind, variant, scale, d, dv, ".".join(map(str, pad)),
                                                                       shift, "".join(map(str, need)), int(want_dbias), tag)
    return Case(name, m, side, off, val, kind, variant, float(scale), d, dv, tuple(pad), shift, tuple(need), bool(want_dbias and need[0]))


KINDS = (("exact", 0, 0.5), ("exact", 1, -2.0), ("masked", 0, 1.0), ("masked", 1, 0.125), ("real", 0, 1.0), ("real", 1, 0.125), ("real", 2, -2.0))


def structure_cases(m, types, n0=0):
    """What every structure is put through on both sides, per (offset width, value type) of `types`: both exact data sets,
    both masks, real data under every scale; widths, padding and the operands' offset rotate; every fifth case asks for no
    dbias."""
    out, n = [], n0
    for side in ("A", "T"):
        for off, val in types:
            for kind, variant, scale in KINDS:
                d, dv = PAIRS[val][n % len(PAIRS[val])]
                out.append(_case(m, side, off, val, kind, variant, scale, d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, n % 5 != 3))
                n += 1
    return out


def width_cases():
    """Every (d, dv) pair on the ragged structure, both sides, exact and real data."""
    m, out, n = structures("ragged")[0], [], 0
    for val in ("f32", "f64"):
        for d, dv in PAIRS[val]:
            for kind, variant, scale in (("exact", n % 2, 2.0), ("real", n % 3, SCALES[n % 3])):
                out.append(_case(m, "AT"[n % 2], ("i32", "i64")[n % 2], val, kind, variant, scale, d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, True, "-w"))
                out.append(_case(m, "TA"[n % 2], ("i64", "i32")[n % 2], val, kind, variant, scale, d, dv, PADS[(n + 1) % len(PADS)], 0, NEED_ALL, True, "-w"))
                n += 1
    return out


def overflow_cases():
    """Scores that reach -inf without a masking bias, on both sides of two structures."""
    out = []
    for i, m in enumerate((structures("ragged")[0], structures("slice_edges")[2])):
        for n, (off, val) in enumerate(ALL_TYPES):
            d, dv = PAIRS[val][(2 + 3 * n + i) % len(PAIRS[val])]
            out.append(_case(m, "AT"[(n + i) % 2], off, val, "exact", 2, (0.5, 2.0)[n % 2], d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, True, "-inf"))
    return out


def single_cases():
    m, out = single_structure(), []
    for n, (off, val) in enumerate(ALL_TYPES):
        for i in range(2):      # (side A only: the rows of A have one entry, the columns — the lines of A^T — are long)
            d, dv = PAIRS[val][(3 + n + 4 * i) % len(PAIRS[val])]
            out.append(_case(m, "A", off, val, "single", 0, (0.5, -2.0)[i], d, dv, PADS[(n + i) % len(PADS)], (n + i) % 2, NEED_ALL, True))
    return out


def alignment_pairs():
    """[(aligned case, the same case with every operand one element off a 16-byte boundary)]: equal bit for bit."""
    out = []
    for m in (structures("ragged")[0], structures("slice_edges")[4]):
        for val in ("f32", "f64"):
            for i, (d, dv) in enumerate(PAIRS[val][1::3]):
                off, side = ("i32", "i64")[i % 2], "AT"[i % 2]
                out.append(tuple(_case(m, side, off, val, "real", i % 3, SCALES[i % 3], d, dv, PADS[0], sh, NEED_ALL, True, "-align") for sh in (0, 1)))
    return out


def repeat_pairs():
    """[(a case, the same case once more on the same plan)]: equal bit for bit."""
    out, n = [], 0
    for fam in ("ragged", "hub"):
        for m in structures(fam):
            for val in ("f32", "f64"):
                d, dv = PAIRS[val][6 if n % 2 else 4]
                off, side = ("i32", "i64")[n % 2], "AT"[n % 2]
                n += 1
                out.append((_case(m, side, off, val, "real", 0, 0.125, d, dv, PADS[1], 0, NEED_ALL, True, "-repeat"),
                            _case(m, side, off, val, "real", 0, 0.125, d, dv, PADS[1], 0, NEED_ALL, True, "-repeat-again")))
    return out


def need_groups():
    """[(the all-three case with dbias, dQ alone without dbias, dK alone, dV alone)]: each output equals the all-three
    execute's bit for bit, and dbias on / off leaves dQ unchanged."""
    out = []
    for i, m in enumerate((structures("ragged")[0], structures("slice_edges")[2])):
        for val in ("f32", "f64"):
            d, dv = PAIRS[val][5 + i]
            off, side = ("i32", "i64")[i], "AT"[i]
            mk = lambda need, db, tag: _case(m, side, off, val, "real", 1, 0.125, d, dv, PADS[2], 0, need, db, "-need" + tag)
            out.append((mk(NEED_ALL, True, ""), mk((1, 0, 0), False, ""), mk((0, 1, 0), False, ""), mk((0, 0, 1), False, "")))
    return out


def hub_sequence():
    """On ONE plan of the hub row per side, in this order: exact data, other operands behind it, a wide d and dv of three
    passes, then narrow ones."""
    m, out = structures("hub")[0], []
    for side, off, val in (("A", "i32", "f32"), ("T", "i64", "f64"), ("T", "i32", "f32")):
        wide, narrow = (65, 3) if val == "f32" else (33, 1)
        for kind, variant, scale, d, dv in (("exact", 0, 1.0, 8, TILE[val]), ("real", 0, 1.0, TILE[val], 8), ("masked", 1, 0.125, wide, wide),
                                            ("real", 1, 0.125, wide, 40), ("real", 2, -2.0, narrow, narrow), ("exact", 1, -2.0, 3, narrow)):
            out.append(_case(m, side, off, val, kind, variant, scale, d, dv, PADS[0], 0, NEED_ALL, True, "-seq"))
    return out


FAMILIES = STRUCTURE_FAMILIES + ("single", "overflow", "widths", "alignment", "repeat", "need", "hub_sequence")


def family(name):
    """The cases of one family, in plan order: cases of one plan_key share a plan, and keep the order they have here."""
    if name == "single":
        return single_cases()
    if name == "overflow":
        return overflow_cases()
    if name == "widths":
        return width_cases()
    if name == "alignment":
        return [c for pair in alignment_pairs() for c in pair]
    if name == "repeat":
        return [c for pair in repeat_pairs() for c in pair]
    if name == "need":
        return [c for g in need_groups() for c in g]
    if name == "hub_sequence":
        return hub_sequence()
    out = []
    for i, m in enumerate(structures(name)):
        out += structure_cases(m, ALL_TYPES if name in ("ragged", "hub") else (ALL_TYPES[i % 4],), 3 * i)
    return out


def plan_key(c):
    return (c.matrix.name, c.side, c.off, c.val)


D_MAX = {"f32": 100, "f64": 50}
DV_MAX = {"f32": 65, "f64": 40}


def table():
    return [c for f in FAMILIES for c in family(f)]


def weight(g):
    """Of a plan group, to deal the groups to batches: merge items times the lanes' work per entry."""
    return sum((len(c.matrix.lens) + c.matrix.n_cols + 2 * sum(c.matrix.lens)) * (2 * -(-c.d // TILE[c.val]) + -(-c.dv // TILE[c.val]))
               * (2 + (c.d + c.dv) // 16) + 3000 for c in g)


# ---- the host program's batch file (tests/cpp/attention_bwd_sim.cpp, whose header comment has the records) ----------------
NAN_BITS = ac.NAN_BITS
ORDER = ("Q", "K", "V", "O", "dO")
# What write_batch and read_results ask of a case.  plan_key: cases of one key share a matrix record; feat_type: the
# MI355_VAL_* of the eight matrices; csr and ops: what csr() and operands() give; to_bits, which makes the bytes of a matrix
# of ORDER of it; d_max, dv_max; dtype / side_dtype: an element of dQ, dK, dV / of dbias as the program writes it; nan,
# canary, side_canary: the bit patterns that the padding of the inputs, all of dQ, dK, dV and dbias start with.
Batch = collections.namedtuple("Batch", "plan_key feat_type csr ops to_bits d_max dv_max dtype side_dtype nan canary side_canary")


def batch_operands(c):
    T = NP[c.val]
    return Batch(plan_key(c), ac.VAL_TYPE[c.val], csr(c), operands(c), np.ascontiguousarray, D_MAX[c.val], DV_MAX[c.val], T, T, NAN_BITS[c.val],
                 word_of(CANARY, T), word_of(CANARY, T))


def write_batch(path, cases, operands=batch_operands):
    """Cases in plan order; returns them in the order their results come back."""
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    last = None
    with open(path, "wb") as f:
        for c in cases:
            o = operands(c)
            n_rows, n_cols, Ap, Aj, _ = o.csr
            if o.plan_key != last:
                last = o.plan_key
                f.write(words(1, ("i32", "i64").index(c.off), o.feat_type, n_rows, n_cols, len(Aj), o.d_max, o.dv_max))
                f.write(Ap.tobytes())
                f.write(Aj.tobytes())
            bias = o.ops["bias"]
            f.write(words(4, c.d, c.dv, *c.pad, c.shift, int(bias is not None), *c.need, int(c.want_dbias), o.nan, o.canary, o.side_canary))
            f.write(struct.pack("<d", c.scale))
            for name in ORDER:
                f.write(o.to_bits(o.ops[name]).tobytes())
            for a in (o.ops["lse"], bias):
                if a is not None:
                    assert a.dtype == o.side_dtype
                    f.write(a.tobytes())
        f.write(words(0))
    return list(cases)


def read_results(path, cases, operands=batch_operands):
    """[(status, padding elements of the outputs that lost their canary, dQ, dK, dV, dbias)] per case (None where not asked
    for); raises if the file is not complete."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            o = operands(c)
            st, bad = struct.unpack("<2q", f.read(16))
            n_rows, n_cols, Ap, Aj, _ = o.csr
            res = [st, bad]
            for want, shape, T in ((c.need[0], (n_rows, c.d), o.dtype), (c.need[1], (n_cols, c.d), o.dtype), (c.need[2], (n_cols, c.dv), o.dtype),
                                   (c.want_dbias, (len(Aj),), o.side_dtype)):
                res.append(np.frombuffer(f.read(int(np.prod(shape)) * np.dtype(T).itemsize), dtype=T).reshape(shape) if want else None)
            out.append(tuple(res))
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return out
