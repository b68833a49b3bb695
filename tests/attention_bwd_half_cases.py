"""The table of fused attention-backward cases with 16-bit Q, K, V, O, dO, dQ, dK and dV (csrc/attention_bwd_half_kernel.hpp,
mi355_spmv_attention_bwd_create_half) that tests/test_attention_bwd_half_sim_cpu.py executes on the host and
tests/test_gpu_attention_bwd_half.py on the device: the same structures, operands and expected results for both.

The eight matrices are binary16 or bfloat16 (2-byte elements); bias, lse, dbias, scale and every operation are fp32.  The
structures, sides "A" / "T", masks, kinds, transpose, expected() and the bound code are tests/attention_bwd_cases.py's,
imported and not copied: a case here has an fp32 twin (widened(c)) on a matrix of a name of its own, whose operands
attention_bwd_cases draws in fp32 and this module rounds to the 16-bit type FIRST — so what the library reads is what
attention_bwd_cases.expected() widens, and the fp64 reference, the row spread and the fp32 bounds are evaluated on the
widened operands by the code that states them.  The 16-bit conversions are tests/multi_half_cases.py's (to_bits,
from_bits, NAN_BITS).  A lane's 16 bytes are VEC = 8 columns, so C in LANES_PER_SLOT lanes per slot give tiles of 8 / 16 /
32 / 64 columns of a role's OUTPUT (d for dQ and dK, dv for dV); both test files assert that geometry.

What the outputs are held to, per kind of data (attention_bwd_cases' kinds):
  exact / masked / single
           the fp32 sums are exact integers (dyadic under the power-of-two scale) whatever the order of addition, so each
           of dQ, dK, dV must EQUAL the exact value rounded once to the 16-bit type — to_bits of the float32 value — the
           sign of a zero apart; dbias (fp32) must equal the reference.  Every expected magnitude is asserted finite in
           fp16 (below 65504): the exact families' scales (0.5, -0.25, 0.25, 0.125) keep the hub line there.  A line
           without a live entry is the +0 bit pattern.  Rows of K and V that only masked entries touch hold the type's NaN
           bits, and no NaN may come out.  Exact variant 2 (a score that reaches -inf on its own under a finite bias) is
           kept for bf16 only: Q[r, 0] = -(the largest finite bf16) against K[:, 0] = 2 overflows fp32.  It is left out
           for fp16, where no product of finite fp16 operands under the table's scales reaches -inf in fp32 (65504 * 2 *
           scale is far inside fp32).
  real     attention_bwd_cases' draws and SCALES, the five input matrices rounded to the 16-bit type first; the row spread
           of v <= 20 and every drawn and expected magnitude finite in fp16 are asserted.  The bound, derived and not
           measured:
             - the kernel's arithmetic on the widened operands is the fp32 kernel's, operation for operation (the product
               of two widened 16-bit values is exact in fp32, so an fma chain rounds no more often than the fp32 kernel's;
               the 8-column lane partition only changes the ORDER of a dot's additions, which the dot bounds do not
               depend on), so attention_bwd_cases' fp32 bound B32 holds for the fp32 line sum x with eps = 2^-24;
             - out is x rounded ONCE to nearest even: |narrow(x) - x| <= u16 |x| where x is normal in the 16-bit type and
               at most half the smallest subnormal below.  With |x| <= |want| + B32:
                   |out - want| <= B32 + u16 (|want| + B32) + sub16 / 2 <= (1 + u16) B32 + u16 |want| + sub16
               u16 = 2^-11 (fp16) / 2^-8 (bf16), sub16 = 2^-24 / 2^-133: the form of attention_half_cases.check().
           dbias is fp32 throughout: held to attention_bwd_cases' e_ds unchanged.
  autograd (the device file only, autograd_extra() below) through sp.sparse_attention_function the backward is given the
           library's OWN 16-bit forward output O' and fp32 lse', not the fp64 forward's.  Against the true gradient (torch
           autograd on the dense masked formulation in fp64 on the widened inputs) the table's bound, evaluated with O' and
           lse' as the operands, gains the first-order propagation of dO = |O' - O| and dl = |lse' - lse| through the
           formulas: delta moves by at most e_r = sum_j |dO_rj| dO_rj (this holds the issue's u16 sum_j |dO_rj O_rj| and
           the forward table's bound on O: the forward's tests hold |O' - O| to (1 + u16) B_O + u16 |O| + sub16, and the
           propagation uses |O' - O| itself, which is never larger), p by p dl_r (1 + dl_r) to second order, so
               e'_ds_n = p_n (e_r + dl_r (1 + dl_r) (|dp_n - delta_r| + e_r))
               dQ: sum_row |scale| e'_ds_n |K[c, j]|;  dK: sum_col |scale| e'_ds_n |Q[r, j]|;
               dV: sum_col p_n dl_r (1 + dl_r) |dO[r, j]|;  dbias: e'_ds_n
           added to the table's bound.  The lse term is not in the issue's statement of the bound; it is needed, because
           lse' is the library's too.  The perturbations are those of the backward's INPUTS, known exactly in the test;
           nothing is taken from the backward's outputs.  A broken forward cannot widen this bound unnoticed: the forward's
           own tests (tests/test_gpu_attention_half.py on tests/attention_half_cases.py) separately hold |O' - O| to
           (1 + u16) B_O + u16 |O| + sub16 and |lse' - lse| to the forward table's lse bound.
Padding columns of the inputs hold the type's NaN bits; the outputs start as a canary that must survive in their padding
columns (and, on the device, behind every operand).  The host program and its batch file are attention_bwd_cases'
(tests/cpp/attention_bwd_sim.cpp): batch_operands() says what differs."""
import collections
import functools

import numpy as np

import attention_bwd_cases as bc
import attention_cases as ac
import attention_half_cases as hc
from attention_bwd_cases import STRUCTURE_FAMILIES, structures, transpose  # noqa: F401
from multi_cases import LANES_PER_SLOT, SLICE_LEN, STEP, word_of
from multi_half_cases import CANARY, NAN_BITS, VAL_TYPE, from_bits, to_bits  # noqa: F401

VECS = ("f16", "bf16")
OFFS = ("i32", "i64")
TYPES = tuple((o, v) for v in VECS for o in OFFS)
VEC = 8                             # columns per 16-byte group
TILE = 64                           # widest tile = max(LANES_PER_SLOT) * VEC
U16, SUB16, F16_MAX = hc.U16, hc.SUB16, hc.F16_MAX
D_MAX = DV_MAX = 129
SCALES = bc.SCALES
ORDER = bc.ORDER
# (d, dv), both output widths: 1; below a lane; every C on both; a full tile; two and three passes on d and on dv; d != dv
PAIRS = ((1, 1), (3, 5), (8, 16), (16, 8), (32, 23), (23, 32), (64, 64), (45, 33), (65, 8), (8, 65), (129, 16), (16, 129), (100, 3), (3, 100))
RAGGED = tuple(range(1, 10)) + (63, 64, 65)     # every masked remainder of a lane's eight columns; the tile edge
# ld - width of Q, K, V, O, dO, dQ, dK, dV; the last keeps rows of width % 8 == 0 on 16-byte boundaries
PADS = bc.PADS + (hc.PADS[-1] * 2,)
NEED_ALL = bc.NEED_ALL
# the exact families under scales that keep the hub line finite in fp16
KINDS = (("exact", 0, 0.5), ("exact", 1, -0.25), ("masked", 0, 0.25), ("masked", 1, 0.125), ("real", 0, 1.0), ("real", 1, 0.125), ("real", 2, -2.0))

Case = collections.namedtuple("Case", "name matrix side off vec kind variant scale d dv pad shift need want_dbias")


def lanes_per_slot(width):
    """C of the first pass of a role whose output has `width` columns: from ceil(min(width, 64) / 8) alone."""
    return hc.lanes_per_slot(min(width, TILE))


def assert_geometry(info):
    """info() of a 16-bit plan agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["widest_tile"] == max(LANES_PER_SLOT) * VEC == TILE
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    for role, w in (("dq", info["d_max"]), ("dk", info["d_max"]), ("dv", info["dv_max"])):
        assert info["passes"][role] == -(-w // TILE)
        assert info["lanes_per_slot"][role] == lanes_per_slot(w)
    assert info["main_kernel"] == "attention_bwd_half_slice_kernel"
    assert info["val_type"] == VAL_TYPE["f32"]


# ---- operands and expected results: attention_bwd_cases' on the fp32 twin ----------------------------------------------------
_twins, _rounded = {}, set()


def widened(c):
    """The fp32 twin of a case: attention_bwd_cases' Case on the same structure under a name of its own (so its data set is
    nobody else's), with Q, K, V, O and dO rounded to c.vec — once, before anybody reads them."""
    if c.name not in _twins:
        m = c.matrix._replace(name="%s~%s" % (c.matrix.name, c.vec))
        # the twin's structure is the case's own arrays (the position structures are made from their matrix's name)
        assert ac._csr.setdefault((m.name, c.off), ac.csr(c.matrix, c.off))[0] is ac.csr(c.matrix, c.off)[0]
        w = bc.Case(c.name, m, c.side, c.off, "f32", c.kind, c.variant, c.scale, c.d, c.dv, c.pad, c.shift, c.need, c.want_dbias)
        key = bc.data_key(w)
        if key not in _rounded:
            assert key not in bc._expected
            ops = bc.operands(w)
            if c.kind == "exact" and c.variant == 2:
                assert c.vec == "bf16", "exact variant 2 needs a type whose largest value times 2 overflows fp32"
                gone = ops["Q"][:, 0] == -np.finfo(np.float32).max
                assert gone.any()
                ops["Q"][gone, 0] = -from_bits(np.uint16(0x7F7F), "bf16")
            for name in ORDER:
                a = ops[name]
                a[...] = from_bits(to_bits(a, c.vec), c.vec).reshape(a.shape)
                if not (c.variant == 2 and c.kind == "exact" and name == "Q"):
                    assert np.nanmax(np.abs(a), initial=0.0) < F16_MAX, (c.name, name)
            _rounded.add(key)
        _twins[c.name] = w
    return _twins[c.name]


def csr(c):
    return bc.csr(widened(c))


def operands(c):
    """attention_bwd_cases' dict as fp32 arrays: Q, K, V, O and dO hold only values that c.vec has; lse and bias are fp32."""
    return bc.operands(widened(c))


def expected(c):
    return bc.expected(widened(c))


def same_but_zero_sign(a, b):
    return hc.same_but_zero_sign(a, b)


def half_bound(b32, want, vec):
    return (1 + U16[vec]) * b32 + U16[vec] * np.abs(want) + SUB16[vec]


def check(c, dQ, dK, dV, dbias, ratios=None, extra=None, want=None):
    """The outputs an execute left: dQ, dK, dV as 16-bit patterns (uint16, compact), dbias as float32; None where the case
    does not ask for one.  ratios: a list that takes the largest error / bound of a real case.  extra: {name: array} added
    to the bound (the autograd comparison's forward terms).  want: {name: array} to compare with in place of expected()'s
    values (the autograd comparison's true gradient); expected() is left as it is."""
    n_rows, n_cols, Ap, Aj, _ = csr(c)
    ex = expected(c)
    got = dict(dQ=dQ, dK=dK, dV=dV, dbias=dbias)
    want_of = want
    shapes = dict(dQ=(n_rows, c.d), dK=(n_cols, c.d), dV=(n_cols, c.dv), dbias=(len(Aj),))
    asked = dict(dQ=c.need[0], dK=c.need[1], dV=c.need[2], dbias=c.want_dbias)
    if c.kind == "real":
        assert ex["spread"].max() <= 20.0, c.name
    for name in ("dQ", "dK", "dV", "dbias"):
        a = got[name]
        assert (a is not None) == bool(asked[name]), "%s: %s" % (c.name, name)
        want = ex[name] if want_of is None else want_of[name]
        assert np.abs(want).max(initial=0.0) < F16_MAX, "%s: the reference of %s is not finite in fp16" % (c.name, name)
        if a is None:
            continue
        a = np.asarray(a)
        if name == "dbias":
            assert a.shape == shapes[name] and a.dtype == np.float32 and not np.any(np.isnan(a)), "%s: dbias" % c.name
            if c.kind != "real":
                assert np.array_equal(a.astype(np.float64), want), "%s: dbias differs from the exact value" % c.name
                continue
            bound = ex["bound"]["dbias"] + (extra["dbias"] if extra else 0.0)
            err = np.abs(a.astype(np.float64) - want)
        else:
            assert a.shape == shapes[name] and a.dtype == np.uint16, "%s: %s" % (c.name, name)
            af = from_bits(a, c.vec).reshape(a.shape)
            assert not np.any(np.isnan(af)), "%s: NaN in %s (lines %s)" % (c.name, name, np.nonzero(np.isnan(af).any(1))[0][:8])
            none = (ex["live_rows"] if name == "dQ" else ex["live_cols"]) == 0
            assert np.all(a[none] == 0), "%s: a line of %s without a live entry is not +0 (lines %s)" % (c.name, name, np.nonzero(none)[0][:8])
            if c.kind != "real":
                want32 = want.astype(np.float32)
                assert np.array_equal(want32.astype(np.float64), want), "%s: the reference of %s is not exact in fp32" % (c.name, name)
                exact = to_bits(want32, c.vec).reshape(a.shape)
                bad = np.nonzero(~same_but_zero_sign(a, exact).all(1))[0]
                assert bad.size == 0, "%s: lines %s of %s differ from the exact value rounded once (got %s, want %s)" % (
                    c.name, bad[:8], name, a[bad[:3]], exact[bad[:3]])
                continue
            bound = half_bound(ex["bound"][name] + (extra[name] if extra else 0.0), want, c.vec)
            err = np.abs(af.astype(np.float64) - want)
        ratio = float((err / bound).max()) if err.size else 0.0
        assert np.all(err <= bound), "%s: %s outside the bound (largest error / bound %g)" % (c.name, name, ratio)
        if ratios is not None:
            ratios.append(ratio)


def autograd_extra(c, O_true, lse_true):
    """The terms the autograd comparison adds to the bound of case c (whose operands O and lse are the library's forward
    outputs) against the gradient of the TRUE forward, O_true and lse_true in fp64: see the module's docstring."""
    n_rows, n_cols, Ap, Aj, _ = csr(c)
    ops = operands(c)
    f = lambda a: a.astype(np.float64)
    rows = np.repeat(np.arange(n_rows), np.diff(Ap.astype(np.int64)))
    scale = float(np.float32(c.scale))
    v = scale * (f(ops["Q"])[rows] * f(ops["K"])[Aj]).sum(1) + (f(ops["bias"]) if ops["bias"] is not None else 0.0)
    with np.errstate(invalid="ignore"):
        dead = np.isneginf(v)
        p = np.where(dead, 0.0, np.exp(np.where(dead, 0.0, v - np.where(dead, 0.0, f(ops["lse"])[rows]))))
        dl = np.where(np.isneginf(lse_true), 0.0, np.abs(f(ops["lse"]) - np.where(np.isneginf(lse_true), 0.0, lse_true)))
    dl = (dl * (1 + dl))[rows]
    e_r = (np.abs(f(ops["dO"])) * np.abs(f(ops["O"]) - O_true)).sum(1)[rows]
    dp = (f(ops["dO"])[rows] * f(ops["V"])[Aj]).sum(1)
    delta = (f(ops["dO"]) * f(ops["O"])).sum(1)[rows]
    e_ds = p * (e_r + dl * (np.abs(dp - delta) + e_r))
    ce = abs(scale) * e_ds
    return dict(dQ=bc._line_sums(rows, n_rows, ce[:, None] * np.abs(f(ops["K"])[Aj])),
                dK=bc._line_sums(Aj, n_cols, ce[:, None] * np.abs(f(ops["Q"])[rows])),
                dV=bc._line_sums(Aj, n_cols, (p * dl)[:, None] * np.abs(f(ops["dO"])[rows])), dbias=e_ds)


def with_forward(c, O_bits, lse):
    """Case c (real) with the operands O and lse replaced by a forward's outputs (16-bit patterns and fp32): a case of a
    name and a data set of its own, so that expected() is evaluated on what the backward is given."""
    w0 = widened(c)
    c2 = c._replace(name=c.name + "-fwd", variant=c.variant + 100)
    w2 = w0._replace(name=c2.name, variant=c2.variant)
    ops = dict(bc.operands(w0))
    ops["O"] = from_bits(np.asarray(O_bits, dtype=np.uint16), c.vec).reshape(ops["O"].shape).copy()
    ops["lse"] = np.asarray(lse, dtype=np.float32).copy()
    bc._operands[bc.data_key(w2)] = ops
    bc._expected.pop(bc.data_key(w2), None)
    _twins[c2.name] = w2
    return c2


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, side, off, vec, kind, variant, scale, d, dv, pad=PADS[0], shift=0, need=NEED_ALL, want_dbias=True, tag=""):
    name = "%s-%s-%s-%s-%s%d-s%g-d%d-dv%d-pad%s-sh%d-need%s-db%d%s" % (m.name, side, off, vec, kind, variant, scale, d, dv, ".".join(map(str, pad)),
                                                                       shift, "".join(map(str, need)), int(want_dbias), tag)
    return Case(name, m, side, off, vec, kind, variant, float(scale), d, dv, tuple(pad), shift, tuple(need), bool(want_dbias and need[0]))


def structure_cases(m, types, n0=0):
    """What every structure is put through on both sides, per (offset width, 16-bit type) of `types`: both exact data sets,
    both masks, real data under every scale; the width pairs, padding and the operands' offset rotate; every fifth case
    asks for no dbias."""
    out, n = [], n0
    for side in ("A", "T"):
        for off, vec in types:
            for kind, variant, scale in KINDS:
                d, dv = PAIRS[n % len(PAIRS)]
                out.append(_case(m, side, off, vec, kind, variant, scale, d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, n % 5 != 3))
                n += 1
    return out


def width_cases():
    """On the ragged structure: every width of RAGGED as d and (in reverse) as dv, then every pair of PAIRS; exact and real."""
    m, out, n = structures("ragged")[0], [], 0
    pairs = tuple(zip(RAGGED, RAGGED[::-1])) + PAIRS
    for d, dv in pairs:
        for kind, variant, scale in (("exact", n % 2, 0.5), ("real", n % 3, SCALES[n % 3])):
            off, vec = TYPES[n % 4]
            out.append(_case(m, "AT"[n % 2], off, vec, kind, variant, scale, d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, True, "-w"))
            n += 1
    return out


def overflow_cases():
    """Scores that reach -inf without a masking bias (bf16 only: see the docstring), on both sides of two structures."""
    out = []
    for i, m in enumerate((structures("ragged")[0], structures("slice_edges")[2])):
        for n, off in enumerate(OFFS):
            d, dv = PAIRS[(2 + 3 * n + i) % len(PAIRS)]
            out.append(_case(m, "AT"[(n + i) % 2], off, "bf16", "exact", 2, (0.5, 2.0)[n % 2], d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, True, "-inf"))
    return out


def single_cases():
    m, out = bc.single_structure(), []
    for n, (off, vec) in enumerate(TYPES):
        d, dv = PAIRS[(3 + 4 * n) % len(PAIRS)]
        out.append(_case(m, "A", off, vec, "single", 0, (0.5, -2.0)[n % 2], d, dv, PADS[n % len(PADS)], n % 2, NEED_ALL, True))
    return out


ALIGN_PAIRS = ((8, 16), (16, 8), (64, 64), (32, 24), (72, 128))     # widths % 8 == 0: the aligned case's lanes take the 16-byte path


def alignment_pairs():
    """[(aligned case, the same case with every operand one ELEMENT off a 16-byte boundary)]: equal bit for bit."""
    out = []
    for m in (structures("ragged")[0], structures("slice_edges")[4]):
        for vec in VECS:
            for i, (d, dv) in enumerate(ALIGN_PAIRS):
                off, side = OFFS[i % 2], "AT"[i % 2]
                out.append(tuple(_case(m, side, off, vec, "real", i % 3, SCALES[i % 3], d, dv, PADS[-1], sh, NEED_ALL, True, "-align") for sh in (0, 1)))
    return out


def repeat_pairs():
    """[(a case, the same case once more on the same plan)]: equal bit for bit."""
    out, n = [], 0
    for fam in ("ragged", "hub"):
        for m in structures(fam):
            for vec in VECS:
                d, dv = PAIRS[7 if n % 2 else 4]
                off, side = OFFS[n % 2], "AT"[n % 2]
                n += 1
                out.append(tuple(_case(m, side, off, vec, "real", 0, 0.125, d, dv, PADS[1], 0, NEED_ALL, True, tag) for tag in ("-repeat", "-repeat-again")))
    return out


def need_groups():
    """[(the all-three case with dbias, dQ alone without dbias, dK alone, dV alone)]: each output equals the all-three
    execute's bit for bit, and dbias on / off leaves dQ unchanged."""
    out = []
    for i, m in enumerate((structures("ragged")[0], structures("slice_edges")[2])):
        for vec in VECS:
            d, dv = PAIRS[7 + i]
            off, side = OFFS[i], "AT"[i]
            mk = lambda need, db: _case(m, side, off, vec, "real", 1, 0.125, d, dv, PADS[2], 0, need, db, "-need")
            out.append((mk(NEED_ALL, True), mk((1, 0, 0), False), mk((0, 1, 0), False), mk((0, 0, 1), False)))
    return out


def hub_sequence():
    """On ONE plan of the hub row per side, in this order: exact data, other operands behind it, wide outputs of three
    passes, then narrow ones."""
    m, out = structures("hub")[0], []
    for side, off, vec in (("A", "i32", "bf16"), ("T", "i64", "f16"), ("T", "i32", "bf16")):
        for kind, variant, scale, d, dv in (("exact", 0, 0.5, 8, TILE), ("real", 0, 1.0, TILE, 8), ("masked", 1, 0.125, 129, 129),
                                            ("real", 1, 0.125, 129, 40), ("real", 2, -2.0, 3, 3), ("exact", 1, -0.25, 3, 1)):
            out.append(_case(m, side, off, vec, kind, variant, scale, d, dv, PADS[0], 0, NEED_ALL, True, "-seq"))
    return out


def fp32_pairs():
    """Exact-family cases whose 16-bit outputs must equal narrow(the fp32 SparseAttentionBackwardPlan's outputs on the
    widened operands) bit for bit (the device file): every fp32 sum is exact in both kernels whatever their geometry."""
    out, n = [], 0
    for m in structures("slice_edges")[:3] + structures("hub")[:1]:
        for kind, variant, scale in KINDS[:4]:
            off, vec = TYPES[n % 4]
            d, dv = PAIRS[(5 + 3 * n) % len(PAIRS)]
            out.append(_case(m, "AT"[n % 2], off, vec, kind, variant, scale, d, dv, PADS[0], 0, NEED_ALL, True, "-fp32"))
            n += 1
    return out


FAMILIES = STRUCTURE_FAMILIES + ("single", "overflow", "widths", "alignment", "repeat", "need", "hub_sequence", "fp32_pairs")
FULL_CROSS = ("ragged", "hub")      # every (offset width, 16-bit type); elsewhere one of the four, rotating


def family(name):
    """The cases of one family, in plan order: cases of one plan_key share a plan, and keep the order they have here."""
    special = dict(single=single_cases, overflow=overflow_cases, widths=width_cases, hub_sequence=hub_sequence, fp32_pairs=fp32_pairs)
    if name in special:
        return special[name]()
    if name in ("alignment", "repeat", "need"):
        return [c for g in dict(alignment=alignment_pairs, repeat=repeat_pairs, need=need_groups)[name]() for c in g]
    out = []
    for i, m in enumerate(structures(name)):
        out += structure_cases(m, TYPES if name in FULL_CROSS else (TYPES[i % 4],), 3 * i)
    return out


def plan_key(c):
    return (c.matrix.name, c.side, c.off, c.vec)


_table = []


def table():
    if not _table:
        _table.extend(c for f in FAMILIES for c in family(f))
    return list(_table)


def weight(g):
    """Of a plan group, to deal the groups to batches: merge items times the lanes' work per entry."""
    return sum((len(c.matrix.lens) + c.matrix.n_cols + 2 * sum(c.matrix.lens)) * (2 * -(-c.d // TILE) + -(-c.dv // TILE))
               * (2 + (c.d + c.dv) // 16) + 3000 for c in g)


# ---- the host program's batch file: attention_bwd_cases.write_batch and read_results on what differs here ------------------
def batch_operands(c):
    return bc.Batch(plan_key(c), VAL_TYPE[c.vec], csr(c), operands(c), lambda a: to_bits(a, c.vec), D_MAX, DV_MAX, np.uint16, np.float32,
                    NAN_BITS[c.vec], int(to_bits(np.float32(CANARY), c.vec).reshape(-1)[0]), word_of(CANARY, np.float32))


write_batch = functools.partial(bc.write_batch, operands=batch_operands)
read_results = functools.partial(bc.read_results, operands=batch_operands)
