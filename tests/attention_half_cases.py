"""The table of fused sparse-attention cases with 16-bit Q, K, V and O (csrc/attention_half_kernel.hpp,
mi355_spmv_attention_create_half) that tests/test_attention_half_sim_cpu.py executes on the host and
tests/test_gpu_attention_half.py on the device: the same structures, operands and expected results for both.

    v[n] = scale * dot(float(Q[r, :d]), float(K[c, :d])) + bias[n];  m_r = max_row v;  l_r = sum_row exp(v - m_r)
    O[r, :dv] = narrow((sum_row exp(v[n] - m_r) float(V[c, :dv])) / l_r);  lse[r] = m_r + log(l_r)

Q, K, V and O are binary16 or bfloat16 (2-byte elements); bias, lse, scale and every operation are fp32.  The structures,
masks, data kinds, reference and bounds are tests/attention_cases.py's, imported and not copied: a case here has an fp32
twin (widened(c)) on a matrix of a name of its own, whose operands attention_cases draws in fp32 and this module rounds to
the 16-bit type FIRST — so what the library reads is what attention_cases.expected() widens, and the fp64 reference, the
row spread and the fp32 bounds are evaluated on the widened operands by the code that states them.  The 16-bit conversions
are tests/multi_half_cases.py's (to_bits, from_bits).  A lane's 16 bytes are VEC = 8 columns, so C in LANES_PER_SLOT lanes
per slot give tiles of 8 / 16 / 32 / 64 columns; both test files assert that geometry.

What O and lse are held to, per kind of data (attention_cases' kinds):
  const    Q = 0, V small integers, bias constant per row over +-1e4 or absent: every exp is 1, every l a count and every
           acc an exact integer sum in fp32, whatever the order.  O[r, j] must equal
               narrow(float32(sum_row V[c, j]) / float32(len_r))
           formed in numpy as ONE float32 division followed by to_bits — bit for bit, the sign of a zero apart.  (The fp64
           quotient rounded straight to 16 bits would skip the kernel's fp32 rounding: a double rounding the kernel does
           not make.)  lse: attention_cases' const bound with the fp32 eps, exactly c_r on a row of one entry.
  masked   const variant 0 with bias = -inf at row_softmax_cases.mask()'s entries: the const expectation on the row with
           those entries deleted; a row without a live entry gives the +0 bit pattern and lse = -inf.
  real     attention_cases' draws and SCALES, Q, K and V rounded to the 16-bit type first; the row spread of v <= 20 is
           asserted, and max |Q| < 65504 after the 1 / |scale| stretch.  The bound, derived and not measured:
             - the kernel's arithmetic on the widened operands is the fp32 kernel's, operation for operation, so
               attention_cases' fp32 bound holds for the fp32 acc / l with eps = 2^-24.  Its score term counts one
               rounding per column of the fma chain; the product of two 16-bit values (at most 11 significand bits each)
               is exact in fp32, so the chain rounds no more often than that (sddmm_half_cases' argument), and the tree,
               the scaling and the bias are what the term already counts;
             - O is that fp32 value x, |x - want| <= B32, rounded ONCE to nearest even: |narrow(x) - x| <= u16 |x| where x is
               normal in the 16-bit type and at most half the smallest subnormal below.  With |x| <= |want| + B32:
                   |O - want| <= B32 + u16 (|want| + B32) + sub16 / 2  <=  (1 + u16) B32 + u16 |want| + sub16
               u16 = 2^-11 (fp16) / 2^-8 (bf16), sub16 = 2^-24 / 2^-133 the smallest subnormal.  check() uses the last form
               (the issue's "u16 |want| plus the smallest subnormal" with the second-order u16 B32 kept, not dropped).
             - O is a convex combination of values in [-1, 1] (a draw of (-1, 1) may round to 1): nothing overflows in fp16.
           lse is fp32 throughout: attention_cases' fp32 bound unchanged.
In EVERY case a row of one live entry must give O[r] = V[c] bit for bit (V[c] is widened exactly, multiplied by
exp(0) = 1, divided by l = 1 and narrowed back), and on const / masked data lse[r] = v exactly.  Padding columns of Q, K
and V hold the type's NaN bits; O starts as a canary that must survive in its padding columns; lse starts as NaN.  The host
program and its batch file are attention_cases' (tests/cpp/attention_sim.cpp): batch_operands() says what differs."""
import collections
import functools

import numpy as np

import attention_cases as ac
from attention_cases import LANES_PER_SLOT, NP, SLICE_LEN, STEP, STRUCTURE_FAMILIES, csr, rows_of, slices, structures  # noqa: F401
from multi_half_cases import CANARY, NAN_BITS, VAL_TYPE, from_bits, to_bits  # noqa: F401

VECS = ("f16", "bf16")
OFFS = ("i32", "i64")
TYPES = tuple((o, v) for v in VECS for o in OFFS)
VEC = 8                             # columns per 16-byte group
TILE = 64                           # widest tile = max(LANES_PER_SLOT) * VEC
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUB16 = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}
F16_MAX = 65504.0
KF, KV = 132, 136                   # columns of the full Q / K and of the full V of a data set (wider than attention_cases')
SCALES, KINDS = ac.SCALES, ac.KINDS
# the (d, dv) pairs that every structure rotates through: C = 1 (with a long score loop on one lane), C = 2, C = 4, C = 8
# with a full tile and two rounds of the d loop with a remainder, two passes, three passes
PAIRS = ((1, 1), (100, 3), (16, 8), (5, 16), (45, 23), (64, 32), (16, 33), (128, 64), (33, 64), (8, 65), (8, 129))
DV_RAGGED = tuple(range(1, 10)) + (63, 64, 65)      # every masked remainder of a lane's eight columns; the tile edge
# element offsets of Ap, Aj, Q, K, V, bias, O, lse from a 16-byte boundary (an element of Q, K, V, O is 2 bytes; of bias, lse 4)
ALIGNED, SHIFTED, SHIFTS = ac.ALIGNED, ac.SHIFTED, ac.SHIFTS
PADS = ac.PADS + ((8, 16, 8, 24),)  # (ldq - d, ldk - d, ldv - dv, ldo - dv); the last keeps rows of width % 8 == 0 aligned

# off / vec: the offset width and the 16-bit type; the other fields are attention_cases.Case's
Case = collections.namedtuple("Case", "name matrix off vec kind variant scale d dv c0 cv0 ldq ldk ldv ldo want_lse shift")


def assert_geometry(info):
    """info() of a 16-bit plan agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["widest_tile"] == max(LANES_PER_SLOT) * VEC == TILE
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    assert info["passes"] == -(-info["dv_max"] // TILE)
    assert info["lanes_per_slot"] == lanes_per_slot(min(info["dv_max"], TILE))
    assert info["main_kernel"] == "attention_half_slice_kernel"
    assert info["val_type"] == VAL_TYPE["f32"]


def lanes_per_slot(dv):
    """C of a pass over a tile of dv <= 64 columns: from ceil(dv / 8) alone."""
    groups = -(-dv // VEC)
    return next((c for c in LANES_PER_SLOT if groups <= c), max(LANES_PER_SLOT))


# ---- operands and expected results: attention_cases' on the fp32 twin ------------------------------------------------------
_twins, _rounded = {}, set()


def widened(c):
    """The fp32 twin of a case: attention_cases' Case on the same structure under a name of its own (so its data set is
    nobody else's), with Q, K and V rounded to c.vec — once, before anybody reads them."""
    if c.name not in _twins:
        m = c.matrix._replace(name="%s~%s" % (c.matrix.name, c.vec))
        w = ac.Case(c.name, m, c.off, "f32", c.kind, c.variant, c.scale, c.d, c.dv, c.c0, c.cv0, c.ldq, c.ldk, c.ldv, c.ldo, c.want_lse, c.shift)
        # the twin's structure is the case's own arrays (the position structures are made from their matrix's name)
        assert ac._csr.setdefault((m.name, c.off), csr(c.matrix, c.off))[0] is csr(c.matrix, c.off)[0]
        key = ac.data_key(w)
        if key not in _rounded:
            kf, kv = ac.KF, ac.KV
            ac.KF, ac.KV = KF, KV       # (attention_cases draws KF and KV columns: this table's, for the twin's first draw)
            try:
                Q, K, V, _ = ac.operands(w)
            finally:
                ac.KF, ac.KV = kf, kv
            assert Q.shape[1] == KF and V.shape[1] == KV
            for a in (Q, K, V):
                a[...] = from_bits(to_bits(a, c.vec), c.vec)
            assert np.abs(Q).max(initial=0.0) < F16_MAX
            _rounded.add(key)
        _twins[c.name] = w
    return _twins[c.name]


def operands(c):
    """(Q, K, V, bias) as fp32 arrays: Q, K and V hold only values that c.vec has; bias (or None) is fp32."""
    return ac.operands(widened(c))


def expected(c):
    """attention_cases.expected() on the widened operands: want, lse, live, and for real data spread, bound, lse_bound."""
    return ac.expected(widened(c))


def data_key(c):
    return ac.data_key(widened(c))


def exact_o_bits(c):
    """const / masked: narrow(float32(sum over the live entries of V[c, j]) / float32(live)), one fp32 division, then to_bits."""
    ex = expected(c)
    live = np.maximum(ex["live"], 1)
    total = np.rint(ex["want"] * live[:, None]).astype(np.float32)
    return to_bits(total / live.astype(np.float32)[:, None], c.vec)


def same_but_zero_sign(a, b):
    """16-bit patterns equal, the sign of a zero apart."""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    return (a == b) | (((a | b) & 0x7FFF) == 0)


def o_bound(c):
    ex = expected(c)
    return (1 + U16[c.vec]) * ex["bound"] + U16[c.vec] * np.abs(ex["want"]) + SUB16[c.vec]


def check(c, O, lse, ratios=None):
    """O: the n_rows x dv 16-bit patterns (uint16) an execute left; lse: its n_rows fp32 values, or None where the case asks
    for none.  ratios: a list that takes the largest error / bound of a real case (the device file records it)."""
    m = c.matrix
    n_rows, lens = len(m.lens), np.asarray(m.lens, dtype=np.int64)
    O = np.asarray(O)
    assert O.shape == (n_rows, c.dv) and O.dtype == np.uint16, c.name
    Of = from_bits(O, c.vec).reshape(n_rows, c.dv)
    assert not np.any(np.isnan(Of)), "%s: NaN in O (rows %s)" % (c.name, np.nonzero(np.isnan(Of).any(1))[0][:8])
    assert (lse is not None) == bool(c.want_lse), c.name
    ex = expected(c)
    Ap, Aj = csr(m, c.off)
    Vc = operands(c)[2][:, c.cv0:c.cv0 + c.dv]
    dead = ex["live"] == 0
    assert np.all(O[dead] == 0), "%s: a row without a live entry is not +0 (rows %s)" % (c.name, np.nonzero(dead)[0][:8])
    one = np.nonzero((lens == 1) & (ex["live"] == 1))[0]
    if one.size:
        assert np.array_equal(O[one], to_bits(Vc[Aj[Ap[one].astype(np.int64)]], c.vec).reshape(one.size, c.dv)), "%s: a row of one entry is not V[c]" % c.name
    if lse is not None:
        lse = np.asarray(lse)
        assert lse.shape == (n_rows,) and lse.dtype == np.float32 and not np.any(np.isnan(lse)), c.name
        assert np.all(np.isneginf(lse[dead])) and not np.any(np.isinf(lse[~dead])), "%s: lse of the rows without a live entry" % c.name
    eps = ac.EPS["f32"]
    ok = ~dead
    if c.kind in ("const", "masked"):
        exact = exact_o_bits(c)
        bad = np.nonzero(~same_but_zero_sign(O, exact).all(1))[0]
        assert bad.size == 0, "%s: rows %s differ from the exact value (got %s, want %s)" % (c.name, bad[:8], O[bad[:4]], exact[bad[:4]])
        if lse is not None:
            bound = eps * (np.abs(ex["lse"][ok]) + 2 * (ac.E_LOG + 1) * np.log(ex["live"][ok]))
            err = np.abs(lse[ok].astype(np.float64) - ex["lse"][ok])
            assert np.all(err <= bound), "%s: lse outside the bound (rows %s)" % (c.name, np.nonzero(ok)[0][np.nonzero(err > bound)[0][:8]])
            single = ok & (ex["live"] == 1)
            assert np.all(lse[single].astype(np.float64) == ex["lse"][single]), "%s: lse of a row of one live entry is not v" % c.name
        return
    assert ex["spread"].max() <= 20.0, c.name
    bound = o_bound(c)
    err = np.abs(Of.astype(np.float64) - ex["want"])
    ratio = float((err / bound).max()) if err.size else 0.0
    bad = np.nonzero((err > bound).any(1))[0]
    assert bad.size == 0, "%s: rows %s outside the bound (largest error / bound %g)" % (c.name, bad[:8], ratio)
    if lse is not None:
        lerr = np.abs(lse[ok].astype(np.float64) - ex["lse"][ok])
        lratio = float((lerr / ex["lse_bound"][ok]).max()) if lerr.size else 0.0
        assert np.all(lerr <= ex["lse_bound"][ok]), "%s: lse outside the bound (largest error / bound %g)" % (c.name, lratio)
        ratio = max(ratio, lratio)
    if ratios is not None:
        ratios.append(ratio)


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, off, vec, kind, variant, scale, d, dv, pad=PADS[0], shift=ALIGNED, want_lse=True, tag=""):
    c0 = 0 if d > KF - 4 else d % 5
    cv0 = 0 if dv > KV - 8 else dv % 7
    name = "%s-%s-%s-%s%d-s%g-d%d-dv%d-pad%s-%s-lse%d%s" % (m.name, off, vec, kind, variant, scale, d, dv, ".".join(map(str, pad)),
                                                           "".join(map(str, shift)), int(want_lse), tag)
    return Case(name, m, off, vec, kind, variant, float(scale), d, dv, c0, cv0, d + pad[0], d + pad[1], dv + pad[2], dv + pad[3],
                bool(want_lse), tuple(shift))


def structure_cases(m, types, n0=0):
    """What every structure is put through, per (offset width, 16-bit type) of `types`: both const data sets, both masks,
    real data under every scale; widths, padding and operand offsets rotate; every seventh case asks for no lse."""
    out, n = [], n0
    for off, vec in types:
        for kind, variant, scale in KINDS:
            d, dv = PAIRS[n % len(PAIRS)]
            out.append(_case(m, off, vec, kind, variant, scale, d, dv, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], n % 7 != 5))
            n += 1
    return out


def width_cases():
    """Every dv of DV_RAGGED on the ragged structure, const and real data, and every pair of PAIRS on real data."""
    m, out, n = structures("ragged")[0], [], 0
    ds = (1, 3, 8, 16, 45, 64, 100, 128)
    for i, dv in enumerate(DV_RAGGED):
        for kind, variant, scale in (("const", 0, 1.0), ("real", n % 3, SCALES[n % 3])):
            off, vec = TYPES[n % 4]
            out.append(_case(m, off, vec, kind, variant, scale, ds[i % len(ds)], dv, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], True, "-w"))
            n += 1
    for d, dv in PAIRS:
        off, vec = TYPES[n % 4]
        out.append(_case(m, off, vec, "real", n % 3, SCALES[n % 3], d, dv, PADS[n % len(PADS)], SHIFTS[n % len(SHIFTS)], True, "-w"))
        n += 1
    return out


ALIGN_PAIRS = ((16, 8), (5, 16), (64, 32), (128, 64), (33, 64), (8, 65), (45, 23))


def alignment_pairs():
    """[(aligned case, the same case with every operand one ELEMENT off a 16-byte boundary)]: equal bit for bit.  The
    padding keeps the aligned case's rows of width % 8 == 0 on 16-byte boundaries: its lanes take the 16-byte path."""
    out = []
    for m in (structures("ragged")[0], structures("slice_edges")[4]):
        for vec in VECS:
            for i, (d, dv) in enumerate(ALIGN_PAIRS):
                off = OFFS[i % 2]
                out.append((_case(m, off, vec, "real", i % 3, SCALES[i % 3], d, dv, PADS[-1], ALIGNED, True, "-align"),
                            _case(m, off, vec, "real", i % 3, SCALES[i % 3], d, dv, PADS[-1], SHIFTED, True, "-align")))
    return out


def repeat_pairs():
    """[(a case, the same case once more on the same plan)]: equal bit for bit."""
    out, n = [], 0
    for fam in ("ragged", "hub"):
        for m in structures(fam):
            for vec in VECS:
                d, dv = PAIRS[7 if n % 2 else 4]
                off = OFFS[n % 2]
                n += 1
                out.append((_case(m, off, vec, "real", 0, 0.125, d, dv, PADS[1], ALIGNED, True, "-repeat"),
                            _case(m, off, vec, "real", 0, 0.125, d, dv, PADS[1], ALIGNED, True, "-repeat-again")))
    return out


def hub_sequence():
    """On ONE plan of the hub row, in this order: const data (every merge of the 30-slice fix-up chain is exp(0)), other
    operands behind it, a wide dv of three passes, then a narrow one."""
    m, out = structures("hub")[0], []
    for off, vec in (("i32", "bf16"), ("i64", "f16")):
        for kind, variant, scale, d, dv in (("const", 0, 1.0, 8, TILE), ("real", 0, 1.0, 8, TILE), ("masked", 1, 0.125, 5, 129),
                                            ("real", 1, 0.125, 40, 129), ("real", 2, -2.0, 40, 3), ("const", 1, -2.0, 3, 3)):
            out.append(_case(m, off, vec, kind, variant, scale, d, dv, PADS[0], ALIGNED, True, "-seq"))
    return out


def fp32_pairs():
    """Cases on the crossing-row structures whose 16-bit O must equal narrow(the fp32 kernel's O on the widened operands) bit
    for bit: dv <= 4, where both kernels run C = 1 — one lane per nonzero, 64 slots a step, the same step and slice edges —
    and the one lane of a slot runs the whole score in ascending columns from +0 in both (4 or 8 columns a round of the same
    fma chain).  Above dv = 4 the fp32 kernel takes C >= 2 where the 16-bit kernel of the same dv takes a smaller C: the
    geometry differs by construction, and there is no pairing."""
    out, n = [], 0
    for m in structures("slice_edges")[:6] + structures("hub")[:1]:
        for dv, d in ((1, 100), (3, 16), (4, 45)):
            off, vec = TYPES[n % 4]
            out.append(_case(m, off, vec, "real", n % 3, SCALES[n % 3], d, dv, PADS[n % 2], ALIGNED, True, "-fp32"))
            n += 1
    return out


FAMILIES = STRUCTURE_FAMILIES + ("widths", "alignment", "repeat", "hub_sequence", "fp32_pairs")
FULL_CROSS = ("ragged", "hub", "one_col")      # every (offset width, 16-bit type); elsewhere two of the four, rotating


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
    if name == "fp32_pairs":
        return fp32_pairs()
    out = []
    for i, m in enumerate(structures(name)):
        types = TYPES if name in FULL_CROSS else (TYPES[i % 4], TYPES[(i + 3) % 4]) if len(structures(name)) < 4 else (TYPES[i % 4],)
        out += structure_cases(m, types, 3 * i)
    return out


def plan_key(c):
    return (c.matrix.name, c.off, c.vec, c.shift[:2])


_table = []


def table():
    if not _table:
        _table.extend(c for f in FAMILIES for c in family(f))
    return list(_table)


def weight(g):
    """Of a plan group, to deal the groups to batches: merge items times the lanes' work per nonzero."""
    return sum((len(c.matrix.lens) + sum(c.matrix.lens)) * -(-c.dv // TILE) * (2 + c.d // 16) + 3000 for c in g)


# ---- the host program's batch file: attention_cases.write_batch and read_results on what differs here ----------------------
def batch_operands(c):
    return ac.Batch(plan_key(c), data_key(c), VAL_TYPE[c.vec], *csr(c.matrix, c.off), *operands(c), lambda a: to_bits(a, c.vec), np.uint16,
                    np.float32, NAN_BITS[c.vec], int(to_bits(np.float32(CANARY), c.vec).reshape(-1)[0]), ac.NAN_BITS["f32"])


write_batch = functools.partial(ac.write_batch, operands=batch_operands)
read_results = functools.partial(ac.read_results, operands=batch_operands)
