"""The table of row-softmax cases (csrc/row_softmax.hip) that tests/test_row_softmax_sim_cpu.py executes on the host and
tests/test_gpu_row_softmax.py on the device: the same structures, operands and expected results for both.

    forward    v = scale * x;  out[n] = exp(v[n] - max_row v) / sum_row exp(v - max_row v)
    backward   t_r = sum_row p * dp;  dx[n] = scale * p[n] * (dp[n] - t_r)

The structures are those of tests/multi_cases.py and tests/sddmm_cases.py (imported, not copied: the kernel cuts its work
exactly as the multi-vector kind does, SLICE_LEN merge items per wave, STEP nonzeros per group), plus one of rows of
power-of-two lengths that cross groups and slices.  Both test files assert the geometry: the host file against the
constants of csrc/row_softmax.hip and csrc/common.hpp, the device file against info() (assert_geometry).

Expected values come from numpy in fp64 (forward_ref, backward_ref).  Kinds of data:
  const    every entry of row r equals c_r, c_r spread over +-1e4 (a kernel that forgets the max overflows): out must be
           val(1) / val(len_r) EXACTLY.  Backward on that p with dp in {-3 .. 3}: exact on rows of power-of-two length
           (every product, sum and difference is then exact in any order; the sign of a zero apart), the bound elsewhere.
  masked   const, with -inf at chosen entries (mask()): exactly +0 there, val(1) / val(unmasked entries of the row)
           elsewhere, +0 everywhere in a row that is masked whole.
  real     x uniform with a row spread D_r <= 20 of v (nothing underflows), scale in SCALES.  Forward bound, eps of the type:
               |got - want| <= eps * want * (2 len_r + 2 E + 2 (max_row |v| + D_r) + 4)
           a worst-case count of the roundings of v, v - m, the sum in any order, the rescales of at most len_r / 64 + 2
           merges and the divide, and E ulps for exp in numerator and denominator.  E = 3: the ROCm installation here
           documents no ulp table for its device math library, so this is the OpenCL full-profile bound for exp that the
           library is written to.  Backward bound:
               |got - want| <= eps |scale| p[n] ((len_r + 2) sum_row |p dp| + 3 (|dp[n]| + |t_r|))  +  the smallest normal
           Nothing in either is measured.
A row of one finite entry must give exactly 1 in every forward case.  On the device one element before and one behind out
hold a canary that must survive (tests/test_gpu_row_softmax.py); on the host every operand is an allocation of exactly nnz
elements."""
import collections
import struct

import numpy as np

import multi_cases as mc
import sddmm_cases as sc
from multi_cases import NP, SLICE_LEN, STEP, bits, slices  # noqa: F401

CANARY = -777.25
E_EXP = 3
SCALES = (1.0, 0.125, -2.0)
GROUPS = SLICE_LEN // STEP          # groups of 64 nonzeros a slice can hold
ALL_TYPES = mc.ALL_TYPES
# element offsets of Ap, Aj, a (x / p), b (dp), out from an aligned base
SHIFTS = ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (0, 0, 1, 0, 0), (0, 0, 0, 0, 1), (0, 0, 0, 1, 0))
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
TINY = {"f32": float(np.finfo(np.float32).tiny), "f64": float(np.finfo(np.float64).tiny)}

Matrix = sc.Matrix
# mode: "fwd" | "bwd"; kind: "const" | "masked" | "real"; variant: the mask's or the draw's; in_place: 0 = out of its own,
# 1 = out is a (out == x; dx == p), 2 = out is b (dx == dp)
Case = collections.namedtuple("Case", "name matrix off val mode kind variant scale in_place shift")


def assert_geometry(info):
    """info() of a plan agrees with the constants the structures are built from."""
    assert info["slice_len"] == SLICE_LEN
    assert info["block_threads"] % STEP == 0 and SLICE_LEN % STEP == 0
    assert info["main_kernel"] == "row_softmax_slice_kernel"


# ---- structures --------------------------------------------------------------------------------------------------------
def pow2_structure(L=SLICE_LEN):
    """Rows of power-of-two lengths inside a group, across groups and across up to nine slices."""
    lens = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 1, 8192, 2, 64, 0, 1024, 4)
    assert sum(1 for r0, r1, n0, nn in slices(lens, L) if nn == L and r1 == r0) >= 8
    return Matrix("pow2_rows", "pow2", lens, 17, 600)


def structures(family):
    if family == "row_ends":
        return mc.row_end_structures()
    if family == "open_row":
        return mc.open_row_structures()
    if family == "slice_edges":
        return mc.slice_edge_structures()
    if family == "ragged":
        return [mc.ragged_structure()]
    if family == "hub":
        return [sc.hub_structure()]
    if family == "empty_runs":
        return [sc.empty_run_structure()]
    if family == "position":
        return sc.position_structures()
    if family == "pow2":
        return [pow2_structure()]
    raise KeyError(family)


def rows_of(m):
    return np.repeat(np.arange(len(m.lens)), m.lens)


def csr(m, off):
    """(Ap, Aj): Aj is never read by the kernels; it holds valid columns all the same."""
    Ap = np.zeros(len(m.lens) + 1, dtype=NP[off])
    np.cumsum(m.lens, out=Ap[1:])
    Aj = (np.arange(int(Ap[-1]), dtype=np.int64) * 7 % max(m.n_cols, 1)).astype(np.int32)
    return Ap, Aj


def mask(m, variant):
    """The masked entries of a structure (bool per nonzero).  Both variants: both sides of every group edge and slice edge
    (the last entry of a group or slice and the first of the next).  Variant 0: the first entry of rows r % 3 == 0, the
    last of rows r % 3 == 1, every row r % 7 == 3 whole, and of every second slice with a crossing row the whole piece of
    the row carried in.  Variant 1: the classes shifted by one, and the whole piece of the row open at the slice's end."""
    lens = np.asarray(m.lens, dtype=np.int64)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    nnz = int(Ap[-1])
    out = np.zeros(nnz, dtype=bool)

    def put(n):
        if 0 <= n < nnz:
            out[n] = True

    for w, (r0, r1, n0, nn) in enumerate(slices(m.lens)):
        for e in range(n0, n0 + nn + 1, STEP):
            put(e - 1)
            if e < n0 + nn:
                put(e)
        put(n0 + nn - 1)
        put(n0 + nn)
        if w % 2 == variant and nn > 0:
            if variant == 0 and Ap[r0] < n0:                        # the piece of the row carried in
                out[n0:min(int(Ap[r0 + 1]), n0 + nn)] = True
            if variant == 1 and r1 < len(lens) and Ap[r1] < n0 + nn:   # the piece of the row open at the end
                out[max(int(Ap[r1]), n0):n0 + nn] = True
    for r in range(len(lens)):
        if lens[r] == 0:
            continue
        if r % 3 == variant:
            put(int(Ap[r]))
        if r % 3 == variant + 1:
            put(int(Ap[r + 1]) - 1)
        if r % 7 == 3 + variant:
            out[Ap[r]:Ap[r + 1]] = True
    return out


# ---- operands and expected results -------------------------------------------------------------------------------------
_operands = {}


def row_constants(m):
    """c_r: multiples of 0.25 spread over +-1e4 (exact in fp32, and so are their products with the SCALES)."""
    rng = np.random.RandomState(m.seed + 7)
    c = np.round(rng.uniform(-1e4, 1e4, size=len(m.lens)) * 4) / 4
    c[::5] = np.where(np.arange(len(c[::5])) % 2 == 0, 1e4, -1e4)
    return c


def forward_ref(x, scale, m):
    """(want, v, row max |v|, row spread D) of a forward in fp64 from the operand as stored."""
    rows, n_rows = rows_of(m), len(m.lens)
    with np.errstate(invalid="ignore", over="ignore"):
        v = scale * x.astype(np.float64)
        top = np.full(n_rows, -np.inf)
        np.maximum.at(top, rows, v)
        e = np.where(np.isneginf(v), 0.0, np.exp(v - np.where(np.isneginf(top), 0.0, top)[rows]))
        s = np.bincount(rows, weights=e, minlength=n_rows)
        want = np.where(s[rows] > 0, e / np.where(s > 0, s, 1.0)[rows], 0.0)
        fin = np.where(np.isneginf(v), np.nan, v)
        lo, hi = np.full(n_rows, np.inf), np.full(n_rows, -np.inf)
        np.fmin.at(lo, rows, fin)
        np.fmax.at(hi, rows, fin)
        vmax = np.where(hi >= lo, np.maximum(np.abs(lo), np.abs(hi)), 0.0)
        spread = np.where(hi >= lo, hi - lo, 0.0)
    return want, v, vmax, spread


def backward_ref(p, dp, scale, m):
    """(want, t, sum_row |p dp|) of a backward in fp64 from the operands as stored."""
    rows, n_rows = rows_of(m), len(m.lens)
    p64, dp64 = p.astype(np.float64), dp.astype(np.float64)
    t = np.bincount(rows, weights=p64 * dp64, minlength=n_rows)
    tabs = np.bincount(rows, weights=np.abs(p64 * dp64), minlength=n_rows)
    return scale * p64 * (dp64 - t[rows]), t, tabs


def operands(c):
    """(a, b) of a case in its value type: (x, None) forward, (p, dp) backward.  Made once and left unchanged."""
    key = (c.matrix.name, c.val, c.mode, c.kind, c.variant, c.scale)
    if key in _operands:
        return _operands[key]
    m, V = c.matrix, NP[c.val]
    rows, nnz = rows_of(m), sum(m.lens)
    lens = np.asarray(m.lens, dtype=np.int64)
    rng = np.random.RandomState(m.seed * 31 + c.variant * 7 + (c.mode == "bwd") + 1000)
    if c.kind in ("const", "masked"):
        x = row_constants(m)[rows].astype(V)
        if c.kind == "masked":
            x[mask(m, c.variant)] = -np.inf
        if c.mode == "fwd":
            res = (x, None)
        else:       # the exact forward output of the const rows, and small integers
            res = ((V(1) / np.maximum(lens, 1).astype(V))[rows], rng.randint(-3, 4, size=nnz).astype(V))
    else:
        base = rng.uniform(-50, 50, size=len(lens))
        spread = rng.uniform(0, 20, size=len(lens))
        spread[::4] = 20.0
        x = ((base[rows] + rng.rand(nnz) * spread[rows] * 0.999) / c.scale).astype(V)
        if c.mode == "fwd":
            res = (x, None)
        else:       # p = a forward's output in the value type, dp in (-1, 1)
            res = (forward_ref(x, c.scale, m)[0].astype(V), (rng.rand(nnz) * 2 - 1).astype(V))
    _operands[key] = res
    return res


def exact_bits(a):
    """The bit patterns as they are (a forward's +0 must be +0)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(c, out):
    """out: the nnz values an execute left."""
    m, V = c.matrix, NP[c.val]
    out = np.asarray(out)
    assert out.shape == (sum(m.lens),) and out.dtype == V, c.name
    assert not np.any(np.isnan(out)), "%s: NaN in out (entries %s)" % (c.name, np.nonzero(np.isnan(out))[0][:8])
    rows, lens = rows_of(m), np.asarray(m.lens, dtype=np.int64)
    eps = EPS[c.val]
    a, b = operands(c)
    if c.mode == "fwd":
        want, v, vmax, spread = forward_ref(a, c.scale, m)
        if c.kind in ("const", "masked"):
            live = np.bincount(rows, weights=~np.isneginf(a), minlength=len(lens)).astype(np.int64)
            exact = np.where(np.isneginf(a), V(0), V(1) / np.maximum(live, 1).astype(V)[rows]).astype(V)
            bad = np.nonzero(exact_bits(out) != exact_bits(exact))[0]
            assert bad.size == 0, "%s: entries %s differ from the exact value (got %s, want %s)" % (c.name, bad[:8], out[bad[:8]], exact[bad[:8]])
            return
        assert spread.max() <= 20.0 + 1e-3, c.name
        one = (lens == 1)[rows]
        assert np.all(out[one] == V(1)), "%s: a row of one entry is not exactly 1" % c.name
        bound = eps * want * (2 * lens[rows] + 2 * E_EXP + 2 * (vmax + spread)[rows] + 4)
    else:
        want, t, tabs = backward_ref(a, b, c.scale, m)
        if c.kind == "const":
            pow2 = ((lens & (lens - 1)) == 0)[rows]
            bad = np.nonzero(bits(out[pow2]) != bits(want[pow2].astype(V)))[0]
            assert bad.size == 0, "%s: power-of-two rows: entries %s differ from the exact value" % (c.name, np.nonzero(pow2)[0][bad[:8]])
        bound = eps * abs(c.scale) * a.astype(np.float64) * ((lens + 2)[rows] * tabs[rows] + 3 * (np.abs(b.astype(np.float64)) + np.abs(t[rows]))) + TINY[c.val]
    err = np.abs(out.astype(np.float64) - want)
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, "%s: entries %s outside the bound (error / bound %s)" % (c.name, bad[:8], (err / bound)[bad[:8]])


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(m, off, val, mode, kind, variant, scale, in_place=0, shift=SHIFTS[0], tag=""):
    name = "%s-%s-%s-%s-%s%d-s%g-ip%d-%s%s" % (m.name, off, val, mode, kind, variant, scale, in_place, "".join(map(str, shift)), tag)
    return Case(name, m, off, val, mode, kind, variant, float(scale), in_place, tuple(shift))


def structure_cases(m, types, n0=0):
    """What every structure is put through, per (offset width, value type) of `types`: const and both masks forward,
    const backward, real forward and backward under every scale; operand offsets rotate."""
    out, n = [], n0
    for off, val in types:
        plan = []
        plan.append(("fwd", "const", 0, 1.0))
        plan.append(("fwd", "masked", 0, 1.0))
        plan.append(("fwd", "masked", 1, 0.125))
        plan.append(("bwd", "const", 0, SCALES[n % 3]))
        for i, scale in enumerate(SCALES):
            plan.append(("fwd", "real", i, scale))
            plan.append(("bwd", "real", i, scale))
        for mode, kind, variant, scale in plan:
            out.append(_case(m, off, val, mode, kind, variant, scale, 0, SHIFTS[n % len(SHIFTS)]))
            n += 1
    return out


def two_types(i):
    """Both value types and both offset widths over a family's structures: structure i takes two of the four pairs."""
    return (ALL_TYPES[0], ALL_TYPES[1]) if i % 2 == 0 else (ALL_TYPES[2], ALL_TYPES[3])


_IN_PLACE_STRUCTURES = ("ragged", "hub", "slice_edges", "pow2")


def in_place_pairs():
    """[(out of place, in place)]: equal bit for bit.  Forward out == x; backward dx == p and dx == dp."""
    out, n = [], 0
    for fam in _IN_PLACE_STRUCTURES:
        for m in structures(fam)[:5]:
            for mode, kind, variant, scale in (("fwd", "real", 0, 1.0), ("fwd", "masked", 1, 0.125), ("bwd", "real", 1, 0.125),
                                               ("bwd", "const", 0, -2.0)):
                off, val = ALL_TYPES[n % 4]
                n += 1
                base = _case(m, off, val, mode, kind, variant, scale, 0, SHIFTS[0], "-inplace")
                for ip in ((1,) if mode == "fwd" else (1, 2)):
                    out.append((base, _case(m, off, val, mode, kind, variant, scale, ip, SHIFTS[0], "-inplace")))
    return out


def repeat_pairs():
    """[(a case, the same case once more on the same plan)]: equal bit for bit."""
    out, n = [], 0
    for fam in ("ragged", "hub"):
        for m in structures(fam):
            for mode in ("fwd", "bwd"):
                off, val = ALL_TYPES[n % 4]
                n += 1
                out.append((_case(m, off, val, mode, "real", 2, -2.0, 0, SHIFTS[0], "-repeat"),
                            _case(m, off, val, mode, "real", 2, -2.0, 0, SHIFTS[0], "-repeat-again")))
    return out


FAMILIES = ("row_ends", "open_row", "slice_edges", "ragged", "hub", "empty_runs", "position", "pow2", "in_place", "repeat")


def family(name):
    """The cases of one family, in plan order: cases of one (matrix, types, matrix offsets) share a plan, and keep the
    order they have here (the hub row's const case first: what follows it on the plan sees its scratch)."""
    if name == "in_place":
        seen, out = set(), []
        for a, b in in_place_pairs():
            for c in (a, b):
                if c.name not in seen:
                    seen.add(c.name)
                    out.append(c)
        return out
    if name == "repeat":
        return [c for pair in repeat_pairs() for c in pair]
    out = []
    for i, m in enumerate(structures(name)):
        out += structure_cases(m, ALL_TYPES if name in ("ragged", "hub", "pow2") else two_types(i), i)
    return out


def plan_key(c):
    return (c.matrix.name, c.off, c.val, c.shift[:2])


def table():
    return [c for f in FAMILIES for c in family(f)]


def weight(g):
    """Of a plan group, to deal the groups to batches: merge items."""
    return sum(len(c.matrix.lens) + sum(c.matrix.lens) + 2000 for c in g)


# ---- the host program's batch file (tests/cpp/row_softmax_sim.cpp, whose header comment has the records) ------------------
def write_batch(path, cases):
    """Cases in plan order; returns them in the order their results come back."""
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    last = None
    with open(path, "wb") as f:
        for c in cases:
            if plan_key(c) != last:
                last = plan_key(c)
                Ap, Aj = csr(c.matrix, c.off)
                f.write(words(1, ("i32", "i64").index(c.off), ("f32", "f64").index(c.val), len(c.matrix.lens), c.matrix.n_cols,
                              int(Ap[-1]), *c.shift[:2]))
                f.write(Ap.tobytes())
                f.write(Aj.tobytes())
            a, b = operands(c)
            f.write(words(4, int(c.mode == "bwd"), c.in_place, c.shift[2], c.shift[3], c.shift[4]))
            f.write(struct.pack("<d", c.scale))
            f.write(a.tobytes())
            if b is not None:
                f.write(b.tobytes())
        f.write(words(0))
    return list(cases)


def read_results(path, cases):
    """[(status, out)] per case; raises if the file is not complete."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            st, count = struct.unpack("<2q", f.read(16))
            assert count == sum(c.matrix.lens), c.name
            out.append((st, np.frombuffer(f.read(count * np.dtype(NP[c.val]).itemsize), dtype=NP[c.val])))
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return out
