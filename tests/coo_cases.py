"""The table of COO -> CSR, symmetric COO -> CSR and CSR-transpose cases (csrc/coo_csr.hip: mi355_spmv_coo_to_csr,
mi355_spmv_coo_to_csr_symmetric, mi355_spmv_csr_transpose) that tests/test_coo_sim_cpu.py executes on the host and
tests/test_gpu_coo_edges.py on the device: the same inputs for both, and one check.

The unit is an LSD radix sort by 8-bit digits with the source index as payload.  A tile is TILE = 4 096 entries, each of
its four waves walks a QUARTER of 1 024 in steps of STEP = 64, and the per-tile digit counts (256 a tile) are scanned in
workgroups of SCAN_CHUNK = 4 096 counts, so a second scan workgroup exists from 17 tiles on (65 537 entries).  The key is
the row (`coo`, `sym`) or the column (`transpose`); its DOMAIN (n_rows, or n_cols) sets the number of passes: 0 for 1, one
up to 256, two up to 65 536, three up to 2^24, four beyond.

Families (Case.family), each for every operation unless it names one:
    counts      every entry count of COUNTS (tile, quarter and step edges, the 16 / 17 tile edge) at domains 256 and 257;
                for `sym` these are stored entries, of mixed kind
    expanded    sym: stored counts whose EXPANDED count is at a tile edge (all off-diagonal 2 047 / 2 048 / 2 049; mixed
                with exactly 4 095 / 4 096 / 4 097 expanded)
    domains     every domain of DOMAINS at the counts CROSS = 1, 65, 4 096, 4 097 and 65 537: every pass count 0 .. 3 at all
                five.  The two domains around 2^24 (three and FOUR passes; their offsets array is 64 MB) stand at BIG_COUNTS
                only, as their size asks; 2^24 + 1 holds keys with top digit 1
    patterns    every key pattern of PATTERNS at 4 097 and 8 193 entries, domains 256 and 65 537 (`sym`: once with diagonal
                entries only, so that the sort meets the pattern itself, once with the pattern reversed as columns)
    types       offsets i32 / i64 x values f32 / f64 / i32 / none x perm asked for or not, fully crossed on three
                structures (`transpose` has offsets only); everywhere else the types are dealt round-robin
    sym         diagonal only, none, mixed; an off-diagonal entry at lane 63 of a step, as the last of a quarter (index
                1 023), of a tile (4 095) and of the list; an entry in both triangles; rectangular; one row
    transpose   runs of 1, 2 and 300 empty rows at the start, in the middle and at the end; a last row that is empty; 70
                empty rows first; one row holding everything; one row; one column; a hub column; 2 x 6 and 6 x 2
    bad         refusals: status 1, a message naming the FIRST offender, every output as it was (the canary)
    workspace   one structure per operation and pass count, run with the workspace prefilled with 0x00, 0xFF and 0x5A
    kernels     (host only) scan_sums, scan_reduce -> scan_sums -> scan_apply and offdiag_count -> scan_sums launched alone at
                sizes the entry points reach only with 2^28 entries

The reference is numpy alone, computed here: a stable argsort of the key, a bincount, and gathers.  Everything is an integer
or a copied bit pattern, so the bar is equality.  Values are a bijection of the entry index (as bits: NaN patterns and
both zeros occur), so no two entries carry the same value and the order inside a row shows in Ax as well as in perm."""
import collections
import struct

import numpy as np

STEP, QUARTER, TILE, SCAN_CHUNK = 64, 1024, 4096, 4096
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097,
          8191, 8192, 8193, 65535, 65536, 65537, 69633)
DOMAINS = (1, 2, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1)
CROSS = (1, 65, 4096, 4097, 65537)
BIG_COUNTS = {1 << 24: (4097,), (1 << 24) + 1: (4097, 65537)}
PATTERNS = ("zeros", "max", "alternate", "ascending", "descending", "distinct64", "lane0", "lane63", "low_const", "high_const",
            "d255_d0", "hub")
PATTERN_COUNTS, PATTERN_DOMAINS = (4097, 8193), (256, 65537)
OPS = ("coo", "sym", "transpose")
OFFS, VALS = ("i32", "i64"), ("f32", "f64", "i32", "none")
PREFILLS = (0x00, 0xFF, 0x5A)
CANARY = 0xC3                      # every byte of every output before the call
NP = {"i32": np.int32, "i64": np.int64}
VAL_BYTES = {"f32": 4, "f64": 8, "i32": 4, "none": 0}
OFF_TYPE = {"i32": 0, "i64": 1}
VAL_TYPE = {"f32": 0, "f64": 1, "i32": 2, "none": -1}      # MI355_VAL_*; none: vals and Ax are null (the call gets F32)
KERNEL_OPS = ("scan_sums", "scan_chain", "offdiag")
FAMILIES = ("counts", "expanded", "domains", "patterns", "types", "sym", "transpose", "bad", "workspace")

# gen + args name the structure (inputs() builds it once); bad: None or (what, where, message); prefill: the workspace's bytes
Case = collections.namedtuple("Case", "name op family gen args off val perm prefill bad")


def passes(domain):
    return (max(domain - 1, 0).bit_length() + 7) // 8


def keys(n, domain, pattern, seed):
    """n keys below `domain` in a pattern, by lane (index mod 64), step and tile of the walk."""
    rng = np.random.RandomState(seed)
    i = np.arange(n, dtype=np.int64)
    top = domain - 1
    if pattern == "random":
        k = rng.randint(0, domain, size=n).astype(np.int64)
        if n:
            k[n // 3] = top                     # the largest key (2^24 + 1: top digit 1) is always there
        if n > 2:
            k[(2 * n) // 3] = 0
    elif pattern == "zeros":
        k = np.zeros(n, dtype=np.int64)
    elif pattern == "max":
        k = np.full(n, top, dtype=np.int64)
    elif pattern == "alternate":
        k = np.where(i % 2 == 0, 0, top)
    elif pattern == "ascending":                # the identity where the domain has room, else each key a run
        k = i if domain >= n else i * domain // n
    elif pattern == "descending":
        k = (n - 1 - i) if domain >= n else (n - 1 - i) * domain // n
    elif pattern == "distinct64":               # 64 different low digits in every step, the high digit by step
        k = (i % 64 * 3 + i // 64 * 7) % 256
        if domain > 65535:
            k = k + (i // 64 * 37) % 256 * 256
    elif pattern in ("lane0", "lane63"):
        k = np.where(i % 64 == (0 if pattern == "lane0" else 63), top, 5 % domain)
    elif pattern == "low_const":                # low digit 7 everywhere, the high digit random (one digit: all equal)
        k = 7 + (rng.randint(0, 256, size=n) * 256 if domain > 65535 else 0) + 0 * i
    elif pattern == "high_const":
        k = rng.randint(0, 256, size=n) + (0x80 * 256 if domain > 65535 else 0)
    elif pattern == "d255_d0":                  # digit 255 beside digit 0, in both digits
        k = np.where(i % 2 == 0, 0x00FF, 0xFF00 if domain > 65535 else 0)
    elif pattern == "hub":                      # one key holds more than a tile where there is room, the rest random
        k = rng.randint(0, domain, size=n).astype(np.int64)
        hub = rng.permutation(n)[:min(n - 64, TILE + 104)]
        k[hub] = domain // 2
    else:
        raise KeyError(pattern)
    k = np.asarray(k, dtype=np.int64)
    assert len(k) == n and (n == 0 or (k.min() >= 0 and k.max() < domain)), (n, domain, pattern)
    return k.astype(np.int32)


def row_lengths_to_offsets(lens):
    Ap = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    return Ap


def random_offsets(n_rows, nnz, seed):
    """Offsets of n_rows rows that hold nnz slots, many rows empty."""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.randint(0, nnz + 1, size=n_rows - 1)) if n_rows > 1 else np.zeros(0, dtype=np.int64)
    return np.concatenate(([0], cuts, [nnz])).astype(np.int64)


# ---- structures: gen(args) -> the inputs of a call --------------------------------------------------------------------------
def _coo(n, domain, pattern, seed=0):
    rng = np.random.RandomState(1000 + seed)
    n_cols = 5 if seed % 2 else 300             # few columns: repeated (row, column) pairs
    return dict(n_rows=domain, n_cols=n_cols, rows=keys(n, domain, pattern, seed), cols=rng.randint(0, n_cols, size=n).astype(np.int32))


def _sym(n, domain, pattern, kind="mixed", seed=0, n_cols=None, n_rows=None):
    """n stored entries inside the leading square of `domain` rows of a symmetric matrix (n_rows x n_cols: the square
    unless given).  kind: diag (cols = rows), mixed (about half off the diagonal), offdiag (every entry off it: needs two
    rows), mirror (cols = the pattern reversed)."""
    rng = np.random.RandomState(2000 + seed)
    rows = keys(n, domain, pattern, seed)
    if kind == "diag" or domain == 1:
        cols = rows.copy()
    elif kind == "mirror":
        cols = rows[::-1].copy()
    else:
        other = rng.randint(0, domain, size=n).astype(np.int32)
        other = np.where(other == rows, (rows + 1) % domain, other).astype(np.int32)
        cols = other if kind == "offdiag" else np.where(rng.rand(n) < 0.5, rows, other).astype(np.int32)
    return dict(n_rows=domain if n_rows is None else n_rows, n_cols=domain if n_cols is None else n_cols, rows=rows, cols=cols)


def _sym_expanded(stored, expanded):
    """`stored` entries of which expanded - stored are off the diagonal, shuffled; 300 rows."""
    rng = np.random.RandomState(stored + expanded)
    rows = rng.randint(0, 300, size=stored).astype(np.int32)
    cols = rows.copy()
    off = rng.permutation(stored)[:expanded - stored]
    cols[off] = (rows[off] + 1 + rng.randint(0, 298, size=len(off))) % 300
    return dict(n_rows=300, n_cols=300, rows=rows, cols=cols)


def _sym_at(n, index, domain=257):
    """Diagonal entries but ONE off-diagonal entry, at `index` (negative: from the end), and a mixed second tile."""
    s = _sym(n, domain, "random", "diag", seed=index % 97)
    index %= n
    s["cols"][index] = (s["rows"][index] + 1) % domain
    tail = np.arange(n) > max(index, TILE)
    s["cols"][tail & (np.arange(n) % 3 == 0)] = 3
    return s


def _sym_both_triangles():
    rows = np.array([2, 0, 1, 2, 2, 1], dtype=np.int32)         # (2,0) (0,2) (1,1) (2,0) again (2,1) (1,1) again
    cols = np.array([0, 2, 1, 0, 1, 1], dtype=np.int32)
    return dict(n_rows=3, n_cols=3, rows=rows, cols=cols)


def _transpose(n, domain, pattern, seed=0, n_rows=None):
    n_rows = max(1, n // 3) if n_rows is None else n_rows
    return dict(n_rows=n_rows, n_cols=domain, Ap=random_offsets(n_rows, n, 3000 + seed), Aj=keys(n, domain, pattern, seed))


def _transpose_lens(lens, n_cols, pattern="random", seed=0):
    Ap = row_lengths_to_offsets(np.asarray(lens, dtype=np.int64))
    return dict(n_rows=len(lens), n_cols=n_cols, Ap=Ap, Aj=keys(int(Ap[-1]), n_cols, pattern, seed))


def _transpose_runs(run, where):
    """Rows of 1 .. 9 entries with `run` empty rows at the start, in the middle or at the end."""
    rng = np.random.RandomState(run + len(where))
    body = rng.randint(1, 10, size=40).tolist()
    lens = {"start": [0] * run + body, "middle": body[:20] + [0] * run + body[20:], "end": body + [0] * run}[where]
    return _transpose_lens(lens, 300, seed=run)


def _transpose_fixed(which):
    if which == "rect2x6":
        return dict(n_rows=2, n_cols=6, Ap=np.array([0, 4, 7], dtype=np.int64), Aj=np.array([5, 0, 3, 0, 1, 5, 2], dtype=np.int32))
    return dict(n_rows=6, n_cols=2, Ap=np.array([0, 1, 1, 3, 4, 4, 7], dtype=np.int64), Aj=np.array([1, 0, 1, 0, 1, 1, 0], dtype=np.int32))


GENS = {"coo": _coo, "sym": _sym, "sym_expanded": _sym_expanded, "sym_at": _sym_at, "sym_both": _sym_both_triangles,
        "transpose": _transpose, "transpose_lens": _transpose_lens, "transpose_runs": _transpose_runs,
        "transpose_fixed": _transpose_fixed}
_inputs = {}


def expand(rows, cols):
    """LoadCoo's rule: entry i, then its mirror if it is off the diagonal -> (row, column, stored index) of each."""
    reps = 1 + (rows != cols)
    src = np.repeat(np.arange(len(rows), dtype=np.int64), reps)
    mirror = np.zeros(len(src), dtype=bool)
    mirror[np.cumsum(reps)[reps == 2] - 1] = True
    return np.where(mirror, cols[src], rows[src]), np.where(mirror, rows[src], cols[src]), src


def values(n, val):
    """A bijection of the entry index, as bits."""
    i = np.arange(n, dtype=np.uint64)
    if val == "none":
        return None
    if val == "f64":
        return (i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x7FF8000000000001)).view(np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(0x7FC00001)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def inputs(c):
    """The arrays of the call as the case passes them (a bad case: with its offence put in); made once, left unchanged."""
    key = (c.gen, c.args, c.bad)
    if key not in _inputs:
        x = GENS[c.gen](*c.args)
        x = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in x.items()}
        if c.op == "sym":
            x["nnz_expanded"] = len(x["rows"]) + int((x["rows"] != x["cols"]).sum())
        if c.bad:
            for name, where, value in c.bad[0]:
                if name == "nnz_expanded":
                    x[name] += value
                else:
                    x[name][where] = value
        _inputs[key] = x
    return _inputs[key]


def nnz_out(c):
    """Entries of Aj / Ax / perm as the caller sizes them."""
    x = inputs(c)
    return x["nnz_expanded"] if c.op == "sym" else len(x["Aj"] if c.op == "transpose" else x["rows"])


def domain(c):
    x = inputs(c)
    return x["n_cols"] if c.op == "transpose" else x["n_rows"]


def expected(c):
    """dict(Ap, Aj, Ax, perm) by numpy: Ap as int64, Ax as bits (None without values), perm as int64."""
    x = inputs(c)
    if c.op == "transpose":
        Ap, Aj = x["Ap"], x["Aj"]
        perm = np.argsort(Aj, kind="stable")
        rows = np.repeat(np.arange(x["n_rows"], dtype=np.int32), np.diff(Ap))
        Apt = row_lengths_to_offsets(np.bincount(Aj, minlength=x["n_cols"]))
        return dict(Ap=Apt, Aj=rows[perm], Ax=None, perm=perm.astype(np.int64))
    rows, cols = x["rows"], x["cols"]
    src = np.arange(len(rows), dtype=np.int64)
    if c.op == "sym":
        rows, cols, src = expand(rows, cols)
    perm = np.argsort(rows, kind="stable")
    vals = values(len(x["rows"]), c.val)
    return dict(Ap=row_lengths_to_offsets(np.bincount(rows, minlength=x["n_rows"])), Aj=cols[perm].astype(np.int32),
                Ax=None if vals is None else vals[src[perm]], perm=src[perm])


def check(c, got):
    """got: dict(status, message, Ap, Aj, Ax, perm) as the call left them — Ap in the case's offset type, Aj int32, Ax as
    unsigned bits or None, perm int64 (transpose: the uint32 slots widened) or None."""
    if c.bad:
        assert got["status"] == 1, "%s: status %s (%s)" % (c.name, got["status"], got["message"])
        assert c.bad[1] in got["message"], "%s: the message is %r, want %r in it" % (c.name, got["message"], c.bad[1])
        for k in ("Ap", "Aj", "Ax", "perm"):
            if got[k] is not None:
                assert np.all(np.ascontiguousarray(got[k]).view(np.uint8) == CANARY), "%s: %s was written" % (c.name, k)
        return
    assert got["status"] == 0, "%s: status %s (%s)" % (c.name, got["status"], got["message"])
    want = expected(c)
    assert got["Ap"].dtype == NP[c.off] and np.array_equal(got["Ap"].astype(np.int64), want["Ap"]), "%s: Ap" % c.name
    assert np.array_equal(got["Aj"], want["Aj"]), "%s: Aj%s" % (c.name, first_difference(got["Aj"], want["Aj"]))
    for k in ("Ax", "perm"):
        present = (c.val != "none") if k == "Ax" else (c.perm or c.op == "transpose")
        assert (got[k] is not None) == present, "%s: %s" % (c.name, k)
        if present:
            assert np.array_equal(got[k], want[k]), "%s: %s%s" % (c.name, k, first_difference(got[k], want[k]))


def first_difference(a, b):
    if len(a) != len(b):
        return " has %d entries, want %d" % (len(a), len(b))
    at = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return " first differs at %d of %d: %s, want %s (%d differ)" % (at[0], len(a), a[at[0]], b[at[0]], len(at)) if len(at) else ""


# ---- the table ---------------------------------------------------------------------------------------------------------
TYPE_PAIRS = [(o, v, p) for o in OFFS for v in VALS for p in (True, False)]


def _bad_cases(add):
    n, d = 2 * TILE + 1, 257
    places = (0, n - 1, TILE - 1, TILE)
    later = lambda where: where + 7 if where + 7 < n else None      # a second offender behind the first, where one fits

    def entries(op, gen, args, kinds):
        x = GENS[gen](*args)
        for what, field, value, (second_field, second_value) in kinds:
            for where in places:
                edits = ((field, where, value),) + (((second_field, later(where), second_value),) if later(where) is not None else ())
                r = value if field == "rows" else int(x["rows"][where])
                cc = value if field == "cols" else int(x["cols"][where])
                add(op, "bad", gen, args, bad=(edits, "entry %d is (row %d, col %d)" % (where, r, cc)), tag="%s_at%d" % (what, where))

    entries("coo", "coo", (n, d, "random", 8),      # 257 rows, 300 columns
            (("row_minus_1", "rows", -1, ("rows", d + 5)), ("row_n_rows", "rows", d, ("cols", 400)), ("col_n_cols", "cols", 300, ("rows", -3))))
    # sym: 257 rows, 400 columns for the rectangular offence: (row 3, col 300) is inside, its mirror (300, 3) is not
    sym_args = (n, d, "random", "mixed", 7, 400)
    entries("sym", "sym", sym_args,
            (("row_minus_1", "rows", -1, ("rows", d + 5)), ("row_n_rows", "rows", d, ("cols", 400)), ("col_n_cols", "cols", 400, ("rows", -3)),
             ("mirror_outside", "cols", 300, ("rows", d + 5))))
    for delta in (-1, 1):
        x = GENS["sym"](*sym_args)
        true = n + int((x["rows"] != x["cols"]).sum())
        add("sym", "bad", "sym", sym_args, bad=((("nnz_expanded", 0, delta),), "nnz_expanded is %d, the stored entries expand to %d" % (true + delta, true)),
            tag="expanded_%+d" % delta)
    t_args = (n, d, "random", 7)
    for what, value, second in (("col_minus_1", -1, d + 3), ("col_n_cols", d, -9)):
        for where in places:
            edits = (("Aj", where, value),) + ((("Aj", later(where), second),) if later(where) is not None else ())
            add("transpose", "bad", "transpose", t_args, bad=(edits, "entry %d of Aj is column %d," % (where, value)), tag="%s_at%d" % (what, where))
    x = GENS["transpose"](*t_args)
    Ap, m = x["Ap"], x["n_rows"]
    mid = m // 2
    for what, edits, text in (("first_not_0", (("Ap", 0, 1),), "Ap[0] is 1, not 0"),
                              ("descent", (("Ap", mid, int(Ap[mid - 1]) - 1), ("Ap", mid + 9, -4)), "Ap[%d] = %d is below Ap[%d]" % (mid, Ap[mid - 1] - 1, mid - 1)),
                              ("last_not_nnz", (("Ap", m, n + 1),), "Ap[%d] = %d, the last offset, is not nnz = %d" % (m, n + 1, n)),
                              ("last_descends", (("Ap", m, int(Ap[m - 1]) - 1),), "Ap[%d] = %d is below Ap[%d]" % (m, Ap[m - 1] - 1, m - 1))):
        add("transpose", "bad", "transpose", t_args, bad=(edits, text), tag=what)


def table():
    out, n_dealt = [], [0]

    def add(op, family, gen, args, off=None, val=None, perm=None, prefill=0x5A, bad=None, tag=None):
        o, v, p = TYPE_PAIRS[n_dealt[0] % len(TYPE_PAIRS)]
        n_dealt[0] += 7                         # (7 and 16 are coprime: every pair comes round)
        off, val, perm = o if off is None else off, v if val is None else val, p if perm is None else perm
        if op == "transpose":
            val, perm = "none", True
        name = "%s-%s-%s-%s-%s-%s%s" % (op, family, tag or "_".join(str(a) for a in args), off, val, "perm" if perm else "noperm",
                                        "" if prefill == 0x5A else "-ws%02x" % prefill)
        out.append(Case(name, op, family, gen, tuple(args), off, val, perm, prefill, bad))

    gen_of = {"coo": "coo", "sym": "sym", "transpose": "transpose"}
    for op in OPS:
        for d in (256, 257):
            for n in COUNTS:
                add(op, "counts", gen_of[op], (n, d, "random"))
        for d in DOMAINS:
            for n in BIG_COUNTS.get(d, CROSS):
                add(op, "domains", gen_of[op], (n, d, "random"), off="i32" if d >= 1 << 24 else None)
        for pattern in PATTERNS:
            for d in PATTERN_DOMAINS:
                for n in PATTERN_COUNTS:
                    if op == "sym":
                        add(op, "patterns", "sym", (n, d, pattern, "diag"))
                        add(op, "patterns", "sym", (n, d, pattern, "mirror"))
                    else:
                        add(op, "patterns", gen_of[op], (n, d, pattern))
        for args in ((4097, 257, "random"), (65, 65537, "random"), (8193, 256, "hub")):
            for o, v, p in (TYPE_PAIRS if op != "transpose" else [(o, "none", True) for o in OFFS]):
                add(op, "types", gen_of[op], args, off=o, val=v, perm=p)
        for d in (1, 256, 257, 65537, (1 << 24) + 1):       # 0, 1, 2, 3 and 4 passes
            for prefill in PREFILLS:
                add(op, "workspace", gen_of[op], (4097 + 64, d, "random", ) + (("mixed", 1) if op == "sym" else (1,)),
                    off="i32", val="none" if op == "transpose" else "f32", perm=True, prefill=prefill)
    for stored in (2047, 2048, 2049):
        add("sym", "expanded", "sym_expanded", (stored, 2 * stored))
    for expanded in (4095, 4096, 4097):
        add("sym", "expanded", "sym_expanded", (3000, expanded))
    for kind in ("diag", "offdiag", "mixed"):
        add("sym", "sym", "sym", (5000, 300, "random", kind), tag="kind_" + kind)
    for what, n, index in (("lane63", 200, 63), ("lane63_step5", 5000, 5 * 64 + 63), ("quarter_last", 5000, QUARTER - 1),
                           ("tile_last", 5000, TILE - 1), ("tile_last_exact", TILE, TILE - 1), ("list_last", 5000, -1),
                           ("list_last_tile_edge", 2 * TILE, -1)):
        add("sym", "sym", "sym_at", (n, index), tag="offdiag_" + what)
    add("sym", "sym", "sym_both", (), tag="both_triangles")
    add("sym", "sym", "sym", (5000, 300, "random", "mixed", 3, 1000), tag="rect_300x1000")
    add("sym", "sym", "sym", (5000, 300, "random", "mixed", 4, 300, 1000), tag="rect_1000x300")
    add("sym", "sym", "sym", (5000, 1, "zeros", "diag"), tag="one_row")
    for run in (1, 2, 300):
        for where in ("start", "middle", "end"):
            add("transpose", "transpose", "transpose_runs", (run, where))
    body = tuple(int(v) for v in np.random.RandomState(70).randint(0, 7, size=90))
    add("transpose", "transpose", "transpose_lens", (body + (0,), 300), tag="last_row_empty")
    add("transpose", "transpose", "transpose_lens", ((0,) * 70 + body, 300), tag="first_70_rows_empty")
    add("transpose", "transpose", "transpose_lens", ((0,) * 9 + (5000,) + (0,) * 9, 300), tag="one_row_holds_all")
    add("transpose", "transpose", "transpose_lens", ((5000,), 300), tag="n_rows_1")
    add("transpose", "transpose", "transpose", (5000, 1, "zeros"), tag="n_cols_1")
    add("transpose", "transpose", "transpose", (8193, 300, "hub"), tag="hub_column")
    add("transpose", "transpose", "transpose_fixed", ("rect2x6",))
    add("transpose", "transpose", "transpose_fixed", ("rect6x2",))
    _bad_cases(lambda op, family, gen, args, bad, tag: add(op, family, gen, args, off="i64", val="f64", perm=True, bad=bad, tag=tag))
    assert len({c.name for c in out}) == len(out)
    return out


Kernel = collections.namedtuple("Kernel", "name op n data")


def kernel_cases():
    """The kernel records: scan_sums alone, the three scan kernels in a row, offdiag_count with scan_sums."""
    out = []
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193, 12293):
        rng = np.random.RandomState(n)
        out.append(Kernel("scan_sums-%d-random" % n, "scan_sums", n, rng.randint(0, 1000, size=n).astype(np.uint32)))
        big = np.full(n, (2 ** 32 - 1) // n, dtype=np.uint32)          # the total is just below 2^32
        big[rng.randint(0, n)] += np.uint32((2 ** 32 - 1) % n)
        assert int(big.astype(np.uint64).sum()) == 2 ** 32 - 1
        out.append(Kernel("scan_sums-%d-full" % n, "scan_sums", n, big))
    for n in [256 * t for t in (1, 16, 17, 32, 33)] + [4097, 8191]:
        out.append(Kernel("scan_chain-%d" % n, "scan_chain", n, np.random.RandomState(n).randint(0, 5000, size=n).astype(np.uint32)))
    for tiles in (1, 2, 17):
        for n in (tiles * TILE, tiles * TILE - 37):
            x = _sym(n, 300, "random", "mixed", seed=tiles)
            out.append(Kernel("offdiag-%d" % n, "offdiag", n, (x["rows"], x["cols"])))
    return out


def kernel_expected(k):
    if k.op == "offdiag":
        rows, cols = k.data
        per_tile = [int((rows[t:t + TILE] != cols[t:t + TILE]).sum()) for t in range(0, k.n, TILE)] + [0]
        data = np.array(per_tile, dtype=np.uint32)
    else:
        data = k.data
    sums = np.zeros(len(data), dtype=np.uint64)         # the exclusive prefix sum, in the kernels' 32 bits
    np.cumsum(data[:-1].astype(np.uint64), out=sums[1:])
    return (sums & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def weight(g):
    """Of a group of cases, to deal them to batches: what the host simulation pays for, roughly — the sort's tile walks per
    pass, and a search per row of the offsets."""
    return sum((nnz_out(c) + 500) * (1 + 2 * passes(domain(c))) + domain(c) // 4 for c in g)


# ---- the host program's batch file (tests/cpp/coo_sim.cpp, whose header comment has the records) -----------------------------
def compact(c):
    """Offsets of 2^24 rows come back as their steps (index, value), not as 64 MB."""
    return domain(c) >= 1 << 24


def write_batch(path, cases, kernels=()):
    words = lambda *v: struct.pack("<%dq" % len(v), *v)
    with open(path, "wb") as f:
        for c in cases:
            x = inputs(c)
            n_rows, n_cols = x["n_rows"], x["n_cols"]
            if c.op == "transpose":
                f.write(words(3, OFF_TYPE[c.off], n_rows, n_cols, len(x["Aj"]), c.prefill, int(compact(c))))
                f.write(x["Ap"].astype(NP[c.off]).tobytes() + x["Aj"].tobytes())
                continue
            vals = values(len(x["rows"]), c.val)
            head = (OFF_TYPE[c.off], VAL_TYPE[c.val], int(c.perm), n_rows, n_cols, len(x["rows"]))
            if c.op == "coo":
                f.write(words(1, *head, c.prefill, int(compact(c))))
            else:
                f.write(words(2, *head, x["nnz_expanded"], c.prefill, int(compact(c))))
            f.write(x["rows"].tobytes() + x["cols"].tobytes() + (vals.tobytes() if vals is not None else b""))
        for k in kernels:
            f.write(words({"scan_sums": 5, "scan_chain": 6, "offdiag": 7}[k.op], k.n))
            f.write(k.data.tobytes() if k.op != "offdiag" else k.data[0].tobytes() + k.data[1].tobytes())
        f.write(words(0))
    return list(cases)


def read_results(path, cases, kernels=()):
    """[dict(status, message, Ap, Aj, Ax, perm)] per case as check() takes it, then [uint32 array] per kernel record when
    asked."""
    out, kout = [], []
    with open(path, "rb") as f:
        take = lambda n, dt: np.frombuffer(f.read(n * np.dtype(dt).itemsize), dtype=dt)
        for c in cases:
            status, n_msg = struct.unpack("<2q", f.read(16))
            message = f.read(n_msg).decode()
            n, n_off = nnz_out(c), domain(c) + 1
            if compact(c):
                m = struct.unpack("<q", f.read(8))[0]
                steps = take(2 * m, np.int64).reshape(m, 2)
                assert m >= 1 and steps[0, 0] == 0
                Ap = np.repeat(steps[:, 1], np.diff(np.concatenate((steps[:, 0], [n_off])))).astype(NP[c.off])
            else:
                Ap = take(n_off, NP[c.off])
            Aj = take(n, np.int32)
            if c.op == "transpose":
                Ax, perm = None, take(n, np.uint32)
                perm = perm if c.bad else perm.astype(np.int64)
            else:
                Ax = take(n, np.uint64 if c.val == "f64" else np.uint32) if c.val != "none" else None
                perm = take(n, np.int64) if c.perm else None
            out.append(dict(status=status, message=message, Ap=Ap, Aj=Aj, Ax=Ax, perm=perm))
        for k in kernels:
            status, count = struct.unpack("<2q", f.read(16))
            assert status == 0, k.name
            kout.append(take(count, np.uint32))
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return (out, kout) if kernels else out
