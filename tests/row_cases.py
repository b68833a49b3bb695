"""The table of chunk_rows cases (csrc/xwindow.hpp: the body of the vector and light kinds' window kernels) that
tests/test_gpu_row_edges.py executes on the device and whose reach tests/test_row_cases_cpu.py proves on the host.

Geometry.  A plan of T lanes per row and BLOCK threads walks chunks of rows_per_chunk rows; a chunk is walked in groups
of STRIDE = (BLOCK / T) * R rows, R = rows_in_flight(sizeof(value), T), and slot r of vector v of a wave is row
r * (64 / T) + v of that wave's rows of the group.  A step is 4 T nonzeros from (lo & ~3); a row longer than
LONG = 4 T long_steps is left to the wave pass (one wave per marked row, in turn), beyond kHugeRow to the whole
workgroup, beyond the plan's giant length (weight-cut plans) to the slice kernels; elements from nnz & ~3 on are added by
scalar code.  Every case creates its plan under the knobs that force T, BLOCK, the rows per chunk, the long-row threshold
and the window of x; plan_of() says what that plan must report, and census() restates the DECOMPOSITION only (which
chunk, group, slot, phase, step count and pass a row gets) — it never computes a y.  Expected values come from the
serial oracle alone.

Data.  Integer values without zeros ({+-1, +-2, +-3} x {+-1, +-2}): every sum is exact in any order and ONE element
leaking into or missing from a row changes it, so a row's neighbours always tell; the groups family gives row r the sum
r + 1 instead (a permuted row mapping is seen); real values in (-1, 1) for the parity bound.  The columns of x that no
row references hold NaN.

Not here: the swept window (chunk_rows_sweep) has its own table, tests/sweep_cases.py, on hand-written plan shapes; the
1 024-thread workgroup of the window kernels needs a band of 16 K columns, and light's dequeue modes of the window
kernels more chunks than the chip holds — they are covered at that size by tests/test_gpu_parity.py,
tests/test_gpu_kept_plans.py and tests/test_gpu_block_shapes.py."""
import collections
import functools
import os
import re

import numpy as np

from kept_structures import probed_rows

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spmv-samples_amd", "csrc")

# the literals the table was written with; source_constants() reads the same from the product's text
WAVE = 64
K_BLOCK, K_WIDE_BLOCK = 256, 512
K_LONG_STEPS = 16
K_HUGE_ROW = 1024
K_MAX_CHUNK_ROWS = 2048
K_WINDOW_BYTES = 36 * 1024
ADAPT_MEANS = (16, 64)               # chunk_rows_any: T = 2 / 8 / 32 at a chunk mean <= 16, <= 64, beyond
ADAPT_LANES = (2, 8, 32)
BALANCED_LONG_STEPS = 4              # long_steps_for: weight-cut plans
GIANT_ROW = 4096                     # the smallest MI355_SPMV_GIANT_ROW the planner honours
LANES = (2, 4, 8, 16, 32, 64)
HW = 96                              # half width of the band the matrices' columns lie in


def rows_in_flight(val_bytes, lanes):
    return 4 if (val_bytes == 4 and lanes < 16) else 2


def source_constants():
    """The same constants from csrc/*, as text: a changed constant fails test_row_cases_cpu instead of moving an edge."""
    read = lambda f: open(os.path.join(CSRC, f)).read()
    common, xw, plan = read("common.hpp"), read("xwindow.hpp"), read("rows_plan.hip")
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    m = re.search(r"constexpr int rows_in_flight\(size_t val_bytes, int lanes_per_row\) \{ return \(val_bytes == 4 && "
                  r"lanes_per_row < (\d+)\) \? (\d+) : (\d+); \}", common)
    adapt = re.search(r"if \(mean <= (\d+)\) chunk_rows<BLOCK, (\d+), R, WINDOW, val_t>\(chunk_begin, chunk_end, nnz, Aj, Ax, x, y, "
                      r"stage, scr\);\s+else if \(mean <= (\d+)\) chunk_rows<BLOCK, (\d+), R, WINDOW, val_t>\(chunk_begin, chunk_end, "
                      r"nnz, Aj, Ax, x, y, stage, scr\);\s+else chunk_rows<BLOCK, (\d+), R,", xw[xw.index("if constexpr (REGULAR)"):].split("return;", 1)[1])
    return {
        "kWave": const(common, "kWave"), "kBlock": const(common, "kBlock"), "kWideBlock": const(common, "kWideBlock"),
        "kLongSteps": const(xw, "kLongSteps"), "kHugeRow": const(xw, "kHugeRow"), "kMaxChunkRows": const(xw, "kMaxChunkRows"),
        "kWindowBytes": (lambda m: int(m.group(1)) * int(m.group(2)))(re.search(r"constexpr int kWindowBytes = (\d+) \* (\d+);", xw)),
        "rows_in_flight": tuple(int(v) for v in m.groups()),
        "adapt": tuple(int(v) for v in adapt.groups()),
        "balanced_long_steps": int(re.search(r"return p\.balanced \? (\d+) : kLongSteps;", plan).group(1)),
        "giant_row_min": int(re.search(r"p\.giant_len = p\.knob\.giant_row >= (\d+) \? p\.knob\.giant_row : fair;", plan).group(1)),
    }


TYPES = {"f32-i32": (np.float32, np.int32), "f64-i64": (np.float64, np.int64), "f32-i64": (np.float32, np.int64)}
ALPHA_BETA = (2.0, -1.0)             # integers: exact on integer data

Geo = collections.namedtuple("Geo", "T block vb R VW WAVES STRIDE")


def geo(T, block, vb):
    R = rows_in_flight(vb, T)
    return Geo(T, block, vb, R, WAVE // T, block // WAVE, (block // T) * R)


# cols: "band" | "stencil"; planted: ((row, position in the row, column), ...); data: "signs" | "rowid"
Matrix = collections.namedtuple("Matrix", "name lens n_cols cols planted data")
# knobs: the environment the plan is created under; vb: bytes of a value; edge: the census states the case is there for
Case = collections.namedtuple("Case", "name family matrix knobs T block vb edge")

STENCIL_GAP = 8000


def n_cols_of(n_rows, cols):
    """37 columns (the stencil: two gaps and 120) beyond the rows: the last ones are referenced by planted entries only."""
    return n_rows + (2 * STENCIL_GAP + 120 if cols == "stencil" else 37)


def matrix(name, lens, cols="band", planted=(), data="signs"):
    lens = tuple(int(v) for v in lens)
    return Matrix(name, lens, n_cols_of(len(lens), cols), cols, tuple(planted), data)


@functools.lru_cache(maxsize=None)
def structure(m):
    """(Ap int64, Aj int32).  band: row r's columns lie in [r - HW, r + HW] clipped to [0, n_rows), sorted, and a row
    the planner probes shows both ends of that range (so the plan's band is exactly [-HW, HW] wherever the clip allows);
    stencil: three bands of half width 40 around row + 40, + STENCIL_GAP and + 2 STENCIL_GAP.  Then the planted columns, as they are."""
    n = len(m.lens)
    lens = np.asarray(m.lens, dtype=np.int64)
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    rng = np.random.default_rng([11, n, nnz])
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(nnz, dtype=np.int64) - Ap[row]
    if m.cols == "stencil":
        Aj = row + 40 + STENCIL_GAP * (pos % 3) + rng.integers(-40, 41, size=nnz)
    else:
        Aj = np.clip(row + rng.integers(-HW, HW + 1, size=nnz), 0, max(n - 1, 0))
    order = np.lexsort((Aj, row))
    Aj = Aj[order]
    if m.cols == "band" and n > 0:
        p = probed_rows(n)
        p = p[lens[p] >= 2]
        Aj[Ap[p]] = np.maximum(p - HW, 0)
        Aj[Ap[p + 1] - 1] = np.minimum(p + HW, n - 1)
    for r, k, c in m.planted:
        assert 0 <= k < lens[r] and 0 <= c < m.n_cols, (m.name, r, k, c)
        Aj[Ap[r] + k] = c
    return Ap, Aj.astype(np.int32)


@functools.lru_cache(maxsize=None)
def operands(m, vb, integer):
    """(Ax, x, y0) in the value type of vb bytes; x holds NaN where no row references it."""
    Ap, Aj = structure(m)
    return operands_of(Ap, Aj, m.n_cols, m.data, vb, integer)


def operands_of(Ap, Aj, n_cols, data, vb, integer):
    """operands() for any structure (tests/sweep_cases.py builds its own)."""
    t = np.float32 if vb == 4 else np.float64
    n_rows, nnz = len(Ap) - 1, int(Ap[-1])
    rng = np.random.default_rng([13, n_rows, nnz, int(integer)])
    if data == "rowid":              # x = 1, values 1 except a row's last: row r sums to r + 1, and no value is 0
        assert integer
        Ax = np.ones(nnz, dtype=t)
        r = np.nonzero(np.diff(Ap))[0]
        last = (r + 1) - (np.diff(Ap)[r] - 1)
        Ax[Ap[r + 1] - 1] = last
        z = r[last == 0]             # (r + 1 == len - 1, so len >= 2: first 2, last -1, the same sum)
        Ax[Ap[z]], Ax[Ap[z + 1] - 1] = 2, -1
        x = np.ones(n_cols, dtype=t)
    elif integer:
        Ax = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), size=nnz).astype(t)
        x = rng.choice(np.array([-2, -1, 1, 2]), size=n_cols).astype(t)
    else:
        lim = np.nextafter(t(1), t(0))
        Ax = np.clip((rng.random(nnz) * 2 - 1).astype(t), -lim, lim)
        x = np.clip((rng.random(n_cols) * 2 - 1).astype(t), -lim, lim)
        x[x == 0] = lim
    used = np.zeros(n_cols, dtype=bool)
    used[Aj] = True
    x[~used] = np.nan
    y0 = rng.integers(-4, 5, size=n_rows).astype(t)
    return Ax, x, y0


# ---- the plan a case must get -----------------------------------------------------------------------------------------
def knobs(T, block, rows, **more):
    k = {"MI355_SPMV_SMALL": "0", "MI355_SPMV_LANES": str(T), "MI355_SPMV_BLOCK": str(block),
         "MI355_SPMV_ROWS_PER_CHUNK": str(rows), "MI355_SPMV_BALANCE": "0"}
    for name, v in more.items():
        k["MI355_SPMV_" + name] = str(v)
    return k


KNOB_NAMES = tuple("MI355_SPMV_" + n for n in ("SMALL", "LANES", "BLOCK", "ROWS_PER_CHUNK", "BALANCE", "LONG_STEPS", "GIANT_ROW",
                                               "GIANT", "WINDOW", "WINDOW_FROM_BAND", "PACK", "SWEEP", "PLAIN", "SEGMENTS"))


def long_steps_of(c):
    ls = int(c.knobs.get("MI355_SPMV_LONG_STEPS", 0))
    return ls if ls > 0 else (BALANCED_LONG_STEPS if balanced(c) else K_LONG_STEPS)


def balanced(c):
    return c.knobs["MI355_SPMV_BALANCE"] == "1"


def window_kind(c):
    if c.knobs.get("MI355_SPMV_WINDOW") == "0":
        return "none"
    if c.matrix.cols == "stencil":
        return "segments"
    return "sampled" if c.knobs.get("MI355_SPMV_WINDOW_FROM_BAND") == "0" else "band"


def plan_of(c):
    """What info() / get_shape must report for the case's plan (rows_plan.hip: shape_for_block under the knobs,
    decide_balance's weight cut)."""
    g = geo(c.T, c.block, c.vb)
    n = len(c.matrix.lens)
    nnz = sum(c.matrix.lens)
    want = int(c.knobs["MI355_SPMV_ROWS_PER_CHUNK"])
    rpc = -(-want // g.STRIDE) * g.STRIDE
    assert g.STRIDE <= rpc <= K_MAX_CHUNK_ROWS, c.name
    out = {"lanes_per_row": c.T, "block_threads": c.block, "rows_per_chunk": rpc, "balanced_chunks": int(balanced(c)),
           "window": window_kind(c), "long_steps": int(c.knobs.get("MI355_SPMV_LONG_STEPS", 0))}
    if balanced(c):
        assert c.block == K_BLOCK
        r0 = max(4, min(rpc, K_MAX_CHUNK_ROWS // 2))
        k = max(1, -(-nnz // n))
        q = 2 * k * r0
        out.update(bal_k=k, bal_q=q, n_chunks=max(1, -(-(nnz + k * n) // q)), rows_cap=2 * r0 + 4)
    else:
        out.update(n_chunks=max(1, -(-n // rpc)), rows_cap=rpc)
    # the packed index: the vector kind's plan with ONE band-placed window and equal-row chunks, unless MI355_SPMV_PACK=0
    # pick_window_elems, one window placed from a band of 2 HW + 1 (a matrix of at least 2 HW rows shows the planner all of it)
    out["band_window_elems"] = min(K_WINDOW_BYTES // c.vb if c.block == K_BLOCK else 1 << 30, (2 * HW + 1 + out["rows_cap"] + 8 + 3) & ~3)
    out["packed"] = out["window"] == "band" and not balanced(c) and c.knobs.get("MI355_SPMV_PACK") != "0" and nnz >= 4
    return out


def chunk_bounds(c):
    """Row boundaries of the plan's chunks (chunk_table_kernel for weight-cut plans)."""
    p = plan_of(c)
    n = len(c.matrix.lens)
    if not balanced(c):
        return [min(i * p["rows_per_chunk"], n) for i in range(p["n_chunks"] + 1)]
    Ap = structure(c.matrix)[0]
    w = Ap + p["bal_k"] * np.arange(n + 1, dtype=np.int64)          # nondecreasing: first r with w[r] >= c Q
    b = [int(np.searchsorted(w, i * p["bal_q"], side="left")) & ~3 for i in range(p["n_chunks"])]
    return [min(v, n) for v in b] + [n]


def band_window(rb, re, n_cols, cap, vb, lo=-HW, hi=HW):
    """xwindow.hpp band_window / place_window (from_band): the window [start, start + len) of the chunk of rows [rb, re)."""
    per16 = 16 // vb
    clip = lambda v: 0 if v < 0 else (n_cols - 1 if v >= n_cols else v)
    l, h = clip(rb + lo), clip(re - 1 + hi)
    span = h - l + 1
    if cap <= 0 or span // 16 > cap:
        return 0, 0
    ln = min(span + per16 - 1, cap, n_cols)
    start = (l + h + 1 - ln) // 2
    if start + ln > n_cols:
        start = n_cols - ln
    start = max(start, 0) & ~(per16 - 1)
    if start + ln > n_cols:
        ln = n_cols - start
    return start, ln


# ---- the census --------------------------------------------------------------------------------------------------------
_census = {}


def census(c):
    """The edge states the case's rows are in, from Ap and the plan's geometry alone (computed once per case)."""
    key = (c.name, c.vb)
    if key not in _census:
        _census[key] = frozenset(_census_of(c))
    return _census[key]


BOUNDARY = ("band_lo", "band_lo-1", "band_hi", "band_hi+1", "window_first", "one_before_window", "window_last", "one_after_window")


def boundary_columns(rb, re, n_cols, cap, vb):
    """The columns on the two edges of the band of the chunk [rb, re) and of its staged window, by name."""
    w_lo, w_len = band_window(rb, re, n_cols, cap, vb)
    return dict(zip(BOUNDARY, (rb - HW, rb - HW - 1, re - 1 + HW, re + HW, w_lo, w_lo - 1, w_lo + w_len - 1, w_lo + w_len)))


def _census_of(c):
    g = geo(c.T, c.block, c.vb)
    Ap, Aj = structure(c.matrix)
    n, nnz = len(c.matrix.lens), int(Ap[-1])
    nnz_vec = nnz & ~3
    bounds = chunk_bounds(c)
    p = plan_of(c)
    giant_len = int(c.knobs.get("MI355_SPMV_GIANT_ROW", 0)) if balanced(c) else 0
    s = set()
    s.add("window_" + p["window"])
    s.add("T%d_R%d_b%d" % (g.T, g.R, g.block))
    if len(bounds) == 2:
        s.add("single_chunk")
        if n < g.STRIDE:
            s.add("below_one_group")
    else:
        last = bounds[-1] - bounds[-2]
        for name, v in (("1", 1), ("S-1", g.STRIDE - 1), ("S", g.STRIDE), ("S+1", g.STRIDE + 1)):
            if last == v:
                s.add("last_chunk=" + name)
    if nnz in (4, 5, 7, 8):
        s.add("nnz%d" % nnz)
    nonempty = np.nonzero(np.diff(Ap))[0]
    if nonempty.size and nonempty[-1] < n - 1:
        s.add("trailing_empty")
    planted = collections.defaultdict(list)
    for r, k, col in c.matrix.planted:
        planted[r].append((k, col))
    for ci in range(len(bounds) - 1):
        rb, re = bounds[ci], bounds[ci + 1]
        rows = re - rb
        if rows <= 0:
            continue
        T = g.T
        if balanced(c):
            mean = int(Ap[re] - Ap[rb]) // rows
            T = ADAPT_LANES[0] if mean <= ADAPT_MEANS[0] else (ADAPT_LANES[1] if mean <= ADAPT_MEANS[1] else ADAPT_LANES[2])
            s.add("adaptT%d" % T)
            if mean in (16, 17, 64, 65):
                s.add("mean%d" % mean)
        cg = Geo(T, g.block, c.vb, g.R, WAVE // T, g.WAVES, (g.block // T) * g.R)     # (a weight-cut plan keeps the plan's R)
        LONG = 4 * T * long_steps_of(c)
        n_groups = -(-rows // cg.STRIDE)
        s.add("groups%s" % (n_groups if n_groups <= 4 else "5+"))
        lens = np.diff(Ap[rb:re + 1])
        # slots: slot r of vector v of wave w of group gi is local row gi * STRIDE + w * VW * R + r * VW + v
        local = np.arange(n_groups * cg.STRIDE)
        empty = np.ones(local.size, dtype=bool)
        empty[:rows] = lens == 0
        real = local < rows
        by_group = empty.reshape(n_groups, cg.STRIDE)
        if (by_group & real.reshape(n_groups, cg.STRIDE)).all(axis=1).any():
            s.add("empty_group")
        vec = empty.reshape(n_groups, g.block // WAVE, g.R, cg.VW) & real.reshape(n_groups, g.block // WAVE, g.R, cg.VW)
        if vec.all(axis=2).any():
            s.add("empty_vector")
        if window_kind(c) == "band":
            # the plan's window: what the band and a chunk's rows need (pick_window_elems), never the whole budget here
            w_lo, w_len = band_window(rb, re, c.matrix.n_cols, p["band_window_elems"], c.vb)
            named = collections.defaultdict(list)             # (the band's upper edge may be the column behind the window)
            for k, v in boundary_columns(rb, re, c.matrix.n_cols, p["band_window_elems"], c.vb).items():
                named[v].append(k)
        wave_rows, huge_rows = 0, 0
        # one visit per row that is deferred, meets the partial group or holds a planted column; the ordinary rows that
        # are left are told apart by (length, phase) alone, so one of each is visited
        lo_all, hi_all = Ap[rb:re], Ap[rb + 1:re + 1]
        own = (lens > LONG) | (hi_all > nnz_vec) | np.isin(np.arange(rb, re), list(planted))
        if giant_len:
            own |= lens > giant_len
        visit = [(int(l), int(lo_all[l]), int(hi_all[l]), nnz_vec) for l in np.nonzero(own)[0]]
        pairs = np.unique(np.stack([lens[~own], lo_all[~own] & 3], axis=1), axis=0) if (~own).any() else ()
        visit += [(-1, int(ph), int(ph + ln_), 1 << 62) for ln_, ph in pairs]
        for l, lo, hi, nnz_vec_ in visit:
            r = rb + l
            ln = hi - lo
            phase = lo & 3
            if ln > LONG or (giant_len and ln > giant_len):
                if giant_len and ln > giant_len:
                    which = "giant"
                    s.add("giant")
                elif ln > K_HUGE_ROW:
                    which = "huge"
                    huge_rows += 1
                    s.add("huge")
                    hi_v = min(hi, nnz_vec)
                    it = -(-(hi_v - (lo & ~3)) // (2 * g.R * g.block * 4))
                    s.add("slabs%s" % (it if it <= 2 else "3+"))
                    if giant_len and ln in (giant_len, giant_len - 1):
                        s.add("below_giant")
                else:
                    which = "wave"
                    wave_rows += 1
                    s.add("wave_pass")
                    s.add("wave_phase%d" % phase)
                    s.add("word%d" % min(l >> 5, 1))
                    if l in (0, 31, 32):
                        s.add("bit%d" % l)
                    for k in (1, 2, 3):
                        for d in (-1, 0, 1):
                            if ln == WAVE * 4 * k + d:
                                s.add("wave256k%d%+d" % (k, d))
            else:
                which = "ordinary"
                if ln == 0:
                    s.add("empty")
                else:
                    hi_c = min(hi, nnz_vec_)
                    steps = max(1, -(-(hi_c - (lo & ~3)) // (4 * T)))
                    s.add("step%s" % (steps if steps <= 3 else "4+"))
                    s.add("phase%d" % phase)
                    if ln <= 4:
                        s.add("len%d@phase%d" % (ln, phase))
                    if ln <= 4 * T and steps == 2:
                        s.add("second_step_by_phase")
                    for k in (0, 1, 2):
                        for d in (-1, 0, 1):
                            if ln == 4 * T * k + d:
                                s.add("k%dd%+d@phase%d" % (k, d, phase))
            for name, v in (("long-1", LONG - 1), ("long", LONG), ("long+1", LONG + 1), ("len=kHuge", K_HUGE_ROW), ("len=kHuge+1", K_HUGE_ROW + 1)):
                if ln == v:
                    s.add(name)
            if ln > 0 and hi > nnz_vec_:
                s.add("tail%d_%s" % (nnz & 3, which))
                if lo >= nnz_vec_:
                    s.add("starts_at_nnz_vec+%d" % (lo - nnz_vec_))
            for k, col in planted.get(r, ()) if l >= 0 else ():
                if col == 0:
                    s.add("col0")
                if col == c.matrix.n_cols - 1:
                    s.add("col_last")
                if window_kind(c) == "band":
                    where = which if which != "ordinary" else ("step0" if (lo + k) - (lo & ~3) < 4 * T else "later_step")
                    inside = w_lo <= col < w_lo + w_len
                    if not inside:
                        s.add("escape_" + where)
                        s.add("escape_low" if col < w_lo else "escape_high")
                    # a column on an edge of the band or of the window, by its name; the window's own first and last
                    # column count only inside it, their neighbours only outside
                    for name in named.get(col, ()):
                        if inside == {"window_first": True, "window_last": True, "one_before_window": False,
                                      "one_after_window": False}.get(name, inside):
                            s.add("%s@%s" % (name, where))
        for name, v in (("1", 1), ("W", cg.WAVES), ("W+1", cg.WAVES + 1), ("2W+1", 2 * cg.WAVES + 1)):
            if wave_rows == v:
                s.add("marked=" + name)
        if huge_rows >= 2:
            s.add("two_huge_in_chunk")
        if huge_rows and wave_rows:
            s.add("huge_and_wave_in_chunk")
    return s


# ---- structures --------------------------------------------------------------------------------------------------------
def at_phase(lens, phase):
    """lens with its last row (a filler of 5..8) changed so that the NEXT row starts at `phase`."""
    assert 5 <= lens[-1] <= 8
    total = sum(lens) - lens[-1]
    lens[-1] = 5 + (phase - total - 5) % 4
    return lens


def probes(lengths, filler=6):
    """filler, probe, filler, probe ...: every probe length at every start phase 0..3, between fillers of 5..8."""
    lens = []
    for L in lengths:
        for phase in range(4):
            lens.append(filler)
            at_phase(lens, phase)
            lens.append(L)
    return lens


def steps_matrix(g):
    T = g.T
    lengths = sorted({4 * T * k + d for k in (0, 1, 2) for d in (-1, 0, 1) if 4 * T * k + d > 0} | {1, 2, 3, 4})
    lens = probes(lengths)
    lens += [0, 7, 0, 0, 5]                                      # empty rows singly and in pairs
    lens += [0] * (2 * g.STRIDE) + [6, 9, 1]                     # a run that covers a whole group, hence every slot of a vector
    return matrix("steps_T%d_R%d_b%d" % (T, g.R, g.block), lens)


def chunked(rpc, chunks, filler=3):
    """Chunks of rpc rows of `filler` nonzeros; chunks[i] = {local row: length, or (length, phase)} overrides.  A phase
    is reached by changing the row in front (the previous chunk's last row for local row 0; chunk 0 starts at phase 0)."""
    lens = []
    for ch in chunks:
        base = len(lens)
        lens += [filler] * rpc
        for l in sorted(ch):
            v = ch[l]
            if isinstance(v, tuple):
                v, phase = v
                i = base + l
                if i == 0:
                    assert phase == 0
                else:
                    assert l - 1 not in ch, "the row in front is an override too"
                    lens[i - 1] = 1 + (phase - sum(lens[:i - 1]) - 1) % 4
            lens[base + l] = v
    return lens


def long_matrix(g, ls):
    """Chunks of 1, W, W + 1 and 2 W + 1 marked rows; marked rows at bits 0, 31, 32 of the bitmap; LONG - 1, LONG, LONG + 1
    and 256 k + d at every phase."""
    rpc = -(-64 // g.STRIDE) * g.STRIDE
    LONG = 4 * g.T * ls
    W = g.WAVES
    m = lambda i: LONG + 1 + (i % 3)                               # marked, a different length each
    spread = lambda cnt: {2 + 2 * i: m(i) for i in range(cnt)}     # local rows 2, 4, ...: word 0 and, from 32 on, word 1
    chunks = [{5: m(0)}, spread(W), spread(W + 1), spread(2 * W + 1), {0: m(0), 31: m(1), 32: m(2)}]
    edge = [v for v in (LONG - 1, LONG, LONG + 1) if v > 0]
    edge += [WAVE * 4 * k + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    for i in range(0, len(edge), 4):                               # four lengths per chunk, each at the four phases
        chunks.append({2 + 4 * (4 * j + ph): (v, ph) for j, v in enumerate(edge[i:i + 4]) for ph in range(4)})
    return matrix("long_T%d_R%d_b%d_ls%d" % (g.T, g.R, g.block, ls), chunked(rpc, chunks))


def huge_matrix(g):
    rpc = -(-64 // g.STRIDE) * g.STRIDE
    slab = g.block * 4 * g.R
    chunks = [{4: (K_HUGE_ROW, 1)}, {9: (K_HUGE_ROW + 1, 2)}, {0: slab}, {7: (2 * slab - 1, 1)}, {7: (2 * slab + 1, 1)},
              {11: (4 * slab + 5, 2)},
              {3: (K_HUGE_ROW + 7, 1), 40: (K_HUGE_ROW + 30, 3)},                              # two huge rows in one chunk
              {2: 4 * g.T + 2, 20: (K_HUGE_ROW + 3, 2), 33: 4 * g.T + 9, 50: 700}]             # a huge row among wave-pass rows
    return matrix("huge_T%d_R%d_b%d" % (g.T, g.R, g.block), chunked(rpc, chunks))


def tail_matrices(g):
    """nnz % 4 in 1..3 with the last row ordinary, long (wave pass) or huge; the last row wholly inside the partial group;
    trailing empty rows; nnz = 4, 5, 7, 8.  (LONG_STEPS = 1: a row beyond 4 T nonzeros is long.)"""
    out = []
    body = [5, 0, 3, 8, 1, 6, 2, 7, 4, 9] * 3
    for r4 in (1, 2, 3):
        for which, base in (("ordinary", 1), ("long", 4 * g.T + 1), ("huge", K_HUGE_ROW + 1)):
            last = base + (r4 - sum(body) - base) % 4
            out.append(("tail%d_%s" % (r4, which), body + [last]))
            out.append(("tail%d_%s_then_empty" % (r4, which), body + [last, 0, 0, 0]))
    for start, ln in ((0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (2, 1)):   # the last row is [nnz_vec + start, + ln)
        lens = body + [7]
        lens[-1] += (start - sum(lens)) % 4                              # the row in front ends at nnz_vec + start
        out.append(("last_row_at_nnz_vec+%d_len%d" % (start, ln), lens + [ln, 0]))
    for nnz in (4, 5, 7, 8):
        out.append(("nnz_%d" % nnz, [1, 0, nnz - 1]))
    return [matrix("%s_T%d_R%d" % (n, g.T, g.R), l) for n, l in out]


def groups_matrices(g):
    """(matrix, rows per chunk wanted): chunks of 1..4 groups with a last chunk of 1, S - 1, S, S + 1 rows; one chunk;
    fewer rows than a group.  Row r sums to r + 1."""
    S = g.STRIDE
    out = []
    ln = lambda n: [1 + (3 * r) % 7 for r in range(n)]
    for n_groups in (1, 2, 3, 4):
        rpc = n_groups * S
        if rpc > K_MAX_CHUNK_ROWS:
            continue
        for name, last in (("1", 1), ("S-1", S - 1), ("S", S), ("S+1", S + 1)):
            if last > rpc or last < 1:
                continue
            out.append((matrix("groups%d_last%s_T%d_R%d" % (n_groups, name, g.T, g.R), ln(2 * rpc + last), data="rowid"), rpc))
    out.append((matrix("single_chunk_T%d_R%d" % (g.T, g.R), ln(2 * S - 5), data="rowid"), 2 * S))
    out.append((matrix("below_one_group_T%d_R%d" % (g.T, g.R), ln(max(S - 3, 1)), data="rowid"), S))
    return out


def window_matrix(g, cols):
    """A band (or a three-band stencil) of three chunks and 100 rows, rows of 9 with one of 3 x 4 T and one of 12 T + 40
    (long under LONG_STEPS = 3) per middle chunk.  Planted, in rows of the MIDDLE chunks that the planner does not probe:
    the two extremes of the chunk's band and the column one beyond each, the first and the last column of the window
    that band_window() stages for the chunk and the column just outside each (the window starts on a 16-byte boundary
    and is padded: its edges are not the band's), column 0 and column n_cols - 1 — each of them in step 0, in a later
    step and in a long row."""
    rpc = -(-512 // g.STRIDE) * g.STRIDE
    n = 3 * rpc + 100
    lens = [9] * n
    probed = set(int(v) for v in probed_rows(n))
    free = lambda r: next(v for v in range(r, r + 12) if v not in probed)
    planted = []
    n_cols = n_cols_of(n, cols)
    cap = min(K_WINDOW_BYTES // g.vb if g.block == K_BLOCK else 1 << 30, (2 * HW + 1 + rpc + 8 + 3) & ~3)
    for chunk in (1, 2):
        rb, re = chunk * rpc, (chunk + 1) * rpc
        b = boundary_columns(rb, re, n_cols_of(n, "band"), cap, g.vb)
        cols10 = [b[k] for k in BOUNDARY] + [0, n_cols - 1]
        assert all(0 < v < n_cols for v in cols10[:8])
        short = [free(rb + 10), free(rb + 30), free(rb + 50)]
        mid_steps, mid_long = free(rb + rpc // 2), free(rb + rpc // 2 + 40)
        assert len(set(short + [mid_steps, mid_long])) == 5
        lens[mid_long], lens[mid_steps] = 12 * g.T + 40, 12 * g.T
        for i, col in enumerate(cols10):                      # positions 0..3 of a row of 9: step 0 at every phase and T
            planted.append((short[i // 4], i % 4, col))
            planted.append((mid_steps, 4 * g.T + 4 + i, col))
            planted.append((mid_long, 10 + i, col))
    return matrix("window_%s_T%d_R%d_b%d_f%d" % (cols, g.T, g.R, g.block, 8 * g.vb), lens, cols=cols, planted=planted)


def adapt_matrix():
    """Segments of equal rows of 3, 16, 17, 40, 64, 65 and 100 nonzeros, each a few weight-cut chunks long, so that whole
    chunks have exactly those means; rows of LONG - 1, LONG, LONG + 1 (4 steps of the chunk's own T) inside the 3-, 40-
    and 100-segments."""
    lens = []
    for m, rows, T in ((3, 700, 2), (16, 420, None), (17, 420, None), (40, 330, 8), (64, 260, None), (65, 260, None), (100, 220, 32)):
        seg = [m] * rows
        if T:
            LONG = 4 * T * BALANCED_LONG_STEPS
            for i, v in enumerate((LONG - 1, LONG, LONG + 1)):
                seg[rows // 2 + 5 * i] = v
        lens += seg
    return matrix("adapt_means", lens)


def giant_matrix():
    lens = [8] * 600
    lens[300:303] = [GIANT_ROW - 1, GIANT_ROW + 1, GIANT_ROW]
    return matrix("adapt_giant", lens)


# ---- the table ---------------------------------------------------------------------------------------------------------
FAMILIES = ("steps", "long", "huge", "tail", "groups", "window", "adapt")
REAL_FAMILIES = ("steps", "long", "huge", "tail", "adapt")
HALF_FAMILIES = ("steps", "long", "tail")        # 16-bit matrix values: the plans that stay chunked (half_matrix_chunked)
ALPHA_BETA_CASES = {"steps": "steps_T8_R4_b256", "long": "long_T8_R4_b256_ls1", "huge": "huge_T16_R2_b256",
                    "tail": "tail3_long_then_empty_T8_R4", "groups": "groups2_lastS+1_T8_R4",
                    "window": "window_band_T8_R4_b256_f32", "adapt": "adapt_means"}      # (their f32-i32 members)
FAMILY_TYPES = {f: ("f32-i32", "f64-i64") + (("f32-i64",) if f in ("steps", "tail") else ()) for f in FAMILIES}
FAMILY_LANES = {"steps": LANES, "long": LANES, "huge": (2, 16, 64), "tail": (2, 8, 64), "groups": LANES, "window": LANES,
                "adapt": (8,)}       # (adapt: the kernel takes T per chunk, 2 / 8 / 32; the plan's own T is not used)


def _case(name, family, m, k, T, block, vb, edge):
    return Case(name, family, m, k, T, block, vb, tuple(edge))


@functools.lru_cache(maxsize=None)
def family(fam, T, vb):
    """The cases of one family at one T and value size (the offset width does not change the structure)."""
    out = []
    if fam == "steps":
        g = geo(T, K_BLOCK, vb)
        m = steps_matrix(g)
        edge = ["step1", "step2", "step3", "empty", "empty_group", "empty_vector", "second_step_by_phase"]
        edge += ["phase%d" % p for p in range(4)] + ["len%d@phase%d" % (l, p) for l in (1, 2, 3, 4) for p in range(4)]
        edge += ["k%dd%+d@phase%d" % (k, d, p) for k in (0, 1, 2) for d in (-1, 0, 1) for p in range(4) if 4 * T * k + d > 0]
        out.append(_case(m.name, fam, m, knobs(T, K_BLOCK, 1), T, K_BLOCK, vb, edge))
    elif fam == "long":
        for block in (K_BLOCK, K_WIDE_BLOCK):
            g = geo(T, block, vb)
            for ls in (1, 2, 0):
                if ls == 0 and (T > 8 or block != K_BLOCK):          # the default of 16 steps where it is still small
                    continue
                m = long_matrix(g, ls or K_LONG_STEPS)
                LONG = 4 * T * (ls or K_LONG_STEPS)
                edge = ["long-1", "long", "long+1", "wave_pass", "marked=1", "marked=W", "marked=W+1", "marked=2W+1",
                        "word0", "word1", "bit0", "bit31", "bit32"] + ["wave_phase%d" % p for p in range(4)]
                edge += ["wave256k%d%+d" % (k, d) for k in (1, 2, 3) for d in (-1, 0, 1) if K_HUGE_ROW >= WAVE * 4 * k + d > LONG]
                more = {"LONG_STEPS": ls} if ls else {}
                out.append(_case(m.name + ("" if ls else "_default"), fam, m, knobs(T, block, 64, **more), T, block, vb, edge))
    elif fam == "huge":
        for block in (K_BLOCK, K_WIDE_BLOCK):
            m = huge_matrix(geo(T, block, vb))
            edge = ["huge", "len=kHuge", "len=kHuge+1", "slabs1", "slabs2", "slabs3+", "two_huge_in_chunk", "huge_and_wave_in_chunk"]
            out.append(_case(m.name, fam, m, knobs(T, block, 64, LONG_STEPS=1), T, block, vb, edge))
    elif fam == "tail":
        g = geo(T, K_BLOCK, vb)
        for m in tail_matrices(g):
            n = m.name
            if n.startswith("tail"):
                which = {"ordinary": "ordinary", "long": "wave", "huge": "huge"}[n.split("_")[1]]
                edge = ["tail%s_%s" % (n[4], which)] + (["trailing_empty"] if "then_empty" in n else [])
            elif n.startswith("last_row"):
                edge = ["starts_at_nnz_vec+%s" % n[len("last_row_at_nnz_vec+")], "trailing_empty"]
            else:
                edge = ["nnz%s" % n.split("_")[1], "single_chunk", "below_one_group"]
            out.append(_case(n, fam, m, knobs(T, K_BLOCK, 1, LONG_STEPS=1), T, K_BLOCK, vb, edge))
    elif fam == "groups":
        g = geo(T, K_BLOCK, vb)
        for m, rpc in groups_matrices(g):
            n = m.name
            if n.startswith("groups"):
                edge = ["groups%s" % n[6], "last_chunk=%s" % n.split("_")[1][4:]]
            else:
                edge = ["single_chunk"] + (["below_one_group"] if n.startswith("below") else ["groups2"])
            out.append(_case(n, fam, m, knobs(T, K_BLOCK, rpc), T, K_BLOCK, vb, edge))
    elif fam == "window":
        band, wide = window_matrix(geo(T, K_BLOCK, vb), "band"), window_matrix(geo(T, K_WIDE_BLOCK, vb), "band")
        stencil = window_matrix(geo(T, K_BLOCK, vb), "stencil")
        esc = ["escape_step0", "escape_later_step", "escape_wave", "escape_low", "escape_high", "col0", "col_last"]
        esc += ["%s@%s" % (b, w) for b in BOUNDARY for w in ("step0", "later_step", "wave")]
        for tag, m, block, more, edge in (
                ("", band, K_BLOCK, {}, ["window_band"] + esc),
                ("", wide, K_WIDE_BLOCK, {}, ["window_band"] + esc),
                ("_unpacked", band, K_BLOCK, {"PACK": 0}, ["window_band"] + esc),
                ("_sampled", band, K_BLOCK, {"WINDOW_FROM_BAND": 0}, ["window_sampled", "col0", "col_last"]),
                ("_none", band, K_BLOCK, {"WINDOW": 0}, ["window_none", "col0", "col_last"]),
                ("", stencil, K_BLOCK, {}, ["window_segments", "col0", "col_last"])):
            out.append(_case(m.name + tag, fam, m, knobs(T, block, 512, LONG_STEPS=3, **more), T, block, vb, edge))
    elif fam == "adapt":
        m = adapt_matrix()
        edge = ["adaptT2", "adaptT8", "adaptT32", "mean16", "mean17", "mean64", "mean65", "long-1", "long", "long+1", "wave_pass"]
        k = knobs(T, K_BLOCK, 128)
        k["MI355_SPMV_BALANCE"] = "1"
        out.append(_case(m.name, fam, m, k, T, K_BLOCK, vb, edge))
        m = giant_matrix()
        k = dict(k, MI355_SPMV_GIANT_ROW=str(GIANT_ROW))
        out.append(_case(m.name, fam, m, k, T, K_BLOCK, vb, ["giant", "below_giant", "huge"]))
    else:
        raise KeyError(fam)
    return tuple(out)


def table(vb=None):
    """Every case; vb = 4 | 8 narrows to one value size."""
    out = []
    for fam in FAMILIES:
        for T in FAMILY_LANES[fam]:
            for b in ((4, 8) if vb is None else (vb,)):
                out += family(fam, T, b)
    return out


def states():
    """{state: the T it must be reached at} — what the census over the whole table must find."""
    want = collections.defaultdict(set)
    for c in table():
        for e in c.edge:
            want[e].add(c.T)
    return want
