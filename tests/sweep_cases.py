"""The table of chunk_rows_sweep cases (csrc/xwindow.hpp: the chunk body of csr_vector_sweep_kernel and
light_rows_sweep_kernel, taken when the band of a matrix is wider than one CU's LDS) that tests/test_gpu_sweep_edges.py
executes on the device and whose reach tests/test_sweep_cases_cpu.py proves on the host.

No planner.  A sweep plan of the planner's needs 512 chunks; but mi355_spmv_plan_create_block does not SHAPE a vector or
light block, it copies a mi355_spmv_plan_shape (rows_plan.hip, inherit_rows_shape), which the header documents as plain
data.  So a case writes its shape by hand — sweep_shape(): window_sweep = 1, 1 024 threads, T lanes per row, `held` rows
per vector, a window of `rounds` rounds of the workgroup's 16-byte groups, the band it likes — and creates a "block" that
starts at row 0 and element 0 and is the whole of a small matrix.  check_shape() asserts, on the host, every condition
launch_rows_sweep (row_launch.hpp) and chunk_lds_bytes rely on: a typo in a case fails here and never reaches the device.

Geometry.  A chunk is ONE group of rows_per_chunk = (1024 / T) * held rows: slot r of vector v of wave w is local row
w * (64 / T) * held + r * (64 / T) + v.  Every lane loads one group of four elements of the row's first step (4 T elements
from lo & ~3) into registers; the chunk's band [chunk_begin + band_lo, chunk_end - 1 + band_hi], clipped to x, rounded
down to a 16-byte group at its start (c_lo) and cut at the last whole group of x at its end (c_hi), is staged in windows
of `cap` columns, and a register slot is added in the pass whose window holds its column.  Columns outside [c_lo, c_hi]
are gathered afterwards, later steps are plain gathers, elements from nnz & ~3 on are added by scalar code.  census()
restates this DECOMPOSITION only — it never computes a y; expected values come from the serial oracle alone.

Data: row_cases' (operands_of) — integers without zeros, exact in any order; "rowid" (row r sums to r + 1); reals in
(-1, 1) for the parity bound; NaN in the columns of x that no row references.

Not here: merge's sweeping runs (merge_rows_kernel with TS > 0).  Merge blocks are shaped on their own, so a hand-written
shape does not reach them; they keep their at-size tests in tests/test_gpu_parity.py and tests/test_gpu_merge_fallbacks.py."""
import collections
import functools
import math
import os
import re

import numpy as np

import row_cases as rc

CSRC = rc.CSRC

# the literals the table was written with; source_constants() reads the same from the product's text
WAVE = 64
K_HUGE_BLOCK = 1024                  # threads of a sweeping workgroup
K_SWEEP_ROWS = 4                     # rows a vector holds at least
SWEEP_ROWS_WIDE = 8                  # ... and in fp32 while (1024 / T) * 8 <= SWEEP_ROWS_WIDE_MAX, i.e. T >= 4
SWEEP_ROWS_WIDE_MAX = 2048
SWEEP_LDS_BYTES = 155 * 1024         # sweep_window_cap: what a workgroup may take of the CU's LDS
ROUND_BYTES = K_HUGE_BLOCK * 16      # one round of the workgroup's 16-byte groups
LANES = rc.LANES
TYPES = rc.TYPES
KINDS = {"vector": 0, "light": 2}    # MI355_KIND_*
OFF_TYPE = {np.int32: 0, np.int64: 1}
VAL_TYPE = {np.float32: 0, np.float64: 1}
KERNEL = {"vector": "csr_vector_sweep_kernel", "light": "light_rows_sweep_kernel"}
LIGHT_STATIC_CHUNKS = 2 * 256        # set_rows_launch: one dequeue per workgroup beyond 2 * light_resident = 2 kCus chunks
SHAPE_BYTES = 208                    # sizeof(mi355_spmv_plan_shape)
ALPHA_BETA = rc.ALPHA_BETA


def source_constants():
    """The same constants from csrc/*, as text: a changed constant fails test_sweep_cases_cpu instead of moving an edge."""
    read = lambda f: open(os.path.join(CSRC, f)).read()
    common, launch, plan = read("common.hpp"), read("row_launch.hpp"), read("rows_plan.hip")
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    rows_for = re.search(r"inline int sweep_rows_for\(int val_type, int lanes_per_row\) \{\s+return \(val_type == MI355_VAL_F32 && "
                         r"\(kHugeBlock / lanes_per_row\) \* (\d+) <= (\d+)\) \? (\d+) : kSweepRows;", common)
    cap = re.search(r"inline int64_t sweep_window_cap\(int64_t val_bytes, int64_t fixed_bytes\) \{\s+const int64_t round = "
                    r"int64_t\(kHugeBlock\) \* (\d+);\s+const int64_t rounds = \((\d+) \* (\d+) - fixed_bytes\) / round;\s+"
                    r"return rounds > 0 \? rounds \* round / val_bytes : 0;", common)
    one_round = re.search(r"p\.window_elems < int\(kHugeBlock \* (\d+) / sizeof\(val_t\)\)", launch)
    resident = re.search(r"static int64_t light_resident\(const Plan& p\) \{\s+if \(p\.sweep\) return kCus;", plan)
    return {
        "kWave": const(common, "kWave"), "kHugeBlock": const(common, "kHugeBlock"), "kSweepRows": const(common, "kSweepRows"),
        "kCus": const(common, "kCus"),
        "sweep_rows_for": tuple(int(v) for v in rows_for.groups()),
        "round_bytes_per_thread": int(cap.group(1)), "lds_bytes": int(cap.group(2)) * int(cap.group(3)),
        "one_round_bytes_per_thread": int(one_round.group(1)),
        "light_resident_is_kCus": resident is not None,
    }


def lds_align16(v):
    return (v + 15) & ~15


def chunk_lds_bytes(window_elems, rows, vb):
    """xwindow.hpp chunk_lds_bytes: window | bounds | results | long-row flags."""
    return lds_align16(window_elems * vb) + lds_align16((rows + 1) * 4) + lds_align16(rows * vb) + lds_align16((rows // 32 + 1) * 4)


def sweep_window_cap(vb, fixed_bytes):
    """common.hpp sweep_window_cap: the elements of the widest window, whole rounds."""
    rounds = (SWEEP_LDS_BYTES - fixed_bytes) // ROUND_BYTES
    return rounds * ROUND_BYTES // vb if rounds > 0 else 0


def sweep_rows_for(vb, T):
    """common.hpp sweep_rows_for: the rows per vector the PLANNER takes."""
    return SWEEP_ROWS_WIDE if (vb == 4 and (K_HUGE_BLOCK // T) * SWEEP_ROWS_WIDE <= SWEEP_ROWS_WIDE_MAX) else K_SWEEP_ROWS


def helds(vb, T):
    """The rows per vector launch_rows_sweep accepts."""
    return (K_SWEEP_ROWS, SWEEP_ROWS_WIDE) if (vb == 4 and T >= 4) else (K_SWEEP_ROWS,)


def check_shape(f):
    """Every condition launch_rows_sweep, chunk_lds_bytes and the kernels rely on, from the field values alone."""
    vb = {0: 4, 1: 8}[f["val_type"]]
    T = f["lanes_per_row"]
    assert f["struct_bytes"] == SHAPE_BYTES and f["kind"] in KINDS.values() and f["off_type"] in (0, 1), f
    assert f["window_sweep"] == 1 and f["small_plain"] == 0 and f["balanced_chunks"] == 0 and f["giant_rows_enabled"] == 0, f
    assert f["block_threads"] == K_HUGE_BLOCK and f["elems_per_lane"] == 4 and f["window_from_band"] == 1, f
    assert T in LANES, f
    vectors = K_HUGE_BLOCK // T
    held = f["rows_per_chunk"] // vectors
    assert f["rows_per_chunk"] == vectors * held, ("rows_per_chunk is not (1024 / T) * held", f)
    assert held == K_SWEEP_ROWS or (vb == 4 and held == SWEEP_ROWS_WIDE and T >= 4), ("held", held, f)
    assert f["rows_cap"] >= f["rows_per_chunk"], ("rows_cap < rows_per_chunk", f)
    round_elems = ROUND_BYTES // vb
    assert f["window_elems"] >= round_elems, ("window below one round", f)
    assert f["window_elems"] % round_elems == 0 and f["window_bytes"] == f["window_elems"] * vb, ("window is not whole rounds", f)
    assert chunk_lds_bytes(f["window_elems"], f["rows_cap"], vb) <= SWEEP_LDS_BYTES, ("LDS beyond the sweep's share", f)
    assert f["window_elems"] <= sweep_window_cap(vb, chunk_lds_bytes(0, f["rows_per_chunk"], vb)), ("window beyond sweep_window_cap", f)
    assert f["n_rows"] >= 1 and f["n_cols"] >= 1 and f["nnz"] >= 4, f          # (nnz < 4: launch_rows takes the plain kernel)
    assert f["n_chunks"] == -(-f["n_rows"] // f["rows_per_chunk"]), f
    assert f["band_lo"] <= f["band_hi"] and f["window_segments"] == 1, f
    return f


def sweep_shape(kind, types, T, held, rounds, band, n_rows, n_cols, nnz):
    """The field values of a hand-written mi355_spmv_plan_shape of a sweep plan (dict, in the structure's field names)."""
    t_val, t_off = TYPES[types]
    vb = np.dtype(t_val).itemsize
    assert held in helds(vb, T), ("no sweep kernel holds %d rows at T = %d, %d-byte values" % (held, T, vb))
    assert isinstance(rounds, int) and rounds >= 1
    rpc = (K_HUGE_BLOCK // T) * held
    elems = rounds * ROUND_BYTES // vb
    f = dict(struct_bytes=SHAPE_BYTES, kind=KINDS[kind], off_type=OFF_TYPE[t_off], val_type=VAL_TYPE[t_val],
             n_rows=n_rows, n_cols=n_cols, nnz=nnz, lanes_per_row=T, elems_per_lane=4, block_threads=K_HUGE_BLOCK,
             balanced_chunks=0, rows_cap=rpc, giant_rows_enabled=0, rows_per_chunk=rpc, n_chunks=-(-n_rows // rpc),
             bal_k=0, bal_q=0, giant_len=0, window_elems=elems, window_bytes=elems * vb, window_from_band=1,
             window_segments=1, probe_ok=1, long_steps=0, band_lo=int(band[0]), band_hi=int(band[1]), window_sweep=1,
             small_plain=0)
    return check_shape(f)


# refusals launch_rows_sweep decides on the host before any launch (MI355_SPMV_EINVAL at execute); check_shape refuses each
def refused_shapes(types):
    vb = np.dtype(TYPES[types][0]).itemsize
    T = 8
    good = sweep_shape("vector", types, T, K_SWEEP_ROWS, 1, (-40, 5000), 700, 6000, 2100)
    rpc = good["rows_per_chunk"]
    out = [("rows_per_chunk_not_vectors_x_held", dict(good, rows_per_chunk=rpc + 4, rows_cap=rpc + 4, n_chunks=-(-700 // (rpc + 4)))),
           ("window_one_element_below_a_round", dict(good, window_elems=good["window_elems"] - 1, window_bytes=good["window_bytes"] - vb)),
           ("rows_cap_below_rows_per_chunk", dict(good, rows_cap=rpc - 1)),
           ("held8_at_T2", dict(good, lanes_per_row=2, rows_per_chunk=512 * 8, rows_cap=512 * 8, n_chunks=1))]
    if vb == 8:
        out.append(("held8_in_fp64", dict(good, rows_per_chunk=2 * rpc, rows_cap=2 * rpc, n_chunks=-(-700 // (2 * rpc)))))
    return out


# ---- matrices ----------------------------------------------------------------------------------------------------------
Geo = collections.namedtuple("Geo", "T held vb VW WAVES rpc P round_elems")


def geo(T, held, vb):
    return Geo(T, held, vb, WAVE // T, K_HUGE_BLOCK // WAVE, (K_HUGE_BLOCK // T) * held, 16 // vb, ROUND_BYTES // vb)


def local_row(g, wave, r, v):
    """row_of: slot r of vector v of wave `wave`."""
    return wave * (g.VW * g.held) + r * g.VW + v


# cols: "band" (random inside the chunk's band, sorted) | "unsorted"; planted: ((row, position in the row, column), ...)
Matrix = collections.namedtuple("Matrix", "name lens n_cols band rpc cols planted data")
# edge: the census states the case is there for
Case = collections.namedtuple("Case", "name family matrix T held vb rounds edge")


def matrix(name, lens, n_cols, band, rpc, cols="band", planted=(), data="signs"):
    return Matrix(name, tuple(int(v) for v in lens), int(n_cols), (int(band[0]), int(band[1])), rpc, cols, tuple(planted), data)


@functools.lru_cache(maxsize=None)
def structure(m):
    """(Ap int64, Aj int32): a row's columns lie in the band of its chunk, clipped to x (anywhere in x where that is
    empty), sorted; then the planted columns, as they are."""
    n = len(m.lens)
    lens = np.asarray(m.lens, dtype=np.int64)
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    rng = np.random.default_rng([17, n, nnz, m.n_cols])
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    rb = (row // m.rpc) * m.rpc
    re_ = np.minimum(rb + m.rpc, n)
    lo = np.maximum(rb + m.band[0], 0)
    hi = np.minimum(re_ - 1 + m.band[1], m.n_cols - 1)
    none = lo > hi
    lo[none], hi[none] = 0, m.n_cols - 1
    Aj = lo + (rng.random(nnz) * (hi - lo + 1)).astype(np.int64)
    if m.cols == "unsorted":
        Aj = Aj[np.lexsort((rng.random(nnz), row))]
    else:
        Aj = Aj[np.lexsort((Aj, row))]
    for r, k, c in m.planted:
        assert 0 <= k < lens[r], (m.name, r, k, c)
        Aj[Ap[r] + k] = c
    assert nnz == 0 or (0 <= Aj.min() and Aj.max() < m.n_cols), m.name
    return Ap, Aj.astype(np.int32)


@functools.lru_cache(maxsize=None)
def operands(m, vb, integer):
    """(Ax, x, y0) as row_cases makes them."""
    Ap, Aj = structure(m)
    return rc.operands_of(Ap, Aj, m.n_cols, m.data, vb, integer)


def chunk_sweep(rb, re_, band, n_cols, vb, cap):
    """chunk_rows_sweep's span of the chunk of rows [rb, re_): l, h, c_lo, c_hi, whole_end and the windows (w0, len)."""
    P = 16 // vb
    l = max(rb + band[0], 0)
    h = min(re_ - 1 + band[1], n_cols - 1)
    assert h >= 0
    whole_end = (n_cols & ~(P - 1)) - 1
    c_lo, c_hi = l & ~(P - 1), min(h, whole_end)
    passes = []
    w0 = c_lo
    while w0 <= c_hi:
        passes.append((w0, min(cap, c_hi + 1 - w0)))
        w0 += cap
    return dict(l=l, h=h, c_lo=c_lo, c_hi=c_hi, whole_end=whole_end, passes=passes)


def chunks_of(c):
    m = c.matrix
    n = len(m.lens)
    return [(rb, min(rb + m.rpc, n)) for rb in range(0, n, m.rpc)]


def cap_of(c):
    return c.rounds * ROUND_BYTES // c.vb


# ---- the census --------------------------------------------------------------------------------------------------------
REG, LATER, TAIL = 0, 1, 2
BELOW, ABOVE, BEYOND = -1, -2, -3    # `where` of a register slot that no pass holds (else: the index of its pass)


def decompose(c):
    """Per stored element k: chunk, wave, slot r, vector v, lane, step, e, kind (REG | LATER | TAIL) and, for register
    slots, `where` (the pass whose window holds the column, or BELOW c_lo / ABOVE c_hi / BEYOND the whole groups of x)."""
    g = geo(c.T, c.held, c.vb)
    m = c.matrix
    Ap, Aj = structure(m)
    n, nnz = len(m.lens), int(Ap[-1])
    k = np.arange(nnz, dtype=np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    chunk, local = row // g.rpc, row % g.rpc
    wave, in_wave = local // (g.VW * g.held), local % (g.VW * g.held)
    r, v = in_wave // g.VW, in_wave % g.VW
    off = k - (Ap[row] & ~3)
    step, lane, e = off // (4 * g.T), (off % (4 * g.T)) // 4, off % 4
    nnz_vec = nnz & ~3
    kind = np.where(k >= nnz_vec, TAIL, np.where(step == 0, REG, LATER))
    cap = cap_of(c)
    where = np.zeros(nnz, dtype=np.int64)
    spans = []
    for ci, (rb, re_) in enumerate(chunks_of(c)):
        s = chunk_sweep(rb, re_, m.band, m.n_cols, c.vb, cap)
        spans.append(s)
        sl = slice(int(Ap[rb]), int(Ap[re_]))
        col = Aj[sl].astype(np.int64)
        w = (col - s["c_lo"]) // cap
        w = np.where(col > s["c_hi"], np.where(col > s["whole_end"], BEYOND, ABOVE), w)
        w = np.where(col < s["c_lo"], BELOW, w)
        where[sl] = w
    return dict(row=row, chunk=chunk, local=local, wave=wave, r=r, v=v, lane=lane, step=step, e=e, kind=kind, where=where,
                col=Aj.astype(np.int64), spans=spans, nnz_vec=nnz_vec)


_census = {}


def census(c):
    key = (c.name, c.T, c.held, c.vb)
    if key not in _census:
        _census[key] = frozenset(_census_of(c))
    return _census[key]


EDGES = ("w0-1", "w0", "last", "last+1")


def _census_of(c):
    g = geo(c.T, c.held, c.vb)
    m = c.matrix
    Ap, Aj = structure(m)
    n, nnz = len(m.lens), int(Ap[-1])
    lens = np.diff(Ap)
    d = decompose(c)
    P = g.P
    cap = cap_of(c)
    s = {"T%d_held%d" % (g.T, g.held), "rounds%d" % c.rounds, "ncols%%P=%d" % (m.n_cols % P)}
    chunks = chunks_of(c)
    s.add("light_static" if len(chunks) <= LIGHT_STATIC_CHUNKS else "light_dequeue_once")
    if len(chunks) == 1:
        s.add("single_chunk")
    last_rows = chunks[-1][1] - chunks[-1][0]
    for name, val in (("1", 1), ("VW-1", g.VW - 1), ("VW", g.VW), ("rpc-1", g.rpc - 1), ("rpc", g.rpc)):
        if last_rows == val and val > 0 and len(chunks) > 1:
            s.add("last_chunk=" + name)
    if nnz in (4, 5, 6, 7):
        s.add("nnz%d" % nnz)
    if nnz & 3:
        s.add("nnz%%4=%d" % (nnz & 3))
    reg = d["kind"] == REG
    for kind, name in ((REG, "register_slot"), (LATER, "later_step"), (TAIL, "scalar_tail")):
        if (d["kind"] == kind).any():
            s.add(name)
    # ---- per chunk: the sweep's span and its windows
    for ci, ((rb, re_), sp) in enumerate(zip(chunks, d["spans"])):
        sl = slice(int(Ap[rb]), int(Ap[re_]))
        col, where, kind = d["col"][sl], d["where"][sl], d["kind"][sl]
        creg = kind == REG
        if not creg.any():
            continue
        npass = len(sp["passes"])
        s.add("passes%d" % npass)
        if npass == 0:
            s.add("empty_sweep")
            assert ((where == BELOW) | (where == ABOVE) | (where == BEYOND))[creg].all()
            continue
        if rb + m.band[0] < 0:
            s.add("clip0")
        s.add("l%%P=%d" % (sp["l"] % P))
        s.add("h%%P=%d" % (sp["h"] % P))
        if sp["h"] > sp["whole_end"]:
            s.add("h_past_whole_end")
        if sp["passes"][-1][1] < cap:
            s.add("partial_last_window")
        else:
            s.add("full_last_window")
        if (sp["c_hi"] + 1) % P:
            s.add("partial_last_group")
        for w0, ln in sp["passes"]:
            full = (min((w0 + ln + P - 1) & ~(P - 1), m.n_cols & ~(P - 1)) - w0) // P
            assert 0 < full <= c.rounds * K_HUGE_BLOCK and w0 % P == 0 and w0 + full * P <= m.n_cols
            s.add("dma_reload_last_group" if full < c.rounds * K_HUGE_BLOCK else "dma_full_window")
        named = collections.defaultdict(list)
        for p, (w0, ln) in enumerate(sp["passes"]):
            for name, v in zip(EDGES, (w0 - 1, w0, w0 + ln - 1, w0 + ln)):
                named[v].append("%s@p%d" % (name, p))
        for name, v in (("c_lo", sp["c_lo"]), ("c_lo-1", sp["c_lo"] - 1), ("l-1", sp["l"] - 1), ("l", sp["l"]), ("h", sp["h"]),
                        ("h+1", sp["h"] + 1), ("c_hi", sp["c_hi"]), ("c_hi+1", sp["c_hi"] + 1), ("whole_end", sp["whole_end"]),
                        ("whole_end+1", sp["whole_end"] + 1), ("col0", 0), ("col_last", m.n_cols - 1)):
            named[v].append(name)
        rcol, rwhere = col[creg], where[creg]
        for p in np.unique(rwhere):
            s.add({BELOW: "outside_below", ABOVE: "outside_above", BEYOND: "beyond_whole_groups"}.get(int(p), "pass%d" % p))
        for v in np.unique(rcol):
            for name in named.get(int(v), ()):
                s.add("col=" + name)
        if ((rcol >= sp["c_lo"]) & (rcol < sp["l"])).any():
            s.add("staged_below_band")
        out = creg & (where < 0) & (where != BEYOND)
        rr, ee = d["r"][sl], d["e"][sl]
        for w_, nm in ((BELOW, "below"), (ABOVE, "above")):
            sel = creg & (where == w_)
            for r_, e_ in set(zip(rr[sel].tolist(), ee[sel].tolist())):
                s.add("%s@r%de%d" % (nm, r_, e_))
        # rows wholly outside; lanes whose four slots are all outside next to a lane of the row with a slot inside
        rows_here = d["row"][sl]
        inside = creg & (where >= 0)
        for r_ in np.unique(rows_here[out]):
            sel = rows_here == r_
            if not (sel & inside).any() and (sel & creg).sum() == (sel).sum():
                s.add("row_all_outside")
            lanes = d["lane"][sl][sel & creg]
            o = out[sel & creg]
            for ln_ in np.unique(lanes):
                mine = lanes == ln_
                if mine.sum() == 4 and o[mine].all() and any((lanes == ln_ + dl).any() and not o[lanes == ln_ + dl].any() for dl in (-1, 1)):
                    s.add("lane_all_outside_neighbour_inside")
    # ---- per row
    lo_all, hi_all = Ap[:-1], Ap[1:]
    nnz_vec = d["nnz_vec"]
    phase = lo_all & 3
    local = np.arange(n) % g.rpc
    full_chunk = (np.arange(n) // g.rpc) < (n // g.rpc)
    steps = np.where(lens > 0, np.maximum(1, -(-(np.minimum(hi_all, nnz_vec) - (lo_all & ~3)) // (4 * g.T))), 0)
    for r_ in np.unique(np.concatenate([np.nonzero(lens == 0)[0][:64], np.unique(np.stack([lens, phase], 1), axis=0, return_index=True)[1],
                                        np.nonzero(hi_all > nnz_vec)[0]])):
        ln, ph = int(lens[r_]), int(phase[r_])
        if ln == 0:
            s.add("len0")
            continue
        st = int(steps[r_])
        s.add("steps%s" % (st if st <= 3 else "4+"))
        if ln <= 4 * g.T and st == 2:
            s.add("second_step_by_phase")
        if ln == 1:
            s.add("len1@phase%d" % ph)
        for k_ in (1, 2):
            for dd in (-1, 0, 1):
                if ln == 4 * g.T * k_ + dd and ln > 1:
                    s.add("k%dd%+d@phase%d" % (k_, dd, ph))
        if ln >= 1900:
            s.add("long_row")
    nonempty = lens > 0
    for w_, wn in ((0, "first"), (g.WAVES - 1, "last")):
        for v_, vn in ((0, "first"), (g.VW - 1, "last")):
            for r_, rn in ((0, "first"), (g.held - 1, "last")):
                at = local == local_row(g, w_, r_, v_)
                if (at & nonempty & full_chunk).any():
                    s.add("corner_wave_%s_vector_%s_slot_%s" % (wn, vn, rn))
    if (full_chunk & (local == g.rpc - 1) & ~nonempty).any():
        s.add("empty_at_chunk_end")
    if ((local == 0) & ~nonempty & (np.arange(n) > 0)).any():
        s.add("empty_at_chunk_start")
    if m.data == "rowid" and n >= 2 * g.rpc:
        s.add("rowid_full_chunk")
    if m.cols == "unsorted":
        for r_ in range(n):
            cc = Aj[Ap[r_]:Ap[r_ + 1]]
            if cc.size > 1 and (np.diff(cc) < 0).any():
                s.add("unsorted_row")
            if cc.size > 1 and np.unique(cc).size < cc.size:
                s.add("duplicate_in_row")
    # ---- the arrays' last, partial group
    r4 = nnz & 3
    if r4 and nonempty.any():
        last = int(np.nonzero(nonempty)[0][-1])
        lo, hi = int(Ap[last]), int(Ap[last + 1])
        if lo < nnz_vec:
            s.add("tail%d_row_crosses" % r4)
        else:
            s.add("tail%d_row_starts_at+%d" % (r4, lo - nnz_vec))
            if lo > nnz_vec:
                s.add("tail_row_starts_inside")
        if last < n - 1:
            s.add("tail%d_empty_behind" % r4)
        if len(chunks) > 1 and last >= chunks[-1][0]:
            s.add("tail_in_last_of_several_chunks")
    # lanes of the last chunk whose step-0 address is clamped to j_max (relative to the chunk's base)
    rb, re_ = chunks[-1]
    base = int(Ap[rb]) & ~3
    j_max = ((nnz - base) & ~3) - 4
    for r_ in range(rb, re_):
        lo, hi = int(Ap[r_]) - base, int(Ap[r_ + 1]) - base
        first = lo & ~3
        j = first + 4 * np.arange(g.T)
        jl = np.where(j < hi, j, first)
        if (jl > j_max).any():
            s.add("j_max_clamp")
            break
    return s


# ---- structures --------------------------------------------------------------------------------------------------------
def band_for(g, passes, rounds=1, lo=-40):
    """A band whose FIRST chunk (l clipped to 0 at lo <= 0) is swept in `passes` windows, the last one partial."""
    cap = rounds * g.round_elems
    return (lo, passes * cap - g.rpc - 5)


def window_row_len(g):
    return min(4 * g.T, 16)


def plant_columns(g, lens, rb, re_, cols, planted, start=0):
    """Plant `cols` in rows of the chunk [rb, re_) — one per row, rows and positions in turn, register slots of step 0 —
    that are at phase 0 and hold no plant yet."""
    taken = {(r, k) for r, k, _ in planted}
    rows_taken = {r for r, _, _ in planted}
    i = start
    total = 0
    Ap = np.concatenate([[0], np.cumsum(lens)])
    stride = next(v for v in (5, 7, 11, 13, 1) if math.gcd(v, re_ - rb) == 1)
    for col in cols:
        while True:
            r = rb + (stride * i + 1) % (re_ - rb)
            i += 1
            k = i % max(1, min(lens[r], 4 * g.T))
            if lens[r] > 0 and Ap[r] % 4 == 0 and r not in rows_taken and (r, k) not in taken:
                break
            total += 1
            assert total < 100000
        planted.append((r, k, col))
        rows_taken.add(r)
        taken.add((r, k))
    return i


def window_matrix(name, g, rounds, band, n_chunks_full, last_rows, n_cols, more_cols=lambda sp: ()):
    """Rows of one step at phase 0; in every chunk, on every window of its sweep: the column in front of it, its first,
    its last and the one behind it; and the named columns of the span (c_lo - 1 ... whole_end + 1, 0, n_cols - 1)."""
    n = n_chunks_full * g.rpc + last_rows
    lens = [window_row_len(g)] * n
    planted = []
    cap = rounds * g.round_elems
    for rb in range(0, n, g.rpc):
        re_ = min(rb + g.rpc, n)
        sp = chunk_sweep(rb, re_, band, n_cols, g.vb, cap)
        cols = []
        for w0, ln in sp["passes"]:
            cols += [w0 - 1, w0, w0 + ln - 1, w0 + ln]
        cols += [sp["c_lo"], sp["c_lo"] - 1, sp["l"] - 1, sp["l"], sp["h"], sp["h"] + 1, sp["c_hi"], sp["c_hi"] + 1, sp["whole_end"],
                 sp["whole_end"] + 1, 0, n_cols - 1]
        cols += list(more_cols(sp))
        cols = [v for v in dict.fromkeys(cols) if 0 <= v < n_cols]
        if len(cols) > re_ - rb:                  # a short chunk: the edges of its windows first
            cols = cols[:re_ - rb]
        plant_columns(g, lens, rb, re_, cols, planted)
    return matrix(name, lens, n_cols, band, g.rpc, planted=planted)


def at_phase(lens, phase):
    return rc.at_phase(lens, phase)


def rows_steps_matrix(g, band, n_cols):
    """Chunk 0: rows of 1, 4T - 1, 4T, 4T + 1, 8T, 8T + 1 at every phase, empty rows, one row of 2 000; chunk 1: full, a
    marked row (5 long among 3s) in the first and last slot of the first and last vector of the first and last wave, an
    empty row at its end and at the start of chunk 2; chunk 2: short."""
    T = g.T
    lengths = sorted({1, 4 * T - 1, 4 * T, 4 * T + 1, 8 * T, 8 * T + 1})
    lens = rc.probes(lengths) + [0, 7, 0, 0, 5, 2000, 6]
    assert len(lens) < g.rpc
    lens += [3] * (g.rpc - len(lens))
    second = [3] * g.rpc
    for w_ in (0, g.WAVES - 1):
        for v_ in (0, g.VW - 1):
            for r_ in (0, g.held - 1):
                second[local_row(g, w_, r_, v_)] = 5
    lens[g.rpc - 1] = 0
    lens += second + [0] + [3] * (g.rpc // 2 + 2)
    return matrix("rows_steps_T%d_h%d_f%d" % (T, g.held, 8 * g.vb), lens, n_cols, band, g.rpc)


def tail_matrices(g, band, n_cols):
    out = []
    body = [5, 0, 3, 8, 1, 6, 2, 7, 4, 9] * 3
    front = [4] * g.rpc                                                 # a full chunk in front: the tail in the last of two
    for r4 in (1, 2, 3):
        last = 5 + (r4 - sum(body) - 5) % 4
        out.append(("tail%d_crosses" % r4, front + body + [last]))
        out.append(("tail%d_crosses_single_chunk" % r4, body + [last]))
        out.append(("tail%d_then_empty" % r4, body + [last, 0, 0, 0]))
    for start, ln in ((0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (2, 1)):   # the last row is [nnz_vec + start, + ln)
        lens = body + [7]
        lens[-1] += (start - sum(lens)) % 4
        out.append(("last_row_at_nnz_vec+%d_len%d" % (start, ln), lens + [ln, 0]))
    for nnz in (4, 5, 6, 7):
        out.append(("nnz_%d" % nnz, [1, 0, nnz - 1]))
    return [matrix("%s_T%d_h%d_f%d" % (nm, g.T, g.held, 8 * g.vb), l, n_cols, band, g.rpc) for nm, l in out]


def blocks_matrix(g, band, n_cols):
    """Three full chunks and five rows; Ap at the chunk boundaries is 1, 2 and 3 mod 4 and the rows behind the last
    boundary lie in the arrays' last, partial group."""
    lens = []
    for i, ph in enumerate((1, 2, 3)):
        lens += [3] * g.rpc
        lens[-1] = 1 + (ph - (sum(lens) - lens[-1]) - 1) % 4
        assert sum(lens) % 4 == ph
    lens += [1, 0, 1, 0, 0]                                              # elements 4q + 3 (a whole group's last) and 4q + 4
    return matrix("blocks_T%d_h%d_f%d" % (g.T, g.held, 8 * g.vb), lens, n_cols, band, g.rpc)


BLOCK_CUTS = ((0, 1, 2, None), (0, 3, None))        # in chunks; None = the end: blocks at Ap % 4 = 1 and 2, and at 3 (in the tail)


# ---- the table ---------------------------------------------------------------------------------------------------------
FAMILIES = ("window", "outside", "rows", "tail", "blocks", "light")
REAL_FAMILIES = ("window", "rows", "tail")
FAMILY_LANES = {"window": (8, 64), "outside": LANES, "rows": LANES, "tail": (2, 8, 64), "blocks": (2, 16, 64), "light": (64,)}
FAMILY_TYPES = {f: ("f32-i32", "f64-i64", "f32-i64") for f in FAMILIES}
FAMILY_TYPES["light"] = ("f64-i64",)
ALPHA_BETA_CASES = {"window": "window_res1_T8_h4_f32", "outside": "outside_slots_T8_h4_f32", "rows": "rows_steps_T8_h4_f32",
                    "tail": "tail3_then_empty_T8_h4_f32", "blocks": "blocks_T16_h4_f32"}      # (their f32-i32 members)


def _case(name, family, m, g, rounds, edge):
    return Case(name, family, m, g.T, g.held, g.vb, rounds, tuple(edge))


@functools.lru_cache(maxsize=None)
def family(fam, T, vb):
    """The cases of one family at one T and value size, for every `held` the kernels have there."""
    out = []
    if fam == "light" and (T, vb) != (64, 8):
        return ()
    for held in helds(vb, T):
        g = geo(T, held, vb)
        P, rpc = g.P, g.rpc
        tag = "T%d_h%d_f%d" % (T, held, 8 * vb)
        if fam == "window":
            # every residue of l and h in a 16-byte group, n_cols % PER16 with it; chunk 0 clipped at column 0, chunk 1
            # inside x, the short chunk 2 reaching past the last whole group of x; three windows of one round
            for i in range(P):
                band = (-40 + i, 2 * g.round_elems + 101 + i)
                n_cols = ((2 * rpc + band[1] + 8) & ~3) + i
                m = window_matrix("window_res%d_%s" % (i, tag), g, 1, band, 2, rpc // 2 + 3, n_cols)
                edge = ["l%%P=%d" % i, "h%%P=%d" % i, "ncols%%P=%d" % i, "clip0", "partial_last_window",
                        "col=c_lo-1", "col=l", "col=h", "col=c_hi", "col=whole_end", "col=col0", "col=col_last", "outside_below",
                        "dma_reload_last_group", "dma_full_window", "rounds1", "passes3"]
                edge += ["col=%s@p%d" % (e, p) for e in EDGES for p in range(3)]
                if i:
                    edge += ["staged_below_band", "h_past_whole_end", "beyond_whole_groups", "col=whole_end+1", "col=l-1"]
                if (i + 1) % P:
                    edge += ["partial_last_group"]
                if i or P == 2:
                    edge += ["col=h+1"]
                out.append(_case(m.name, fam, m, g, 1, edge))
            for passes in (1, 2, 5, 16):
                band = band_for(g, passes)
                n = rpc + rpc // 4 + 1
                m = window_matrix("window_passes%d_%s" % (passes, tag), g, 1, band, 1, rpc // 4 + 1, n + band[1] + 12)
                edge = ["passes%d" % passes] + ["col=%s@p%d" % (e, p) for e in EDGES[1:] for p in range(passes)]
                out.append(_case(m.name, fam, m, g, 1, edge + ["pass%d" % (passes - 1), "partial_last_window"]))
            # a sweep that ends on the last column of a full window (len == cap in the last pass)
            band = (-40, 2 * g.round_elems - rpc)
            m = window_matrix("window_full_last_%s" % tag, g, 1, band, 1, 3, rpc + 3 + band[1] + 13)
            out.append(_case(m.name, fam, m, g, 1, ["full_last_window", "passes2", "dma_full_window"]))
            for rounds in (2, 9):                  # the DMA loop over u; 9: what the planner takes at these T
                band = band_for(g, 2, rounds)
                n = rpc + rpc // 4 + 1
                m = window_matrix("window_rounds%d_%s" % (rounds, tag), g, rounds, band, 1, rpc // 4 + 1, n + band[1] + 12 + (1 if rounds == 9 else 0))
                edge = ["rounds%d" % rounds, "passes2", "dma_reload_last_group", "dma_full_window"]
                out.append(_case(m.name, fam, m, g, rounds, edge + ["col=%s@p%d" % (e, p) for e in EDGES[1:] for p in range(2)]))
        elif fam == "outside":
            band = (60, 2 * g.round_elems + 500)
            n = 2 * rpc + rpc // 2
            n_cols = n + band[1] + 16
            L = 8 if T == 2 else 12
            lens = [L] * n
            planted = []
            spans = [chunk_sweep(rb, min(rb + rpc, n), band, n_cols, vb, g.round_elems) for rb in range(0, n, rpc)]
            for ci in (1, 2):                       # (their c_lo > 0; chunk 2 is short: the slots of its first waves)
                rb = ci * rpc
                sp = spans[ci]
                for r_ in range(held):
                    for e_ in range(4):
                        for which, wave, col in (("below", 1, sp["c_lo"] - 1 - 3 * e_), ("above", 2, sp["c_hi"] + 1 + 5 * e_)):
                            planted.append((rb + local_row(g, wave, r_, (e_ + (which == "above")) % g.VW), e_, col))
            sp = spans[1]
            wave4 = rpc + local_row(g, 4, 0, 0)
            planted += [(wave4, k_, sp["c_lo"] - 2 - k_ if k_ % 2 else sp["c_hi"] + 2 + k_) for k_ in range(L)]       # a row wholly outside
            lane_row = rpc + local_row(g, 5, held - 1, g.VW - 1)
            first = 0 if T == 2 else 4
            planted += [(lane_row, first + k_, sp["c_hi"] + 7 + k_) for k_ in range(4)]                            # one lane wholly outside
            m = matrix("outside_slots_%s" % tag, lens, n_cols, band, rpc, planted=planted)
            edge = ["%s@r%de%d" % (w_, r_, e_) for w_ in ("below", "above") for r_ in range(held) for e_ in range(4)]
            out.append(_case(m.name, fam, m, g, 1, edge + ["row_all_outside", "lane_all_outside_neighbour_inside", "outside_below", "outside_above"]))
            # rectangular: the last chunk's band lies wholly beyond n_cols — nothing is swept, every slot is gathered
            band = (200, 2 * g.round_elems)
            n = 2 * rpc + 9
            m = matrix("outside_empty_sweep_%s" % tag, [L] * n, 2 * rpc + 150, band, rpc)
            out.append(_case(m.name, fam, m, g, 1, ["empty_sweep", "passes0"]))
            band = (-40, 2 * g.round_elems + 500)
            n = rpc + 40
            lens = [L] * n
            planted = [(7, 0, 900), (7, 5, 900), (rpc + 3, 1, 1234), (rpc + 3, 2, 1234), (rpc + 3, 6, 1234)]
            m = matrix("outside_unsorted_%s" % tag, lens, n + band[1] + 8, band, rpc, cols="unsorted", planted=planted)
            out.append(_case(m.name, fam, m, g, 1, ["unsorted_row", "duplicate_in_row"]))
        elif fam == "rows":
            band = (-40, 2 * g.round_elems + 300)
            m = rows_steps_matrix(g, band, 3 * rpc + band[1])
            edge = ["len0", "steps1", "steps2", "steps3", "steps4+", "second_step_by_phase", "long_row", "later_step", "empty_at_chunk_start"]
            edge += ["len1@phase%d" % p for p in range(4)]
            edge += ["k%dd%+d@phase%d" % (k_, dd, p) for k_, dd in ((1, -1), (1, 0), (1, 1), (2, 0), (2, 1)) for p in range(4) if 4 * T * k_ + dd > 1]
            edge += ["corner_wave_%s_vector_%s_slot_%s" % (a, b, c_) for a in ("first", "last") for b in ("first", "last") for c_ in ("first", "last")]
            edge.append("empty_at_chunk_end")
            out.append(_case(m.name, fam, m, g, 1, edge))
            ln = lambda n_: [1 + (3 * r_) % 7 for r_ in range(n_)]
            m = matrix("rows_rowid_%s" % tag, ln(2 * rpc), 2 * rpc + band[1], band, rpc, data="rowid")
            out.append(_case(m.name, fam, m, g, 1, ["rowid_full_chunk", "last_chunk=rpc"]))
            for name, last in (("1", 1), ("VW-1", g.VW - 1), ("VW", g.VW), ("rpc-1", rpc - 1)):
                if last < 1 or (name == "VW" and g.VW == 1):
                    continue
                m = matrix("rows_last%s_%s" % (name, tag), ln(rpc + last), 2 * rpc + band[1], band, rpc, data="rowid")
                out.append(_case(m.name, fam, m, g, 1, ["last_chunk=" + name]))
        elif fam == "tail":
            band = (-40, 2 * g.round_elems + 300)
            for m in tail_matrices(g, band, rpc + 40 + band[1]):
                nm = m.name
                if nm.startswith("tail"):
                    edge = ["tail%s_row_crosses" % nm[4], "scalar_tail"] + (["j_max_clamp"] if T > 2 else [])
                    edge += ["tail%s_empty_behind" % nm[4]] if "then_empty" in nm else []
                    edge += ["single_chunk"] if "single" in nm or "then_empty" in nm else ["tail_in_last_of_several_chunks"]
                elif nm.startswith("last_row"):
                    start, ln_ = int(nm[len("last_row_at_nnz_vec+")]), int(nm.split("_len")[1][0])
                    edge = ["tail%d_row_starts_at+%d" % (start + ln_, start), "tail%d_empty_behind" % (start + ln_), "j_max_clamp"]
                    edge += ["tail_row_starts_inside"] if start else []
                else:
                    edge = ["nnz%s" % nm.split("_")[1], "single_chunk"]
                out.append(_case(nm, fam, m, g, 1, edge))
        elif fam == "blocks":
            band = (-40, 2 * g.round_elems + 300)
            m = blocks_matrix(g, band, 3 * rpc + band[1] + 3)
            out.append(_case(m.name, fam, m, g, 1, ["passes3", "nnz%4=1", "tail1_row_starts_at+0"]))
        elif fam == "light":
            # one dequeue per workgroup: more than 2 x 256 chunks (set_rows_launch); rows of 0..4, a short last chunk
            n = (LIGHT_STATIC_CHUNKS + 1) * rpc - 47
            band = (-40, 2 * g.round_elems + 300)
            m = matrix("light_dequeue_once_%s" % tag, [(7 * r_) % 5 for r_ in range(n)], n + band[1], band, rpc)
            out.append(_case(m.name, fam, m, g, 1, ["light_dequeue_once", "passes3", "len0"]))
        else:
            raise KeyError(fam)
    return tuple(out)


def table(vb=None):
    out = []
    for fam in FAMILIES:
        for T in FAMILY_LANES[fam]:
            for b in ((4, 8) if vb is None else (vb,)):
                out += family(fam, T, b)
    return out


def block_cuts(c):
    """The row cuttings of a blocks case: lists of (r0, r1)."""
    n = len(c.matrix.lens)
    rpc = c.matrix.rpc
    out = []
    for cuts in BLOCK_CUTS:
        rows = [n if v is None else v * rpc for v in cuts]
        out.append(list(zip(rows[:-1], rows[1:])))
    return out


# ---- the smallest matrix the planner itself sweeps (the planner-made tie) ------------------------------------------------
TIE_KNOBS = {"MI355_SPMV_SWEEP": "1", "MI355_SPMV_BALANCE": "0", "MI355_SPMV_SMALL": "0"}
TIE_HALF_BAND = {4: 20000, 8: 10000}


def tie_matrix(vb):
    """512 chunks at T = 64 (65 536 rows in fp32, eight rows per vector; 32 768 in fp64, four): the 256 probed rows are
    129-256 long, every other row 3; columns in [row, row + 2 HW] (no clip: n_cols = n + 2 HW + 1), the probed rows' first
    and last columns spread evenly over the band — one cluster, no segments — with both extremes shown.  Returns (Ap, Aj,
    n_cols, band)."""
    held = sweep_rows_for(vb, WAVE)
    g = geo(WAVE, held, vb)
    n = LIGHT_STATIC_CHUNKS * g.rpc
    hw = TIE_HALF_BAND[vb]
    lens = np.full(n, 3, dtype=np.int64)
    probed = rc.probed_rows(n)
    lens[probed] = 129 + (np.arange(probed.size) * 127) // (probed.size - 1)
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    nnz = int(Ap[-1])
    rng = np.random.default_rng([19, n, nnz])
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    off = (rng.random(nnz) * (2 * hw + 1)).astype(np.int64)
    Aj = row + off
    Aj = Aj[np.lexsort((Aj, row))]
    for i, p_ in enumerate(probed):              # first columns at offsets 0 .. < HW (0 shown), last at > HW .. 2 HW (2 HW shown)
        first, last = (i * hw) // probed.size, 2 * hw - ((probed.size - 1 - i) * hw) // probed.size
        inner = np.sort(first + (rng.random(int(lens[p_]) - 2) * (last - first + 1)).astype(np.int64))
        Aj[Ap[p_]:Ap[p_ + 1]] = p_ + np.concatenate([[first], inner, [last]])
    return Ap, Aj.astype(np.int32), n + 2 * hw + 1, (0, 2 * hw)
