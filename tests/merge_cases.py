"""The table of merge_tile_kernel cases (csrc/merge_path.hip) that tests/test_gpu_merge_edges.py executes on the device
and whose reach tests/test_merge_cases_cpu.py proves on the host: structures built from the kernel's geometry, never
from literals.

Geometry: the merge of the row ends with the nonzeros (the nonzeros of row r come before its end: nonzero n of row r
is item n + r, the end of row r is item Ap[r + 1] + r) is cut into tiles of TILE = BLOCK * IPT - 4 items; thread T of
a tile walks items T * IPT .. T * IPT + IPT of it, 64 threads are a wave, and a workgroup walks a run of
MI355_MERGE_TPS consecutive tiles.  (BLOCK, IPT) is (256, 8) or, under MI355_MERGE_BLOCK=512 and plus-times, (512, 4).

census() restates that DECOMPOSITION only (which thread sees which items, and what the kernel's predicates make of
them); it never computes a y.  Expected values come from the serial oracle alone.  The row-parallel run kernel
(merge_rows_kernel), which this table keeps away with MI355_MERGE_ROWS=0, has its own in tests/merge_run_cases.py.

Data: integer-valued ({-3..3} x {-2..2}: exact in any order), and for the float types a second, real-valued pass over
the thread-edge, tail and run families.  In float cases the columns of x that no row references hold NaN."""
import collections

import numpy as np

VARIANTS = ((256, 8), (512, 4))      # (BLOCK, IPT) = info()["block_threads"], info()["elems_per_lane"]
TILE = 2044                          # = BLOCK * IPT - 4 for both = info()["tile_items"]
WAVE = 64                            # kWave
FILL = 37                            # the long rows between the edges: every thread sees at most one of their ends
MIN_LONG = 18                        # >= 2 * IPT + 2 for both variants
INF = 1 << 40
assert all(b * i - 4 == TILE and MIN_LONG >= 2 * i + 2 for b, i in VARIANTS)

NP_OFF = {"i32": np.int32, "i64": np.int64}
# value-type case -> (type of x and y, type the matrix is stored in; None: a pattern matrix) — test_gpu_merge_shared.TYPES
TYPES = {"f32": (np.float32, np.float32), "f64": (np.float64, np.float64), "i32": (np.int32, np.int32),
         "f32-under-f64": (np.float64, np.float32), "pattern-f32": (np.float32, None)}
ALL_TYPES = tuple((off, val, sr) for off in ("i32", "i64") for val in TYPES for sr in ("plus_times", "min_plus"))
TWO_TYPES = (("i32", "f32", "plus_times"), ("i64", "f64", "plus_times"))
ALPHA_BETA = (2.0, -1.0)             # integers: exact on integer data

Matrix = collections.namedtuple("Matrix", "name lens n_cols seed escapes")
# knobs: the environment the plan is created under; block: 256 | 512; edge: the census states the case is there for;
# window: the plan must have a window of x; unaligned: Aj / Ax are views one element off 16-byte alignment (non-VEC)
Case = collections.namedtuple("Case", "name family matrix knobs block edge window unaligned")


def ipt_of(block):
    return dict(VARIANTS)[block]


# ---- structures ------------------------------------------------------------------------------------------------------
class Rows:
    """Row lengths, with the merge item count kept so that a row end can be put on a chosen item."""

    def __init__(self, lens=()):
        self.lens = list(lens)
        self.items = sum(self.lens) + len(self.lens)

    def add(self, *lens):
        self.lens += list(lens)
        self.items += sum(lens) + len(lens)
        return self

    def end_at(self, item):
        """One more row whose row-end item is `item` (its last nonzero, if it has one, is item - 1)."""
        n = item - self.items
        assert n >= 0, (item, self.items)
        return self.add(n)

    def fill_to(self, item, fill=FILL):
        """Long rows (>= MIN_LONG nonzeros each), the last of which ends on `item`."""
        while item - self.items >= 2 * (fill + 1):
            self.add(fill)
        assert item - self.items >= MIN_LONG, (item, self.items)
        return self.end_at(item)


def item(block, t, thread, k=0):
    """Item k of thread `thread` of tile t."""
    return t * TILE + thread * ipt_of(block) + k


def ragged(seed, n, hi=41):
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, hi, size=n)
    lens[rng.rand(n) < 0.2] = 0
    return [int(v) for v in lens]


def thread_edge_matrices(block):
    ipt = ipt_of(block)
    out = []
    # equal rows of every length 1 .. 2 IPT + 1 (of the 8-item variant: the 4-item one gets lengths up to 4 IPT + 1).
    # Rows of L nonzeros put two ends L + 1 items apart: both fall into one thread's IPT items only for L <= IPT - 2.
    # L = IPT - 1 is already simple — with the first end on item `before` the next one is at best the following
    # thread's first item, re2 - re = IPT - 1 >= cnt - before - 1 — so the waves walk up to IPT - 2, not IPT - 1.
    for L in range(1, 2 * 8 + 2):
        out.append(("equal_%d" % L, [L] * (3 * TILE // (L + 1) + 3), ()))
    # a row end on item k of its thread for every k: rows of 2 IPT + 1 items move the end by one item per row (the
    # waves are simple); with an empty row behind every end the waves walk
    out.append(("end_on_every_item_simple_b%d" % block, [2 * ipt] * (3 * TILE // (2 * ipt + 1) + 2), ()))
    out.append(("end_on_every_item_walking_b%d" % block, [2 * ipt - 1, 0] * (3 * TILE // (2 * ipt + 1) + 2), ()))
    return out


def re2_matrices(block):
    """The boundary of `simple`: a thread whose first row end is item `before`, and the next end `delta` items from the
    thread's last item + 1 (delta = -1: the thread's last item, not simple; 0: the next thread's first; +1: its second).
    One probe per wave, lane 21."""
    ipt = ipt_of(block)
    waves = block // WAVE

    def probes(specs):
        r = Rows()
        for i, (before, behind) in enumerate(specs):
            w = i + 1
            r.fill_to(item(block, w // waves, (w % waves) * WAVE + 21, before))
            r.add(*behind)
        return r.fill_to(r.items + 5 * FILL).lens

    margin = [(b, [ipt - b - 1 + d]) for b in range(ipt) for d in (-1, 0, 1) if ipt - b - 1 + d >= 0]
    empty = [(b, [0]) for b in range(ipt)]                   # re2 == re; before == IPT - 1: the end is the last item
    empty2 = [(b, [0, 0]) for b in (ipt - 1, ipt - 2)]       # ... and a second empty row behind it
    return [("re2_margin_b%d" % block, probes(margin), ()), ("re2_empty_row_b%d" % block, probes(empty + empty2), ())]


def walker(r, block, t, thread):
    """Thread `thread` of tile t gets IPT - 3 nonzeros, a row end, the end of an empty row and a nonzero: it alone of its
    neighbourhood is not simple."""
    return r.fill_to(item(block, t, thread, ipt_of(block) - 3)).add(0)


def mixed_wave_matrices(block):
    ipt = ipt_of(block)
    mid = (block // WAVE) // 2
    out = []
    r = Rows([ipt - 3, 0])                                   # lane 0 of wave 0 of tile 0 (no carry yet) ...
    walker(r, block, 1, 0)                                   # ... and of tile 1, behind the row tile 0 left open
    out.append(("walker_lane0_wave0", r.fill_to(2 * TILE + 300).lens))
    r = walker(Rows(), block, 1, mid * WAVE + 63)
    out.append(("walker_lane63_middle_wave", r.fill_to(2 * TILE + 300).lens))
    r = Rows().fill_to(item(block, 1, mid * WAVE + 63, ipt - 2)).add(0, 0, 0)
    out.append(("walkers_across_two_waves", r.fill_to(2 * TILE + 300).lens))
    r = Rows().fill_to(2 * TILE - 3).add(0, 0, 0, 0, 0)       # ends on the last two items of tile 1 and the first three of tile 2
    out.append(("walkers_across_two_tiles", r.fill_to(3 * TILE + 300).lens))
    return [("%s_b%d" % (n, block), l, ()) for n, l in out]


def scan_matrix(block):
    waves = block // WAVE
    r = Rows().fill_to(item(block, 1, 10, 3))
    r.end_at(item(block, 1, WAVE + 10, 3))                   # opens in wave 0, closes in wave 1
    r.end_at(item(block, 1, 3 * WAVE + 10, 3))               # opens in wave 1, closes in wave 3
    r.fill_to(item(block, 2, 5, 2))
    r.end_at(item(block, 2, (waves - 1) * WAVE + 7, 1))      # opens in wave 0, closes in the last wave
    r.fill_to(item(block, 3, 20, 0))
    r.end_at(item(block, 5, 30, 1))                          # tile 4 has no row end: total folds unflagged wave sums only
    r.fill_to(item(block, 6, 2 * WAVE, 0))                   # last nonzero = last item of wave 1, end = first item of wave 2
    return [("scan_b%d" % block, r.fill_to(6 * TILE + 1500).lens, ())]


def tile_edge_matrices():
    out = []
    r = Rows().fill_to(2 * TILE - 1).fill_to(3 * TILE)       # an end as the last item of tile 1, one as the first of tile 3
    out.append(("end_last_and_first_item_of_tile", r.fill_to(4 * TILE + 700).lens))
    out.append(("tile_of_row_ends_only", [5] + [0] * (2 * TILE + 10) + [3]))
    r = Rows().fill_to(TILE - 1)                             # whole tiles of exactly tr row ends, BLOCK - 1 .. BLOCK + 1 of both variants
    for i, tr in enumerate(b + e for b, _ in VARIANTS for e in (-1, 0, 1)):
        if i % 2 == 0:
            r.add(TILE - tr).add(*[0] * (tr - 1))
        else:
            r.add(*[0] * (tr - 1)).add(TILE - tr)
        assert r.items % TILE == 0
    out.append(("row_ends_around_the_prefetch", r.add(7).lens))
    out.append(("tiles_of_nonzeros_only", [10, 3 * TILE + 100, 10]))
    for n in (1,) + tuple(i + 1 for _, i in VARIANTS):       # a last tile of 1 item and of IPT + 1 items
        out.append(("last_tile_of_%d_items" % n, Rows(ragged(50 + n, 150)).end_at(2 * TILE + n - 1).lens))
    out.append(("items_a_multiple_of_the_tile", Rows(ragged(60, 150)).end_at(2 * TILE - 1).lens))
    out.append(("items_one_below_a_multiple", Rows(ragged(61, 150)).end_at(2 * TILE - 2).lens))
    return [(n, l, ()) for n, l in out]


def tail_matrices():
    out = [("tile_starts_at_every_shift", ragged(70, 620), ())]
    for r4 in range(4):                                      # nnz % 4, the tail inside the last tile
        r = Rows(ragged(80 + r4, 240))
        nnz = sum(r.lens)
        out.append(("tail_%d_inside_last_tile" % r4, r.add(9 + (r4 - nnz - 9) % 4).lens, ()))
    for c in range(3):                                       # the last tile STARTS inside the tail: y0 % 4 == 1, c nonzeros in it
        r = Rows(ragged(90 + c, 150))
        r.add(4 + (1 - sum(r.lens) - 4) % 4)
        r.add(*[0] * (2 * TILE - r.items))
        out.append(("last_tile_starts_inside_tail_%d" % (c + 1), r.add(c, 0, 0).lens, ()))
    for nnz in range(1, 8):
        out.append(("nnz_%d" % nnz, [1, 0, nnz - 1], ()))
    return out


def runs_matrix():
    """13 tiles: a row through six tiles (three runs and more at 1, 2 and 3 tiles per run), short rows closed inside a
    thread, rows of ~100 that the run boundaries cut, a row end on the last item of tile 11 (a run boundary at 1, 2 and 3
    tiles per run: that run's carry is the identity) and a short last tile."""
    r = Rows().fill_to(TILE // 2).end_at(6 * TILE + TILE // 2)
    r.add(*[1, 2, 0, 3] * 20)
    r.fill_to(12 * TILE - 1, fill=97)
    return [("runs", r.add(50, 0, 3).lens, ())]


def window_matrix():
    """Rows of 40 in a band (column = row + position) of 4 096 columns, and single columns ~3 000 away: on element
    0..3 of a 16-byte group, on the first and the last nonzero of a tile, and on both sides of a tile cut inside a group.
    No escape is the first or last nonzero of its row, so no sampled row widens the window towards it."""
    lens = [40] * 520
    xs, ys = coords(lens)
    esc = {1004, 1009, 1014, 1019}
    for t in range(1, len(ys) - 1):
        esc |= {int(ys[t]) - 1, int(ys[t])}
    Ap = np.concatenate(([0], np.cumsum(lens)))
    esc -= set(Ap.tolist()) | set((Ap - 1).tolist())           # (a cut on a row's edge: the census asks for the others)
    return [("band_with_escapes", lens, tuple(sorted(esc)))]


# ---- the decomposition -------------------------------------------------------------------------------------------------
def coords(lens):
    """(row, nnz) of every tile boundary: how many row ends lie before diagonal t * TILE, and the nonzeros that leaves."""
    lens = np.asarray(lens, dtype=np.int64)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    ends = Ap[1:] + np.arange(len(lens))
    items = len(lens) + int(Ap[-1])
    diag = np.minimum(np.arange(-(-items // TILE) + 1) * TILE, items)
    xs = np.searchsorted(ends, diag, "left")
    return xs, diag - xs


def census(lens, block, tps=1, escapes=(), tile_coords=None):
    """The states of merge_tile_kernel<block, IPT> that a matrix of these row lengths reaches, as a set of names."""
    ipt, waves = ipt_of(block), block // WAVE
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    nnz = int(Ap[-1])
    items = n + nnz
    ends = Ap[1:] + np.arange(n)
    xs, ys = coords(lens) if tile_coords is None else [np.asarray(a, dtype=np.int64) for a in tile_coords]
    T = len(xs) - 1
    diag = xs + ys
    tr, tn = np.diff(xs), np.diff(ys)
    out = {"nnz=%d" % nnz} if nnz < 8 else set()
    # per tile
    out |= {"shift%d" % s for s in set((ys[:-1] & 3).tolist())}
    for name, hit in (("tile_of_nonzeros_only", (tr == 0) & (tn == TILE)), ("tile_of_row_ends_only", (tn == 0) & (tr == TILE)),
                      ("second_row_end_loop", tr > block)):
        if hit.any():
            out.add(name)
    out |= {"tr=BLOCK%+d" % e for e in (-1, 0, 1) if (tr == block + e).any()}
    is_end = np.zeros(items + 1, dtype=bool)
    is_end[ends] = True
    if is_end[diag[1:-1] - 1].any():
        out.add("end_is_last_item_of_tile")
    if is_end[diag[1:-1]].any():
        out.add("end_is_first_item_of_tile")
    last = int(tr[-1] + tn[-1])
    out |= {"last_tile_of_%s" % k for k, v in (("1_item", 1), ("IPT+1_items", ipt + 1), ("TILE_items", TILE), ("TILE-1_items", TILE - 1))
            if last == v}
    nnz_vec = nnz & ~3
    if nnz >= 4:
        out.add("tail_%d_%s" % (nnz % 4, "before_last_tile" if ys[-2] > nnz_vec else "inside_last_tile"))
    # per thread
    tid = np.arange(block)
    D0 = diag[:-1, None] + np.minimum(tid * ipt, (tr + tn)[:, None])
    D1 = np.minimum(D0 + ipt, diag[1:, None])
    cnt = D1 - D0
    X = np.searchsorted(ends, D0, "left")
    Y = D0 - X
    Ape = np.concatenate((Ap[1:], [INF, INF]))
    x1 = xs[1:, None]
    re = np.where(X < x1, Ape[X], INF)
    re2 = np.where(X + 1 < x1, Ape[X + 1], INF)
    before = re - Y
    has_end = before < cnt
    margin = (re2 - re) - (cnt - before - 1)
    simple = ~has_end | (margin >= 0)
    n_ends = np.searchsorted(ends, D1, "left") - X
    assert np.array_equal(n_ends > 0, has_end)
    wave_simple = simple.reshape(T, waves, WAVE).all(-1)
    in_simple = np.repeat(wave_simple, WAVE, axis=1)
    for k in range(ipt):
        if (has_end & (before == k) & in_simple).any():
            out.add("end_on_item_%d_simple" % k)
        if (has_end & (before == k) & ~in_simple).any():
            out.add("end_on_item_%d_walking" % k)
    full = has_end & (cnt == ipt)
    out |= {"re2_margin%+d" % m for m in (-1, 0, 1) if (full & (margin == m) & (re2 > re)).any()}
    out |= {"re2_margin%+d_before_%d" % (m, b) for m in (-1, 0, 1) for b in range(ipt) if (full & (margin == m) & (before == b)).any()}
    if (full & (re2 == re) & ~simple).any():
        out.add("empty_row_behind_first_end")
    if (full & (re2 == re) & (before == cnt - 1)).any():
        out.add("empty_row_behind_end_on_last_item")
    if (n_ends >= 2).any():
        out.add("row_closed_inside_a_thread")
    if ((cnt == 0) & ((tr + tn)[:, None] > 0)).any():
        out.add("threads_without_items")
    # per wave
    out |= {name for name, hit in (("wave_simple", wave_simple), ("wave_walking", ~wave_simple)) if hit.any()}
    lane = tid & (WAVE - 1)
    wave = tid // WAVE
    for t in range(T):
        walking = np.nonzero(~wave_simple[t])[0]
        odd = np.nonzero(~simple[t])[0]
        if 0 < len(walking) < waves and (cnt[t].reshape(waves, WAVE).sum(-1) > 0).all():
            out.add("tile_of_both_wave_modes")
        if len(odd) == 1 and odd[0] == 0:
            out.add("only_walker_is_lane0_of_wave0" + ("_behind_an_open_row" if t > 0 and Ap[xs[t]] < ys[t] else ""))
        if len(odd) == 1 and lane[odd[0]] == WAVE - 1 and 0 < wave[odd[0]] < waves - 1:
            out.add("only_walker_is_lane63_of_a_middle_wave")
        if len(odd) == 2 and lane[odd[0]] == WAVE - 1 and odd[1] == odd[0] + 1:
            out.add("walkers_across_two_waves")
        if t + 1 < T and list(walking) == [waves - 1] and list(np.nonzero(~wave_simple[t + 1])[0]) == [0]:
            out.add("walkers_across_two_tiles")
        # scan: the row a thread's first end closes was opened by the last thread before it that holds an end
        holders = np.nonzero(has_end[t])[0]
        if len(holders) == 0 and t > 0:
            out.add("tile_without_row_end")
        for a, b in zip(holders[:-1], holders[1:]):
            dist = wave[b] - wave[a]
            if dist in (1, 2):
                out.add("row_closes_%d_waves_on" % dist)
            if dist >= 1 and wave[b] == waves - 1:
                out.add("row_closes_in_last_wave")
        first_of_wave = has_end[t] & (before[t] == 0) & (lane == 0) & (wave > 0) & (lens[np.minimum(X[t], n - 1)] > 0)
        if first_of_wave.any():
            out.add("end_is_first_item_of_a_wave")
    # runs
    n_super = -(-T // tps)
    cut = np.minimum(np.arange(n_super + 1) * tps, T)
    carry_row = xs[cut[1:]]
    out.add("one_run" if n_super == 1 else "several_runs")
    if tps > T:
        out.add("more_tiles_per_run_than_tiles")
    inner = carry_row[:-1]
    if len(inner) >= 2 and (inner[1:] == inner[:-1]).any():
        out.add("row_spans_three_runs")
    if len(inner) >= 2 and (inner[1:] != inner[:-1]).any():
        out.add("neighbour_runs_carry_different_rows")
    if len(inner) and (Ap[inner] == ys[cut[1:-1]]).any():
        out.add("run_ends_on_a_row_end")
    assert carry_row[-1] == n                                 # (the last run's carry row is n_rows for EVERY matrix: no state of its own)
    # window escapes (nonzero numbers whose column lies far outside the band)
    esc = np.asarray(escapes, dtype=np.int64)
    if len(esc):
        out |= {"escape_on_element_%d" % e for e in set((esc & 3).tolist())}
        inner_y = ys[1:-1]
        if np.isin(inner_y, esc).any():
            out.add("escape_on_first_nonzero_of_tile")
        if np.isin(inner_y - 1, esc).any():
            out.add("escape_on_last_nonzero_of_tile")
        cut_in_group = inner_y[(inner_y & 3) != 0]
        if np.isin(cut_in_group - 1, esc).any():
            out.add("escape_left_of_a_cut_inside_a_group")
        if np.isin(cut_in_group, esc).any():
            out.add("escape_right_of_a_cut_inside_a_group")
    return out


def states(block):
    """Every state the table must reach for this variant."""
    ipt = ipt_of(block)
    out = {"shift%d" % s for s in range(4)} | {"nnz=%d" % k for k in range(1, 8)}
    out |= {"tile_of_nonzeros_only", "tile_of_row_ends_only", "second_row_end_loop", "tr=BLOCK-1", "tr=BLOCK+0", "tr=BLOCK+1",
            "end_is_last_item_of_tile", "end_is_first_item_of_tile", "last_tile_of_1_item", "last_tile_of_IPT+1_items",
            "last_tile_of_TILE_items", "last_tile_of_TILE-1_items"}
    out |= {"tail_%d_inside_last_tile" % r for r in range(4)} | {"tail_%d_before_last_tile" % r for r in (1, 2, 3)}
    out |= {"end_on_item_%d_%s" % (k, m) for k in range(ipt) for m in ("simple", "walking")}
    out |= {"re2_margin%+d" % m for m in (-1, 0, 1)}
    out |= {"re2_margin%+d_before_%d" % (m, b) for m in (-1, 0, 1) for b in range(ipt) if ipt - b - 1 + m >= 0}
    out |= {"empty_row_behind_first_end", "empty_row_behind_end_on_last_item", "row_closed_inside_a_thread",
            "threads_without_items", "wave_simple", "wave_walking", "tile_of_both_wave_modes",
            "only_walker_is_lane0_of_wave0", "only_walker_is_lane0_of_wave0_behind_an_open_row",
            "only_walker_is_lane63_of_a_middle_wave", "walkers_across_two_waves", "walkers_across_two_tiles",
            "tile_without_row_end", "row_closes_1_waves_on", "row_closes_2_waves_on", "row_closes_in_last_wave",
            "end_is_first_item_of_a_wave", "one_run", "several_runs", "more_tiles_per_run_than_tiles", "row_spans_three_runs",
            "neighbour_runs_carry_different_rows", "run_ends_on_a_row_end"}
    out |= {"escape_on_element_%d" % e for e in range(4)}
    out |= {"escape_on_first_nonzero_of_tile", "escape_on_last_nonzero_of_tile", "escape_left_of_a_cut_inside_a_group",
            "escape_right_of_a_cut_inside_a_group"}
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------
FAMILIES = ("thread_edges", "re2", "mixed_waves", "scan", "tile_edges", "tail", "unaligned", "runs", "window")
FAMILY_TYPES = {f: ALL_TYPES if f in ("thread_edges", "re2", "tile_edges", "runs") else TWO_TYPES for f in FAMILIES}
# the second, real-valued pass (float types).  The tail family has it because a slot of the array tail that keeps the
# clamped group's product holds another nonzero's a * x: on integer data in {-3..3} x {-2..2} the two are equal often
# enough that a shortened tail store went unseen in seven of its cases; on real data they never are.
REAL_FAMILIES = ("thread_edges", "tail", "runs")
BASE = {"MI355_MERGE_ROWS": "0", "MI355_MERGE_TPS": "2", "MI355_MERGE_FUSED": "1"}


def _knobs(block, **kw):
    k = dict(BASE)
    if block == 512:
        k["MI355_MERGE_BLOCK"] = "512"
    k.update({"MI355_" + name: str(v) for name, v in kw.items()})
    return k


_seed = [1000]


def _cases(family, block, matrices, edges, n_cols=1500, window=False, unaligned=False, tag="", **kw):
    out = []
    for (name, lens, esc), edge in zip(matrices, edges):
        _seed[0] += 1
        m = Matrix(name, tuple(int(v) for v in lens), n_cols, _seed[0], tuple(esc))
        out.append(Case("%s-b%d%s" % (name, block, tag), family, m, _knobs(block, **kw), block, tuple(edge), window, unaligned))
    return out


def _table(block):
    ipt = ipt_of(block)
    _seed[0] = 1000 * block
    out = []
    ms = thread_edge_matrices(block)
    edges = [("wave_walking",) if L < ipt - 1 else ("wave_simple",) for L in range(1, 18)]
    edges.append(["end_on_item_%d_simple" % k for k in range(ipt)])
    edges.append(["end_on_item_%d_walking" % k for k in range(ipt)])
    out += _cases("thread_edges", block, ms, edges)
    margin = ["re2_margin%+d_before_%d" % (m, b) for m in (-1, 0, 1) for b in range(ipt) if ipt - b - 1 + m >= 0]
    out += _cases("re2", block, re2_matrices(block), [margin + ["re2_margin-1", "re2_margin+0", "re2_margin+1"],
                                                      ["empty_row_behind_first_end", "empty_row_behind_end_on_last_item"]])
    out += _cases("mixed_waves", block, mixed_wave_matrices(block), [
        ("only_walker_is_lane0_of_wave0", "only_walker_is_lane0_of_wave0_behind_an_open_row", "tile_of_both_wave_modes"),
        ("only_walker_is_lane63_of_a_middle_wave", "tile_of_both_wave_modes"),
        ("walkers_across_two_waves", "tile_of_both_wave_modes"), ("walkers_across_two_tiles", "tile_of_both_wave_modes")])
    out += _cases("scan", block, scan_matrix(block), [("row_closes_1_waves_on", "row_closes_2_waves_on", "row_closes_in_last_wave",
                                                       "tile_without_row_end", "end_is_first_item_of_a_wave")])
    tile_edge = {
        "end_last_and_first_item_of_tile": ("end_is_last_item_of_tile", "end_is_first_item_of_tile"),
        "tile_of_row_ends_only": ("tile_of_row_ends_only", "second_row_end_loop"),
        "row_ends_around_the_prefetch": ("tr=BLOCK-1", "tr=BLOCK+0", "tr=BLOCK+1", "second_row_end_loop"),
        "tiles_of_nonzeros_only": ("tile_of_nonzeros_only", "tile_without_row_end"),
        "last_tile_of_1_items": ("threads_without_items", "last_tile_of_1_item"),
        "last_tile_of_%d_items" % (ipt + 1): ("threads_without_items", "last_tile_of_IPT+1_items"),
        "items_a_multiple_of_the_tile": ("last_tile_of_TILE_items",),
        "items_one_below_a_multiple": ("last_tile_of_TILE-1_items",)}
    ms = tile_edge_matrices()
    out += _cases("tile_edges", block, ms, [tile_edge.get(m[0], ("threads_without_items",)) for m in ms])
    tails = tail_matrices()
    edges = [["shift%d" % s for s in range(4)]] + [("tail_%d_inside_last_tile" % r,) for r in range(4)]
    edges += [("tail_%d_before_last_tile" % r,) for r in (1, 2, 3)] + [("nnz=%d" % k,) for k in range(1, 8)]
    out += _cases("tail", block, tails, edges)
    runs = runs_matrix()
    by_name = {m[0]: m for m in tails + tile_edge_matrices() + runs}
    # the 4-byte body on structures from above, with their edges (that the body is the non-VEC one follows from the
    # pointers' alignment alone, which the device test asserts: info() has no field for it)
    for name, edge in (("tail_3_inside_last_tile", ("tail_3_inside_last_tile",)),
                       ("row_ends_around_the_prefetch", ("tr=BLOCK+0", "second_row_end_loop")),
                       ("runs", ("several_runs", "row_closed_inside_a_thread", "run_ends_on_a_row_end")), ("nnz_5", ("nnz=5",))):
        out += _cases("unaligned", block, [by_name[name]], [edge], unaligned=True, tag="-unaligned", MERGE_FUSED=0)
    for tps in (1, 2, 3, 1000):
        edge = ["row_closed_inside_a_thread"]
        edge += ["one_run", "more_tiles_per_run_than_tiles"] if tps == 1000 else [
            "several_runs", "row_spans_three_runs", "neighbour_runs_carry_different_rows", "run_ends_on_a_row_end"]
        # (the 512-thread kernel never searches its own coordinates: the search kernel in front, 1 and 16 lanes)
        for fused, lanes in ((1, 0), (0, 1), (0, 16)) if block == 256 else ((0, 1), (0, 16)):
            kw = dict(MERGE_TPS=tps, MERGE_FUSED=fused)
            if lanes:
                kw["MERGE_SEARCH_LANES"] = lanes
            out += _cases("runs", block, runs, [edge], tag="-tps%d-fused%d-lanes%d" % (tps, fused, lanes), **kw)
    esc = ["escape_on_element_%d" % e for e in range(4)] + [
        "escape_on_first_nonzero_of_tile", "escape_on_last_nonzero_of_tile", "escape_left_of_a_cut_inside_a_group",
        "escape_right_of_a_cut_inside_a_group"]
    for win in (1, 0):
        out += _cases("window", block, window_matrix(), [esc], n_cols=4096, window=bool(win), tag="-window%d" % win,
                      MERGE_TPS=5, SPMV_WINDOW=win)
    return out


_tables = {}


def table(block):
    if block not in _tables:
        _tables[block] = _table(block)
    return _tables[block]


def family(name, block):
    return [c for c in table(block) if c.family == name]


def tps_of(case):
    return int(case.knobs["MI355_MERGE_TPS"])


FUSED_MAX_DIAGONALS = 32             # merge_search_in_kernel: a run of more diagonals than this is never searched in the kernel


def fused_of(case):
    """Whether the plan's tile kernel is the one that searches its own coordinates (merge_plan.hip,
    merge_search_in_kernel, under an explicit MI355_MERGE_FUSED; the 512-thread kernel never does)."""
    return case.knobs["MI355_MERGE_FUSED"] == "1" and tps_of(case) + 1 <= FUSED_MAX_DIAGONALS and case.block == 256


def n_kernels_of(case, n_tiles):
    n_super = -(-n_tiles // tps_of(case))
    return (2 if n_super > 1 else 1) + (0 if fused_of(case) else 1)


# ---- operands ------------------------------------------------------------------------------------------------------------
_arrays = {}


def arrays(m, integer):
    """(Ap int64, Aj, Ax float64, x float64, y0 float64, used columns) of a matrix; made once and left unchanged.  The
    columns come from half of the columns (a band matrix: column = row + position, escapes ~3 000 further on); the
    caller casts, and puts NaN into the columns of a float x that are not used."""
    key = (m.name, m.seed, integer)
    if key not in _arrays:
        rng = np.random.RandomState(m.seed)
        lens = np.asarray(m.lens, dtype=np.int64)
        Ap = np.concatenate(([0], np.cumsum(lens)))
        nnz = int(Ap[-1])
        if m.escapes:
            rows = np.repeat(np.arange(len(lens)), lens)
            Aj = rows + (np.arange(nnz) - Ap[rows])
            esc = np.asarray(m.escapes)
            Aj[esc] = 3000 + (Aj[esc] + esc) % 1000
        else:
            pool = np.sort(rng.choice(m.n_cols, size=m.n_cols // 2, replace=False))
            Aj = pool[rng.randint(0, len(pool), size=nnz)]
        assert nnz == 0 or (Aj.min() >= 0 and Aj.max() < m.n_cols)
        if integer:
            Ax, x, y0 = rng.randint(-3, 4, size=nnz), rng.randint(-2, 3, size=m.n_cols), rng.randint(-5, 6, size=len(lens))
        else:
            Ax, x, y0 = rng.rand(nnz) * 2 - 1, rng.rand(m.n_cols) * 2 - 1, rng.rand(len(lens)) * 2 - 1
        used = np.zeros(m.n_cols, dtype=bool)
        used[Aj] = True
        _arrays[key] = (Ap, Aj.astype(np.int32), Ax.astype(np.float64), x.astype(np.float64), y0.astype(np.float64), used)
    return _arrays[key]


def operands(m, val, integer):
    """(Aj, matrix values as stored or None, the same widened to the vector type, x, y0) in the types of value case `val`."""
    t_vec, t_mat = TYPES[val]
    Ap, Aj, Ax, x, y0, used = arrays(m, integer)
    stored = None if t_mat is None else Ax.astype(t_mat)
    wide = np.ones(Aj.size, dtype=t_vec) if t_mat is None else stored.astype(t_vec)
    xv = x.astype(t_vec)
    if t_vec != np.int32:
        xv[~used] = np.nan
    return Aj, stored, wide, xv, y0.astype(t_vec)
