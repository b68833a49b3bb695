"""Structures that can be written over one another in the same device buffers, for tests/test_gpu_kept_plans.py.

The one-shot entry points find a kept plan again by the pointers and sizes of Ap / Aj (capi.hip, OneShotKey), so a plan
shaped for one structure may meet any other of the same sizes.  A GROUP here fixes (n_rows, n_cols, nnz, offset type,
value type); every structure of a group has exactly those sizes (row lengths are padded or trimmed to the group's nnz),
is deterministic, and is named after the plan shape it is meant to produce.  Nothing here needs a GPU
(tests/test_kept_structures_cpu.py checks the catalogue itself).

Every structure also carries a few PLANTED rows — not among the 256 rows the planner probes — whose first entry is
the group's NaN column or its Inf column wherever the row lies, so that those two columns are referenced from inside
a staged window (by the rows around them, in the banded structures) and from far outside any."""
import numpy as np

PROBED = 256                       # analyze.hip, probe_kernel: rows ((n - 1) * t) // 255


class Group:
    def __init__(self, name, n_rows, per_row, off, val, band_hw, stencil_gap, hub_len, head_rows, structures,
                 giant_len=1_500_000):
        self.name, self.n_rows, self.n_cols, self.per_row = name, n_rows, n_rows, per_row
        self.nnz = n_rows * per_row
        self.off, self.val = np.dtype(off), np.dtype(val)
        self.band_hw = band_hw             # half width of the group's narrow band (the liar's probed rows show the same)
        self.stencil_gap = stencil_gap     # distance between the three bands of the stencil
        self.hub_len = hub_len             # the power law's hub rows: below the giant threshold of a fresh plan
        self.head_rows = head_rows         # its heavy head: rows of 8 x per_row
        self.giant_len = min(giant_len, self.nnz // 2)
        self.structures = tuple(structures)
        self.nan_col = n_rows // 3 + 1
        self.inf_col = 2 * n_rows // 3 + 2
        self.integer_values = self.val == np.float32

    def __repr__(self):
        return self.name


# Sizes.  large: the 512- and 1 024-thread plans, the sweep, and — the reason it has 2.2 M rows rather than 1.5 M — a
# merge grid of more than 2 048 runs of 16 tiles (69 M+ items), the size from which merge_tile_kernel takes its
# coordinates from a search kernel in front (merge_plan.hip, merge_search_in_kernel).  f64: 1.2 M rows, so that the
# weight-cut plan is cut into 2 x 1 024 chunks, more than twice what stays resident: LIGHT's persistent grid.
# small32 / small8: under SMALL_PLAIN_NNZ nonzeros with two mean row lengths, i.e. two lane widths of the plain kernel.
LARGE = ("band_narrow", "band_1024", "band_sweep", "stencil", "scatter", "powerlaw", "powerlaw_band", "ragged", "giant",
         "liar")
GROUPS = {g.name: g for g in (
    Group("large", 2_200_000, 32, np.int32, np.float32, 300, 200_000, 20_000, 4096, LARGE),
    Group("f64", 1_200_000, 24, np.int64, np.float64, 4096, 150_000, 12_000, 4096,
          ("band_narrow", "stencil", "powerlaw_band", "scatter", "liar")),
    Group("small32", 100_000, 32, np.int32, np.float32, 300, 20_000, 3_000, 512,
          ("band_narrow", "stencil", "scatter", "powerlaw", "powerlaw_band", "ragged", "giant", "liar")),
    Group("small8", 200_000, 8, np.int32, np.float32, 300, 40_000, 3_000, 512,
          ("band_narrow", "stencil", "scatter", "powerlaw", "ragged", "giant", "liar")),
)}
NEVER_KEPT = ("giant",)            # a fresh plan for it holds a giant-row list: it only ever comes second, as B
# the plan shape each structure is meant to produce (reported with the structure; the census in the GPU file is what checks)
MEANT_FOR = {
    "band_narrow": "one band-placed window", "band_1024": "one band-placed window in a 1 024-thread workgroup",
    "band_sweep": "a swept window", "stencil": "a window segment per band", "scatter": "no window, equal-row chunks",
    "powerlaw": "weight-cut chunks", "powerlaw_band": "weight-cut chunks with a window",
    "ragged": "weight-cut chunks, the item walk", "giant": "a giant-row list", "liar": "whatever the narrow band takes",
}


def probed_rows(n):
    return ((n - 1) * np.arange(PROBED, dtype=np.int64)) // (PROBED - 1)


def planted_rows(n):
    """24 rows spread over the matrix, none of them probed."""
    r = ((n - 1) * (2 * np.arange(24, dtype=np.int64) + 1)) // 48 + 3
    return np.setdiff1d(np.minimum(r, n - 1), probed_rows(n))


def hub_rows(n, count=40):
    r = ((n - 1) * (2 * np.arange(count, dtype=np.int64) + 1)) // (2 * count) + 1
    return np.setdiff1d(np.minimum(r, n - 1), np.concatenate([probed_rows(n), planted_rows(n)]))


def giant_row(n):
    return n // 3 + 7


def fit_lengths(lens, total, free, lo=0, hi=None):
    """Pad or trim lens[free] (kept inside [lo, hi]) until lens sums to `total`."""
    lens = lens.astype(np.int64)
    free = np.asarray(free)
    for _ in range(64):
        diff = total - int(lens.sum())
        if diff == 0:
            return lens
        room = (hi - lens[free]) if diff > 0 else (lens[free] - lo)
        idx = free[room > 0]
        if idx.size == 0:
            break
        q, r = divmod(abs(diff), idx.size)
        step = np.full(idx.size, q, dtype=np.int64)
        step[:r] += 1
        step = np.minimum(step, room[room > 0])
        lens[idx] += step if diff > 0 else -step
    raise ValueError("row lengths cannot reach %d" % total)


def _offsets(g, lens):
    Ap = np.zeros(g.n_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    assert int(Ap[-1]) == g.nnz, (int(Ap[-1]), g.nnz)
    return Ap


def _rows_of(g, lens):
    return np.repeat(np.arange(g.n_rows, dtype=np.int32), lens)


def _band_rows(g, rows, hw, rng, k):
    """k sorted columns inside [row - hw, row + hw] for each of `rows`; shape (len(rows), k)."""
    cols = rows.astype(np.int32)[:, None] + rng.integers(-hw, hw + 1, size=(rows.size, k), dtype=np.int32)
    np.clip(cols, 0, g.n_cols - 1, out=cols)
    cols.sort(axis=1)
    return cols


def _fixed_band(g, hw, rng):
    n, k = g.n_rows, g.per_row
    cols = _band_rows(g, np.arange(n, dtype=np.int32), hw, rng, k)
    p = probed_rows(n)                         # the probe reads a row's first and last column: show it the whole band
    cols[p, 0] = np.maximum(p - hw, 0)
    cols[p, -1] = np.minimum(p + hw, n - 1)
    return np.full(n, k, dtype=np.int64), cols.reshape(-1)


def _stencil(g, rng, w=40):
    n, k, gap = g.n_rows, g.per_row, g.stencil_gap
    part = np.array([k - 2 * (k // 3), k // 3, k // 3])          # entries in the centre / lower / upper band
    centre = np.repeat(np.array([0, -gap, gap], dtype=np.int32), part)
    rows = np.arange(n, dtype=np.int32)[:, None]
    jitter = rng.integers(-w, w + 1, size=(n, k), dtype=np.int32)
    cols = rows + centre[None, :] + jitter
    outside = (cols < 0) | (cols >= n)                            # a band that leaves the matrix: those entries join the centre
    cols[outside] = np.broadcast_to(rows, cols.shape)[outside] + jitter[outside]
    np.clip(cols, 0, n - 1, out=cols)
    cols.sort(axis=1)
    return np.full(n, k, dtype=np.int64), cols.reshape(-1)


def _powerlaw_lengths(g):
    n, k = g.n_rows, g.per_row
    lens = np.zeros(n, dtype=np.int64)
    lens[:g.head_rows] = 8 * k
    hubs = hub_rows(n)
    hubs = hubs[hubs >= g.head_rows]
    lens[hubs] = g.hub_len
    rest = np.ones(n, dtype=bool)
    rest[:g.head_rows] = False
    rest[hubs] = False
    return fit_lengths(lens, g.nnz, np.nonzero(rest)[0], 0, 4 * k)


def _scattered(g, rng, count):
    return rng.integers(0, g.n_cols, size=count, dtype=np.int32)


def _liar(g, rng):
    n, k = g.n_rows, g.per_row
    p = probed_rows(n)
    p_long = (k / 2) / (100 - k / 2)       # short rows of 0..k, long ones of 0..200: the mean is the group's k
    lens = np.where(rng.random(n) >= p_long, rng.integers(0, k + 1, size=n), rng.integers(0, 201, size=n)).astype(np.int64)
    lens[p] = k
    free = np.ones(n, dtype=bool)
    free[p] = False
    free &= lens > 0                                              # (the empty rows stay empty)
    lens = fit_lengths(lens, g.nnz, np.nonzero(free)[0], 1, 200)
    Ap = _offsets(g, lens)
    Aj = _scattered(g, rng, g.nnz)
    band = _band_rows(g, p, g.band_hw, rng, k)
    band[:, 0] = np.maximum(p - g.band_hw, 0)
    band[:, -1] = np.minimum(p + g.band_hw, n - 1)
    Aj[(Ap[p][:, None] + np.arange(k)[None, :]).reshape(-1)] = band.reshape(-1)
    return lens, Aj


def build(g, name):
    """(Ap, Aj, what the structure is meant for): Ap in the group's offset type, Aj int32."""
    if name not in g.structures:
        raise KeyError("%s has no structure %s" % (g.name, name))
    n, k = g.n_rows, g.per_row
    rng = np.random.default_rng([sorted(MEANT_FOR).index(name), n, k])
    if name == "band_narrow":
        lens, Aj = _fixed_band(g, g.band_hw, rng)
    elif name == "band_1024":
        lens, Aj = _fixed_band(g, 16384 if g.val == np.float32 else 8192, rng)
    elif name == "band_sweep":
        lens, Aj = _fixed_band(g, 40_000 if g.val == np.float32 else 20_000, rng)
    elif name == "stencil":
        lens, Aj = _stencil(g, rng)
    elif name == "scatter":
        lens, Aj = np.full(n, k, dtype=np.int64), _scattered(g, rng, g.nnz)
    elif name == "powerlaw":
        lens = _powerlaw_lengths(g)
        Aj = _scattered(g, rng, g.nnz)
    elif name == "powerlaw_band":
        lens = _powerlaw_lengths(g)
        Aj = _rows_of(g, lens) + rng.integers(-1500, 1501, size=g.nnz, dtype=np.int32)
        np.clip(Aj, 0, n - 1, out=Aj)
    elif name == "ragged":
        lens = np.zeros(n, dtype=np.int64)
        full = np.nonzero(rng.random(n) >= 0.9)[0]
        lens[full] = rng.integers(5 * k, 15 * k + 1, size=full.size)
        lens = fit_lengths(lens, g.nnz, full, 1, 40 * k)
        Aj = _scattered(g, rng, g.nnz)
        Aj[1::7] = Aj[0:-1:7]                                     # duplicates, next to each other
    elif name == "giant":
        lens = np.zeros(n, dtype=np.int64)
        lens[giant_row(n)] = g.giant_len
        rest = np.ones(n, dtype=bool)
        rest[giant_row(n)] = False
        lens = fit_lengths(lens, g.nnz, np.nonzero(rest)[0], 0, 4 * k)
        Aj = _scattered(g, rng, g.nnz)
    elif name == "liar":
        lens, Aj = _liar(g, rng)
    else:
        raise KeyError(name)
    Ap = _offsets(g, lens)
    rows = planted_rows(n)
    rows = rows[lens[rows] > 0]
    Aj[Ap[rows]] = np.where(np.arange(rows.size) % 2 == 0, g.nan_col, g.inf_col).astype(np.int32)
    return Ap.astype(g.off), np.ascontiguousarray(Aj, dtype=np.int32), MEANT_FOR[name]


def values(g):
    """(Ax, x) of the cross-product tests.  fp32 groups: small integers — every sum is exact in any order (the longest
    row, 1.5 M nonzeros of magnitude <= 6, stays below 2^24); the fp64 group: uniform reals in (-1, 1)."""
    rng = np.random.default_rng([7, g.n_rows, g.per_row])
    if g.integer_values:
        return (rng.integers(-3, 4, size=g.nnz).astype(g.val), rng.integers(-2, 3, size=g.n_cols).astype(g.val))
    return (rng.random(g.nnz) * 2 - 1).astype(g.val), (rng.random(g.n_cols) * 2 - 1).astype(g.val)


def real_values(g):
    """(Ax, x) of the row-block tests (tests/test_gpu_block_shapes.py): uniform reals in (-1, 1) in the group's value
    type, the fp32 groups included — two orders of summation then give different bits — from a seed of its own."""
    rng = np.random.default_rng([9, g.n_rows, g.per_row])
    lim = np.nextafter(g.val.type(1), g.val.type(0))              # (the cast to fp32 may round up to 1)
    draw = lambda n: np.clip((rng.random(n) * 2 - 1).astype(g.val), -lim, lim)
    return draw(g.nnz), draw(g.n_cols)


def nan_values(g):
    """(Ax, x) of the NaN / Inf test: Ax in {1, 2, 3}; x = 1 except NaN at one column and +Inf at another."""
    rng = np.random.default_rng([8, g.n_rows, g.per_row])
    x = np.ones(g.n_cols, dtype=g.val)
    x[g.nan_col] = np.nan
    x[g.inf_col] = np.inf
    return rng.integers(1, 4, size=g.nnz).astype(g.val), x


# Phase variants.  A row block is a 16-byte-aligned view of the whole arrays that starts at element Ap[first row] & ~3, so
# its Ap[0] is that row's position modulo 4, its phase.  The structures with rows of one length — a multiple of 4 —
# start every row, and so every block, at phase 0; with the first d entries of row 1 gone every later row starts at
# phase (-d) & 3.  Row 1 is neither probed nor planted.  The structures of UNALIGNED have row starts of every phase as
# they are (and a row 1 that may be short or empty).
UNALIGNED = ("ragged", "giant", "liar")
SHIFT_ROW = 1


def phase_shifts(g, name):
    """The shifts d the row-block tests run a structure at: all four on the small groups, 0 and one odd d on the big
    ones (a different one each), 0 alone for the structures that are unaligned already."""
    if name in UNALIGNED:
        return (0,)
    if g.nnz <= 4_100_000:
        return (0, 1, 2, 3)
    return (0, 1) if g.val == np.float32 else (0, 3)


def phase_shifted(Ap, Aj, d):
    """(Ap, Aj) with the first d entries of row 1 deleted: n_rows as before, nnz - d nonzeros."""
    if d == 0:
        return Ap, Aj
    a = int(Ap[SHIFT_ROW])
    assert int(Ap[SHIFT_ROW + 1]) - a >= d
    Ap = Ap.copy()
    Ap[SHIFT_ROW + 1:] -= d
    return Ap, np.concatenate([Aj[:a], Aj[a + d:]])


def rows_referencing(Ap, Aj, col):
    """Boolean per row: does it hold `col`?"""
    c = np.zeros(Aj.size + 1, dtype=np.int64)
    np.cumsum(Aj == col, out=c[1:])
    Ap = Ap.astype(np.int64)
    return (c[Ap[1:]] - c[Ap[:-1]]) > 0


def nan_expected(g, Ap, Aj, Ax):
    """y = A x for nan_values(g), from the structure alone: NaN in the rows that reference the NaN column, +Inf in those
    that reference only the Inf column, the exact sum of the row's values (x = 1) everywhere else."""
    c = np.zeros(Aj.size + 1, dtype=np.float64)
    np.cumsum(Ax, dtype=np.float64, out=c[1:])
    Ap64 = Ap.astype(np.int64)
    y = (c[Ap64[1:]] - c[Ap64[:-1]]).astype(g.val)
    has_nan = rows_referencing(Ap, Aj, g.nan_col)
    has_inf = rows_referencing(Ap, Aj, g.inf_col)
    y[has_inf] = np.inf
    y[has_nan] = np.nan
    return y
