"""The structure catalogue of tests/kept_structures.py, checked without a GPU: what the GPU tests of kept one-shot
plans (tests/test_gpu_kept_plans.py) and of row-block plans (tests/test_gpu_block_shapes.py) assume about their inputs
holds before anything goes to a device."""
import numpy as np
import pytest

import kept_structures as ks

CASES = [(g.name, s) for g in ks.GROUPS.values() for s in g.structures]


@pytest.fixture(scope="module")
def group_values():
    cache = {}

    def get(g):
        if g.name not in cache:
            cache.clear()                       # one group's values at a time
            cache[g.name] = ks.values(g)
        return cache[g.name]
    return get


def test_groups_hold_what_the_gpu_tests_need():
    from small_path import SMALL_PLAIN_NNZ
    assert set(ks.GROUPS) >= {"large", "f64", "small32", "small8"}
    large, f64 = ks.GROUPS["large"], ks.GROUPS["f64"]
    assert large.off == np.int32 and large.val == np.float32 and f64.off == np.int64 and f64.val == np.float64
    assert set(large.structures) >= {"band_narrow", "band_1024", "band_sweep", "stencil", "scatter", "powerlaw", "ragged",
                                     "giant", "liar"}
    assert set(f64.structures) >= {"band_narrow", "stencil", "scatter", "liar"} and \
        {"powerlaw", "powerlaw_band"} & set(f64.structures)
    for name in ("small32", "small8"):
        g = ks.GROUPS[name]
        assert g.nnz <= SMALL_PLAIN_NNZ and g.off == np.int32 and g.val == np.float32
    assert ks.GROUPS["small32"].per_row != ks.GROUPS["small8"].per_row       # two lane widths of the plain kernel
    for g in ks.GROUPS.values():
        n = g.n_rows
        assert len(set(ks.probed_rows(n))) == ks.PROBED
        assert not set(ks.planted_rows(n)) & set(ks.probed_rows(n)) and ks.planted_rows(n).size >= 16
        assert not set(ks.hub_rows(n)) & (set(ks.probed_rows(n)) | set(ks.planted_rows(n)))
        assert ks.giant_row(n) not in set(ks.probed_rows(n)) | set(ks.planted_rows(n))
        assert g.nan_col != g.inf_col and 0 <= g.nan_col < g.n_cols and 0 <= g.inf_col < g.n_cols


@pytest.mark.parametrize("group", list(ks.GROUPS))
def test_real_values_are_reals_in_every_group(group):
    """The values of the row-block tests: reals strictly inside (-1, 1) in the group's type — the fp32 groups too, whose
    cross-product values are integers that sum to the same bits in any order — deterministic, of a seed of their own."""
    g = ks.GROUPS[group]
    Ax, x = ks.real_values(g)
    assert Ax.dtype == g.val and x.dtype == g.val and Ax.shape == (g.nnz,) and x.shape == (g.n_cols,)
    for a in (Ax, x):
        assert np.abs(a).max() < 1 and a.min() < -0.99 and a.max() > 0.99 and abs(float(a.mean(dtype=np.float64))) < 0.01
        assert np.unique(a[:1000]).size > 990 and np.count_nonzero(a[:1000] == np.round(a[:1000])) == 0
    Ax2, x2 = ks.real_values(g)
    assert np.array_equal(Ax, Ax2) and np.array_equal(x, x2)
    del Ax2, x2
    old_Ax, old_x = ks.values(g)
    assert not np.array_equal(Ax[:1000], old_Ax[:1000]) and not np.array_equal(x[:1000], old_x[:1000])
    # what the integers cannot show: one row of per_row products summed forwards and backwards differs in some row
    k = g.per_row
    prod = (Ax[:1000 * k] * x[np.arange(1000 * k) % g.n_cols]).reshape(1000, k)
    fwd, bwd = np.zeros(1000, dtype=g.val), np.zeros(1000, dtype=g.val)
    for j in range(k):
        fwd += prod[:, j]
        bwd += prod[:, k - 1 - j]
    assert np.count_nonzero(fwd != bwd) > 100


def check_phase_shifts(g, name, Ap, Aj):
    """ks.phase_shifted at every shift the row-block tests use for this structure: row 1 loses its first d entries and
    nothing else changes — not the sizes but for d, not a probed or planted row — and every later row start, so every cut
    a partition can make, has phase (its old phase - d) & 3."""
    from small_path import SMALL_PLAIN_NNZ
    n = g.n_rows
    Ap64 = Ap.astype(np.int64)
    lens = np.diff(Ap64)
    shifts = ks.phase_shifts(g, name)
    special = np.concatenate([ks.probed_rows(n), ks.planted_rows(n)])
    assert ks.SHIFT_ROW == 1 and ks.SHIFT_ROW not in set(special.tolist()) and shifts[0] == 0
    starts = Ap64[:-1][lens > 0]
    if name in ks.UNALIGNED:
        assert shifts == (0,)
        assert set((starts & 3).tolist()) == {0, 1, 2, 3}           # unaligned as they are
    else:
        assert lens[ks.SHIFT_ROW] >= 8
        assert set(shifts) == {0, 1, 2, 3} if g.nnz <= SMALL_PLAIN_NNZ else (len(shifts) >= 2 and all(0 <= d <= 3 for d in shifts))
    if name in ("band_narrow", "band_1024", "band_sweep", "stencil", "scatter"):
        assert not np.any(starts & 3)                               # rows of one length, a multiple of 4: phase 0 only
    sample = np.concatenate([special, np.arange(0, n, max(1, n // 500)), [0, 1, 2, n - 1]])
    for d in shifts[1:]:
        Ap_d, Aj_d = ks.phase_shifted(Ap, Aj, d)
        assert Ap_d.dtype == Ap.dtype and Aj_d.dtype == Aj.dtype and Ap_d.shape == Ap.shape
        assert int(Ap_d[0]) == 0 and int(Ap_d[-1]) == g.nnz - d == Aj_d.size
        assert (g.nnz - d <= SMALL_PLAIN_NNZ) == (g.nnz <= SMALL_PLAIN_NNZ)  # a small group stays one, a big one big
        Ad64 = Ap_d.astype(np.int64)
        lens_d = np.diff(Ad64)
        assert lens_d[ks.SHIFT_ROW] == lens[ks.SHIFT_ROW] - d and np.count_nonzero(lens_d != lens) == 1
        assert np.array_equal(Ad64[:2], Ap64[:2]) and np.array_equal(Ad64[2:], Ap64[2:] - d)
        if name not in ks.UNALIGNED and name in ("band_narrow", "band_1024", "band_sweep", "stencil", "scatter"):
            assert set((Ad64[2:-1] & 3).tolist()) == {(-d) & 3}       # every row start after row 1: one non-zero phase
        assert np.array_equal(Aj_d[:Ad64[1]], Aj[:Ap64[1]]) and np.array_equal(Aj_d[Ad64[2]:], Aj[Ap64[2]:])
        assert np.array_equal(Aj_d[Ad64[1]:Ad64[2]], Aj[Ap64[1] + d:Ap64[2]])
        for r in sample:                                            # the probed and planted rows: as they were
            if r != ks.SHIFT_ROW:
                assert np.array_equal(Aj_d[Ad64[r]:Ad64[r + 1]], Aj[Ap64[r]:Ap64[r + 1]]), (name, d, r)
    Ap_0, Aj_0 = ks.phase_shifted(Ap, Aj, 0)
    assert Ap_0 is Ap and Aj_0 is Aj


@pytest.mark.parametrize("group,name", CASES)
def test_structure(group, name, group_values):
    g = ks.GROUPS[group]
    Ap, Aj, meant = ks.build(g, name)
    n, k = g.n_rows, g.per_row
    # the group's sizes and types, valid CSR
    assert meant and Ap.dtype == g.off and Aj.dtype == np.int32
    assert Ap.shape == (n + 1,) and Aj.shape == (g.nnz,) and int(Ap[0]) == 0 and int(Ap[-1]) == g.nnz
    lens = np.diff(Ap.astype(np.int64))
    assert lens.min() >= 0
    assert int(Aj.min()) >= 0 and int(Aj.max()) < g.n_cols
    # deterministic
    if g.nnz <= 4_000_000:
        Ap2, Aj2, _ = ks.build(g, name)
        assert np.array_equal(Ap, Ap2) and np.array_equal(Aj, Aj2)
    Ap64 = Ap.astype(np.int64)
    probed = ks.probed_rows(n)

    def offsets_of(rows):
        idx = np.concatenate([np.arange(Ap64[r], Ap64[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
        return Aj[idx].astype(np.int64) - np.repeat(rows, lens[rows])

    if name in ("band_narrow", "band_1024", "band_sweep"):
        hw = {"band_narrow": g.band_hw, "band_1024": 16384 if g.val == np.float32 else 8192,
              "band_sweep": 40_000 if g.val == np.float32 else 20_000}[name]
        assert lens.min() == lens.max() == k
        off = offsets_of(probed)
        assert off.min() == -hw and off.max() == hw               # the probe sees the whole band
        assert np.abs(offsets_of(np.setdiff1d(np.arange(0, n, 997), ks.planted_rows(n)))).max() <= hw
    if name == "stencil":
        assert lens.min() == lens.max() == k
        off = offsets_of(np.setdiff1d(np.arange(g.stencil_gap + 100, n - g.stencil_gap - 100, 1009), ks.planted_rows(n)))
        bands = np.round(off / g.stencil_gap).astype(np.int64)
        assert set(bands.tolist()) == {-1, 0, 1} and np.abs(off - bands * g.stencil_gap).max() <= 40
    if name == "scatter":
        assert lens.min() == lens.max() == k
    if name in ("powerlaw", "powerlaw_band"):
        hubs = ks.hub_rows(n)
        hubs = hubs[hubs >= g.head_rows]
        assert hubs.size >= 30 and np.all(lens[hubs] == g.hub_len)
        assert np.all(lens[:g.head_rows] == 8 * k)
        # below the threshold from which a fresh plan would cut a row into slices (rows_plan.hip, find_giant_rows)
        fair = max(4096, min(65536, (g.nnz // 2048 + 1023) & ~1023))
        assert lens.max() == g.hub_len < fair
    if name == "ragged":
        assert np.count_nonzero(lens == 0) >= 0.88 * n and lens[lens > 0].min() >= k
        r = int(np.argmax(lens))
        row = Aj[Ap64[r]:Ap64[r + 1]]
        assert np.any(np.diff(row) < 0) and np.unique(row).size < row.size        # unsorted, with duplicates
    if name == "giant":
        assert lens[ks.giant_row(n)] == g.giant_len > 65536 and np.count_nonzero(lens > 4 * k) == 1
    if name == "liar":
        # what the planner probes looks like the narrow band ...
        assert np.all(lens[probed] == k)
        off = offsets_of(probed)
        assert off.min() == -g.band_hw and off.max() == g.band_hw
        first, last = Aj[Ap64[probed]], Aj[Ap64[probed + 1] - 1]
        assert np.all(np.abs(first - probed) <= g.band_hw) and np.all(np.abs(last - probed) <= g.band_hw)
        # ... and nothing else does
        others = np.setdiff1d(np.arange(1, n, 499), probed)
        others = others[lens[others] > 0]
        assert np.mean(np.abs(offsets_of(others)) > 10 * g.band_hw) > 0.5
        assert lens.min() == 0 and 150 <= lens.max() <= 200 and np.count_nonzero(lens == 0) > n // 200
    check_phase_shifts(g, name, Ap, Aj)
    # the NaN and Inf columns: referenced, from far away at least (the planted rows), and in the banded structures
    # from the rows around them too
    for col in (g.nan_col, g.inf_col):
        rows = np.nonzero(ks.rows_referencing(Ap, Aj, col))[0]
        assert rows.size >= 1
        assert np.any(np.abs(rows - col) > n // 8), name
        if name in ("band_narrow", "band_1024", "band_sweep", "stencil", "powerlaw_band"):
            f32 = g.val == np.float32
            near = {"band_narrow": g.band_hw, "band_1024": 16384 if f32 else 8192, "band_sweep": 40_000 if f32 else 20_000,
                    "stencil": 40, "powerlaw_band": 1500}[name]
            assert np.any(np.abs(rows - col) <= near), name       # (inside the structure's own band)
    has_nan = ks.rows_referencing(Ap, Aj, g.nan_col)
    assert np.any(ks.rows_referencing(Ap, Aj, g.inf_col) & ~has_nan) and not np.all(has_nan)
    # integer groups: every partial sum of every row is an integer below 2^24
    Ax, x = group_values(g)
    if g.integer_values:
        assert np.all(Ax == np.round(Ax)) and np.abs(Ax).max() <= 3 and np.abs(x).max() <= 2
        c = np.zeros(g.nnz + 1, dtype=np.float64)
        np.cumsum(np.abs(Ax.astype(np.float64) * x[Aj]), out=c[1:])
        assert (c[Ap64[1:]] - c[Ap64[:-1]]).max() < 2 ** 24
    else:
        assert np.abs(Ax).max() < 1 and np.abs(x).max() < 1 and np.unique(Ax[:1000]).size > 900
    # the NaN / Inf expectation agrees with a plain per-row evaluation on a sample of rows
    Axn, xn = ks.nan_values(g)
    want = ks.nan_expected(g, Ap, Aj, Axn)
    sample = np.concatenate([np.nonzero(has_nan)[0][:20], ks.planted_rows(n), np.arange(0, n, max(1, n // 200))])
    with np.errstate(invalid="ignore"):
        for r in sample:
            s = np.sum(Axn[Ap64[r]:Ap64[r + 1]].astype(np.float64) * xn[Aj[Ap64[r]:Ap64[r + 1]]].astype(np.float64))
            assert (np.isnan(s) and np.isnan(want[r])) or s == want[r], (name, r)
