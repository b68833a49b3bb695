"""The packed index of banded VECTOR plans (include/mi355_spmv.h, MI355_PLAN_NO_INDEX_COPY).

A default VECTOR plan of a banded matrix holds one 16-bit window-relative index per nonzero and its kernel streams that
instead of Aj.  The arithmetic and its order are those of the unpacked plan, so every result here is compared BIT FOR
BIT with a plan created with MI355_PLAN_NO_INDEX_COPY, and with the oracle: fp32 matrices carry small integers (every
order of summation gives the same bits, so y equals oracle.spmv_serial exactly), fp64 ones carry reals and are held to
conftest.parity_bound.

Every test asserts from plan.info() that the plan under test IS packed and runs csr_vector_window_kernel: none of them
can pass on an unpacked plan.  The matrices have about 20 000 rows: a 256-thread plan of 128-row chunks (fp32, 32 per
row), i.e. some 150 chunks, whose first and last windows are clamped at column 0 and at n_cols.

Band: one row that the structure probe reads (analyze.hip, probe_kernel: the first and last column of 256 rows), in the
middle of its chunk, holds the columns r - 300 and r + 300 first and last, so the plan's band is [-300, 300]; every
other row stays inside [r - 298, r + 298] and below n_cols - 3.  The margins are what makes "no escapes" a fact about
these matrices: a chunk's window is its band span plus 3 elements (fp32), centred and then rounded DOWN to 16 bytes
(xwindow.hpp, place_window), so it can end up to 2 columns short of the band's upper edge, and up to 3 short of n_cols
where it is clamped there — such a column is an escape (in an unpacked plan: a gather from memory), never an error.
test_escaped_columns_... plants columns that are far outside."""
import os

import numpy as np
import pytest
import torch

from conftest import parity_bound
from small_path import forced

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HW = 300
EDGE = 2                   # columns a window may end short of the band's upper edge (see above)
TOP = 3                    # ... and of n_cols, where it is clamped there
BAND_ROW = 7842            # = (N - 1) * 100 // 255: a row the probe reads, 34 rows into its 128-row chunk
N = 20000
KERNEL = "csr_vector_window_kernel"
TORCH = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}
K_LONG_STEPS = 16          # xwindow.hpp, kLongSteps


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def probe_rows(n_rows):
    """Rows the structure probe reads (analyze.hip, probe_kernel: r = (n_rows - 1) * t / 255)."""
    return {((n_rows - 1) * t) // 255 for t in range(256)}


def band(n_rows, n_cols, lens, seed):
    """CSR structure: row r has lens[r] sorted columns inside [r - h, r + h] clipped to the matrix (repeated when the
    row is longer than the band is wide), the two ends of that range first and last; h = HW for BAND_ROW, HW - EDGE for
    the others."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    Ap = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=Ap[1:])
    row = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    pos = np.arange(Ap[-1], dtype=np.int64) - Ap[row]
    half = np.full(n_rows, HW - EDGE, dtype=np.int64)
    assert BAND_ROW in probe_rows(n_rows) and lens[BAND_ROW] > 1
    half[BAND_ROW] = HW
    lo = np.maximum(row - half[row], 0)
    hi = np.minimum(row + half[row], n_cols - 1 - TOP)
    # position i of a row of length L sits in the i-th of L equal slices of [lo, hi]
    width = hi - lo + 1
    L = lens[row]
    a = lo + pos * width // L
    b = lo + (pos + 1) * width // L
    Aj = a + (rng.random(Ap[-1]) * np.maximum(b - a, 1)).astype(np.int64)
    Aj = np.minimum(Aj, hi)
    Aj[pos == 0] = lo[pos == 0]
    last = pos == L - 1
    Aj[last & (L > 1)] = hi[last & (L > 1)]
    return Ap, Aj.astype(np.int32)


class Matrix:
    """A structure on the device with its values, x, and the oracle's answers (computed once, never changed)."""

    def __init__(self, oracle, n_rows, n_cols, lens, seed, val=np.float32, off=np.int32, plant=None):
        Ap, Aj = band(n_rows, n_cols, lens, seed)
        self.planted = plant(Ap, Aj, n_cols) if plant else 0
        rng = np.random.default_rng(seed + 1)
        nnz = int(Ap[-1])
        if val == np.float32:       # small integers: sums are exact
            Ax = rng.integers(-3, 4, size=nnz).astype(val)
            x = rng.integers(-4, 5, size=n_cols).astype(val)
        else:
            Ax = (rng.random(nnz) * 2 - 1).astype(val)
            x = (rng.random(n_cols) * 2 - 1).astype(val)
        Ap = Ap.astype(off)
        self.n_rows, self.n_cols, self.nnz, self.val, self.dt = n_rows, n_cols, nnz, val, TORCH[val]
        self.h_Ap = Ap.astype(np.int64)
        self.Ap, self.Aj, self.Ax, self.x = dev(Ap), dev(Aj), dev(Ax), dev(x)
        if val == np.float32:
            self.serial = dev(oracle.spmv_serial(Ap, Aj, Ax, x))
        else:
            y64, bound = parity_bound(oracle, Ap, Aj, Ax, x, 8)
            self.y64, self.bound = dev(y64), dev(bound)

    def plan(self, sp, flags=0):
        return sp.Plan("vector", self.n_rows, self.n_cols, self.nnz, self.Ap, self.Aj, self.dt, flags=flags)

    def poisoned(self):
        return torch.full((self.n_rows,), float("nan"), dtype=self.dt, device=DEV)

    def run(self, plan):
        y = plan.execute(self.Ax, self.x, self.poisoned())
        torch.cuda.synchronize()
        return y

    def check_oracle(self, y, what):
        assert not torch.isnan(y).any(), "%s: NaN left in y" % what
        if self.val == np.float32:
            bad = torch.nonzero(y != self.serial).flatten()
            assert bad.numel() == 0, "%s: %d rows differ from the serial oracle, first %s: got %s, want %s" % (
                what, bad.numel(), bad[:5].tolist(), y[bad[:5]].tolist(), self.serial[bad[:5]].tolist())
        else:
            bad = torch.nonzero(~((y - self.y64).abs() <= self.bound)).flatten()
            assert bad.numel() == 0, "%s: %d rows outside the parity bound, first %s" % (what, bad.numel(), bad[:5].tolist())


def assert_packed(plan, m, escapes=0):
    """The precondition of every test: the plan holds a packed index and runs the banded kernel."""
    info = plan.info()
    assert not forced(), "a MI355_* knob forces a code path: %s" % info["knobs"]
    assert info["main_kernel"] == KERNEL, info
    assert info["window_elems"] > 0 and info["window_segments"] == 1 and info["balanced_chunks"] == 0, info
    assert info["packed_index_bytes"] >= 2 * m.nnz, info
    assert info["packed_index_bytes"] <= 2 * m.nnz + 512, info
    assert info["scratch_bytes"] >= info["packed_index_bytes"], info
    assert info["packed_index_escapes"] == escapes, info
    return info


def assert_unpacked(plan):
    info = plan.info()
    assert info["packed_index_bytes"] == 0 and info["packed_index_escapes"] == 0, info
    return info


def check_against_unpacked(sp, m, what, escapes=0):
    """Packed against the oracle and, bit for bit, against a plan that holds no index copy."""
    packed = m.plan(sp)
    plain = m.plan(sp, flags=sp.capi.PLAN_NO_INDEX_COPY)
    try:
        info = assert_packed(packed, m, escapes)
        info0 = assert_unpacked(plain)
        assert info0["main_kernel"] == KERNEL, info0
        for f in ("lanes_per_row", "block_threads", "rows_per_chunk", "window_elems", "n_chunks"):
            assert info[f] == info0[f], (f, info, info0)
        y = m.run(packed)
        m.check_oracle(y, what)
        y0 = m.run(plain)
        bad = torch.nonzero(y != y0).flatten()
        assert bad.numel() == 0, "%s: %d rows differ from the unpacked plan, first %s; %s" % (
            what, bad.numel(), bad[:5].tolist(), info)
        return info, y
    finally:
        packed.destroy()
        plain.destroy()


_CACHE = {}


def matrix(oracle, key, *args, **kw):
    if key not in _CACHE:
        _CACHE[key] = Matrix(oracle, *args, **kw)
    return _CACHE[key]


def band32(oracle, val=np.float32, off=np.int32, n_cols=N):
    return matrix(oracle, ("band32", val, off, n_cols), N, n_cols, np.full(N, 32), 11, val=val, off=off)


def lens27(empty):
    lens = np.full(N, 27)
    if empty:
        lens[[0, 5, 4097, 4098, 12345, N - 1]] = 0      # (the first and last rows among them)
        lens[777] = 26                                   # ... and nnz % 4 != 0
    return lens


def band27(oracle, empty=False):
    m = matrix(oracle, ("band27", empty), N, N, lens27(empty), 27)
    assert (m.nnz % 4 != 0) == empty
    return m


# 1. the band itself: three type combinations, square and not
@pytest.mark.parametrize("val,off", [(np.float32, np.int32), (np.float32, np.int64), (np.float64, np.int32)],
                         ids=["f32-i32", "f32-i64", "f64-i32"])
@pytest.mark.parametrize("n_cols", [N, N - 200], ids=["square", "fewer-cols"])
def test_band_equals_oracle_and_unpacked_plan(sp, oracle, val, off, n_cols):
    m = band32(oracle, val, off, n_cols)
    info, _ = check_against_unpacked(sp, m, "band32 %s" % n_cols)
    # the first and the last chunk's windows are clamped at column 0 and at n_cols: the band reaches past both
    assert info["rows_per_chunk"] < N and 0 - HW < 0 and (N - 1) + HW >= m.n_cols


# 2. rows that are not whole 16-byte groups: 27 per row; empty rows and a partial last group
@pytest.mark.parametrize("empty", [False, True], ids=["27", "27-empty-rows-tail"])
def test_rows_that_straddle_groups_and_chunks(sp, oracle, empty):
    check_against_unpacked(sp, band27(oracle, empty), "band27 empty=%s" % empty)


# 3. columns outside every window
def test_escaped_columns_are_counted_and_read_from_aj(sp, oracle):
    rows = [5003 + 997 * i for i in range(9)]
    assert not set(rows) & probe_rows(N)

    def plant(Ap, Aj, n_cols):
        for i, r in enumerate(rows):       # a middle position of the row: its first and last column keep the band
            Aj[Ap[r] + 5 + i] = 0 if i % 2 == 0 else n_cols - 1
        return len(rows)

    m = matrix(oracle, "escapes", N, N, np.full(N, 32), 11, plant=plant)
    assert m.planted == 9 and min(rows) > 2 * HW + 2048 and max(rows) < N - 2 * HW - 2048   # far outside any window
    check_against_unpacked(sp, m, "escapes", escapes=m.planted)


# 4. long rows: beyond one step of the row's vector, and beyond kLongSteps steps (the long-row pass reads Aj)
def test_long_rows_inside_a_packed_plan(sp, oracle):
    lens = np.full(N, 32)
    lens[3001] = 100
    lens[9002] = 700
    lens[15000:15023] = 0      # (as many nonzeros fewer: the mean row, and with it the lanes per row, stay at 32 / 8)
    m = matrix(oracle, "long", N, N, lens, 13)
    info, _ = check_against_unpacked(sp, m, "long rows")
    step = 4 * info["lanes_per_row"]
    assert 100 > step and 100 <= K_LONG_STEPS * step < 700, info


# 5. kept plans and the knob
def test_kept_plans_and_the_knob_hold_no_index(sp, oracle):
    m = band32(oracle)
    sp.capi.cache_release()
    p = sp.Plan.acquire("vector", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, m.dt)
    info = assert_unpacked(p)
    assert info["main_kernel"] == KERNEL, info
    p.release()
    sp.capi.cache_release()
    y = m.poisoned()
    sp.spmv("vector", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, m.Ax, m.x, y)
    m.check_oracle(y, "one-shot")
    p = sp.Plan.acquire("vector", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, m.dt)      # the plan that call kept
    assert_unpacked(p)
    p.release()
    sp.capi.cache_release()

    assert "MI355_SPMV_PACK" not in os.environ
    os.environ["MI355_SPMV_PACK"] = "0"
    sp.capi.lib().mi355_spmv_knobs_reload()
    try:
        p = m.plan(sp)
        info = assert_unpacked(p)
        assert "MI355_SPMV_PACK=0" in info["knobs"], info
        m.check_oracle(m.run(p), "MI355_SPMV_PACK=0")
        p.destroy()
    finally:
        del os.environ["MI355_SPMV_PACK"]
        sp.capi.lib().mi355_spmv_knobs_reload()
    p = m.plan(sp)
    assert_packed(p, m)
    p.destroy()


# 6. row blocks: every block packed, the concatenated y the whole plan's
def test_blocks_are_packed_and_equal_the_whole_plan(sp, oracle):
    m = band27(oracle, empty=True)
    whole = m.plan(sp)
    blocks = []
    try:
        assert_packed(whole, m)
        y1 = m.run(whole)
        m.check_oracle(y1, "whole plan")
        shape = whole.shape()
        rows, chunks, nnzs = whole.partition(3)
        assert len(rows) == 4 and all(b > a for a, b in zip(rows, rows[1:])), rows
        phases = set()
        y = m.poisoned()
        for b in range(3):
            r0, r1 = rows[b], rows[b + 1]
            a, j, _, lo = sp.dist.block_view(m.Ap, m.Aj, m.Ax, r0, r1)
            nnz_end = int(m.h_Ap[r1]) - lo
            plan = sp.Plan.block("vector", shape, r0, chunks[b], chunks[b + 1] - chunks[b], nnzs[b], r1 - r0, m.n_cols,
                                 nnz_end, a, j, m.dt)
            blocks.append(plan)
            info = plan.info()
            assert info["main_kernel"] == KERNEL and info["packed_index_bytes"] >= 2 * nnz_end, (b, info)
            assert info["packed_index_escapes"] == 0, (b, info)
            phases.add(nnzs[b] & 3)
            plan.execute(m.Ax[lo:lo + nnz_end], m.x, y[r0:r1])
        torch.cuda.synchronize()
        assert phases - {0}, "every block starts at 16-byte phase 0: %s" % nnzs
        bad = torch.nonzero(y != y1).flatten()
        assert bad.numel() == 0, "%d rows of the blocks differ from the whole plan, first %s" % (bad.numel(), bad[:5].tolist())
    finally:
        for plan in blocks:
            plan.destroy()
        whole.destroy()


# 7. alpha / beta and a captured, replayed execute
def test_alpha_beta_and_graph_replay_equal_the_unpacked_plan(sp, oracle):
    m = band32(oracle)
    packed, plain = m.plan(sp), m.plan(sp, flags=sp.capi.PLAN_NO_INDEX_COPY)
    try:
        assert_packed(packed, m)
        assert_unpacked(plain)
        y_old = dev(np.random.default_rng(5).integers(-8, 9, size=m.n_rows).astype(np.float32))
        got = []
        for p in (packed, plain):
            p.set_alpha_beta(2.0, -1.0)
            got.append(p.execute(m.Ax, m.x, y_old.clone()))
            p.set_alpha_beta(1.0, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(got[0], got[1])
        assert torch.equal(got[0], 2.0 * m.serial - y_old)     # (small integers: exact)

        y = m.poisoned()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            packed.execute(m.Ax, m.x, y, stream=s)             # warm-up outside the capture
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                packed.execute(m.Ax, m.x, y, stream=s)
            y.fill_(float("nan"))
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, m.run(plain))
        m.check_oracle(y, "graph replay")
    finally:
        packed.destroy()
        plain.destroy()
