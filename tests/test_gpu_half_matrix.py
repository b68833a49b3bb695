"""Matrix values stored in 16 bits (fp16 / bf16) under fp32 x and y on the vector kind (include/mi355_spmv.h,
MI355_VAL_F16 / MI355_VAL_BF16).

Every value is made by rounding fp32 data to the 16-bit type ON THE HOST (np.float16; torch.bfloat16); `widened` is
those 16-bit values cast back to fp32, which is exact.  A 16-bit plan is the fp32 vector plan of the same structure and
flags with another stored type, so on the shapes the 16-bit chunked kernels are built for — equal-row chunks with one
window of x or none, 256 / 512 / 1 024 threads, with the packed index and without — its shape is the fp32 plan's byte
for byte and its y equals the fp32 plan's y on `widened` BIT FOR BIT.  Every other shape runs the plain one-pass kernel
and is held to conftest.parity_bound.

Every test first asserts from plan.info() / plan.shape() the kernel and the shape it means to exercise, and that no
MI355_* knob forces a code path.

Matrices.  The ~20 000-row bands of tests/test_gpu_packed_index.py (half width 300, 32 per row, a planted probe row with
its margins, so that "packed, no escapes" is a fact about them; the generator is written again below), 256-thread plans.
The 512-thread, the 1 024-thread and the no-window shape: large/band_narrow, large/band_1024 and small8/scatter of
tests/kept_structures.py, the smallest structures tests/test_gpu_block_shapes.py has for those census lines."""
import numpy as np
import pytest
import torch

import kept_structures as ks
from conftest import parity_bound
from plan_census import one_band
from small_path import forced, small_on  # noqa: F401  (small_on: a fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HW = 300
EDGE = 2                   # columns a window may end short of the band's upper edge (xwindow.hpp, place_window)
TOP = 3                    # ... and of n_cols, where it is clamped there
BAND_ROW = 7842            # = (N - 1) * 100 // 255: a row the probe reads, 34 rows into its 128-row chunk
N = 20000
WINDOW = "csr_vector_window_kernel"
PLAIN = "csr_vector_kernel"
K_LONG_STEPS = 16          # xwindow.hpp, kLongSteps
K_HUGE_ROW = 1024          # xwindow.hpp, kHugeRow
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
MAT_CODE = {torch.float16: 4, torch.bfloat16: 5}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rounded(a32, dtype):
    """(the 16-bit values on the device, `widened` on the host) of fp32 host data, rounded on the host."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if dtype == torch.float16:
        h = a32.astype(np.float16)
        return dev(h), h.astype(np.float32)
    h = torch.from_numpy(a32).to(torch.bfloat16)
    return h.to(DEV), h.to(torch.float32).numpy()


def probe_rows(n_rows):
    """Rows the structure probe reads (analyze.hip, probe_kernel: r = (n_rows - 1) * t / 255)."""
    return {((n_rows - 1) * t) // 255 for t in range(256)}


def band(n_rows, n_cols, lens, seed):
    """CSR structure: row r has lens[r] sorted columns inside [r - h, r + h] clipped to the matrix (repeated when the
    row is longer than the band is wide), the two ends of that range first and last; h = HW for BAND_ROW, HW - EDGE for
    the others, and nothing above n_cols - 1 - TOP."""
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
    width = hi - lo + 1
    L = lens[row]
    a = lo + pos * width // L          # position i of a row of length L sits in the i-th of L equal slices of [lo, hi]
    b = lo + (pos + 1) * width // L
    Aj = a + (rng.random(Ap[-1]) * np.maximum(b - a, 1)).astype(np.int64)
    Aj = np.minimum(Aj, hi)
    Aj[pos == 0] = lo[pos == 0]
    last = pos == L - 1
    Aj[last & (L > 1)] = hi[last & (L > 1)]
    return Ap, Aj.astype(np.int32)


class Matrix:
    """A structure on the device with fp32 source values, x, and per 16-bit type the rounded values, `widened`, and the
    oracle's answers for `widened` (each computed once, never changed)."""

    def __init__(self, oracle, Ap, Aj, n_cols, seed, off=np.int32, integers=False, values=None):
        self.oracle, self.integers = oracle, integers
        self.n_rows, self.n_cols, self.nnz = Ap.size - 1, n_cols, int(Ap[-1])
        rng = np.random.default_rng(seed)
        if values is not None:
            self.h_Ax, self.h_x = values
        elif integers:             # small integers: exact in both 16-bit types, and every order of summation gives the same bits
            self.h_Ax = rng.integers(-3, 4, size=self.nnz).astype(np.float32)
            self.h_x = rng.integers(-4, 5, size=n_cols).astype(np.float32)
        else:
            self.h_Ax = (rng.random(self.nnz) * 2 - 1).astype(np.float32)
            self.h_x = (rng.random(n_cols) * 2 - 1).astype(np.float32)
        self.h_Ap, self.h_Aj = Ap.astype(off), Aj
        self.Ap, self.Aj, self.x = dev(self.h_Ap), dev(Aj), dev(self.h_x)
        self._typed = {}

    def typed(self, dtype):
        """(Ax16 on the device, widened on the device, reference) — reference: the serial oracle's y for integer values,
        (y64, bound) of conftest.parity_bound for reals, both on `widened`."""
        if dtype not in self._typed:
            Ax16, widened = rounded(self.h_Ax, dtype)
            if self.integers:
                assert np.array_equal(widened, self.h_Ax)
                want = dev(self.oracle.spmv_serial(self.h_Ap, self.h_Aj, widened, self.h_x))
            else:
                y64, bound = parity_bound(self.oracle, self.h_Ap, self.h_Aj, widened, self.h_x, 8)
                want = (dev(y64), dev(bound))
            self._typed[dtype] = (Ax16, dev(widened), want)
        return self._typed[dtype]

    def plan(self, sp, dtype=None, flags=0, kind="vector"):
        """The 16-bit plan of `dtype`, or the fp32 plan (dtype None)."""
        return sp.Plan(kind, self.n_rows, self.n_cols, self.nnz, self.Ap, self.Aj, torch.float32, flags=flags, mat_dtype=dtype)

    def poisoned(self):
        return torch.full((self.n_rows,), float("nan"), dtype=torch.float32, device=DEV)

    def run(self, plan, Ax, x=None):
        y = plan.execute(Ax, self.x if x is None else x, self.poisoned())
        torch.cuda.synchronize()
        return y

    def check_oracle(self, y, dtype, what):
        assert not torch.isnan(y).any(), "%s: NaN left in y" % what
        want = self.typed(dtype)[2]
        if self.integers:
            bad = torch.nonzero(y != want).flatten()
            assert bad.numel() == 0, "%s: %d rows differ from the serial oracle, first %s: got %s, want %s" % (
                what, bad.numel(), bad[:5].tolist(), y[bad[:5]].tolist(), want[bad[:5]].tolist())
        else:
            y64, bound = want
            bad = torch.nonzero(~((y.to(torch.float64) - y64).abs() <= bound)).flatten()
            assert bad.numel() == 0, "%s: %d rows outside the parity bound, first %s: got %s, oracle %s" % (
                what, bad.numel(), bad[:5].tolist(), y[bad[:5]].tolist(), y64[bad[:5]].tolist())


_CACHE = {}


def cached(key, make, big=False):
    """Built once per session; one `big` matrix (2.2 M rows) at a time."""
    if key not in _CACHE:
        if big:
            for k in [k for k, (_, was_big) in _CACHE.items() if was_big]:
                del _CACHE[k]
            torch.cuda.empty_cache()
        _CACHE[key] = (make(), big)
    return _CACHE[key][0]


def band32(oracle, off=np.int32, integers=False):
    def make():
        Ap, Aj = band(N, N, np.full(N, 32), 11)
        return Matrix(oracle, Ap, Aj, N, 12, off=off, integers=integers)
    return cached(("band32", off, integers), make)


def catalogue(oracle, gname, name):
    """A structure of tests/kept_structures.py with that catalogue's real values."""
    def make():
        g = ks.GROUPS[gname]
        Ap, Aj, _ = ks.build(g, name)
        return Matrix(oracle, Ap.astype(np.int64), Aj, g.n_cols, 0, off=g.off.type, values=ks.real_values(g))
    return cached((gname, name), make, big=ks.GROUPS[gname].n_rows > 1_000_000)


def fields(sh):
    return {f: getattr(sh, f) if isinstance(getattr(sh, f), int) else list(getattr(sh, f)) for f, _ in sh._fields_}


def assert_fast_path(plan, dtype, threads, window, packed, escapes=None):
    """The precondition of every fast-path test: the plan stores `dtype`, computes in fp32 and runs the chunked kernel
    of the asked shape."""
    info, sh = plan.info(), plan.shape()
    assert not forced(), "a MI355_* knob forces a code path: %s" % info["knobs"]
    assert plan.mat_type() == MAT_CODE[dtype] and info["val_type"] == 0 and sh.val_type == 0, info
    assert info["main_kernel"] == WINDOW and info["n_kernels"] == 1 and info["balanced_chunks"] == 0, info
    assert info["block_threads"] == threads and sh.small_plain == 0 and sh.window_sweep == 0, info
    if window:
        assert one_band("vector", threads)("vector", info, {"window_from_band": sh.window_from_band}), (info, fields(sh))
    else:
        assert info["window_elems"] == 0 and info["window_segments"] == 0, info
    if packed:
        assert 2 * plan.nnz <= info["packed_index_bytes"] <= 2 * plan.nnz + 512, info
        if escapes is not None:
            assert info["packed_index_escapes"] == escapes, info
    else:
        assert info["packed_index_bytes"] == 0 and info["packed_index_escapes"] == 0, info
    return info, sh


def check_against_fp32(sp, m, dtype, flags, threads, window, packed, what, escapes=None):
    """The 16-bit plan against the fp32 plan of the same flags on `widened` (shape byte for byte, y bit for bit) and
    against the oracle."""
    Ax16, widened, _ = m.typed(dtype)
    p16, p32 = m.plan(sp, dtype, flags), m.plan(sp, None, flags)
    try:
        info, sh = assert_fast_path(p16, dtype, threads, window, packed, escapes)
        info32, sh32 = p32.info(), p32.shape()
        assert bytes(sh) == bytes(sh32), "%s: the 16-bit plan's shape differs from the fp32 plan's: %s, fp32 %s" % (
            what, fields(sh), fields(sh32))
        assert info == info32, "%s: the 16-bit plan's info differs from the fp32 plan's: %s, fp32 %s" % (what, info, info32)
        y = m.run(p16, Ax16)
        y32 = m.run(p32, widened)
        bad = torch.nonzero(y != y32).flatten()
        assert bad.numel() == 0, "%s: %d rows differ from the fp32 plan on the widened values, first %s: got %s, fp32 %s; %s" % (
            what, bad.numel(), bad[:5].tolist(), y[bad[:5]].tolist(), y32[bad[:5]].tolist(), info)
        m.check_oracle(y, dtype, what)
        return info, y
    finally:
        p16.destroy()
        p32.destroy()


# 1. integers: exact in either type, so y is the serial oracle's bit for bit
@pytest.mark.parametrize("off", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integers_equal_the_serial_oracle(sp, oracle, dtype, off):
    m = band32(oracle, off, integers=True)
    Ax16 = m.typed(dtype)[0]
    plan = m.plan(sp, dtype)
    try:
        assert_fast_path(plan, dtype, 256, window=True, packed=True, escapes=0)
        m.check_oracle(m.run(plan, Ax16), dtype, "integers")
    finally:
        plan.destroy()


# 2. reals on every fast-path shape, packed and with NO_INDEX_COPY
SHAPES = {"256": (None, None, 256, True), "512": ("large", "band_narrow", 512, True),
          "1024": ("large", "band_1024", 1024, True), "no-window": ("small8", "scatter", 256, False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("no_copy", [False, True], ids=["packed", "no-index-copy"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reals_equal_the_fp32_plan_on_every_fast_path_shape(sp, oracle, shape, no_copy, dtype):
    gname, name, threads, window = SHAPES[shape]
    m = band32(oracle) if gname is None else catalogue(oracle, gname, name)
    flags = sp.capi.PLAN_NO_INDEX_COPY if no_copy else 0
    check_against_fp32(sp, m, dtype, flags, threads, window, packed=window and not no_copy, what="%s %s" % (shape, flags))


# 3. kernel features
def ragged(oracle):
    """Lengths 0 .. 70 with every fifth row or so empty (mean below 32: 8 lanes per row), one row beyond kLongSteps
    steps of its vector (the wave-per-row pass), one beyond kHugeRow (the workgroup's pass), nnz % 4 != 0."""
    def make():
        rng = np.random.default_rng(70)
        lens = rng.integers(0, 71, size=N)
        lens[rng.random(N) < 0.2] = 0
        lens[[0, 5, N - 1]] = 0
        lens[BAND_ROW] = 32
        lens[3001] = 700
        lens[9002] = 1100
        lens[777] = 33
        if lens.sum() % 4 == 0:
            lens[777] = 34
        Ap, Aj = band(N, N, lens, 71)
        return Matrix(oracle, Ap, Aj, N, 72)
    return cached("ragged", make)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("no_copy", [False, True], ids=["packed", "no-index-copy"])
def test_ragged_rows_long_rows_and_a_partial_last_group(sp, oracle, no_copy, dtype):
    m = ragged(oracle)
    lens = np.diff(m.h_Ap.astype(np.int64))
    assert m.nnz % 4 != 0 and lens.min() == 0 and 60 < lens[lens < 100].max() <= 70
    flags = sp.capi.PLAN_NO_INDEX_COPY if no_copy else 0
    info, _ = check_against_fp32(sp, m, dtype, flags, 256, True, packed=not no_copy, what="ragged", escapes=0)
    step = 4 * info["lanes_per_row"]
    assert K_LONG_STEPS * step < 700 <= K_HUGE_ROW < 1100, info


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_escaped_columns(sp, oracle, dtype):
    rows = [5003 + 997 * i for i in range(9)]
    assert not set(rows) & probe_rows(N) and min(rows) > 2 * HW + 2048 and max(rows) < N - 2 * HW - 2048

    def make():
        Ap, Aj = band(N, N, np.full(N, 32), 11)
        for i, r in enumerate(rows):       # a middle position of the row: its first and last column keep the band
            Aj[Ap[r] + 5 + i] = 0 if i % 2 == 0 else N - 1
        return Matrix(oracle, Ap, Aj, N, 13)
    m = cached("escapes", make)
    info, _ = check_against_fp32(sp, m, dtype, 0, 256, True, packed=True, what="escapes", escapes=len(rows))
    assert info["packed_index_escapes"] > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_alpha_beta_a_side_stream_a_graph_replay_and_a_second_execute(sp, oracle, dtype):
    m = band32(oracle)
    Ax16, widened, (y64, bound) = m.typed(dtype)
    p16, p32 = m.plan(sp, dtype), m.plan(sp, None)
    try:
        assert_fast_path(p16, dtype, 256, window=True, packed=True, escapes=0)
        y1 = m.run(p16, Ax16)
        m.check_oracle(y1, dtype, "first execute")
        assert torch.equal(m.run(p16, Ax16), y1), "a second execute gave other bits"

        # y = alpha A x + beta y_old: the fp32 plan's bits, and the fp64 formula within the row's bound scaled by |alpha|
        # plus the two fp32 roundings of the scaling (each below 2^-24 of the larger of its operand and its result)
        alpha, beta = -0.5, 0.25
        y_old = dev((np.random.default_rng(5).random(m.n_rows) * 2 - 1).astype(np.float32))
        got = []
        for p, Ax in ((p16, Ax16), (p32, widened)):
            p.set_alpha_beta(alpha, beta)
            got.append(p.execute(Ax, m.x, y_old.clone()))
            p.set_alpha_beta(1.0, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(got[0], got[1]), "alpha / beta: differs from the fp32 plan"
        want = alpha * y64 + beta * y_old.to(torch.float64)
        tol = abs(alpha) * bound + 2.0 ** -23 * ((alpha * y64).abs() + (beta * y_old.to(torch.float64)).abs() + want.abs())
        assert bool(((got[0].to(torch.float64) - want).abs() <= tol).all()), "alpha / beta: outside the bound"

        # a side stream; one capture, replayed on a new x
        x2_host = (np.random.default_rng(6).random(m.n_cols) * 2 - 1).astype(np.float32)
        x_buf = m.x.clone()
        y = m.poisoned()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            p16.execute(Ax16, x_buf, y, stream=s)             # warm-up outside the capture, on the side stream
            s.synchronize()
            assert torch.equal(y, y1), "side stream: other bits"
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                p16.execute(Ax16, x_buf, y, stream=s)
            x_buf.copy_(dev(x2_host))
            y.fill_(float("nan"))
            g.replay()
        torch.cuda.synchronize()
        assert not torch.isnan(y).any()
        assert torch.equal(y, m.run(p32, widened, x=x_buf)), "graph replay on a new x: differs from the fp32 plan"
        y64_2, bound_2 = parity_bound(oracle, m.h_Ap, m.h_Aj, widened.cpu().numpy(), x2_host, 8)
        assert bool(((y.to(torch.float64) - dev(y64_2)).abs() <= dev(bound_2)).all()), "graph replay: outside the bound"
    finally:
        p16.destroy()
        p32.destroy()


# 4. shapes the 16-bit chunked kernels are not built for: the plain kernel, and the plan says so
def powerlaw(oracle):
    def make():
        rng = np.random.default_rng(40)
        lens = rng.integers(0, 17, size=N)
        hubs = [1234, 9000, 15001]
        lens[hubs] = 30000
        Ap = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(lens, out=Ap[1:])
        Aj = rng.integers(0, N, size=int(Ap[-1]), dtype=np.int32)
        return Matrix(oracle, Ap, Aj, N, 41)
    return cached("powerlaw", make)


def two_bands(oracle):
    """60 000 rows, 16 entries around the diagonal and 16 around 20 000 columns below it (around the diagonal again in
    the rows that have no such columns): the two bands are further apart than any one window of x spans."""
    def make():
        n, gap, w = 60000, 20000, 40
        rng = np.random.default_rng(50)
        rows = np.arange(n, dtype=np.int64)[:, None]
        centre = np.repeat(np.array([-gap, 0], dtype=np.int64), 16)[None, :]
        jitter = rng.integers(-w, w + 1, size=(n, 32))
        cols = rows + centre + jitter
        outside = cols < 0
        cols[outside] = (np.broadcast_to(rows, cols.shape) + jitter)[outside]
        np.clip(cols, 0, n - 1, out=cols)
        cols.sort(axis=1)
        Ap = np.arange(n + 1, dtype=np.int64) * 32
        return Matrix(oracle, Ap, cols.reshape(-1).astype(np.int32), n, 51)
    return cached("two_bands", make)


def check_plain(m, plan, dtype, Ax16, what, shape_says):
    info, sh = plan.info(), plan.shape()
    assert not forced(), "a MI355_* knob forces a code path: %s" % info["knobs"]
    assert shape_says(sh), "%s: not the plan shape the case is about: %s" % (what, fields(sh))
    assert plan.mat_type() == MAT_CODE[dtype] and info["val_type"] == 0, info
    assert info["main_kernel"] == PLAIN and info["window_elems"] == 0 and info["window_segments"] == 0, info
    assert info["n_kernels"] == 1 and info["packed_index_bytes"] == 0, info
    assert info["grid_blocks"] == -(-m.n_rows // (256 // info["lanes_per_row"])), info
    y = m.run(plan, Ax16)
    m.check_oracle(y, dtype, what)
    return y


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["weight-cut", "two-bands", "offset-Ax"])
def test_other_shapes_run_the_plain_kernel(sp, oracle, case, dtype):
    """Weight-cut chunks, several bands — and, on the weight-cut plan, Ax passed as a view one element into its
    buffer (2 bytes: no 8-byte group is aligned).  The shape is still the fp32 plan's."""
    m = two_bands(oracle) if case == "two-bands" else powerlaw(oracle)
    says = (lambda sh: sh.window_segments >= 2) if case == "two-bands" else (lambda sh: sh.balanced_chunks == 1)
    Ax16 = m.typed(dtype)[0]
    if case == "offset-Ax":
        buf = torch.empty(m.nnz + 1, dtype=dtype, device=DEV)
        buf[1:].copy_(Ax16)
        Ax16 = buf[1:]
        assert Ax16.data_ptr() % 8 == 2 and Ax16.is_contiguous()
    p16, p32 = m.plan(sp, dtype), m.plan(sp, None)
    try:
        assert bytes(p16.shape()) == bytes(p32.shape())
        assert p32.info()["main_kernel"] == WINDOW
        check_plain(m, p16, dtype, Ax16, case, says)
    finally:
        p16.destroy()
        p32.destroy()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_fast_path_plan_takes_the_plain_kernel_for_an_unaligned_ax(sp, oracle, dtype):
    """The alignment of Ax is known at the execute only: the plan (and its report) is the chunked one, the execute on a
    view one element into its buffer runs the plain kernel; the same plan then runs the aligned values again."""
    m = band32(oracle)
    Ax16 = m.typed(dtype)[0]
    buf = torch.empty(m.nnz + 1, dtype=dtype, device=DEV)
    buf[1:].copy_(Ax16)
    assert buf[1:].data_ptr() % 8 == 2
    plan = m.plan(sp, dtype)
    try:
        assert_fast_path(plan, dtype, 256, window=True, packed=True, escapes=0)
        m.check_oracle(m.run(plan, buf[1:]), dtype, "offset Ax")
        m.check_oracle(m.run(plan, Ax16), dtype, "aligned Ax")
    finally:
        plan.destroy()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_small_matrix_runs_the_plain_kernel_with_the_fp32_plans_bits(sp, oracle, small_on, dtype):
    m = band32(oracle)
    Ax16, widened, _ = m.typed(dtype)
    p16, p32 = m.plan(sp, dtype), m.plan(sp, None)
    try:
        assert bytes(p16.shape()) == bytes(p32.shape()) and p16.info() == p32.info()
        y = check_plain(m, p16, dtype, Ax16, "small_plain", lambda sh: sh.small_plain == 1)
        assert torch.equal(y, m.run(p32, widened)), "small_plain: differs from the fp32 plan"
    finally:
        p16.destroy()
        p32.destroy()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_auto_becomes_vector(sp, oracle, dtype):
    m = band32(oracle)
    plan = m.plan(sp, dtype, kind="auto")
    try:
        info, _ = assert_fast_path(plan, dtype, 256, window=True, packed=True, escapes=0)
        assert info["kind"] == 0
        with pytest.raises(RuntimeError, match="not supported"):
            plan.set_semiring("min_plus")
    finally:
        plan.destroy()


# 5. narrow_values: the device's rounding is the host's
def narrow_inputs():
    rng = np.random.default_rng(99)
    wide = (rng.standard_normal(1_000_000) * 10.0 ** rng.uniform(-9, 6, size=1_000_000)).astype(np.float32)
    f = np.float32
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(f).max, -np.finfo(f).max, np.finfo(f).tiny,
                         1e-45, -1e-45,                                     # fp32 subnormals
                         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, -(1 + 2.0 ** -11),   # fp16 halfway cases
                         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, -(1 + 2.0 ** -8),       # bf16 halfway cases
                         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 5 * 2.0 ** -24,      # fp16 subnormals, halfway
                         2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1023 * 2.0 ** -24, 6e-8, -6e-6,
                         65504.0, 65519.99, 65520.0, 65536.0, -65520.0, 1e6, -1e6, 3.0e38, 3.39e38, 3.4e38],   # overflow
                        dtype=f)
    return np.concatenate([wide, specials, (rng.random(4096) * 2.0 ** -14).astype(f)])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_narrow_values_rounds_as_the_host_does(sp, dtype):
    src = torch.from_numpy(narrow_inputs())
    want = src.to(dtype)                                            # the host's rounding
    got = sp.narrow_values(src.to(DEV), dtype)
    torch.cuda.synchronize()
    assert got.dtype == dtype and got.shape == src.shape
    got = got.cpu()
    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any()) and bool((want == 0).any())
    same = (got.view(torch.int16) == want.view(torch.int16)) | (torch.isnan(got) & torch.isnan(want))
    bad = torch.nonzero(~same).flatten()
    assert bad.numel() == 0, "%d values differ from tensor.to(%s), first %s: src %s, got %s, want %s" % (
        bad.numel(), dtype, bad[:5].tolist(), src[bad[:5]].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    out = torch.zeros(src.numel() + 3, dtype=dtype, device=DEV)
    assert sp.narrow_values(src.to(DEV), dtype, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out[:src.numel()].cpu().view(torch.int16), got.view(torch.int16)) and bool((out[src.numel():] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_plan_on_narrowed_values_equals_the_plan_on_host_rounded_values(sp, oracle, dtype):
    m = band32(oracle)
    Ax16 = m.typed(dtype)[0]
    narrowed = sp.narrow_values(dev(m.h_Ax), dtype)
    plan = m.plan(sp, dtype)
    try:
        assert_fast_path(plan, dtype, 256, window=True, packed=True, escapes=0)
        assert torch.equal(narrowed.view(torch.int16), Ax16.view(torch.int16))
        assert torch.equal(m.run(plan, narrowed), m.run(plan, Ax16))
    finally:
        plan.destroy()
