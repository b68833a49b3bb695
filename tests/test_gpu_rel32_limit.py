"""The exit of the row kinds' chunk prologue to chunk_rows_wide (csrc/row_chunk_window.inc, row_chunk_sweep.inc): a chunk
whose nonzeros span more than 32-bit chunk-relative offsets reach is summed one wave per row with 64-bit indices.  No
real matrix of a test's size gets there, so MI355_SPMV_REL32_LIMIT=64 makes every chunk of more than 64 nonzeros take it,
in each of the five kernels that hold the prologue: csr_vector_window_kernel (fp32 / fp64, and with the matrix in 16
bits), light_rows_window_kernel (chunk by index, chunk from the counters, and the persistent loop of weight-cut chunks),
csr_vector_sweep_kernel and light_rows_sweep_kernel.

Every case creates the same plan twice, under the default limit and under 64, asserts from plan.info() / plan.shape()
that both are the shape the case is about, and requires the two y to be equal bit for bit (and equal to a sum made with
torch).  The wide path adds in another order: the data are small integers, so every sum is exact in fp32 and in the
16-bit types and no tolerance is needed.

Matrices (built on the device): L nonzeros in every row, spread over a band of half width hw around the diagonal; row
EMPTY_ROW is empty, and the last row is longer by 1 to 3 so that nnz % 4 != 0 and that row ends inside the arrays' last,
partial 16-byte group.  4 000 rows where a workgroup takes the chunk of its index.  LIGHT hands chunks out by its
counters only beyond two chunks per workgroup slot (rows_plan.hip, set_rows_launch), and a sweep plan needs two chunks
per CU (shape_sweep): those cases take the smallest matrices that get there, a few million short rows."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIMIT = 64
EMPTY_ROW = 5
CUS = 256                  # common.hpp, kCus
SLOTS_PER_CU = 4           # no row kernel keeps more workgroups on a CU (launch bounds: rows_plan.hip, light_resident)
VAL = {"f32": torch.float32, "f64": torch.float64}
BOTH = [("i32", "f32"), ("i64", "f64")]


@contextlib.contextmanager
def knobs(sp, **env):
    """MI355_* knobs for the plans created inside (a plan keeps the knobs of its creation)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    sp.capi.lib().mi355_spmv_knobs_reload()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        sp.capi.lib().mi355_spmv_knobs_reload()


class Matrix:
    def __init__(self, n, per_row, hw, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        lens = torch.full((n,), per_row, dtype=torch.int64, device=DEV)
        lens[EMPTY_ROW] = 0
        lens[n - 1] += 1
        while int(lens.sum()) % 4 == 0:
            lens[n - 1] += 1
        Ap = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(lens, 0, out=Ap[1:])
        self.n, self.nnz = n, int(Ap[-1])
        self.row = torch.repeat_interleave(torch.arange(n, device=DEV), lens)
        pos = torch.arange(self.nnz, device=DEV) - Ap[self.row]
        Aj = self.row - hw + pos * (2 * hw) // lens[self.row]          # ascending in a row, its ends near the band's edges
        self.Aj = Aj.clamp_(0, n - 1).to(torch.int32)
        self.Ap = {"i32": Ap.to(torch.int32), "i64": Ap}
        self.Ax = torch.randint(-3, 4, (self.nnz,), generator=g, device=DEV)
        self.x = torch.randint(-4, 5, (n,), generator=g, device=DEV)
        prod = self.Ax * self.x[self.Aj.long()]
        self.want = torch.zeros(n, dtype=torch.int64, device=DEV).index_add_(0, self.row, prod)
        assert self.nnz % 4 != 0 and int(lens[n - 1]) > 0 and int(self.want.abs().max()) < 2048

    def y(self, sp, kind, off, val_dtype, mat_dtype, expect):
        p = sp.Plan(kind, self.n, self.n, self.nnz, self.Ap[off], self.Aj, val_dtype, mat_dtype=mat_dtype)
        try:
            info, sh = p.info(), p.shape()
            assert sh.small_plain == 0 and info["n_kernels"] == 1, info           # (not the plain kernel, no giant rows)
            assert self.nnz > 2 * LIMIT * info["n_chunks"], info                  # (chunks far above the limit)
            expect(info, sh)
            y = torch.full((self.n,), float("nan"), dtype=val_dtype, device=DEV)
            p.execute(self.Ax.to(mat_dtype or val_dtype), self.x.to(val_dtype), y)
            torch.cuda.synchronize()
        finally:
            p.destroy()
        info.pop("knobs")
        return y, info

    def check(self, sp, kind, off, val, expect, mat_dtype=None, **env):
        with knobs(sp, **env):
            y_default, info_default = self.y(sp, kind, off, VAL[val], mat_dtype, expect)
        with knobs(sp, MI355_SPMV_REL32_LIMIT=str(LIMIT), **env):
            y_wide, info_wide = self.y(sp, kind, off, VAL[val], mat_dtype, expect)
        assert info_wide == info_default, (info_wide, info_default)
        print("%s %s %s %s: %s, %d chunks on %d workgroups of %d threads" % (
            kind, off, val, mat_dtype, info_wide["main_kernel"], info_wide["n_chunks"], info_wide["grid_blocks"],
            info_wide["block_threads"]))
        assert torch.equal(y_default, self.want.to(VAL[val])), "default limit: y differs from the sum made with torch"
        bad = torch.nonzero(y_wide != y_default).flatten()
        assert torch.equal(y_wide, y_default), "%d rows differ under MI355_SPMV_REL32_LIMIT=%d, first %s: %s, default %s" % (
            bad.numel(), LIMIT, bad[:5].tolist(), y_wide[bad[:5]].tolist(), y_default[bad[:5]].tolist())


_CACHE = {}


def matrix(name):
    """Built once per session."""
    if name not in _CACHE:
        _CACHE[name] = {"small": lambda: Matrix(4000, 9, 40, 1),
                        "many_chunks": lambda: Matrix(4_400_000, 4, 40, 2),
                        "wide_band_f32": lambda: Matrix(2_200_000, 4, 40_000, 3),
                        "wide_band_f64": lambda: Matrix(2_200_000, 4, 20_000, 4)}[name]()
    return _CACHE[name]


def window_of(kernel, balanced=0):
    def expect(info, sh):
        assert info["main_kernel"] == kernel and sh.window_sweep == 0 and info["balanced_chunks"] == balanced, info
    return expect


def equal_rows_with_a_window(kernel):
    def expect(info, sh):
        window_of(kernel)(info, sh)
        assert info["window_elems"] > 0 and info["window_segments"] < 2 and info["grid_blocks"] == info["n_chunks"] > 1, info
    return expect


@pytest.mark.parametrize("val", ["f32", "f64"])
@pytest.mark.parametrize("off", ["i32", "i64"])
def test_vector_window_kernel(sp, off, val):
    matrix("small").check(sp, "vector", off, val, equal_rows_with_a_window("csr_vector_window_kernel"))


@pytest.mark.parametrize("mat_dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("off", ["i32", "i64"])
def test_vector_window_kernel_of_a_16_bit_matrix(sp, off, mat_dtype):
    """(equal-row chunks, one window, no giant rows: the shape the 16-bit chunked kernels are built for — rows_plan.hip,
    half_matrix_chunked — so this is h16::csr_vector_window_kernel and not its plain kernel)"""
    matrix("small").check(sp, "vector", off, "f32", equal_rows_with_a_window("csr_vector_window_kernel"), mat_dtype=mat_dtype)


@pytest.mark.parametrize("off,val", BOTH)
def test_light_window_kernel_chunk_by_index(sp, off, val):
    def expect(info, sh):
        equal_rows_with_a_window("light_rows_window_kernel")(info, sh)
        assert info["n_chunks"] <= 2 * CUS, info                  # (at most two chunks per workgroup slot: static mode)
    matrix("small").check(sp, "light", off, val, expect)


@pytest.mark.parametrize("off,val", BOTH)
def test_light_window_kernel_chunk_from_the_counters(sp, off, val):
    def expect(info, sh):
        window_of("light_rows_window_kernel")(info, sh)
        assert info["grid_blocks"] == info["n_chunks"] > 2 * SLOTS_PER_CU * CUS, info     # (one dequeue per workgroup)
    matrix("many_chunks").check(sp, "light", off, val, expect)


@pytest.mark.parametrize("off,val", BOTH)
def test_vector_weight_cut_chunks(sp, off, val):
    def expect(info, sh):
        window_of("csr_vector_window_kernel", balanced=1)(info, sh)
        assert info["grid_blocks"] == info["n_chunks"] > 1, info
    matrix("small").check(sp, "vector", off, val, expect, MI355_SPMV_BALANCE="1")


@pytest.mark.parametrize("off,val", BOTH)
def test_light_weight_cut_chunks_in_the_persistent_loop(sp, off, val):
    """One workgroup per CU (MI355_LIGHT_BLOCKS_PER_CU=1) and more than two chunks for each: every workgroup dequeues
    again after chunk_rows_wide."""
    def expect(info, sh):
        window_of("light_rows_window_kernel", balanced=1)(info, sh)
        assert info["grid_blocks"] == CUS and info["n_chunks"] > 2 * CUS, info
    matrix("many_chunks").check(sp, "light", off, val, expect, MI355_SPMV_BALANCE="1", MI355_LIGHT_BLOCKS_PER_CU="1")


@pytest.mark.parametrize("kind,kernel", [("vector", "csr_vector_sweep_kernel"), ("light", "light_rows_sweep_kernel")])
@pytest.mark.parametrize("off,val", BOTH)
def test_sweep_kernels(sp, off, val, kind, kernel):
    """A band of 80 001 columns in fp32, 40 001 in fp64: wider than any window of x (at most ~39 K fp32 / ~19 K fp64
    elements) and narrow enough for the sweep to pay with 4 nonzeros per row (rows_plan.hip, shape_sweep)."""
    def expect(info, sh):
        assert info["main_kernel"] == kernel and sh.window_sweep == 1 and info["block_threads"] == 1024, info
        assert info["balanced_chunks"] == 0 and info["grid_blocks"] == info["n_chunks"], info
    matrix("wide_band_" + val).check(sp, kind, off, val, expect)
