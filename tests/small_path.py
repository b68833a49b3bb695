"""The two ways a small regular matrix can run, for the GPU suite.

tests/conftest.py switches the product's small-matrix choice off for the whole suite (MI355_SPMV_SMALL=0: the chunked
kernels); the library's DEFAULT sends every regular VECTOR or LIGHT matrix of up to kSmallPlainNnz nonzeros to the
plain one-pass kernel csr_vector_kernel (rows_plan.hip, shape_rows: small_plain).  The `path` fixture runs a test under either:
  default  MI355_SPMV_SMALL unset, the knobs re-read (which also drops the kept one-shot plans)
  chunked  MI355_SPMV_SMALL=0, the knobs re-read
and puts the environment back afterwards.  Merge ignores the knob, so `kind_paths` gives it the chunked arm only; the
chunked arm keeps the test ids the suite had before the default arm was added."""
import contextlib
import os

import pytest

KNOB = "MI355_SPMV_SMALL"
PLAIN = "csr_vector_kernel"
SMALL_PLAIN_NNZ = 4_100_000        # common.hpp, kSmallPlainNnz
BLOCK = 256                        # common.hpp, kBlock
# why a small matrix with a hub row is not on the plain kernel: shape_rows takes it only for chunks of equal rows
WEIGHT_CUT = "weight-cut chunks (rows_plan.hip, decide_balance: its chunk weighs more than twice the mean chunk)"


def forced():
    """Another MI355_* knob forces a code path (scripts/gpu_env_matrix.sh): the kernel assertions do not hold then."""
    return any(k.startswith("MI355_") for k in os.environ if k not in ("MI355_SPMV_LIB", KNOB))


@contextlib.contextmanager
def small_choice(sp, path):
    saved = os.environ.get(KNOB)
    if path == "default":
        os.environ.pop(KNOB, None)
    elif path == "chunked":
        os.environ[KNOB] = "0"
    else:
        raise ValueError(path)
    sp.capi.lib().mi355_spmv_knobs_reload()
    try:
        yield path
    finally:
        if saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = saved
        sp.capi.lib().mi355_spmv_knobs_reload()


@pytest.fixture(params=["default", "chunked"])
def path(request, sp):
    with small_choice(sp, request.param):
        yield request.param


@pytest.fixture()
def small_on(sp):
    with small_choice(sp, "default"):
        yield


def kind_paths(kinds):
    """(kind, path) parameters for @pytest.mark.parametrize("kind,path", ..., indirect=["path"])."""
    out = []
    for k in kinds:
        out.append(pytest.param(k, "chunked", id=k))
        if k != "merge":
            out.append(pytest.param(k, "default", id=k + "-default"))
    return out


def plain_lanes(nnz, n_rows):
    """Lanes per row of the plain kernel: shape_rows' rule restated — two elements per lane up to a mean of 32 per row,
    four beyond, the smallest power of two from 2 to 64 that covers the mean row."""
    mean = nnz // n_rows
    per_lane = 2 if mean <= 32 else 4
    t = 2
    while t < 64 and per_lane * t < mean:
        t *= 2
    return t


def check_kernel(plan, path, elsewhere=None, lanes=None):
    """The kernel a VECTOR / LIGHT plan took.  Default arm: the plain kernel unless `elsewhere` names why the rule sends
    this case to the chunked kernels; chunked arm: never the plain kernel.  Skipped under a forcing knob."""
    if forced() or plan.kind == "merge":
        return
    info, sh = plan.info(), plan.shape()
    if path == "default" and elsewhere is None:
        assert sh.small_plain == 1 and info["main_kernel"] == PLAIN, info
        assert info["window_elems"] == 0 and info["window_segments"] == 0, info
        if plan.n_rows > 0:
            assert info["grid_blocks"] == -(-plan.n_rows // (BLOCK // info["lanes_per_row"])), info
        if lanes is not None:
            assert info["lanes_per_row"] == lanes, info
    else:
        assert sh.small_plain == 0 and info["main_kernel"] != PLAIN, (elsewhere, info)
