"""Row-block plans of every plan shape against the whole matrix's plan.

The multi-GPU design rests on one claim (README.md; include/mi355_spmv.h, "row-block plans"): for the row-local kinds,
VECTOR and LIGHT, a plan made by mi355_spmv_plan_create_block sums every row exactly as the whole matrix's plan does,
so the concatenated y is the one-GPU y bit for bit.  A block plan does not shape itself: it copies the launch shape out
of mi355_spmv_plan_shape (rows_plan.hip, inherit_rows_shape) and every copied field belongs to one plan shape.  Here the claim
is tried on the structure catalogue of tests/kept_structures.py, whose structures are named after the plan shapes they
produce, the small groups under both arms of the small-matrix choice, and a census at the end asserts that the whole
plans whose blocks were checked cover the plan space.

What this file must not be blind to:
  values   reals in (-1, 1) in fp32 as well (ks.real_values): with the catalogue's small integers every order of
           summation gives the same bits
  phase    the banded structures have rows of 32 / 24 / 8 entries, so every block of theirs starts at 16-byte phase 0;
           ks.phase_shifted deletes the first d entries of row 1 and every later row start, so every cut, has phase
           (-d) & 3 (Ap[0] of the block's view, nnz_begin, nnz_read)

Block against whole is exact; whole against the oracle and everything of the merge kind is held to
conftest.parity_bound; NaN / Inf to ks.nan_expected."""
import contextlib

import numpy as np
import pytest
import torch

import kept_structures as ks
from conftest import parity_bound
from plan_census import PLAIN, REPORT, describe, has_giant_list, plain_lanes, row_kind_lines
from small_path import forced, small_choice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROW_KINDS = ("vector", "light")
KINDS = ("vector", "merge", "light")
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
INHERITED = ("lanes_per_row", "block_threads", "balanced_chunks", "window_elems", "window_segments", "main_kernel")
PARTS = (3, 8, 64)                 # (every structure of the catalogue keeps two or more non-empty blocks at each)
NAN_PARTS = 8
SCALINGS = ((-0.75, 3.0, "y0"), (2.5, 0.0, "nan"))     # (alpha, beta, what y holds before)

# (group, arm of the small-matrix choice or None): the plain one-pass kernel (small_plain = 1) and the chunked kernels
# each hand their shape on to blocks; merge ignores that choice
ARMS = [("large", None), ("f64", None), ("small32", "default"), ("small32", "chunked"), ("small8", "default"),
        ("small8", "chunked")]
SHAPES = [(gname, arm, name, d) for gname, arm in ARMS for name in ks.GROUPS[gname].structures
          for d in ks.phase_shifts(ks.GROUPS[gname], name)]


def _id(*parts):
    return "-".join(str(p) if not isinstance(p, int) else "d%d" % p for p in parts if p is not None)


BLOCK_CASES = [pytest.param(gname, arm, name, d, kind, id=_id(gname, arm, name, d, kind))
               for gname, arm, name, d in SHAPES for kind in ROW_KINDS]
NAN_CASES = [pytest.param(gname, arm, name, d, kind, id=_id(gname, arm, name, d, kind))
             for gname, arm, name, d in SHAPES for kind in KINDS if not (kind == "merge" and arm == "default")]
# the library's own cutting: the unshifted structure and its last shift
CUT_CASES = [pytest.param(gname, arm, name, d, kind, id=_id(gname, arm, name, d, kind))
             for gname, arm, name, d in SHAPES for kind in KINDS if not (kind == "merge" and arm == "default")
             if d in (0, ks.phase_shifts(ks.GROUPS[gname], name)[-1])]

_GROUPS = {}       # group name -> GroupState
_WHOLE = {}        # (group, arm, kind, structure, d) -> the whole plan whose blocks were checked: info, extra, phases
_COUNT = {"cases": 0, "blocks": 0, "empty": 0}


class Case:
    """One (structure, shift) of a group on the device, with the oracle's answers."""

    def __init__(self, oracle, gs, name, d, Ap, Aj):
        g = gs.g
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.g, self.name, self.d, self.dt = g, name, d, gs.dt
        self.n_rows, self.n_cols, self.nnz = g.n_rows, g.n_cols, g.nnz - d
        assert Aj.size == self.nnz and int(Ap[-1]) == self.nnz
        self.Ap, self.Aj = dev(Ap), dev(Aj)
        self.Ap_host = Ap.astype(np.int64)
        # the values of nnz - d nonzeros: the group's, from the front
        self.Ax, self.Axn, self.x, self.xn = gs.Ax[:self.nnz], gs.Axn[:self.nnz], gs.x, gs.xn
        y64, bound = parity_bound(oracle, Ap, Aj, gs.h_Ax[:self.nnz], gs.h_x, 8)
        self.y64, self.bound = dev(y64), dev(bound)
        self.want_nan = dev(ks.nan_expected(g, Ap, Aj, gs.h_Axn[:self.nnz]))

    def outside(self, y):
        """Rows of y outside the parity bound around the oracle's fp64 result."""
        return torch.nonzero(~((y.to(torch.float64) - self.y64).abs() <= self.bound)).flatten()


class GroupState:
    """One group on the device: its values and every (structure, shift) — built once per module; the host keeps the
    row offsets only."""

    def __init__(self, oracle, g):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.g, self.dt = g, TORCH[g.val]
        self.h_Ax, self.h_x = ks.real_values(g)
        self.h_Axn, h_xn = ks.nan_values(g)
        self.Ax, self.x, self.Axn, self.xn = dev(self.h_Ax), dev(self.h_x), dev(self.h_Axn), dev(h_xn)
        rng = np.random.default_rng([10, g.n_rows, g.per_row])
        self.y0 = dev((rng.random(g.n_rows) * 2 - 1).astype(g.val))
        self.cases = {}
        for name in g.structures:
            Ap, Aj, _ = ks.build(g, name)
            for d in ks.phase_shifts(g, name):
                Ap_d, Aj_d = ks.phase_shifted(Ap, Aj, d)
                self.cases[(name, d)] = Case(oracle, self, name, d, Ap_d, Aj_d)
            del Ap, Aj
        del self.h_Ax, self.h_x, self.h_Axn


def case(oracle, gname, name, d):
    if gname not in _GROUPS:
        _GROUPS[gname] = GroupState(oracle, ks.GROUPS[gname])
    return _GROUPS[gname], _GROUPS[gname].cases[(name, d)]


def arm_of(sp, arm):
    return small_choice(sp, arm) if arm else contextlib.nullcontext()


def poisoned(c, value=float("nan")):
    return torch.full((c.n_rows,), value, dtype=c.dt, device=DEV)


def differing(y, ref):
    """Rows where y and ref differ in bits, NaN equal to NaN."""
    return torch.nonzero(~((y == ref) | (torch.isnan(y) & torch.isnan(ref)))).flatten()


class Block:
    def __init__(self, b, plan, r0, r1, lo, n, phase):
        self.b, self.plan, self.r0, self.r1, self.lo, self.n, self.phase = b, plan, r0, r1, lo, n, phase
        self.info = plan.info()


def check_cuts(c, rows, chunks, nnzs, where):
    assert rows[0] == 0 and rows[-1] == c.n_rows and all(a <= b for a, b in zip(rows, rows[1:])), (where, rows)
    assert all(r % 4 == 0 or r == c.n_rows for r in rows), (where, rows)
    assert nnzs == [int(c.Ap_host[r]) for r in rows], (where, nnzs)
    assert all(a <= b for a, b in zip(chunks, chunks[1:])), (where, chunks)


def make_blocks(sp, kind, c, shape, rows, chunks, nnzs, where):
    """A plan per non-empty block of the cut, through dist.block_view and Plan.block.  A cut that leaves fewer than two
    non-empty blocks checks nothing: that fails."""
    blocks = []
    for b in range(len(rows) - 1):
        r0, r1 = rows[b], rows[b + 1]
        if r1 == r0:
            _COUNT["empty"] += 1
            continue
        a, j, _, lo = sp.dist.block_view(c.Ap, c.Aj, c.Ax, r0, r1)
        nnz_end = int(c.Ap_host[r1]) - lo
        assert j.numel() == nnz_end and lo == nnzs[b] & ~3
        plan = sp.Plan.block(kind, shape, r0, chunks[b], chunks[b + 1] - chunks[b], nnzs[b], r1 - r0, c.n_cols, nnz_end,
                             a, j, c.dt)
        blocks.append(Block(b, plan, r0, r1, lo, nnz_end, nnzs[b] & 3))
    _COUNT["blocks"] += len(blocks)
    assert len(blocks) >= 2, "%s: %d non-empty blocks of %d" % (where, len(blocks), len(rows) - 1)
    return blocks


def run_blocks(blocks, Ax, x, y):
    for k in blocks:
        k.plan.execute(Ax[k.lo:k.lo + k.n], x, y[k.r0:k.r1])
    torch.cuda.synchronize()
    return y


def destroy(blocks):
    for k in blocks:
        k.plan.destroy()


def mismatch(what, where, blocks, whole_info, rows, y, ref):
    """The failure text: the first differing rows, their block, its phase, and both info() dictionaries."""
    lines = ["%s: %s: %d rows differ, first %s" % (where, what, rows.numel(), rows[:5].tolist()),
             "  whole plan %s" % whole_info]
    seen = set()
    for r in rows[:5].tolist():
        k = next(k for k in blocks if k.r0 <= r < k.r1)
        lines.append("  row %d: block %d, rows [%d, %d), phase %d: got %r, want %r" % (
            r, k.b, k.r0, k.r1, k.phase, y[r].item(), ref[r].item()))
        if k.b not in seen:
            seen.add(k.b)
            lines.append("    block plan %s" % k.info)
    return "\n".join(lines)


def check_row_kind(sp, oracle, gname, arm, name, d, kind):
    """Assertions 1, 2, 3 and 6 of one (group, arm, structure, shift, kind); records the whole plan for the census."""
    gs, c = case(oracle, gname, name, d)
    where = _id(gname, arm, name, d, kind)
    failures = []
    with arm_of(sp, arm):
        whole = sp.Plan(kind, c.n_rows, c.n_cols, c.nnz, c.Ap, c.Aj, c.dt)
        info, _, extra = describe(whole)
        shape = whole.shape()
        # 1. the whole plan: every row written, inside the bound around the oracle
        y1 = whole.execute(c.Ax, c.x, poisoned(c))
        torch.cuda.synchronize()
        assert not torch.isnan(y1).any(), "%s: the whole plan left NaN in y; %s" % (where, info)
        bad = c.outside(y1)
        assert bad.numel() == 0, "%s: whole plan outside the parity bound in %d rows, first %s: got %s, oracle %s; %s" % (
            where, bad.numel(), bad[:5].tolist(), y1[bad[:5]].tolist(), c.y64[bad[:5]].tolist(), info)
        scaled = []
        for alpha, beta, before in SCALINGS:
            whole.set_alpha_beta(alpha, beta)
            scaled.append(whole.execute(c.Ax, c.x, gs.y0.clone() if before == "y0" else poisoned(c)))
        torch.cuda.synchronize()
        whole.set_alpha_beta(1.0, 0.0)
        record = _WHOLE.setdefault((gname, arm, kind, name, d), {"info": info, "extra": extra, "phases": set()})
        for parts in PARTS:
            cut = "%s parts=%d" % (where, parts)
            rows, chunks, nnzs = whole.partition(parts)
            check_cuts(c, rows, chunks, nnzs, cut)
            blocks = make_blocks(sp, kind, c, shape, rows, chunks, nnzs, cut)
            try:
                # 2. the launch shape is the whole plan's, and so is every bit of y
                for k in blocks:
                    assert {f: k.info[f] for f in INHERITED} == {f: info[f] for f in INHERITED}, \
                        "%s: block %d did not inherit the whole plan's shape: %s, whole %s" % (cut, k.b, k.info, info)
                y = run_blocks(blocks, c.Ax, c.x, poisoned(c))
                assert not torch.isnan(y).any(), "%s: the blocks left NaN in y" % cut
                rows_bad = differing(y, y1)
                if rows_bad.numel():
                    failures.append(mismatch("blocks against the whole plan", cut, blocks, info, rows_bad, y, y1))
                # 6. a second execute gives the same bits
                again = run_blocks(blocks, c.Ax, c.x, poisoned(c))
                rows_bad = differing(again, y)
                if rows_bad.numel():
                    failures.append(mismatch("second execute against the first", cut, blocks, info, rows_bad, again, y))
                # 3. alpha / beta through the blocks (a giant row's finish adds alpha * sum to beta * y_old in its slice)
                for (alpha, beta, before), want in zip(SCALINGS, scaled):
                    for k in blocks:
                        k.plan.set_alpha_beta(alpha, beta)
                    y = run_blocks(blocks, c.Ax, c.x, gs.y0.clone() if before == "y0" else poisoned(c))
                    assert not torch.isnan(y).any(), "%s: alpha=%s beta=%s left NaN in y" % (cut, alpha, beta)
                    rows_bad = differing(y, want)
                    if rows_bad.numel():
                        failures.append(mismatch("alpha=%s beta=%s" % (alpha, beta), cut, blocks, info, rows_bad, y, want))
                record["phases"].update(k.phase for k in blocks)
            finally:
                destroy(blocks)
        whole.destroy()
    _COUNT["cases"] += len(PARTS)
    if failures:
        print("\n".join(failures))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("gname,arm,name,d,kind", BLOCK_CASES)
def test_blocks_of_every_shape_reproduce_the_whole_plan_bit_for_bit(sp, oracle, gname, arm, name, d, kind):
    """Real values, every shift: the whole plan writes every row inside the parity bound; for 3, 8 and 64 parts the
    cuts are chunk boundaries, every non-empty block inherits the launch shape, and the blocks' y equals the whole
    plan's bit for bit — plain, executed twice, and under two alpha / beta."""
    check_row_kind(sp, oracle, gname, arm, name, d, kind)


@pytest.mark.parametrize("gname,arm,name,d,kind", NAN_CASES)
def test_nan_and_inf_reach_only_their_rows_through_blocks(sp, oracle, gname, arm, name, d, kind):
    """ks.nan_values through the blocks of 8 parts: column numbers are global while a block's band is shifted by its
    first row, so a window staged for the wrong columns, or a padded 16-byte group, would leak a neighbour's NaN / Inf or
    miss its own.  y starts at -1, which no row can sum to (Ax in {1, 2, 3}, x = 1 / NaN / +Inf)."""
    gs, c = case(oracle, gname, name, d)
    where = _id(gname, arm, name, d, kind)
    with arm_of(sp, arm):
        whole = sp.Plan(kind, c.n_rows, c.n_cols, c.nnz, c.Ap, c.Aj, c.dt)
        info = whole.info()
        rows, chunks, nnzs = whole.partition(NAN_PARTS)
        check_cuts(c, rows, chunks, nnzs, where)
        blocks = make_blocks(sp, kind, c, whole.shape() if kind != "merge" else None, rows, chunks, nnzs, where)
        whole.destroy()
        try:
            y = run_blocks(blocks, c.Axn, c.xn, poisoned(c, -1.0))
        finally:
            destroy(blocks)
    want = c.want_nan
    assert bool(torch.isnan(want).any()) and bool(torch.isposinf(want).any())
    rows_bad = differing(y, want)
    assert rows_bad.numel() == 0, mismatch("NaN / Inf expectation", where, blocks, info, rows_bad, y, want)


@pytest.mark.parametrize("gname,arm,name,d,kind", CUT_CASES)
def test_the_librarys_own_cutting(sp, oracle, gname, arm, name, d, kind):
    """DistPlan.local with 8 blocks on one device and DistPlan.rank with world = 1 and 4 sub-blocks: bit for bit the
    whole plan's y (vector, light), inside the parity bound (merge).  Merge blocks made with Plan.block and no shape are
    held to the same bound."""
    gs, c = case(oracle, gname, name, d)
    where = _id(gname, arm, name, d, kind)

    def check(what, y, y1):
        assert not torch.isnan(y).any(), "%s: %s left NaN in y" % (where, what)
        bad = c.outside(y) if kind == "merge" else differing(y, y1)
        assert bad.numel() == 0, "%s: %s: %d rows %s, first %s: got %s, want %s" % (
            where, what, bad.numel(), "outside the parity bound" if kind == "merge" else "differ from the whole plan's",
            bad[:5].tolist(), y[bad[:5]].tolist(), (c.y64 if kind == "merge" else y1)[bad[:5]].tolist())

    with arm_of(sp, arm):
        whole = sp.Plan(kind, c.n_rows, c.n_cols, c.nnz, c.Ap, c.Aj, c.dt)
        y1 = whole.execute(c.Ax, c.x, poisoned(c))
        torch.cuda.synchronize()
        check("the whole plan", y1, y1)
        shape = whole.shape()
        rows, chunks, nnzs = whole.partition(4)
        if kind == "merge":
            rows8, chunks8, nnzs8 = whole.partition(NAN_PARTS)
            check_cuts(c, rows8, chunks8, nnzs8, where)
            blocks = make_blocks(sp, kind, c, None, rows8, chunks8, nnzs8, where)
            try:
                check("Plan.block without a shape", run_blocks(blocks, c.Ax, c.x, poisoned(c)), y1)
            finally:
                destroy(blocks)
        whole.destroy()
        dist = sp.DistPlan.local(kind, c.n_rows, c.n_cols, c.nnz, c.Ap, c.Aj, c.dt, parts=8, devices=[0])
        try:
            cuts = dist.cuts()
            assert len(cuts) == 9 and cuts[0] == 0 and cuts[-1] == c.n_rows, (where, cuts)
            y = dist.execute(c.Ax, c.x, poisoned(c))
            torch.cuda.synchronize()
            check("DistPlan.local", y, y1)
        finally:
            dist.destroy()
        dist = sp.DistPlan.rank(kind, 0, 1, None, 4, rows, chunks, nnzs, shape, c.n_cols, c.n_rows, c.nnz, c.Ap, c.Aj, c.dt)
        try:
            y = dist.execute(c.Ax, c.x, poisoned(c))
            torch.cuda.synchronize()
            check("DistPlan.rank", y, y1)
        finally:
            dist.destroy()


# a banded, a multi-band and a weight-cut structure, with what the whole plan's shape must show for the case to be that one
ROUND_TRIP = {"band_narrow": lambda sh: sh.window_segments == 1 and sh.window_from_band == 1 and sh.balanced_chunks == 0,
              "stencil": lambda sh: sh.window_segments >= 2,
              "powerlaw": lambda sh: sh.balanced_chunks == 1}


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("name", sorted(ROUND_TRIP))
def test_a_block_that_is_the_whole_matrix_has_the_whole_plans_shape(sp, oracle, name, kind):
    """The two directions of the block shape (rows_plan.hip, export_rows_shape / inherit_rows_shape) undo each other: a
    block plan over all rows and all chunks of the whole plan, made from the whole plan's shape, reports that shape byte
    for byte."""
    gs, c = case(oracle, "large", name, 0)
    whole = sp.Plan(kind, c.n_rows, c.n_cols, c.nnz, c.Ap, c.Aj, c.dt)
    shape = whole.shape()
    whole.destroy()
    fields = lambda sh: {f: getattr(sh, f) if isinstance(getattr(sh, f), int) else list(getattr(sh, f)) for f, _ in sh._fields_}
    assert ROUND_TRIP[name](shape), "large/%s %s: not the plan shape the case is about: %s" % (name, kind, fields(shape))
    block = sp.Plan.block(kind, shape, 0, 0, shape.n_chunks, 0, c.n_rows, c.n_cols, c.nnz, c.Ap, c.Aj, c.dt)
    again = block.shape()
    block.destroy()
    assert bytes(again) == bytes(shape), "large/%s %s: the block's shape differs from the whole plan's: block %s, whole %s" % (
        name, kind, fields(again), fields(shape))


WINDOWED = ("one band-placed window", "window_segments >= 2", "sweep kernel", "chunks with a window")


def test_census_of_the_block_plans(sp, oracle):
    """The whole plans whose blocks were checked in this file include every shape of the row-local plan space, the
    windowed ones with a block that began at a non-zero 16-byte phase, and the chunked and the plain kernel each saw
    phases 1, 2 and 3.  (Whatever the tests above did not check in this session — a run of this test alone — is checked
    here first.)"""
    if forced():
        pytest.skip("a forcing knob decides the plan shapes")
    for gname, arm, name, d in SHAPES:
        for kind in ROW_KINDS:
            if (gname, arm, kind, name, d) not in _WHOLE:
                check_row_kind(sp, oracle, gname, arm, name, d, kind)
    records = [(key, rec["info"], rec["extra"], rec["phases"]) for key, rec in _WHOLE.items()]
    tag = lambda key: _id(key[0], key[1], key[3], key[4])
    lines = []
    for label, holds in row_kind_lines():
        lines.append((label, lambda key, i, e, ph, holds=holds: holds(key[2], i, e)))
        if any(w in label for w in WINDOWED):
            lines.append((label + ", a block at a non-zero phase",
                          lambda key, i, e, ph, holds=holds: holds(key[2], i, e) and bool(ph - {0})))
    for kind in ROW_KINDS:
        lines.append(("%s: a giant-row list (n_kernels == 3)" % kind,
                      lambda key, i, e, ph, kind=kind: key[2] == kind and has_giant_list(kind, i)))
        for phase in (1, 2, 3):
            lines.append(("%s: the chunked kernels, a block at phase %d" % (kind, phase),
                          lambda key, i, e, ph, kind=kind, phase=phase: key[2] == kind and i["main_kernel"] != PLAIN and phase in ph))
            lines.append(("%s: the plain kernel, a block at phase %d" % (kind, phase),
                          lambda key, i, e, ph, kind=kind, phase=phase: key[2] == kind and i["main_kernel"] == PLAIN and phase in ph))
    lanes = {kind: plain_lanes(kind, [(key[2], i) for key, i, e, ph in records]) for kind in ROW_KINDS}
    missing = ["%s: the plain kernel with two lane widths (have %s)" % (kind, lanes[kind])
               for kind in ROW_KINDS if len(lanes[kind]) < 2]
    print("census of the whole plans whose blocks were checked: %d (structure, kind, cut, phase) cases, %d block plans, "
          "%d empty blocks skipped" % (_COUNT["cases"], _COUNT["blocks"], _COUNT["empty"]))
    for kind in ROW_KINDS:
        print("  %s: the plain kernel with lanes per row %s" % (kind, lanes[kind]))
    for label, holds in lines:
        found = sorted({tag(key) for key, i, e, ph in records if holds(key, i, e, ph)})
        print("  %-72s %s" % (label, ", ".join(found) or "MISSING"))
        if not found:
            missing.append(label)
    if missing:
        for key, i, e, ph in sorted(records, key=str):
            print("  ", key, {k: i[k] for k in REPORT}, e, "phases", sorted(ph))
    assert not missing, "no whole plan whose blocks were checked has these shapes: %s" % missing
