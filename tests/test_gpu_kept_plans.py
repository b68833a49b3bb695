"""Kept one-shot plans of every shape against every structure.

The one-shot entry points keep their plans and find them again by the pointers and sizes of Ap / Aj (capi.hip,
OneShotKey; INTEGRATION.md, "What the one-shot entry points retain"): a kept plan holds launch-shape decisions only and
every shape has a fallback in the kernels, so a plan shaped for structure A must compute structure B, written over A in
the same buffers, correctly — at worst slowly.  Here that is tried for every ordered pair of the catalogue in
tests/kept_structures.py, every kind, in fp32 / int32 and fp64 / int64, through Plan.acquire / release (which plan ran
is read, not inferred) and through the one-shot symbol itself.

fp32 groups carry small integers: every result equals oracle.spmv_serial bit for bit.  The fp64 group carries reals and
is held to conftest.parity_bound.  y is NaN-poisoned before every execute.  A census at the end asserts that the plans
kept as A cover the plan space, so that the catalogue cannot decay into one shape.

The same file carries NaN / Inf in x under the staged windows: the small test of test_gpu_parity.py takes no window."""
import contextlib
import os

import numpy as np
import pytest
import torch

import kept_structures as ks
from conftest import parity_bound
from plan_census import REPORT, has_giant_list, merge_lines, plain_lanes, row_kind_lines
from plan_census import describe as describe_plan
from small_path import forced, small_choice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["vector", "merge", "light"]
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}

# (group, arm of the small-matrix choice or None): the small groups run under the library's default, where the plain
# kernel is among the kept plans, and again under the chunked kernels; merge ignores that choice
ARMS = [("large", None), ("f64", None), ("small32", "default"), ("small32", "chunked"), ("small8", "default"),
        ("small8", "chunked")]
CASES = [pytest.param(gname, arm, kind, a, id="-".join(filter(None, (gname, arm, kind, a))))
         for gname, arm in ARMS for kind in KINDS if not (kind == "merge" and arm == "default")
         for a in ks.GROUPS[gname].structures if a not in ks.NEVER_KEPT]
NAN_CASES = [pytest.param(gname, kind, s, id="-".join((gname, kind, s)))
             for gname in ("large", "f64") for kind in KINDS for s in ks.GROUPS[gname].structures]

_STATE = {}        # group name -> State (device memory is not the constraint; the host keeps nothing of a structure)
_KEPT = {}         # (group, arm, kind, A) -> the plan kept as A: info, shape fields
_FRESH = {}        # (group, arm, kind, structure) -> info of a fresh plan
_PAIRS = [0]


class State:
    """One group on the device: the masters of every structure, one live Ap / Aj that they are copied over, values, and
    per structure the expectation of the cross-product test and of the NaN / Inf test."""

    def __init__(self, oracle, g):
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.g, self.dt = g, TORCH[g.val]
        Ax, x = ks.values(g)
        Axn, xn = ks.nan_values(g)
        self.Ax, self.x, self.Axn, self.xn = d(Ax), d(x), d(Axn), d(xn)
        self.master, self.want, self.want_nan = {}, {}, {}
        for name in g.structures:
            Ap, Aj, _ = ks.build(g, name)
            self.master[name] = (d(Ap), d(Aj))
            if g.integer_values:
                self.want[name] = (d(oracle.spmv_serial(Ap, Aj, Ax, x)),)
            else:
                y64, bound = parity_bound(oracle, Ap, Aj, Ax, x, 8)
                self.want[name] = (d(y64), d(bound))
            self.want_nan[name] = d(ks.nan_expected(g, Ap, Aj, Axn))
            del Ap, Aj
        self.Ap = torch.empty_like(self.master[g.structures[0]][0])
        self.Aj = torch.empty_like(self.master[g.structures[0]][1])
        self.y = torch.empty(g.n_rows, dtype=self.dt, device=DEV)

    def overwrite(self, name):
        self.Ap.copy_(self.master[name][0])
        self.Aj.copy_(self.master[name][1])
        torch.cuda.synchronize()

    def poisoned(self):
        return self.y.fill_(float("nan"))

    def wrong(self, name):
        """None, or what is wrong with self.y as the product of structure `name`."""
        torch.cuda.synchronize()
        y = self.y
        n_nan = int(torch.isnan(y).sum())
        if n_nan:
            return "%d rows are NaN (first %s)" % (n_nan, torch.nonzero(torch.isnan(y))[:5, 0].tolist())
        if self.g.integer_values:
            bad = y != self.want[name][0]
        else:
            y64, bound = self.want[name]
            bad = (y - y64).abs() > bound
        n_bad = int(bad.sum())
        if n_bad == 0:
            return None
        rows = torch.nonzero(bad)[:5, 0]
        return "%d wrong rows, first %s: got %s, want %s" % (n_bad, rows.tolist(), y[rows].tolist(),
                                                             self.want[name][0][rows].tolist())


def state(oracle, gname):
    if gname not in _STATE:
        _STATE[gname] = State(oracle, ks.GROUPS[gname])
    return _STATE[gname]


def arm_of(sp, arm):
    return small_choice(sp, arm) if arm else contextlib.nullcontext()


def describe(sp, plan):
    return describe_plan(plan)


def acquire(sp, st, kind):
    g = st.g
    return sp.Plan.acquire(kind, g.n_rows, g.n_cols, g.nnz, st.Ap, st.Aj, st.dt)


def fresh_info(sp, st, gname, arm, kind, name):
    """info() of a plan created for `name` from nothing (the live buffers must hold it)."""
    key = (gname, arm, kind, name)
    if key not in _FRESH:
        g = st.g
        p = sp.Plan(kind, g.n_rows, g.n_cols, g.nnz, st.Ap, st.Aj, st.dt)
        _FRESH[key] = p.info()
        p.destroy()
    return _FRESH[key]


def keep_as_a(sp, st, gname, arm, kind, a):
    """Steps 1-2: the cache emptied, the live buffers overwritten with A, a fresh plan acquired and recorded."""
    sp.capi.cache_release()
    st.overwrite(a)
    plan = acquire(sp, st, kind)
    what = describe(sp, plan)
    _KEPT[(gname, arm, kind, a)] = (what[0], what[2])
    return plan, what


@pytest.mark.parametrize("gname,arm,kind,a", CASES)
def test_kept_plan_meets_every_structure_of_its_sizes(sp, oracle, gname, arm, kind, a):
    st = state(oracle, gname)
    g = st.g
    failures = []
    with arm_of(sp, arm):
        for b in g.structures:
            _PAIRS[0] += 1
            plan, (info_a, shape_a, _) = keep_as_a(sp, st, gname, arm, kind, a)
            where = "A=%s B=%s kind=%s %s: plan kept as A %s" % (a, b, kind, "-".join(filter(None, (gname, arm))),
                                                                   {k: info_a[k] for k in REPORT})
            plan.execute(st.Ax, st.x, st.poisoned())
            bad = st.wrong(a)
            plan.release()
            if bad:
                failures.append("%s\n    its own structure: %s" % (where, bad))
                continue
            st.overwrite(b)
            plan = acquire(sp, st, kind)
            info_b, shape_b, _ = describe(sp, plan)
            if os.environ.get("MI355_SPMV_PLAN_CACHE") == "0":      # (forced off: every acquire makes a plan)
                pass
            elif not has_giant_list(kind, info_a):
                if (info_b, shape_b) != (info_a, shape_a):
                    failures.append("%s\n    the second acquire did not return the kept plan: %s" % (where, info_b))
            elif info_b != fresh_info(sp, st, gname, arm, kind, b):
                failures.append("%s\n    a plan with a giant-row list was kept: %s" % (where, info_b))
            plan.execute(st.Ax, st.x, st.poisoned())
            bad = st.wrong(b)
            plan.release()
            if bad:
                failures.append("%s\n    acquired plan on B: %s" % (where, bad))
                continue
            sp.spmv(kind, g.n_rows, g.n_cols, g.nnz, st.Ap, st.Aj, st.Ax, st.x, st.poisoned())
            bad = st.wrong(b)
            if bad:
                failures.append("%s\n    one-shot call on B: %s" % (where, bad))
        sp.capi.cache_release()
    if failures:
        print("\n".join(failures))
    assert not failures, "%d of %d structures wrong under the plan kept for %s:\n%s" % (
        len(failures), len(g.structures), a, "\n".join(failures))


@pytest.mark.parametrize("gname,kind,name", NAN_CASES)
def test_nan_and_inf_reach_only_their_rows_under_staged_windows(sp, oracle, gname, kind, name):
    """Ax in {1, 2, 3}, x = 1 except NaN at one column and +Inf at another, both referenced from inside the staged window
    (the rows around them) and from far outside it (the planted rows): NaN exactly in the rows that hold the NaN column,
    +Inf exactly in those that hold only the Inf column, the exact sum elsewhere — a masked lane, a padded 16-byte
    LDS-DMA group or a sweep pass must not leak a neighbour's value."""
    st = state(oracle, gname)
    g = st.g
    sp.capi.cache_release()
    st.overwrite(name)
    plan = sp.Plan(kind, g.n_rows, g.n_cols, g.nnz, st.Ap, st.Aj, st.dt)
    info = plan.info()
    plan.execute(st.Axn, st.xn, st.poisoned())
    torch.cuda.synchronize()
    plan.destroy()
    y, want = st.y, st.want_nan[name]
    where = "%s %s %s %s" % (gname, name, kind, {k: info[k] for k in REPORT})
    nan_y, nan_w = torch.isnan(y), torch.isnan(want)
    assert bool(nan_w.any()) and bool(torch.isposinf(want).any())
    assert torch.equal(nan_y, nan_w), "%s: NaN in %d rows, expected in %d; first differing rows %s" % (
        where, int(nan_y.sum()), int(nan_w.sum()), torch.nonzero(nan_y != nan_w)[:5, 0].tolist())
    bad = (y != want) & ~nan_w
    assert not bool(bad.any()), "%s: %d rows differ, first %s: got %s, want %s" % (
        where, int(bad.sum()), torch.nonzero(bad)[:5, 0].tolist(), y[bad][:5].tolist(), want[bad][:5].tolist())


def census_lines():
    """(label, predicate over (kind, info, extra)) — every shape the plans kept as A must include (plan_census.py)."""
    return row_kind_lines() + merge_lines()


def test_census_of_the_plans_kept_as_a(sp, oracle):
    """The plans kept as A over this whole file include every shape of the plan space the promise covers.  (Whatever
    the cross-product tests of this session did not record — a run of this test alone — is recorded here first.)"""
    if forced():
        pytest.skip("a forcing knob decides the plan shapes")
    for gname, arm in ARMS:
        for kind in KINDS:
            for a in ks.GROUPS[gname].structures:
                if a in ks.NEVER_KEPT or (kind == "merge" and arm == "default") or (gname, arm, kind, a) in _KEPT:
                    continue
                with arm_of(sp, arm):
                    plan, _ = keep_as_a(sp, state(oracle, gname), gname, arm, kind, a)
                    plan.destroy()
    lanes = {kind: plain_lanes(kind, [(k, i) for (g_, arm, k, a), (i, e) in _KEPT.items()])
             for kind in ("vector", "light")}
    missing = ["%s: the plain kernel with two lane widths (have %s)" % (kind, lanes[kind])
               for kind in ("vector", "light") if len(lanes[kind]) < 2]
    print("census of the plans kept as A (%d pairs run in this session)" % _PAIRS[0])
    for kind in ("vector", "light"):
        print("  %s: the plain kernel with lanes per row %s" % (kind, lanes[kind]))
    for label, holds in census_lines():
        found = ["-".join(filter(None, (g_, arm, a))) for (g_, arm, k, a), (i, e) in _KEPT.items() if holds(k, i, e)]
        print("  %-58s %s" % (label, ", ".join(found) or "MISSING"))
        if not found:
            missing.append(label)
    if missing:
        for key, (i, e) in sorted(_KEPT.items(), key=str):
            print("  ", key, {k: i[k] for k in REPORT}, e)
    assert not missing, "no plan kept as A has these shapes: %s" % missing
