#!/usr/bin/env python3
"""Every shape the MERGE planner gives, as text: for each matrix below and each knob setting, create a MERGE plan —
never execute it — and print one line per matrix: the default plan in words, then per setting the first 8 hex digits
of the SHA-256 of the whole of Plan.info() and bytes(Plan.shape()).  --full prints a line per plan with those two whole
(the info as JSON, the shape as hex): 380 KB, for finding what differs.  Two builds of the library plan alike exactly
when their outputs are byte-identical (profiles/merge_plan_shapes.txt is the record, in the short form).

Matrices: every structure of every group of tests/kept_structures.py, the S32-band shape in fp64, a band of half-width
40 000 at 2^22 x 32 (the sweep plan) and the C4 stencil stand-in.  Settings: the default knobs, each knob of KNOBS in
turn (applied through mi355_spmv_knobs_reload), and a pattern matrix under the default knobs.  The census at the end
counts the plans under each `merge:` line of tests/plan_census.py; a line nobody matches fails the script.

  python scripts/merge_plan_shapes.py [--full] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = [("MI355_MERGE_BLOCK", "512"), ("MI355_MERGE_TPS", "4"), ("MI355_MERGE_ROWS", "0"), ("MI355_MERGE_ROWS", "1"),
         ("MI355_MERGE_FUSED", "0"), ("MI355_MERGE_FUSED", "1"), ("MI355_MERGE_SEGMENTS", "0"),
         ("MI355_MERGE_WIDE_WINDOW", "0"), ("MI355_SPMV_WINDOW", "0"), ("MI355_SPMV_WINDOW", "1"), ("MI355_SPMV_SWEEP", "1")]


def matrices(sp, torch, dev):
    """(name, n_rows, n_cols, nnz, Ap, Aj, val_dtype), one at a time."""
    import numpy as np
    import kept_structures as ks
    for g in ks.GROUPS.values():
        val = torch.float32 if g.val == np.float32 else torch.float64
        for name in g.structures:
            Ap, Aj, _ = ks.build(g, name)
            yield "%s/%s" % (g.name, name), g.n_rows, g.n_cols, g.nnz, torch.from_numpy(Ap).to(dev), torch.from_numpy(Aj).to(dev), val
    for name, m in (("s32-band-f64", lambda: sp.synth.banded_fixed(1 << 22, 32, 4096, 1, dev, val_dtype=torch.float64)),
                    ("band-40000", lambda: sp.synth.banded_fixed(1 << 22, 32, 40000, 1, dev)),
                    ("c4-stencil", lambda: sp.synth.workload("c4-nlpkkt", device=dev))):
        m = m()
        yield name, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, m.Ax.dtype


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import __graft_entry__ as g
    import plan_census
    sp = g.load_package()
    dev = torch.device("cuda:0")
    for k, _ in KNOBS:
        os.environ.pop(k, None)
    census = [[label, test, 0] for label, test in plan_census.merge_lines()]
    lines = []

    def record(name, setting, n_rows, n_cols, nnz, Ap, Aj, val, mat_dtype=None):
        p = sp.Plan("merge", n_rows, n_cols, nnz, Ap, Aj, val, mat_dtype=mat_dtype)
        info, shape, extra = plan_census.describe(p)
        p.destroy()
        for line in census:
            line[2] += bool(line[1]("merge", info, extra))
        whole = "%s | %s" % (json.dumps(info, sort_keys=True), shape.hex())
        if a.full:
            lines.append("%s | %s | %s" % (name, setting, whole))
        elif setting == "default":
            lines.append("%s | %s %d threads, grid %d, %d kernels, window %d x %d |" % (
                name, info["main_kernel"], info["block_threads"], info["grid_blocks"], info["n_kernels"],
                info["window_elems"], info["window_segments"]))
        if not a.full:
            lines[-1] += " %s:%s" % (setting.replace("MI355_", ""), hashlib.sha256(whole.encode()).hexdigest()[:8])

    for name, n_rows, n_cols, nnz, Ap, Aj, val in matrices(sp, torch, dev):
        record(name, "default", n_rows, n_cols, nnz, Ap, Aj, val)
        record(name, "pattern", n_rows, n_cols, nnz, Ap, Aj, val, "pattern")
        for knob, value in KNOBS:
            os.environ[knob] = value
            sp.capi.lib().mi355_spmv_knobs_reload()
            try:
                record(name, "%s=%s" % (knob, value), n_rows, n_cols, nnz, Ap, Aj, val)
            finally:
                del os.environ[knob]
                sp.capi.lib().mi355_spmv_knobs_reload()
        print(lines[-1][:200], flush=True)
        del Ap, Aj
    for label, _, count in census:
        lines.append("census | %-60s %d" % (label, count))
    print("\n".join(lines[-len(census):]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    missing = [label for label, _, count in census if count == 0]
    if missing:
        sys.exit("no plan under: %s" % "; ".join(missing))


if __name__ == "__main__":
    main()
