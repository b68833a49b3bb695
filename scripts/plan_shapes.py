#!/usr/bin/env python3
"""Every shape a planner gives, as text: for each matrix below and each setting, create the plans — never execute
them — and print one line per matrix (and kind): the default plan in words, then per setting the first 8 hex digits of the
SHA-256 of the whole of Plan.info() and bytes(Plan.shape()) of every plan made under it.  --full FILE also writes a line
per plan with those two whole (the info as JSON, the shape as hex), for finding what differs.  Two builds of the library
plan alike exactly when their outputs are byte-identical (the records, in the short form:
profiles/merge_plan_shapes.txt, profiles/rows_plan_shapes.txt).

Matrices: every structure of every group of tests/kept_structures.py, the S32-band shape in fp64, a band of half-width
40 000 at 2^22 x 32 (the sweep plan) and the C4 stencil stand-in.

  --kind merge   one MERGE plan per setting: the default knobs, each knob of MERGE_KNOBS in turn (applied through
                 mi355_spmv_knobs_reload), and a pattern matrix under the default knobs
  --kind rows    VECTOR and LIGHT; per setting the whole plan and its row blocks, cut into 3 by
                 mi355_spmv_plan_partition and made by mi355_spmv_plan_create_block from the whole plan's shape (what
                 a block inherits): the default knobs, MI355_PLAN_NO_INDEX_COPY, and each knob of ROW_KNOBS in turn

The census at the end counts the plans under each line of tests/plan_census.py for the kind (merge_lines /
row_kind_lines; whole plans only); a line nobody matches fails the script.

  python scripts/plan_shapes.py --kind merge|rows [--out FILE] [--full FILE]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_KNOBS = [("MI355_MERGE_BLOCK", "512"), ("MI355_MERGE_TPS", "4"), ("MI355_MERGE_ROWS", "0"), ("MI355_MERGE_ROWS", "1"),
               ("MI355_MERGE_FUSED", "0"), ("MI355_MERGE_FUSED", "1"), ("MI355_MERGE_SEGMENTS", "0"),
               ("MI355_MERGE_WIDE_WINDOW", "0"), ("MI355_SPMV_WINDOW", "0"), ("MI355_SPMV_WINDOW", "1"), ("MI355_SPMV_SWEEP", "1")]
ROW_KNOBS = [("MI355_SPMV_BLOCK", "256"), ("MI355_SPMV_BLOCK", "512"), ("MI355_SPMV_WINDOW", "0"), ("MI355_SPMV_WINDOW", "1"),
             ("MI355_SPMV_WINDOW_FROM_BAND", "0"), ("MI355_SPMV_SEGMENTS", "0"), ("MI355_SPMV_SWEEP", "1"),
             ("MI355_SPMV_BALANCE", "1"), ("MI355_SPMV_SMALL", "0"), ("MI355_SPMV_LANES", "16"), ("MI355_LIGHT_CHUNK_DIV", "2")]
PARTS = 3


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
    ap.add_argument("--kind", choices=("merge", "rows"), required=True)
    ap.add_argument("--out")
    ap.add_argument("--full")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import __graft_entry__ as g
    import plan_census
    sp = g.load_package()
    dev = torch.device("cuda:0")
    knobs = MERGE_KNOBS if a.kind == "merge" else ROW_KNOBS
    kinds = ("merge",) if a.kind == "merge" else ("vector", "light")
    for k, _ in knobs:
        os.environ.pop(k, None)
    census = [[label, test, 0] for label, test in (plan_census.merge_lines() if a.kind == "merge" else plan_census.row_kind_lines())]
    lines, full = [], []

    def plans(kind, n_rows, n_cols, nnz, Ap, Aj, val, **how):
        """(what, info, shape bytes) of the plan and, for the row kinds, of its row blocks; counts the plan in the census."""
        p = sp.Plan(kind, n_rows, n_cols, nnz, Ap, Aj, val, **how)
        info, shape, extra = plan_census.describe(p)
        for line in census:
            line[2] += bool(line[1](kind, info, extra))
        out = [("whole", info, shape)]
        if kind != "merge":
            rows, chunks, nnzs = p.partition(PARTS)
            for b in range(PARTS):
                if rows[b + 1] == rows[b]:
                    out.append(("block %d" % b, {}, b""))
                    continue
                Ap_b, Aj_b, _, lo = sp.dist.block_view(Ap, Aj, Aj, rows[b], rows[b + 1])
                blk = sp.Plan.block(kind, p.shape(), rows[b], chunks[b], chunks[b + 1] - chunks[b], nnzs[b], rows[b + 1] - rows[b],
                                    n_cols, int(Ap[rows[b + 1]].item()) - lo, Ap_b, Aj_b, val, **how)
                out.append(("block %d" % b, blk.info(), bytes(blk.shape())))
                blk.destroy()
        p.destroy()
        return out

    def record(name, kind, setting, *matrix, **how):
        made = plans(kind, *matrix, **how)
        text = ["%s | %s" % (json.dumps(info, sort_keys=True), shape.hex()) for _, info, shape in made]
        if a.kind == "rows":
            name, text = "%s | %s" % (name, kind), ["%s | %s" % (what, t) for (what, _, _), t in zip(made, text)]
        full.extend("%s | %s | %s" % (name, setting, t) for t in text)
        if setting == "default":
            info = made[0][1]
            lines.append("%s | %s %d threads, grid %d, %d kernels, window %d x %d |" % (
                name, info["main_kernel"], info["block_threads"], info["grid_blocks"], info["n_kernels"],
                info["window_elems"], info["window_segments"]))
        lines[-1] += " %s:%s" % (setting.replace("MI355_", ""), hashlib.sha256("\n".join(text).encode()).hexdigest()[:8])

    for name, *matrix in matrices(sp, torch, dev):
        for kind in kinds:
            record(name, kind, "default", *matrix)
            if a.kind == "merge":
                record(name, kind, "pattern", *matrix, mat_dtype="pattern")
            else:
                record(name, kind, "PLAN_NO_INDEX_COPY", *matrix, flags=sp.capi.PLAN_NO_INDEX_COPY)
            for knob, value in knobs:
                os.environ[knob] = value
                sp.capi.lib().mi355_spmv_knobs_reload()
                try:
                    record(name, kind, "%s=%s" % (knob, value), *matrix)
                finally:
                    del os.environ[knob]
                    sp.capi.lib().mi355_spmv_knobs_reload()
            print(lines[-1][:200], flush=True)
        del matrix
    tail = ["census | %-60s %d" % (label, count) for label, _, count in census]
    print("\n".join(tail), flush=True)
    for path, text in ((a.out, lines), (a.full, full)):
        if path:
            with open(path, "w") as f:
                f.write("\n".join(text + tail) + "\n")
    missing = [label for label, _, count in census if count == 0]
    if missing:
        sys.exit("no plan under: %s" % "; ".join(missing))


if __name__ == "__main__":
    main()
