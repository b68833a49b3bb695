#!/usr/bin/env python3
"""Time one row-softmax execute and one backward (sp.RowSoftmaxPlan: softmax over the stored entries of every row, one pass
over x for the rows that lie inside a slice) and record it (profiles/row_softmax_timing.txt):

  s32-band      the S32-band target (band of +-4096, 32 per row: every row lies inside a slice)
  s32-rand      2^22 rows x 32, uniformly random columns
  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows that cross many slices)

fp32 and fp64, int32 offsets, against two things in the same process:
  (a) copy    a device copy of nnz values (out.copy_(x)): the floor of a forward, 2 x value bytes per nonzero
  (b) torch   torch.sparse.softmax(A, dim=1) on the same matrix as a COO tensor whose values are x, where this torch build
              runs it on the device and the matrix fits (not on c5-rmat24: the COO indices alone are 4 GB); what a caller
              could do before.  A loose check that both computed the same thing is recorded with it.
One process; per (workload, type) all sides are warmed up, then timed in interleaved rounds, each round one batch between
two events on one stream and each timed batch under its own time limit (a batch that has not finished by then ends the run
with status 3).  Reported: the median round with the fastest and the slowest (us per execute), forward / copy, and the
forward's algorithmic bytes — nnz x 2 values + (n_rows + 1) x 4 — as a fraction of 8 TB/s.

  python scripts/row_softmax_timing.py --out DIR [--rounds 9] [--shapes s32-band,s32-rand,c3-webgoogle,c5-rmat24] [--types f32,f64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-rand": 3, "c5-rmat24": 1, "c3-webgoogle": 5, "s32-band": 3}      # executes per timed round
LIMIT_S = 60.0                                                                  # per timed batch
PEAK = 8e12                                                                     # bytes / s


def timed(torch, fn, batch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(batch):
        fn()
    t1.record()
    deadline = time.monotonic() + LIMIT_S
    while not t1.query():
        if time.monotonic() > deadline:
            sys.stderr.write("a timed batch did not finish within %.0f s\n" % LIMIT_S)
            sys.stderr.flush()
            os._exit(3)
        time.sleep(0.0005)
    return t0.elapsed_time(t1) * 1e3 / batch


def torch_side(torch, m, x):
    """torch.sparse.softmax on the matrix as COO with values x, or (None, why not)."""
    try:
        rows = torch.repeat_interleave(torch.arange(m.n_rows, device=x.device), (m.Ap[1:] - m.Ap[:-1]).long())
        A = torch.sparse_coo_tensor(torch.stack([rows, m.Aj.long()]), x, (m.n_rows, m.n_cols), is_coalesced=True)
        torch.sparse.softmax(A, dim=1)
        torch.cuda.synchronize()
        return (lambda: torch.sparse.softmax(A, dim=1)), None
    except Exception as e:     # this build does not run it on the device, or the matrix does not fit
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:120])


def time_shape(sp, torch, workload, types, rounds, scale_down):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev, scale_down=scale_down)
    res = []
    for tname in types:
        dt = {"f32": torch.float32, "f64": torch.float64}[tname]
        plan = sp.RowSoftmaxPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt)
        plan.set_scale(0.125)
        x = (sp.synth.dense_vector(m.nnz, torch.float32, 7, dev) * 8).to(dt)
        dp = sp.synth.dense_vector(m.nnz, torch.float32, 11, dev).to(dt)
        p = torch.full((m.nnz,), float("nan"), dtype=dt, device=dev)
        dx = torch.full((m.nnz,), float("nan"), dtype=dt, device=dev)
        cp = torch.empty_like(x)
        sides = {"forward": lambda: plan.execute(x, p), "backward": lambda: plan.backward(p, dp, dx), "copy": lambda: cp.copy_(x)}
        r = {"workload": workload, "type": tname, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "rounds": rounds,
             "batch": BATCH.get(workload, 3), "n_slices": plan.info()["n_slices"], "scratch_bytes": plan.info()["scratch_bytes"]}
        if workload != "c5-rmat24":
            fn, why = torch_side(torch, m, x * 0.125)
            if fn is not None:
                sides["torch"] = fn
                plan.execute(x, p)
                want = fn().coalesce().values()
                r["max_abs_diff"] = float((p - want).abs().max()) if want.numel() == p.numel() else float("nan")
                del want
            else:
                r["torch_not_run"] = why
        else:
            r["torch_not_run"] = "the COO indices alone are 4 GB"
        for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
            timed(torch, fn, 1)
        us = {side: [] for side in sides}
        for _ in range(rounds):
            for side, fn in sides.items():
                us[side].append(timed(torch, fn, r["batch"]))
        plan.destroy()
        for side in us:
            v = sorted(us[side])
            r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
        r["forward_over_copy"] = r["forward"]["median_us"] / r["copy"]["median_us"]
        r["backward_over_copy"] = r["backward"]["median_us"] / r["copy"]["median_us"]
        r["bytes"] = m.nnz * 2 * x.element_size() + (m.n_rows + 1) * 4
        r["fraction_of_peak"] = r["bytes"] / (r["forward"]["median_us"] * 1e-6) / PEAK
        res.append(r)
        print(json.dumps(r), flush=True)
        del x, dp, p, dx, cp, sides
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--shapes", default="s32-band,s32-rand,c3-webgoogle,c5-rmat24")
    ap.add_argument("--types", default="f32,f64")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("row_softmax_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/row_softmax_timing.py: one row-softmax forward and one backward against a device copy of nnz values and "
             "torch.sparse.softmax, int32 offsets, scale 0.125%s; one process, %d interleaved rounds, us per execute (median, "
             "fastest..slowest round); bytes = the forward's algorithmic bytes, %% = the fraction of 8 TB/s they give"
             % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "row_softmax_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, a.types.split(","), a.rounds, a.scale_down):
            f, b, c = r["forward"], r["backward"], r["copy"]
            line = ("%-12s %s %9d rows %10d nnz %7d slices | forward %10.1f us (%.1f..%.1f) %6.3f GB %5.1f%% | backward %10.1f us "
                    "(%.1f..%.1f) | copy %10.1f us (%.1f..%.1f) | forward / copy %.2f backward / copy %.2f" % (
                        r["workload"], r["type"], r["n_rows"], r["nnz"], r["n_slices"], f["median_us"], f["min_us"], f["max_us"],
                        r["bytes"] / 1e9, 100 * r["fraction_of_peak"], b["median_us"], b["min_us"], b["max_us"], c["median_us"],
                        c["min_us"], c["max_us"], r["forward_over_copy"], r["backward_over_copy"]))
            if "torch" in r:
                t = r["torch"]
                line += " | torch %10.1f us (%.1f..%.1f) forward / torch %.3f | max|diff| %.2e" % (
                    t["median_us"], t["min_us"], t["max_us"], f["median_us"] / t["median_us"], r["max_abs_diff"])
            else:
                line += " | torch not run (%s)" % r["torch_not_run"]
            lines.append(line)
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
