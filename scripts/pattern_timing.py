#!/usr/bin/env python3
"""Time a pattern MERGE plan (MI355_VAL_PATTERN: no Ax stream) against the valued MERGE plan of the same matrix executed
with Ax = ones — the code path a caller with a value-free matrix had to take before — and record it
(profiles/pattern_timing.txt):

  c3   the C3 web-Google stand-in (916 428 rows, 5.1 M entries, fp32, int32 offsets)
  c5   the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows, fp32, int32 offsets)
  s32  the S32-band target (2^22 rows x 32, band of +-4096, fp32): informational — the valued plan takes the
       row-parallel run kernel there, which has no pattern form

One process; per shape both plans are warmed up, then timed in interleaved rounds (valued, pattern, valued, ...), each
round a batch of back-to-back executes between two events on one stream.  Reported per plan: the median round, the
fastest and the slowest (us per call), and the plan's main_kernel.  A shape passes when the pattern plan's median is no
slower than the valued plan's median by more than the spread (slowest - fastest round) of the valued plan in this run.
The two results are also compared bit for bit.

  python scripts/pattern_timing.py --out DIR [--rounds 15] [--shapes c3,c5,s32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c3": ("c3-webgoogle", 50), "c5": ("c5-rmat24", 5), "s32": ("s32-band", 20)}   # workload, executes per round


def time_shape(sp, torch, name, rounds):
    workload, batch = SHAPES[name]
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev)
    ones = torch.ones(m.nnz, dtype=torch.float32, device=dev)
    x = sp.synth.dense_vector(m.n_cols, torch.float32, 11, dev)
    plans = {"valued": sp.Plan("merge", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32),
             "pattern": sp.Plan("merge", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, mat_dtype="pattern")}
    ys = {k: torch.full((m.n_rows,), float("nan"), device=dev) for k in plans}
    run = {"valued": lambda: plans["valued"].execute(ones, x, ys["valued"]),
           "pattern": lambda: plans["pattern"].execute(None, x, ys["pattern"])}
    for k in plans:                      # warm-up: code objects, clocks, caches
        for _ in range(max(3, batch // 2)):
            run[k]()
    torch.cuda.synchronize()
    equal = bool(torch.equal(ys["valued"].view(torch.int32), ys["pattern"].view(torch.int32)))
    us = {k: [] for k in plans}
    for _ in range(rounds):
        for k in ("valued", "pattern"):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(batch):
                run[k]()
            t1.record()
            t1.synchronize()
            us[k].append(t0.elapsed_time(t1) * 1e3 / batch)
    out = {"shape": name, "workload": workload, "n_rows": m.n_rows, "nnz": m.nnz, "rounds": rounds, "batch": batch,
           "bitwise_equal": equal}
    for k in plans:
        v = sorted(us[k])
        info = plans[k].info()
        out[k] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "main_kernel": info["main_kernel"],
                  "n_kernels": info["n_kernels"], "window_elems": info["window_elems"], "grid_blocks": info["grid_blocks"]}
        plans[k].destroy()
    spread = out["valued"]["max_us"] - out["valued"]["min_us"]
    out["valued_spread_us"] = spread
    out["pattern_over_valued"] = out["pattern"]["median_us"] / out["valued"]["median_us"]
    out["not_slower"] = bool(out["pattern"]["median_us"] <= out["valued"]["median_us"] + spread)
    # matrix bytes per call: Ap + Aj (+ Ax); x and y on top for both
    out["matrix_bytes_valued"] = 4 * (m.n_rows + 1) + 8 * m.nnz
    out["matrix_bytes_pattern"] = 4 * (m.n_rows + 1) + 4 * m.nnz
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--shapes", default="c3,c5,s32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/pattern_timing.py: MERGE plan with Ax = ones (valued) against the pattern MERGE plan, fp32 vectors, "
             "int32 offsets; one process, %d interleaved rounds per plan, us per execute (median, fastest..slowest round)" % a.rounds]
    ok = True
    for name in a.shapes.split(","):
        r = time_shape(sp, torch, name, a.rounds)
        print(json.dumps(r), flush=True)
        v, p = r["valued"], r["pattern"]
        lines.append("%-4s %-14s %9d rows %10d nnz | valued %-18s %9.1f us (%.1f..%.1f) | pattern %-18s %9.1f us (%.1f..%.1f) | "
                     "pattern/valued %.3f | valued spread %.1f us | not slower: %s | bitwise equal: %s" % (
                         r["shape"], r["workload"], r["n_rows"], r["nnz"], v["main_kernel"], v["median_us"], v["min_us"],
                         v["max_us"], p["main_kernel"], p["median_us"], p["min_us"], p["max_us"], r["pattern_over_valued"],
                         r["valued_spread_us"], r["not_slower"], r["bitwise_equal"]))
        if name != "s32":                # the band is informational
            ok = ok and r["not_slower"]
    text = "\n".join(lines) + "\n"
    open(os.path.join(a.out, "pattern_timing.txt"), "w").write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
