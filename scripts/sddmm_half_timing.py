#!/usr/bin/env python3
"""Time one SDDMM execute on 16-bit U and V (sp.SddmmPlan(..., torch.float32, vec_dtype=torch.bfloat16 / torch.float16))
against one fp32 SddmmPlan execute at the same k on the same matrix in the same process, and record it
(profiles/sddmm_half_timing.txt):

  s32-rand      2^22 rows x 32, uniformly random columns (gather-bound)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows)
  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  s32-band      the S32-band target (band of +-4096)

fp32 values (Ax, out), int32 offsets, k in {8, 16, 32, 64, 128}, valued (Ax) and pattern (Ax = None).  The 16-bit
operands are the fp32 ones rounded to the type, so all three sides make the same gathers: rows of 2k bytes against rows
of 4k, with half the lanes per slot.  One process; per (workload, k, valued) all sides are warmed up, then timed in
interleaved rounds, each round one batch between two events on one stream and each timed batch under its own time limit
(a batch that has not finished by then ends the run with status 3).  Reported: the median round with the fastest and the
slowest (us per execute) of each side, and bf16 / fp32 and fp16 / fp32 from this run's own fp32 figure.  A loose check that
the same thing was computed goes with each line: max |out16 - out32| (the 16-bit operands are rounded, so it is of the
size of their rounding, not of fp32's).

  python scripts/sddmm_half_timing.py --out DIR [--rounds 9] [--shapes s32-rand,c5-rmat24,c3-webgoogle,s32-band] [--ks 8,16,32,64,128]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-rand": 3, "c5-rmat24": 1, "c3-webgoogle": 5, "s32-band": 3}      # executes per timed round
LIMIT_S = 60.0                                                                  # per timed batch


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


def time_shape(sp, torch, workload, ks, rounds, scale_down):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev, scale_down=scale_down)
    types = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
    plans = {name: sp.SddmmPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, vec_dtype=t) for name, t in types.items()}
    outs = {name: torch.full((m.nnz,), float("nan"), device=dev) for name in types}
    res = []
    for k in ks:
        U = sp.synth.dense_vector(m.n_rows * k, torch.float32, 7, dev).view(m.n_rows, k)
        V = sp.synth.dense_vector(m.n_cols * k, torch.float32, 11, dev).view(m.n_cols, k)
        ops = {name: (U, V) if t is None else (U.to(t), V.to(t)) for name, t in types.items()}
        for valued in (True, False):
            ax = m.Ax if valued else None
            sides = {name: (lambda n=name: plans[n].execute(ax, ops[n][0], ops[n][1], outs[n])) for name in types}
            for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
                timed(torch, fn, 1)
            r = {"workload": workload, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "k": k, "valued": valued,
                 "rounds": rounds, "batch": BATCH.get(workload, 3), "max_abs": float(outs["fp32"].abs().max())}
            for name in ("bf16", "fp16"):
                r["max_abs_diff_" + name] = float((outs[name] - outs["fp32"]).abs().max())
            us = {side: [] for side in sides}
            for _ in range(rounds):
                for side, fn in sides.items():
                    us[side].append(timed(torch, fn, r["batch"]))
            for side in us:
                v = sorted(us[side])
                r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
            for name in ("bf16", "fp16"):
                r[name + "_over_fp32"] = r[name]["median_us"] / r["fp32"]["median_us"]
            res.append(r)
            print(json.dumps(r), flush=True)
        del U, V, ops, sides
    for p in plans.values():
        p.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--shapes", default="s32-rand,c5-rmat24,c3-webgoogle,s32-band")
    ap.add_argument("--ks", default="8,16,32,64,128")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("sddmm_half_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# scripts/sddmm_half_timing.py: one SDDMM execute on 16-bit U / V against one fp32 SddmmPlan execute at the same k, "
             "fp32 Ax / out, int32 offsets%s; one process, %d interleaved rounds, us per execute (median, fastest..slowest round); "
             "the ratios are medians of this run" % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "sddmm_half_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, ks, a.rounds, a.scale_down):
            side = lambda n: "%s %10.1f us (%.1f..%.1f)" % (n, r[n]["median_us"], r[n]["min_us"], r[n]["max_us"])
            lines.append("%-12s %9d rows %10d nnz k %3d %-7s | %s | %s | %s | bf16 / fp32 %.3f  fp16 / fp32 %.3f | max|diff| %.2e %.2e of %.2e" % (
                r["workload"], r["n_rows"], r["nnz"], r["k"], "valued" if r["valued"] else "pattern", side("fp32"), side("bf16"),
                side("fp16"), r["bf16_over_fp32"], r["fp16_over_fp32"], r["max_abs_diff_bf16"], r["max_abs_diff_fp16"], r["max_abs"]))
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
