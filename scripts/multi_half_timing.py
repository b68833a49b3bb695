#!/usr/bin/env python3
"""Time one 16-bit multi-vector execute (sp.MultiPlan with float16 / bfloat16 vectors, fp32 arithmetic) against one
fp32 MultiPlan execute on the same structure — what a caller who holds X in 16 bits ran before, without the widening
and narrowing passes it also needed — and record it (profiles/multi_half_timing.txt):

  s32-rand      2^22 rows x 32, uniformly random columns (the gather-bound target)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows)
  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  s32-band      the S32-band target (band of +-4096): the windowed VECTOR kernel's home ground

Vector types bf16 and fp16, the matrix in the vectors' type and in fp32, int32 offsets, k in {8, 16, 32, 64}.  One
process; per (workload, k) every side is warmed up, then timed in interleaved rounds (fp32, bf16, bf16 + fp32 matrix,
fp16, fp16 + fp32 matrix, fp32, ...), each round one batch between two events on one stream and each timed batch under
its own time limit (a batch that has not finished by then ends the run with status 3).  Reported: the median round
with the fastest and the slowest (us per execute of all k vectors), the ratio of the medians 16-bit / fp32, and the
fp32 side's own round-to-round spread (slowest / fastest round).

  python scripts/multi_half_timing.py --out DIR [--rounds 5] [--shapes ...] [--ks 8,16,32,64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-rand": 3, "c5-rmat24": 1, "c3-webgoogle": 10, "s32-band": 5}      # executes per timed round
LIMIT_S = 60.0                                                                   # per timed batch
SIDES = (("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32"))     # (vectors, matrix)


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


def time_shape(sp, torch, workload, ks, rounds):
    dev = torch.device("cuda:0")
    T = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    m = sp.synth.workload(workload, device=dev)
    Ax = {"f32": m.Ax, "f16": m.Ax.to(torch.float16), "bf16": m.Ax.to(torch.bfloat16)}
    out = []
    for k in ks:
        X32 = sp.synth.dense_vector(m.n_cols * k, torch.float32, 11, dev).view(m.n_cols, k)
        X = {"f32": X32, "f16": X32.to(torch.float16), "bf16": X32.to(torch.bfloat16)}
        Y = {t: torch.full((m.n_rows, k), float("nan"), dtype=T[t], device=dev) for t in T}
        plans = {"f32": sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, k)}
        runs = {"f32": lambda: plans["f32"].execute(m.Ax, X["f32"], Y["f32"])}
        for vec, mat in SIDES:
            name = vec if mat == vec else vec + "+f32mat"
            plans[name] = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, T[vec], k, mat_dtype=T[mat])
            runs[name] = (lambda p, a, x, y: lambda: p.execute(a, x, y))(plans[name], Ax[mat], X[vec], Y[vec])
        for _ in range(2):              # warm-up: code objects, clocks, caches
            for fn in runs.values():
                timed(torch, fn, 1)
        # a loose check that the same thing was computed: the 16-bit result against the fp32 one, relative to its size
        scale = float(Y["f32"].abs().max())
        diff = {t: float((Y[t].float() - Y["f32"]).abs().max()) for t in ("f16", "bf16")}
        batch = BATCH.get(workload, 3)
        us = {name: [] for name in runs}
        for _ in range(rounds):
            for name, fn in runs.items():
                us[name].append(timed(torch, fn, batch))
        infos = {name: p.info() for name, p in plans.items()}
        for p in plans.values():
            p.destroy()
        r = {"workload": workload, "n_rows": m.n_rows, "nnz": m.nnz, "k": k, "rounds": rounds, "batch": batch,
             "max_abs_y": scale, "max_abs_diff": diff, "sides": {}}
        for name, v in us.items():
            v = sorted(v)
            r["sides"][name] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "passes": infos[name]["passes"],
                                "kernel": infos[name]["main_kernel"], "scratch_bytes": infos[name]["scratch_bytes"]}
        base = r["sides"]["f32"]
        r["fp32_spread"] = base["max_us"] / base["min_us"]
        for name, s in r["sides"].items():
            s["over_fp32"] = s["median_us"] / base["median_us"]
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="s32-rand,c5-rmat24,c3-webgoogle,s32-band")
    ap.add_argument("--ks", default="8,16,32,64")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("multi_half_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# scripts/multi_half_timing.py: one 16-bit multi-vector execute against one fp32 multi-vector execute on the same "
             "structure, int32 offsets; one process, %d interleaved rounds, us per k vectors: median (fastest..slowest round); "
             "x = median / fp32 median; spread = the fp32 side's slowest / fastest round" % a.rounds]
    path = os.path.join(a.out, "multi_half_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, ks, a.rounds):
            s = r["sides"]
            line = "%-12s %9d rows %10d nnz k %2d | fp32 %d pass %9.1f us (%.1f..%.1f) spread %.3f" % (
                r["workload"], r["n_rows"], r["nnz"], r["k"], s["f32"]["passes"], s["f32"]["median_us"], s["f32"]["min_us"],
                s["f32"]["max_us"], r["fp32_spread"])
            for name in s:
                if name != "f32":
                    line += " | %s %d pass %9.1f us (%.1f..%.1f) x %.3f" % (name, s[name]["passes"], s[name]["median_us"],
                                                                           s[name]["min_us"], s[name]["max_us"], s[name]["over_fp32"])
            line += " | max|diff| f16 %.2e bf16 %.2e of %.2e" % (r["max_abs_diff"]["f16"], r["max_abs_diff"]["bf16"], r["max_abs_y"])
            lines.append(line)
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
