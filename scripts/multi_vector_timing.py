#!/usr/bin/env python3
"""Time one multi-vector execute (sp.MultiPlan, Y = A X for k vectors in one pass over A) against k executes of the
`auto` plan on the same matrix — what a caller with k right-hand sides had to do before — and record it
(profiles/multi_vector_timing.txt):

  s32-rand   2^22 rows x 32, uniformly random columns (the gather-bound target)
  c5-rmat24  the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows)
  s32-band   the S32-band target (band of +-4096): the windowed VECTOR kernel's home ground

fp32, int32 offsets, k in {4, 8, 16, 32}.  One process; per (workload, k) both sides are warmed up, then timed in
interleaved rounds (single x k, multi, single x k, ...), each round one batch between two events on one stream and
each timed batch under its own time limit (a batch that has not finished by then ends the run with status 3).
Reported: the median round with the fastest and the slowest (us per execute of all k vectors), multi / (k x single),
and the effective bytes per vector of each side: (Ap + Aj + Ax once per pass over A, X and Y once) / k.

  python scripts/multi_vector_timing.py --out DIR [--rounds 9] [--shapes s32-rand,c5-rmat24,s32-band] [--ks 4,8,16,32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-rand": 3, "c5-rmat24": 1, "s32-band": 5}      # executes of all k vectors per timed round
LIMIT_S = 60.0                                               # per timed batch


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
    m = sp.synth.workload(workload, device=dev)
    single = sp.Plan("auto", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32)
    sinfo = single.info()
    out = []
    for k in ks:
        X = sp.synth.dense_vector(m.n_cols * k, torch.float32, 11, dev).view(m.n_cols, k)
        xs = [X[:, j].contiguous() for j in range(k)]
        ys = [torch.full((m.n_rows,), float("nan"), device=dev) for _ in range(k)]
        Y = torch.full((m.n_rows, k), float("nan"), device=dev)
        multi = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, k)
        minfo = multi.info()

        def run_single():
            for j in range(k):
                single.execute(m.Ax, xs[j], ys[j])

        def run_multi():
            multi.execute(m.Ax, X, Y)

        for fn in (run_single, run_multi, run_single, run_multi):       # warm-up: code objects, clocks, caches
            timed(torch, fn, 1)
        # the two sides agree to summation order (fp32: a loose check that the same thing was computed)
        err = max(float((Y[:, j] - ys[j]).abs().max()) for j in range(k))
        scale = max(float(ys[j].abs().max()) for j in range(k))
        batch = BATCH.get(workload, 3)
        us = {"single": [], "multi": []}
        for _ in range(rounds):
            us["single"].append(timed(torch, run_single, batch))
            us["multi"].append(timed(torch, run_multi, batch))
        multi.destroy()
        r = {"workload": workload, "n_rows": m.n_rows, "nnz": m.nnz, "k": k, "rounds": rounds, "batch": batch,
             "single_kernel": sinfo["main_kernel"], "multi_kernel": minfo["main_kernel"], "multi_passes": minfo["passes"],
             "multi_scratch_bytes": minfo["scratch_bytes"], "max_abs_diff": err, "max_abs_y": scale}
        for side in us:
            v = sorted(us[side])
            r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
        r["multi_over_k_single"] = r["multi"]["median_us"] / r["single"]["median_us"]
        matrix = 4 * (m.n_rows + 1) + 8 * m.nnz
        r["bytes_per_vector_single"] = matrix + 4 * (m.n_cols + m.n_rows)
        r["bytes_per_vector_multi"] = matrix * minfo["passes"] / k + 4 * (m.n_cols + m.n_rows)
        out.append(r)
        print(json.dumps(r), flush=True)
    single.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--shapes", default="s32-rand,c5-rmat24,s32-band")
    ap.add_argument("--ks", default="4,8,16,32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("multi_vector_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# scripts/multi_vector_timing.py: k executes of the auto plan (single x k) against one multi-vector execute, fp32, "
             "int32 offsets; one process, %d interleaved rounds, us per k vectors (median, fastest..slowest round); "
             "B/vec = effective bytes per vector (matrix streams / k + x + y)" % a.rounds]
    path = os.path.join(a.out, "multi_vector_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, ks, a.rounds):
            s, mu = r["single"], r["multi"]
            lines.append("%-10s %9d rows %10d nnz k %2d | single x k %-24s %10.1f us (%.1f..%.1f) %6.2f GB/vec | multi %-18s "
                         "%d pass %10.1f us (%.1f..%.1f) %6.2f GB/vec | multi / (k x single) %.3f | max|diff| %.2e of %.2e" % (
                             r["workload"], r["n_rows"], r["nnz"], r["k"], r["single_kernel"], s["median_us"], s["min_us"],
                             s["max_us"], r["bytes_per_vector_single"] / 1e9, r["multi_kernel"], r["multi_passes"],
                             mu["median_us"], mu["min_us"], mu["max_us"], r["bytes_per_vector_multi"] / 1e9,
                             r["multi_over_k_single"], r["max_abs_diff"], r["max_abs_y"]))
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
