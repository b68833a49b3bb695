#!/usr/bin/env python3
"""Time one multi-vector execute over a semiring (sp.MultiPlan: pattern (or, and), pattern (min, +), valued fp32
(min, +)) against k executes of the corresponding MERGE plan with plan.set_semiring — what a caller with k vectors and a
graph had to do before — and record it (profiles/multi_semiring_timing.txt):

  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows)

fp32 vectors, int32 offsets, k in {4, 8, 16, 32}.  One process; per (workload, case, k) both sides are warmed up, then
timed in interleaved rounds (merge x k, multi, merge x k, ...), each round one batch between two events on one stream and
each timed batch under its own time limit (a batch that has not finished by then ends the run with status 3).
Reported: the median round with the fastest and the slowest (us per execute of all k vectors), multi / (k x merge), and
the effective bytes per vector of each side: (Ap + Aj [+ Ax] once per pass over A, X and Y once) / k.  No threshold is
set: the expectation to confirm or refute is multi < k x merge for k >= 4.

  python scripts/multi_semiring_timing.py --out DIR [--rounds 7] [--shapes c3-webgoogle,c5-rmat24] [--ks 4,8,16,32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"c3-webgoogle": 5, "c5-rmat24": 1}                  # executes of all k vectors per timed round
LIMIT_S = 60.0                                               # per timed batch
CASES = (("pattern", "or_and"), ("pattern", "min_plus"), ("valued", "min_plus"))


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
    out = []
    for mat, semiring in CASES:
        pattern = mat == "pattern"
        mat_dtype = "pattern" if pattern else torch.float32
        Ax = None if pattern else m.Ax
        merge = sp.Plan("merge", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, mat_dtype=mat_dtype)
        merge.set_semiring(semiring)
        for k in ks:
            X = sp.synth.dense_vector(m.n_cols * k, torch.float32, 11, dev).view(m.n_cols, k)
            if semiring == "or_and":
                X = (X > 0.8).to(torch.float32)                     # a frontier: a tenth of the vertices
            xs = [X[:, j].contiguous() for j in range(k)]
            ys = [torch.full((m.n_rows,), float("nan"), device=dev) for _ in range(k)]
            Y = torch.full((m.n_rows, k), float("nan"), device=dev)
            multi = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, k, mat_dtype=mat_dtype, semiring=semiring)
            minfo = multi.info()

            def run_merge():
                for j in range(k):
                    merge.execute(Ax, xs[j], ys[j])

            def run_multi():
                multi.execute(Ax, X, Y)

            for fn in (run_merge, run_multi, run_merge, run_multi):     # warm-up: code objects, clocks, caches
                timed(torch, fn, 1)
            same = all(bool(torch.equal(Y[:, j], ys[j])) for j in range(k))      # min / max / or do not round
            batch = BATCH.get(workload, 3)
            us = {"merge": [], "multi": []}
            for _ in range(rounds):
                us["merge"].append(timed(torch, run_merge, batch))
                us["multi"].append(timed(torch, run_multi, batch))
            multi.destroy()
            r = {"workload": workload, "matrix": mat, "semiring": semiring, "n_rows": m.n_rows, "nnz": m.nnz, "k": k,
                 "rounds": rounds, "batch": batch, "merge_kernel": merge.info()["main_kernel"], "multi_passes": minfo["passes"],
                 "same_bits": same}
            for side in us:
                v = sorted(us[side])
                r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
            r["multi_over_k_merge"] = r["multi"]["median_us"] / r["merge"]["median_us"]
            matrix = 4 * (m.n_rows + 1) + (4 if pattern else 8) * m.nnz
            r["bytes_per_vector_merge"] = matrix + 4 * (m.n_cols + m.n_rows)
            r["bytes_per_vector_multi"] = matrix * minfo["passes"] / k + 4 * (m.n_cols + m.n_rows)
            out.append(r)
            print(json.dumps(r), flush=True)
        merge.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="c3-webgoogle,c5-rmat24")
    ap.add_argument("--ks", default="4,8,16,32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("multi_semiring_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# scripts/multi_semiring_timing.py: k executes of the MERGE plan under a semiring (merge x k) against one multi-vector "
             "execute, fp32 vectors, int32 offsets; one process, %d interleaved rounds, us per k vectors (median, fastest..slowest "
             "round); B/vec = effective bytes per vector (matrix streams / k + x + y)" % a.rounds]
    path = os.path.join(a.out, "multi_semiring_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, ks, a.rounds):
            s, mu = r["merge"], r["multi"]
            lines.append("%-12s %9d rows %10d nnz %-7s %-8s k %2d | merge x k %-22s %10.1f us (%.1f..%.1f) %6.3f GB/vec | multi "
                         "%d pass %10.1f us (%.1f..%.1f) %6.3f GB/vec | multi / (k x merge) %.3f | same bits %s" % (
                             r["workload"], r["n_rows"], r["nnz"], r["matrix"], r["semiring"], r["k"], r["merge_kernel"],
                             s["median_us"], s["min_us"], s["max_us"], r["bytes_per_vector_merge"] / 1e9, r["multi_passes"],
                             mu["median_us"], mu["min_us"], mu["max_us"], r["bytes_per_vector_multi"] / 1e9,
                             r["multi_over_k_merge"], r["same_bits"]))
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
