#!/usr/bin/env python3
"""Time one SDDMM execute (sp.SddmmPlan: dot(U[r], V[c]) at every stored entry of A, one pass over A) against one
multi-vector execute (sp.MultiPlan, Y = A X) at the same k on the same matrix in the same process, and record it
(profiles/sddmm_timing.txt):

  s32-rand      2^22 rows x 32, uniformly random columns (gather-bound)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows)
  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  s32-band      the S32-band target (band of +-4096)

fp32, int32 offsets, k in {8, 16, 32, 64}, valued (Ax) and pattern (Ax = None; the multi side is then a pattern plan).
Both make the same gathers of rows of V / X; SDDMM re-reads a row of U that consecutive nonzeros share and writes 4 bytes
per nonzero where the multi kind writes a row of Y.  On c3-webgoogle only, where it fits in memory, the torch expression
(U[rows] * V[Aj]).sum(1) — what a caller could do before — is timed as well.  One process; per (workload, k, valued)
all sides are warmed up, then timed in interleaved rounds, each round one batch between two events on one stream and
each timed batch under its own time limit (a batch that has not finished by then ends the run with status 3).
Reported: the median round with the fastest and the slowest (us per execute), sddmm / multi, and SDDMM's algorithmic
bytes — nnz x (4 + 4 valued + 4 out) + (n_rows + 1) x 4 + (n_rows + n_cols) x k x 4 — as a fraction of 8 TB/s.

  python scripts/sddmm_timing.py --out DIR [--rounds 9] [--shapes s32-rand,c5-rmat24,c3-webgoogle,s32-band] [--ks 8,16,32,64]
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


def time_shape(sp, torch, workload, ks, rounds, scale_down):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev, scale_down=scale_down)
    sddmm = sp.SddmmPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32)
    with_torch = workload == "c3-webgoogle"
    rows = torch.repeat_interleave(torch.arange(m.n_rows, device=dev), (m.Ap[1:] - m.Ap[:-1]).long()) if with_torch else None
    aj = m.Aj.long() if with_torch else None
    out = torch.full((m.nnz,), float("nan"), device=dev)
    res = []
    for k in ks:
        U = sp.synth.dense_vector(m.n_rows * k, torch.float32, 7, dev).view(m.n_rows, k)
        V = sp.synth.dense_vector(m.n_cols * k, torch.float32, 11, dev).view(m.n_cols, k)
        Y = torch.full((m.n_rows, k), float("nan"), device=dev)
        for valued in (True, False):
            multi = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, k, mat_dtype=None if valued else "pattern")
            ax = m.Ax if valued else None
            sides = {"sddmm": lambda: sddmm.execute(ax, U, V, out), "multi": lambda: multi.execute(ax, V, Y)}
            if with_torch:
                sides["torch"] = (lambda: (U[rows] * V[aj]).sum(1) * m.Ax) if valued else (lambda: (U[rows] * V[aj]).sum(1))
            for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
                timed(torch, fn, 1)
            r = {"workload": workload, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "k": k, "valued": valued,
                 "rounds": rounds, "batch": BATCH.get(workload, 3), "multi_passes": multi.info()["passes"]}
            if with_torch:      # a loose check that the same thing was computed (fp32, another order of addition)
                want = sides["torch"]()
                r["max_abs_diff"], r["max_abs"] = float((out - want).abs().max()), float(want.abs().max())
                del want
            us = {side: [] for side in sides}
            for _ in range(rounds):
                for side, fn in sides.items():
                    us[side].append(timed(torch, fn, r["batch"]))
            multi.destroy()
            for side in us:
                v = sorted(us[side])
                r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
            r["sddmm_over_multi"] = r["sddmm"]["median_us"] / r["multi"]["median_us"]
            r["bytes"] = m.nnz * (4 + (4 if valued else 0) + 4) + (m.n_rows + 1) * 4 + (m.n_rows + m.n_cols) * k * 4
            r["fraction_of_peak"] = r["bytes"] / (r["sddmm"]["median_us"] * 1e-6) / PEAK
            res.append(r)
            print(json.dumps(r), flush=True)
        del U, V, Y
    sddmm.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--shapes", default="s32-rand,c5-rmat24,c3-webgoogle,s32-band")
    ap.add_argument("--ks", default="8,16,32,64")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("sddmm_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# scripts/sddmm_timing.py: one SDDMM execute against one multi-vector execute at the same k, fp32, int32 offsets%s; "
             "one process, %d interleaved rounds, us per execute (median, fastest..slowest round); bytes = SDDMM's algorithmic "
             "bytes, %% = the fraction of 8 TB/s they give" % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "sddmm_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, ks, a.rounds, a.scale_down):
            s, mu = r["sddmm"], r["multi"]
            line = ("%-12s %9d rows %10d nnz k %2d %-7s | sddmm %10.1f us (%.1f..%.1f) %6.3f GB %5.1f%% | multi %d pass %10.1f us "
                    "(%.1f..%.1f) | sddmm / multi %.3f" % (
                        r["workload"], r["n_rows"], r["nnz"], r["k"], "valued" if r["valued"] else "pattern", s["median_us"],
                        s["min_us"], s["max_us"], r["bytes"] / 1e9, 100 * r["fraction_of_peak"], r["multi_passes"], mu["median_us"],
                        mu["min_us"], mu["max_us"], r["sddmm_over_multi"]))
            if "torch" in r:
                t = r["torch"]
                line += " | torch %10.1f us (%.1f..%.1f) sddmm / torch %.3f | max|diff| %.2e of %.2e" % (
                    t["median_us"], t["min_us"], t["max_us"], s["median_us"] / t["median_us"], r["max_abs_diff"], r["max_abs"])
            lines.append(line)
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
