#!/usr/bin/env python3
"""Time one fused sparse-attention execute (sp.SparseAttentionPlan: O = softmax(scale Q K^T on A) V in one pass over A)
against the three-plan chain it replaces, and record it (profiles/attention_timing.txt):

  s32-band      the S32-band target (band of +-4096, 32 per row: every row lies inside a slice)
  s32-rand      2^22 rows x 32, uniformly random columns
  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows that cross many slices)

fp32, int32 offsets, d = dv in {16, 32, 64}, scale d^-0.5, in the same process:
  (a) fused   one SparseAttentionPlan.execute (no lse)
  (b) chain   SddmmPlan.execute -> RowSoftmaxPlan.execute in place -> MultiPlan.execute on the same operands, all plans
              created beforehand: what a caller did before
  (c) dense   on c3-webgoogle, where n_rows x n_cols fp32 scores fit in 8 GB (they do not at full size: recorded as not
              run): torch.softmax(masked_fill(Q K^T * scale, ~mask, -inf)) @ V
A loose check that (a) and (b) computed the same thing is recorded with the times.  One process; per (workload, d) all
sides are warmed up, then timed in interleaved rounds, each round one batch between two events on one stream and each
timed batch under its own time limit (a batch that has not finished by then ends the run with status 3).  Reported: the
median round with the fastest and the slowest (us per execute) and fused / chain.

  python scripts/attention_timing.py --out DIR [--rounds 7] [--shapes s32-band,s32-rand,c3-webgoogle,c5-rmat24] [--widths 16,32,64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-rand": 3, "c5-rmat24": 1, "c3-webgoogle": 5, "s32-band": 3}      # executes per timed round
LIMIT_S = 60.0                                                                  # per timed batch
DENSE_LIMIT = 8 << 30                                                           # bytes of dense fp32 scores


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


def time_shape(sp, torch, workload, widths, rounds, scale_down):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev, scale_down=scale_down)
    dt = torch.float32
    res = []
    for d in widths:
        scale = d ** -0.5
        Q = sp.synth.dense_vector(m.n_rows * d, dt, 7, dev).reshape(m.n_rows, d)
        K = sp.synth.dense_vector(m.n_cols * d, dt, 11, dev).reshape(m.n_cols, d)
        V = sp.synth.dense_vector(m.n_cols * d, dt, 13, dev).reshape(m.n_cols, d)
        fused = sp.SparseAttentionPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d, d)
        fused.set_scale(scale)
        p1 = sp.SddmmPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt)
        p2 = sp.RowSoftmaxPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt)
        p2.set_scale(scale)
        p3 = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d)
        O = torch.full((m.n_rows, d), float("nan"), dtype=dt, device=dev)
        Y = torch.full((m.n_rows, d), float("nan"), dtype=dt, device=dev)
        S = torch.empty(m.nnz, dtype=dt, device=dev)

        def chain():
            p1.execute(None, Q, K, S)
            p2.execute(S, S)
            p3.execute(S, V, Y)

        sides = {"fused": lambda: fused.execute(Q, K, V, O), "chain": chain}
        info = fused.info()
        r = {"workload": workload, "d": d, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "rounds": rounds,
             "batch": BATCH.get(workload, 3), "n_slices": info["n_slices"], "passes": info["passes"], "scratch_bytes": info["scratch_bytes"]}
        fused.execute(Q, K, V, O)
        chain()
        torch.cuda.synchronize()
        r["max_abs_diff"] = float((O - Y).abs().max())
        if workload == "c3-webgoogle":
            if m.n_rows * m.n_cols * 4 <= DENSE_LIMIT:
                rows = torch.repeat_interleave(torch.arange(m.n_rows, device=dev), (m.Ap[1:] - m.Ap[:-1]).long())
                mask = torch.zeros((m.n_rows, m.n_cols), dtype=torch.bool, device=dev)
                mask[rows, m.Aj.long()] = True
                dense = lambda: torch.nan_to_num(torch.softmax((Q @ K.t() * scale).masked_fill(~mask, float("-inf")), dim=1)) @ V
                r["dense_max_abs_diff"] = float((dense() - O).abs().max())
                sides["dense"] = dense
            else:
                r["dense_not_run"] = "%d x %d fp32 scores are %.0f GB" % (m.n_rows, m.n_cols, m.n_rows * m.n_cols * 4 / 2 ** 30)
        for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
            timed(torch, fn, 1)
        us = {side: [] for side in sides}
        for _ in range(rounds):
            for side, fn in sides.items():
                us[side].append(timed(torch, fn, r["batch"]))
        for p in (fused, p1, p2, p3):
            p.destroy()
        for side in us:
            v = sorted(us[side])
            r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
        r["fused_over_chain"] = r["fused"]["median_us"] / r["chain"]["median_us"]
        res.append(r)
        print(json.dumps(r), flush=True)
        del Q, K, V, O, Y, S, sides
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="s32-band,s32-rand,c3-webgoogle,c5-rmat24")
    ap.add_argument("--widths", default="16,32,64")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("attention_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/attention_timing.py: one fused sparse-attention execute against the chain SddmmPlan -> RowSoftmaxPlan (in place) -> "
             "MultiPlan on the same operands, fp32, int32 offsets, d = dv, scale d^-0.5%s; one process, %d interleaved rounds, us per "
             "execute (median, fastest..slowest round)" % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "attention_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, [int(w) for w in a.widths.split(",")], a.rounds, a.scale_down):
            f, c = r["fused"], r["chain"]
            line = ("%-12s d=dv=%-3d %9d rows %10d nnz %7d slices %d pass | fused %10.1f us (%.1f..%.1f) | chain %10.1f us (%.1f..%.1f) | "
                    "fused / chain %.3f | max|diff| %.2e" % (r["workload"], r["d"], r["n_rows"], r["nnz"], r["n_slices"], r["passes"], f["median_us"],
                                                           f["min_us"], f["max_us"], c["median_us"], c["min_us"], c["max_us"],
                                                           r["fused_over_chain"], r["max_abs_diff"]))
            if "dense" in r:
                t = r["dense"]
                line += " | dense %10.1f us (%.1f..%.1f) fused / dense %.4f max|diff| %.2e" % (
                    t["median_us"], t["min_us"], t["max_us"], f["median_us"] / t["median_us"], r["dense_max_abs_diff"])
            elif "dense_not_run" in r:
                line += " | dense not run (%s)" % r["dense_not_run"]
            lines.append(line)
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
