#!/usr/bin/env python3
"""Time one fused sparse-attention execute on 16-bit Q, K, V and O (sp.SparseAttentionPlan(vec_dtype=))
against the fp32 fused execute and against the 16-bit chain, and record it (profiles/attention_half_timing.txt).
scripts/attention_timing.py's method and shapes:

  s32-band      the S32-band target (band of +-4096, 32 per row: every row lies inside a slice)
  s32-rand      2^22 rows x 32, uniformly random columns
  c3-webgoogle  the C3 web-Google stand-in (916 428 rows, 5.1 M entries)
  c5-rmat24     the C5 R-MAT-24 stand-in (2^24 rows, 2^28 entries, hub rows that cross many slices)

int32 offsets, d = dv in {16, 32, 64, 128}, scale d^-0.5, bf16 and fp16, in the same process:
  fused32   one fp32 SparseAttentionPlan.execute (no lse) on the widened operands
  fused16   one SparseAttentionPlan(vec_dtype).execute (no lse)
  chain16   SddmmPlan(vec_dtype).execute -> RowSoftmaxPlan.execute in place -> MultiPlan(vec_dtype, mat_dtype=float32).execute
            on the same 16-bit operands, all plans created beforehand
Recorded: (a) fused16 / fused32, (b) fused16 / chain16, (c) the largest |fused16 - chain16| (both are 16-bit values of
magnitude <= 1).  One process; per (workload, d) all sides are warmed up, then timed in interleaved rounds, each round one
batch between two events on one stream and each timed batch under its own time limit (a batch that has not finished by
then ends the run with status 3).  Reported: the median round with the fastest and the slowest (us per execute).

  python scripts/attention_half_timing.py --out DIR [--rounds 7] [--shapes s32-band,...] [--widths 16,32,64,128] [--types bf16,f16]
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


def time_shape(sp, torch, workload, widths, types, rounds, scale_down):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev, scale_down=scale_down)
    f32 = torch.float32
    res = []
    for d in widths:
        scale = d ** -0.5
        plans, sides, outs = [], {}, {}
        full = {"Q": sp.synth.dense_vector(m.n_rows * d, f32, 7, dev).reshape(m.n_rows, d),
                "K": sp.synth.dense_vector(m.n_cols * d, f32, 11, dev).reshape(m.n_cols, d),
                "V": sp.synth.dense_vector(m.n_cols * d, f32, 13, dev).reshape(m.n_cols, d)}
        S = torch.empty(m.nnz, dtype=f32, device=dev)
        fused32 = sp.SparseAttentionPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, d, d)
        fused32.set_scale(scale)
        plans.append(fused32)
        O32 = torch.full((m.n_rows, d), float("nan"), dtype=f32, device=dev)
        sides["fused32"] = lambda Q=full["Q"], K=full["K"], V=full["V"]: fused32.execute(Q, K, V, O32)
        r = {"workload": workload, "d": d, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "rounds": rounds,
             "batch": BATCH.get(workload, 3), "passes32": fused32.info()["passes"]}
        for name in types:
            T = {"bf16": torch.bfloat16, "f16": torch.float16}[name]
            Q, K, V = (full[k].to(T) for k in "QKV")
            fused = sp.SparseAttentionPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, d, d, vec_dtype=T)
            fused.set_scale(scale)
            p1 = sp.SddmmPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, vec_dtype=T)
            p2 = sp.RowSoftmaxPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32)
            p2.set_scale(scale)
            p3 = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, T, d, mat_dtype=f32)
            plans += [fused, p1, p2, p3]
            O = torch.full((m.n_rows, d), float("nan"), dtype=T, device=dev)
            Y = torch.full((m.n_rows, d), float("nan"), dtype=T, device=dev)
            outs[name] = (O, Y)

            def chain(p1=p1, p2=p2, p3=p3, Q=Q, K=K, V=V, Y=Y):
                p1.execute(None, Q, K, S)
                p2.execute(S, S)
                p3.execute(S, V, Y)

            sides["fused16-" + name] = lambda fused=fused, Q=Q, K=K, V=V, O=O: fused.execute(Q, K, V, O)
            sides["chain16-" + name] = chain
            info = fused.info()
            r["passes16"], r["lanes_per_slot16"], r["n_slices"] = info["passes"], info["lanes_per_slot"], info["n_slices"]
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        for name in types:
            O, Y = outs[name]
            r["max_abs_diff-" + name] = float((O.float() - Y.float()).abs().max())
            r["max_abs_diff32-" + name] = float((O.float() - O32).abs().max())
        for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
            timed(torch, fn, 1)
        us = {side: [] for side in sides}
        for _ in range(rounds):
            for side, fn in sides.items():
                us[side].append(timed(torch, fn, r["batch"]))
        for p in plans:
            p.destroy()
        for side in us:
            v = sorted(us[side])
            r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
        res.append(r)
        print(json.dumps(r), flush=True)
        del full, S, O32, sides, outs, plans
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="s32-band,s32-rand,c3-webgoogle,c5-rmat24")
    ap.add_argument("--widths", default="16,32,64,128")
    ap.add_argument("--types", default="bf16,f16")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("attention_half_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    types = a.types.split(",")
    lines = ["# scripts/attention_half_timing.py: one fused sparse-attention execute on 16-bit Q, K, V, O against the fp32 fused execute "
             "(a = fused16 / fused32) and against the 16-bit chain SddmmPlan(vec_dtype) -> RowSoftmaxPlan (in place) -> "
             "MultiPlan(vec_dtype, mat_dtype=float32) (b = fused16 / chain16; c = max |fused16 - chain16|), int32 offsets, d = dv, "
             "scale d^-0.5%s; one process, %d interleaved rounds, us per execute (median, fastest..slowest round)"
             % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "attention_half_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, [int(w) for w in a.widths.split(",")], types, a.rounds, a.scale_down):
            f32 = r["fused32"]
            for name in types:
                f, c = r["fused16-" + name], r["chain16-" + name]
                lines.append("%-12s d=dv=%-3d %-4s %9d rows %10d nnz %7d slices %d pass C=%d (fp32 %d pass) | fused16 %10.1f us (%.1f..%.1f) | "
                             "fused32 %10.1f us (%.1f..%.1f) | chain16 %10.1f us (%.1f..%.1f) | a fused16 / fused32 %.3f | b fused16 / chain16 %.3f | "
                             "c max|diff| %.2e (to fused32 %.2e)"
                             % (r["workload"], r["d"], name, r["n_rows"], r["nnz"], r["n_slices"], r["passes16"], r["lanes_per_slot16"], r["passes32"],
                                f["median_us"], f["min_us"], f["max_us"], f32["median_us"], f32["min_us"], f32["max_us"], c["median_us"],
                                c["min_us"], c["max_us"], f["median_us"] / f32["median_us"], f["median_us"] / c["median_us"],
                                r["max_abs_diff-" + name], r["max_abs_diff32-" + name]))
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
