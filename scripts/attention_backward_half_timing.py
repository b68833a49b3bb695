#!/usr/bin/env python3
"""Time one fused attention-backward execute on 16-bit Q, K, V, O, dO, dQ, dK, dV (sp.SparseAttentionBackwardHalfPlan,
DESIGN.md §3.15.3) against what a 16-bit caller ran before it, and record it (profiles/attention_backward_half_timing.txt).
scripts/attention_backward_timing.py's method and shapes:

  s32-band, s32-rand, c3-webgoogle, c5-rmat24      the shapes of scripts/attention_timing.py

int32 offsets, d = dv in {16, 32, 64, 128}, scale d^-0.5, bf16 and fp16, in the same process:
  fused16   one SparseAttentionBackwardHalfPlan.execute, all three outputs, no dbias
  (a)       one fp32 SparseAttentionBackwardPlan.execute on the widened operands
  (b)       (a) plus the five .float() widenings of Q, K, V, O, dO and the three narrowings of dQ, dK, dV
  split     fused16 with dQ alone, dK alone and dV alone (each: the delta kernel, the role's passes and its fix-up)
The per-kernel split (delta, the three roles, the fix-ups) comes from runs of their own under the profiler, one per
(shape, width, type), with no counters, and is appended to the record by --kernel-stats:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/attention_backward_half_timing.py --out TMP --rounds 2 \
      --shapes s32-band --widths 64 --types bf16
  python scripts/attention_backward_half_timing.py --out profiles --kernel-stats "s32-band d=dv=64 bf16=DIR" [...]
O and lse come from the 16-bit forward.  One process; per (workload, d) all sides are warmed up, then timed in interleaved
rounds, each round one batch between two events on one stream and each timed batch under its own time limit (a batch that
has not finished by then ends the run with status 3).  Reported: the median round with the fastest and the slowest (us per
execute).  Expectations stated in advance: fused16 / (a) <= 1 at d = dv = 16 and 32; < 1 at 64 and 128.

  python scripts/attention_backward_half_timing.py --out DIR [--rounds 7] [--shapes ...] [--widths 16,32,64,128] [--types bf16,f16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-rand": 2, "c5-rmat24": 1, "c3-webgoogle": 5, "s32-band": 2}      # executes per timed round
LIMIT_S = 90.0                                                                  # per timed batch


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
        vec = lambda n, seed: sp.synth.dense_vector(n * d, f32, seed, dev).reshape(n, d)
        full = {"Q": vec(m.n_rows, 7), "K": vec(m.n_cols, 11), "V": vec(m.n_cols, 13), "dO": vec(m.n_rows, 17)}
        for name in types:
            T = {"bf16": torch.bfloat16, "f16": torch.float16}[name]
            Q, K, V, dO = (full[k].to(T) for k in ("Q", "K", "V", "dO"))
            fwd = sp.SparseAttentionPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, d, d, vec_dtype=T)
            fwd.set_scale(scale)
            lse = torch.empty(m.n_rows, dtype=f32, device=dev)
            O = fwd.execute(Q, K, V, lse=lse)
            fwd.destroy()
            fused = sp.SparseAttentionBackwardHalfPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, T, d, d)
            fused.set_scale(scale)
            p32 = sp.SparseAttentionBackwardPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, d, d)
            p32.set_scale(scale)
            out = [torch.full((n, d), float("nan"), dtype=T, device=dev) for n in (m.n_rows, m.n_cols, m.n_cols)]
            out32 = [torch.full((n, d), float("nan"), dtype=f32, device=dev) for n in (m.n_rows, m.n_cols, m.n_cols)]
            wide = [t.float() for t in (Q, K, V, O, dO)]

            def widen_run_narrow():
                w = [t.float() for t in (Q, K, V, O, dO)]
                p32.execute(*w, lse, dQ=out32[0], dK=out32[1], dV=out32[2])
                return [t.to(T) for t in out32]

            sides = {"fused16": lambda: fused.execute(Q, K, V, O, dO, lse, dQ=out[0], dK=out[1], dV=out[2]),
                     "a": lambda: p32.execute(*wide, lse, dQ=out32[0], dK=out32[1], dV=out32[2]),
                     "b": widen_run_narrow,
                     "dq": lambda: fused.execute(Q, K, V, O, dO, lse, dQ=out[0], need=(False, False, False)),
                     "dk": lambda: fused.execute(Q, K, V, O, dO, lse, dK=out[1], need=(False, False, False)),
                     "dv": lambda: fused.execute(Q, K, V, O, dO, lse, dV=out[2], need=(False, False, False))}
            info, info32 = fused.info(), p32.info()
            r = {"workload": workload, "d": d, "type": name, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "rounds": rounds,
                 "batch": BATCH.get(workload, 2), "n_slices": info["n_slices"], "n_slices_t": info["n_slices_t"], "passes16": info["passes"]["dq"],
                 "lanes_per_slot16": info["lanes_per_slot"]["dq"], "passes32": info32["passes"]["dq"]}
            for fn in sides.values():
                fn()
            torch.cuda.synchronize()
            r["max_rel_diff"] = max(float((x.float() - y).abs().max() / y.abs().max()) for x, y in zip(out, out32))
            for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
                timed(torch, fn, 1)
            us = {side: [] for side in sides}
            for _ in range(rounds):
                for side, fn in sides.items():
                    us[side].append(timed(torch, fn, r["batch"]))
            fused.destroy()
            p32.destroy()
            for side in us:
                v = sorted(us[side])
                r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
            res.append(r)
            print(json.dumps(r), flush=True)
            del Q, K, V, dO, O, lse, out, out32, wide, sides
        del full
    return res


def kernel_split(label, directory):
    """One line from a profiler run's kernel statistics (the *kernel_stats.csv under `directory`): the average duration of
    every 16-bit backward kernel, per launch."""
    import csv
    import glob
    import re
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not paths:
        sys.exit("no *kernel_stats.csv under %s" % directory)
    parts = []
    rows = [r for r in csv.DictReader(open(paths[0])) if "attention_bwd_half_" in r["Name"]]
    role = {"0": "DQ", "1": "DK", "2": "DV"}
    for r in sorted(rows, key=lambda r: r["Name"]):
        m = re.search(r"attention_bwd_half_(\w+?)_kernel<([^>]*)>", r["Name"])
        kind, targs = m.group(1), [t.strip() for t in m.group(2).split(",")]
        name = "%s slice C=%s" % (role[targs[3]], targs[2]) if kind == "slice" else kind
        parts.append("%s %.1f us x %d launches" % (name, float(r["AverageNs"]) / 1e3, int(r["Calls"])))
    return "kernels %-28s | %s" % (label, " | ".join(parts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="s32-band,s32-rand,c3-webgoogle,c5-rmat24")
    ap.add_argument("--widths", default="16,32,64,128")
    ap.add_argument("--types", default="bf16,f16")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    ap.add_argument("--kernel-stats", nargs="*", default=None, metavar="LABEL=DIR",
                    help="append the per-kernel split of profiler runs to DIR/attention_backward_half_timing.txt and stop")
    a = ap.parse_args()
    if a.kernel_stats is not None:
        path = os.path.join(a.out, "attention_backward_half_timing.txt")
        lines = ["# per-kernel split: rocprofv3 --kernel-trace --stats, one run per line (its own process, no counters), average per launch; "
                 "the fix-up's launches are those of all three roles"]
        lines += [kernel_split(*item.split("=", 1)) if item.count("=") == 1 else kernel_split(item.rsplit("=", 1)[0], item.rsplit("=", 1)[1])
                  for item in a.kernel_stats]
        with open(path, "a") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("attention_backward_half_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/attention_backward_half_timing.py: one fused attention-backward execute on 16-bit matrices (fused16) against (a) one fp32 "
             "fused execute on the widened operands and (b) that execute plus five .float() widenings and three narrowings; split = fused16 "
             "with dQ / dK / dV alone (each with the delta kernel and its fix-up); int32 offsets, d = dv, scale d^-0.5%s; one process, %d "
             "interleaved rounds, us per execute (median, fastest..slowest round); expectations (DESIGN.md 3.15.3): fused16 / a <= 1 at 16 and "
             "32, < 1 at 64 and 128" % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "attention_backward_half_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, [int(w) for w in a.widths.split(",")], a.types.split(","), a.rounds, a.scale_down):
            f, x, y = r["fused16"], r["a"], r["b"]
            ra = f["median_us"] / x["median_us"]
            ok = ra <= 1.0 if r["d"] <= 32 else ra < 1.0
            lines.append("%-12s d=dv=%-3d %-4s %9d rows %10d nnz %7d + %7d slices %d pass C=%d (fp32 %d pass) | fused16 %10.1f us (%.1f..%.1f) | "
                         "a fp32 %10.1f us (%.1f..%.1f) | b fp32 + casts %10.1f us (%.1f..%.1f) | fused16 / a %.3f | fused16 / b %.3f | "
                         "split dQ %.1f dK %.1f dV %.1f us | max rel diff to a %.2e | expectation %s"
                         % (r["workload"], r["d"], r["type"], r["n_rows"], r["nnz"], r["n_slices"], r["n_slices_t"], r["passes16"],
                            r["lanes_per_slot16"], r["passes32"], f["median_us"], f["min_us"], f["max_us"], x["median_us"], x["min_us"], x["max_us"],
                            y["median_us"], y["min_us"], y["max_us"], ra, f["median_us"] / y["median_us"], r["dq"]["median_us"],
                            r["dk"]["median_us"], r["dv"]["median_us"], r["max_rel_diff"], "HOLDS" if ok else "FAILED"))
            with open(path, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
