#!/usr/bin/env python3
"""Time the heads of sparse attention in one call against the same heads call by call, and record it
(profiles/attention_heads_timing.txt):

  s32-band, s32-rand, c3-webgoogle, c5-rmat24      the shapes of scripts/attention_timing.py
  target-2^14, target-2^17                         the target's shape (32 entries per row in a band) at 2^14 and 2^17 rows

d = dv in {16, 32, 64}, fp32 and bf16, int32 offsets, scale d^-0.5, forward and backward (all three outputs, no dbias), the
interleaved (n, H, d) layout, H = 8 where the operands of a run stay under 32 GB and otherwise the largest power of two that
does (the line says which).  The two sides, on the SAME object in the same process:
  (a) heads    one execute on 3-D operands (mi355_spmv_attention[_bwd]_execute_heads)
  (b) single   H executes, one per head, on the 2-D views of the same tensors
A check that (a) and (b) wrote the same bits is recorded with the times.  Per line both sides are warmed up, then timed in
interleaved rounds, each round one batch between two events on one stream and each timed batch under its own time limit; the
script ends at the first failure.  Reported: the median round with the fastest and the slowest (us per H heads), heads /
single, and each side's spread (slowest - fastest) / median.  The expectations, stated before anything was measured:
  1  on target-2^14, where one head's grid is smaller than the device, heads < single;
  2  on every other shape heads is not slower than single by more than single's own spread in the same run.

  python scripts/attention_heads_timing.py --out DIR [--rounds 7] [--shapes ...] [--widths 16,32,64] [--types f32,bf16] [--directions fwd,bwd]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 90.0              # per timed batch
BUDGET = 32 * 2 ** 30       # bytes of operands per run
SMALL = "target-2^14"


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


def structure(sp, torch, name, scale_down):
    dev = torch.device("cuda:0")
    if name.startswith("target-2^"):
        return sp.synth.banded_fixed((1 << int(name.split("^")[1])) // scale_down, 32, 4096, 1, dev, name=name)
    return sp.synth.workload(name, device=dev, scale_down=scale_down)


def time_line(sp, torch, m, workload, d, vec, direction, rounds):
    dev = torch.device("cuda:0")
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[vec]
    es = 4 if vec == "f32" else 2
    matrices = 4 if direction == "fwd" else 8            # Q K V O; and dO dQ dK dV
    H = 8
    while H > 1 and H * d * es * matrices * max(m.n_rows, m.n_cols) > BUDGET:
        H //= 2
    scale = d ** -0.5
    rnd = lambda n, seed: sp.synth.dense_vector(n * H * d, torch.float32, seed, dev).reshape(n, H, d).to(dt)
    Q, K, V = rnd(m.n_rows, 7), rnd(m.n_cols, 11), rnd(m.n_cols, 13)
    fwd = sp.SparseAttentionPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, d, d, vec_dtype=None if vec == "f32" else dt, n_heads_max=H)
    fwd.set_scale(scale)
    lse = torch.empty((H, m.n_rows), dtype=torch.float32, device=dev)
    O = fwd.execute(Q, K, V, lse=lse)
    if direction == "fwd":
        plan, outs = fwd, [[torch.full_like(O, float("nan")), torch.full_like(lse, float("nan"))] for _ in range(2)]
        heads = lambda: plan.execute(Q, K, V, out=outs[0][0], lse=outs[0][1])

        def single():
            for h in range(H):
                plan.execute(Q[:, h], K[:, h], V[:, h], out=outs[1][0][:, h], lse=outs[1][1][h])
    else:
        fwd.destroy()
        dO = rnd(m.n_rows, 17)
        if vec == "f32":
            plan = sp.SparseAttentionBackwardPlan.with_heads(H, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d, d)
        else:
            plan = sp.SparseAttentionBackwardHalfPlan.with_heads(H, m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d, d)
        plan.set_scale(scale)
        outs = [[torch.full_like(t, float("nan")) for t in (Q, K, V)] for _ in range(2)]
        heads = lambda: plan.execute(Q, K, V, O, dO, lse, dQ=outs[0][0], dK=outs[0][1], dV=outs[0][2])

        def single():
            for h in range(H):
                plan.execute(Q[:, h], K[:, h], V[:, h], O[:, h], dO[:, h], lse[h], dQ=outs[1][0][:, h], dK=outs[1][1][:, h], dV=outs[1][2][:, h])
    sides = {"heads": heads, "single": single}
    info = plan.info()
    batch = max(1, min(20, int(4e6 // (m.nnz * H // 8 + 1)) + 1))
    r = {"workload": workload, "direction": direction, "type": vec, "d": d, "H": H, "n_rows": m.n_rows, "nnz": m.nnz, "n_slices": info["n_slices"],
         "grid_blocks": info["grid_blocks"], "scratch_bytes": info["scratch_bytes"], "rounds": rounds, "batch": batch}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    r["same_bits"] = all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(*outs))
    for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
        timed(torch, fn, 1)
    us = {side: [] for side in sides}
    for _ in range(rounds):
        for side, fn in sides.items():
            us[side].append(timed(torch, fn, batch))
    plan.destroy()
    for side in us:
        v = sorted(us[side])
        r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "spread": (v[-1] - v[0]) / v[len(v) // 2]}
    r["heads_over_single"] = r["heads"]["median_us"] / r["single"]["median_us"]
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="target-2^14,target-2^17,s32-band,s32-rand,c3-webgoogle,c5-rmat24")
    ap.add_argument("--widths", default="16,32,64")
    ap.add_argument("--types", default="f32,bf16")
    ap.add_argument("--directions", default="fwd,bwd")
    ap.add_argument("--scale-down", type=int, default=1, help="shrink the row counts (a trial of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("attention_heads_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/attention_heads_timing.py: one execute of H heads (3-D operands, interleaved (n, H, d)) against H single-head executes on the "
             "same object, int32 offsets, d = dv, scale d^-0.5%s; one process, %d interleaved rounds, us per H heads (median, fastest..slowest round), "
             "spread = (slowest - fastest) / median; expectations: 1 (%s) heads < single; 2 (every other shape) heads <= single * (1 + single's spread)"
             % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds, SMALL)]
    path = os.path.join(a.out, "attention_heads_timing.txt")
    for workload in a.shapes.split(","):
        m = structure(sp, torch, workload, a.scale_down)
        for direction in a.directions.split(","):
            for vec in a.types.split(","):
                for d in [int(w) for w in a.widths.split(",")]:
                    r = time_line(sp, torch, m, workload, d, vec, direction, a.rounds)
                    h, s = r["heads"], r["single"]
                    if workload == SMALL:
                        verdict = "expectation 1 %s" % ("HOLDS" if h["median_us"] < s["median_us"] else "FAILED")
                    else:
                        verdict = "expectation 2 %s" % ("HOLDS" if h["median_us"] <= s["median_us"] * (1 + s["spread"]) else "FAILED")
                    lines.append("%-12s %s %-4s d=dv=%-3d H=%d%s %9d rows %10d nnz %7d slices | heads %10.1f us (%.1f..%.1f, spread %.3f) | "
                                 "single %10.1f us (%.1f..%.1f, spread %.3f) | heads / single %.3f | same bits %s | %s"
                                 % (workload, direction, vec, d, r["H"], "" if r["H"] == 8 else " (32 GB)", r["n_rows"], r["nnz"], r["n_slices"],
                                    h["median_us"], h["min_us"], h["max_us"], h["spread"], s["median_us"], s["min_us"], s["max_us"], s["spread"],
                                    r["heads_over_single"], r["same_bits"], verdict))
                    with open(path, "w") as fh:
                        fh.write("\n".join(lines) + "\n")
                    if not r["same_bits"]:
                        sys.exit("the heads execute and the single-head executes differ: " + lines[-1])
        del m
        torch.cuda.empty_cache()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
