#!/usr/bin/env python3
"""Time one fused attention-backward execute (sp.SparseAttentionBackwardPlan: dQ, dK and dV from O, dO and lse) against the
call-by-call chain of DESIGN.md 3.14 on the plans that existed before it, and record it
(profiles/attention_backward_timing.txt):

  s32-band, s32-rand, c3-webgoogle, c5-rmat24      the shapes of scripts/attention_timing.py

fp32, int32 offsets, d = dv in {16, 32, 64}, scale d^-0.5, in the same process:
  (a) fused   one SparseAttentionBackwardPlan.execute, all three outputs, no dbias
  (b) chain   S = SddmmPlan(Q, K); P = exp(scale S - lse[row]) (torch, in place: a fused caller has no P);
              dP = SddmmPlan(dO, V); dV = TransposedMultiPlan(P, dO); dS = RowSoftmaxPlan.backward(P, dP);
              dQ = MultiPlan(dS, K); dK = TransposedMultiPlan(dS, Q) — every plan, S / P, dP, dS and the outputs made beforehand;
              only the gather lse[row] makes an nnz-sized temporary per execute (counted in the chain's bytes per call)
A loose check that (a) and (b) computed the same thing is recorded with the times, and the bytes each side needs per call
beyond its operands and outputs (fused: none; chain: S / P, dP and dS of nnz values).  One process; per (workload, d) both
sides are warmed up, then timed in interleaved rounds, each round one batch between two events on one stream and each timed
batch under its own time limit.  Reported: the median round with the fastest and the slowest (us per execute) and
fused / chain.

  python scripts/attention_backward_timing.py --out DIR [--rounds 7] [--shapes ...] [--widths 16,32,64]
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


def time_shape(sp, torch, workload, widths, rounds, scale_down):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev, scale_down=scale_down)
    dt = torch.float32
    rows = torch.repeat_interleave(torch.arange(m.n_rows, device=dev), (m.Ap[1:] - m.Ap[:-1]).long())
    res = []
    for d in widths:
        scale = d ** -0.5
        vec = lambda n, seed: sp.synth.dense_vector(n * d, dt, seed, dev).reshape(n, d)
        Q, K, V, dO = vec(m.n_rows, 7), vec(m.n_cols, 11), vec(m.n_cols, 13), vec(m.n_rows, 17)
        fwd = sp.SparseAttentionPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d, d)
        fwd.set_scale(scale)
        lse = torch.empty(m.n_rows, dtype=dt, device=dev)
        O = fwd.execute(Q, K, V, lse=lse)
        fwd.destroy()
        fused = sp.SparseAttentionBackwardPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d, d)
        fused.set_scale(scale)
        p1 = sp.SddmmPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt)
        p2 = sp.RowSoftmaxPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt)
        p2.set_scale(scale)
        p3 = sp.MultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d)
        p4 = sp.TransposedMultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, dt, d)
        out = [torch.full((n, d), float("nan"), dtype=dt, device=dev) for n in (m.n_rows, m.n_cols, m.n_cols)]
        ref = [torch.full((n, d), float("nan"), dtype=dt, device=dev) for n in (m.n_rows, m.n_cols, m.n_cols)]
        S, dP, dS = (torch.empty(m.nnz, dtype=dt, device=dev) for _ in range(3))

        def chain():
            p1.execute(None, Q, K, S)
            S.mul_(scale).sub_(lse[rows]).exp_()        # P, in place
            p1.execute(None, dO, V, dP)
            p4.execute(S, dO, ref[2])
            p2.backward(S, dP, dS)
            p3.execute(dS, K, ref[0])
            p4.execute(dS, Q, ref[1])

        sides = {"fused": lambda: fused.execute(Q, K, V, O, dO, lse, dQ=out[0], dK=out[1], dV=out[2]), "chain": chain}
        info = fused.info()
        r = {"workload": workload, "d": d, "n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "rounds": rounds, "batch": BATCH.get(workload, 2),
             "n_slices": info["n_slices"], "n_slices_t": info["n_slices_t"], "passes": info["passes"]["dq"],
             "fused_held_bytes": info["held_bytes"] + info["scratch_bytes"], "fused_bytes_per_call": 0,
             "chain_bytes_per_call": 3 * 4 * m.nnz + 4 * m.nnz}      # S / P, dP, dS, and the lse[rows] temporary
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        r["max_rel_diff"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(out, ref))
        for fn in list(sides.values()) * 2:         # warm-up: code objects, clocks, caches
            timed(torch, fn, 1)
        us = {side: [] for side in sides}
        for _ in range(rounds):
            for side, fn in sides.items():
                us[side].append(timed(torch, fn, r["batch"]))
        for p in (fused, p1, p2, p3, p4):
            p.destroy()
        for side in us:
            v = sorted(us[side])
            r[side] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
        r["fused_over_chain"] = r["fused"]["median_us"] / r["chain"]["median_us"]
        res.append(r)
        print(json.dumps(r), flush=True)
        del Q, K, V, dO, O, lse, out, ref, S, dP, dS, sides
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
        sys.exit("attention_backward_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/attention_backward_timing.py: one fused attention-backward execute (dQ, dK, dV) against the call-by-call chain of "
             "DESIGN.md 3.14 (P formed from one sddmm and lse), fp32, int32 offsets, d = dv, scale d^-0.5%s; one process, %d interleaved rounds, "
             "us per execute (median, fastest..slowest round); expectation (DESIGN.md 3.15.2): fused / chain <= 1 at d = dv = 16"
             % ("" if a.scale_down == 1 else ", rows / %d" % a.scale_down, a.rounds)]
    path = os.path.join(a.out, "attention_backward_timing.txt")
    for workload in a.shapes.split(","):
        for r in time_shape(sp, torch, workload, [int(w) for w in a.widths.split(",")], a.rounds, a.scale_down):
            f, c = r["fused"], r["chain"]
            verdict = "" if r["d"] != 16 else " | expectation %s" % ("HOLDS" if r["fused_over_chain"] <= 1.0 else "FAILED")
            lines.append("%-12s d=dv=%-3d %9d rows %10d nnz %7d + %7d slices | fused %10.1f us (%.1f..%.1f) | chain %10.1f us (%.1f..%.1f) | "
                         "fused / chain %.3f | bytes per call: fused %d, chain %d (fused holds %d per structure) | max rel diff %.2e%s"
                         % (r["workload"], r["d"], r["n_rows"], r["nnz"], r["n_slices"], r["n_slices_t"], f["median_us"], f["min_us"], f["max_us"],
                            c["median_us"], c["min_us"], c["max_us"], r["fused_over_chain"], r["fused_bytes_per_call"], r["chain_bytes_per_call"],
                            r["fused_held_bytes"], r["max_rel_diff"], verdict))
            with open(path, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
