#!/usr/bin/env python3
"""Time VECTOR plans whose matrix is stored in 16 bits (MI355_VAL_F16 / MI355_VAL_BF16 under fp32 x and y) against the
fp32 VECTOR plan of the same structure, each with the packed index (the default) and with MI355_PLAN_NO_INDEX_COPY, and
record it (profiles/half_matrix_timing.txt):

  s32    the S32-band target (2^22 rows x 32, band of +-4096, int32 offsets)
  mid    the same band with 2^18 rows: a mid-size matrix, one round of the chip
  cant   the C2 cant stand-in (62 451 rows, ~4.0 M entries): a small matrix, every plan runs the plain one-pass kernel

One process; per shape the six plans are warmed up, then timed in interleaved rounds (fp32, f16, bf16, fp32 no-copy, ...),
each round a batch of back-to-back executes between two events on one stream.  Reported per plan: the median round, the
fastest and the slowest (us per call), its main_kernel and the bytes per nonzero it streams; per 16-bit plan its ratio to
the fp32 plan of the same flags next to the ratio of the algorithmic bytes (Ap, index, values, x once, y once) and to the
spread (slowest - fastest round) of that fp32 plan.  No threshold: the record says what was measured.  The 16-bit values
are the fp32 ones narrowed by mi355_spmv_narrow_values; every 16-bit y is compared bit for bit with the fp32 plan's y on
the widened values.

  python scripts/half_matrix_timing.py --out DIR [--rounds 15] [--shapes s32,mid,cant]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"s32": ("s32-band", 20), "mid": ("mid-band-2^18", 50), "cant": ("c2-cant", 50)}   # workload, executes per round


def matrix(sp, name, dev):
    if name == "mid":
        return sp.synth.banded_fixed(1 << 18, 32, 4096, 1, dev, name="S32-band-2^18")
    return sp.synth.workload(SHAPES[name][0], device=dev)


def time_shape(sp, torch, name, rounds):
    workload, batch = SHAPES[name]
    dev = torch.device("cuda:0")
    m = matrix(sp, name, dev)
    x = sp.synth.dense_vector(m.n_cols, torch.float32, 11, dev)
    types = (("fp32", None), ("f16", torch.float16), ("bf16", torch.bfloat16))
    keys, plans, values, ys = [], {}, {}, {}
    for flag_name, flags in (("packed", 0), ("no-copy", sp.capi.PLAN_NO_INDEX_COPY)):
        for tname, dtype in types:
            k = "%s %s" % (tname, flag_name)
            keys.append(k)
            plans[k] = sp.Plan("vector", m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, torch.float32, flags=flags, mat_dtype=dtype)
            values[k] = m.Ax if dtype is None else sp.narrow_values(m.Ax, dtype)
            ys[k] = torch.full((m.n_rows,), float("nan"), device=dev)
    run = {k: (lambda k=k: plans[k].execute(values[k], x, ys[k])) for k in keys}
    for k in keys:                       # warm-up: code objects, clocks, caches
        for _ in range(max(3, batch // 2)):
            run[k]()
    torch.cuda.synchronize()
    # bit for bit: the 16-bit plan against the fp32 plan of the same flags on the widened values
    equal = {}
    for k in keys:
        if k.startswith("fp32"):
            continue
        ref = torch.full((m.n_rows,), float("nan"), device=dev)
        plans["fp32 " + k.split(" ", 1)[1]].execute(values[k].to(torch.float32), x, ref)
        torch.cuda.synchronize()
        equal[k] = bool(torch.equal(ys[k].view(torch.int32), ref.view(torch.int32)))
    us = {k: [] for k in keys}
    for _ in range(rounds):
        for k in keys:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(batch):
                run[k]()
            t1.record()
            t1.synchronize()
            us[k].append(t0.elapsed_time(t1) * 1e3 / batch)
    out = {"shape": name, "workload": workload, "n_rows": m.n_rows, "nnz": m.nnz, "rounds": rounds, "batch": batch,
           "bitwise_equal_to_fp32_on_widened": equal, "plans": {}}
    for k in keys:
        v = sorted(us[k])
        info = plans[k].info()
        idx = 2 if info["packed_index_bytes"] > 0 else 4
        val = 4 if k.startswith("fp32") else 2
        out["plans"][k] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "main_kernel": info["main_kernel"],
                           "block_threads": info["block_threads"], "window_elems": info["window_elems"],
                           "bytes_per_nnz": idx + val,
                           "algorithmic_bytes": m.nnz * (idx + val) + 4 * (m.n_rows + 1) + 4 * m.n_cols + 4 * m.n_rows}
        plans[k].destroy()
    for k in keys:
        if k.startswith("fp32"):
            continue
        base = out["plans"]["fp32 " + k.split(" ", 1)[1]]
        p = out["plans"][k]
        p["over_fp32"] = p["median_us"] / base["median_us"]
        p["bytes_over_fp32"] = p["algorithmic_bytes"] / base["algorithmic_bytes"]
        p["fp32_spread_us"] = base["max_us"] - base["min_us"]
        p["ahead_by_more_than_the_fp32_spread"] = bool(base["median_us"] - p["median_us"] > p["fp32_spread_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--shapes", default="s32,mid,cant")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    os.makedirs(a.out, exist_ok=True)
    lines = ["# scripts/half_matrix_timing.py: VECTOR plans, fp32 x and y, int32 offsets, the matrix in fp32 / fp16 / bf16, with the "
             "packed index and with MI355_PLAN_NO_INDEX_COPY; one process, %d interleaved rounds per plan, us per execute "
             "(median, fastest..slowest round); B/nnz = index + value bytes streamed per nonzero" % a.rounds]
    for name in a.shapes.split(","):
        r = time_shape(sp, torch, name, a.rounds)
        print(json.dumps(r), flush=True)
        lines.append("%s %s: %d rows, %d nnz" % (r["shape"], r["workload"], r["n_rows"], r["nnz"]))
        for k, p in r["plans"].items():
            line = "  %-13s %-26s %4d threads  %d B/nnz  %9.1f us (%.1f..%.1f)" % (
                k, p["main_kernel"], p["block_threads"], p["bytes_per_nnz"], p["median_us"], p["min_us"], p["max_us"])
            if "over_fp32" in p:
                line += " | /fp32 %.3f (bytes predict %.3f) | fp32 spread %.1f us | ahead by more than it: %s | bitwise equal to fp32 on widened: %s" % (
                    p["over_fp32"], p["bytes_over_fp32"], p["fp32_spread_us"], p["ahead_by_more_than_the_fp32_spread"],
                    r["bitwise_equal_to_fp32_on_widened"][k])
            lines.append(line)
    text = "\n".join(lines) + "\n"
    open(os.path.join(a.out, "half_matrix_timing.txt"), "w").write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
