#!/usr/bin/env python3
"""Time the transposed multi-vector execute (sp.TransposedMultiPlan, Y = A^T X with Ax read in place through the slot map)
against what it replaces, and record it (profiles/multi_transposed_timing.txt).  Per shape and k, four things:

  (a) one TransposedMultiPlan.execute
  (b) one plain MultiPlan.execute on the materialised Apt, Ajt, Ax[perm]: the floor; (a) / (b) is the price of the gather
      inside the walk
  (c) what a caller did per step before: torch.index_select(Ax, 0, perm), then (b)
  (d) torch.sparse.mm(A.t(), X), on the C3 stand-in only

and per shape, once: sp.csr_transpose and the whole create of a TransposedMultiPlan against the device coo_to_csr of the
same entries (wall clock around a synchronised call: creates synchronise).

fp32, int32 offsets, k in {8, 16, 32, 64}; shapes s32-band, s32-rand, c3-webgoogle, c5-rmat24.  One process; per (shape, k)
every side is warmed up, then timed in interleaved rounds, each round one batch between two events on one stream and each
timed batch under its own time limit (a batch that has not finished by then ends the run with status 3).  Reported: the
median round with the fastest and the slowest, in us per execute.

  python scripts/multi_transposed_timing.py --out DIR [--rounds 7] [--shapes ...] [--ks 8,16,32,64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = {"s32-band": 3, "s32-rand": 2, "c3-webgoogle": 10, "c5-rmat24": 1}
LIMIT_S = 60.0


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


def wall_us(torch, fn, repeats=3):
    """The median wall-clock time of a call that synchronises (a create), device idle before it."""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
        if hasattr(r, "destroy"):
            r.destroy()
        del r
    return sorted(out)[len(out) // 2]


def time_shape(sp, torch, workload, ks, rounds):
    dev = torch.device("cuda:0")
    m = sp.synth.workload(workload, device=dev)
    f32 = torch.float32
    rows = torch.repeat_interleave(torch.arange(m.n_rows, dtype=torch.int32, device=dev), (m.Ap[1:] - m.Ap[:-1]).long())
    create = {"csr_transpose_us": wall_us(torch, lambda: sp.csr_transpose(m.n_rows, m.n_cols, m.Ap, m.Aj)),
              "create_transposed_us": wall_us(torch, lambda: sp.TransposedMultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, 8)),
              "coo_to_csr_us": wall_us(torch, lambda: sp.coo_to_csr(m.n_cols, m.n_rows, m.Aj, rows, m.Ax))}
    del rows
    Apt, Ajt, perm = sp.csr_transpose(m.n_rows, m.n_cols, m.Ap, m.Aj)
    perm64 = perm.long()
    Axt = torch.index_select(m.Ax, 0, perm64)
    out = []
    for k in ks:
        X = sp.synth.dense_vector(m.n_rows * k, f32, 11, dev).view(m.n_rows, k)
        Y = [torch.full((m.n_cols, k), float("nan"), device=dev) for _ in range(2)]
        tp = sp.TransposedMultiPlan(m.n_rows, m.n_cols, m.nnz, m.Ap, m.Aj, f32, k)
        plain = sp.MultiPlan(m.n_cols, m.n_rows, m.nnz, Apt, Ajt, f32, k)
        sides = {"a_transposed": lambda: tp.execute(m.Ax, X, Y[0]),
                 "b_plain_materialised": lambda: plain.execute(Axt, X, Y[1]),
                 "c_index_select_then_plain": lambda: plain.execute(torch.index_select(m.Ax, 0, perm64), X, Y[1])}
        if workload == "c3-webgoogle":
            A = torch.sparse_csr_tensor(m.Ap.long(), m.Aj.long(), m.Ax, (m.n_rows, m.n_cols)).to_sparse_coo().t().coalesce()
            sides["d_torch_sparse_mm"] = lambda: torch.sparse.mm(A, X)
        for _ in range(2):
            for fn in sides.values():
                timed(torch, fn, 1)
        same = bool(torch.equal(Y[0].view(torch.int32), Y[1].view(torch.int32)))
        batch = BATCH.get(workload, 2)
        us = {s: [] for s in sides}
        for _ in range(rounds):
            for s, fn in sides.items():
                us[s].append(timed(torch, fn, batch))
        info = tp.info()
        tp.destroy()
        plain.destroy()
        r = dict(create, workload=workload, n_rows=m.n_rows, n_cols=m.n_cols, nnz=m.nnz, k=k, rounds=rounds, batch=batch,
                 kernel=info["main_kernel"], passes=info["passes"], a_equals_b_bit_for_bit=same)
        for s in us:
            v = sorted(us[s])
            r[s] = {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}
        r["a_over_b"] = r["a_transposed"]["median_us"] / r["b_plain_materialised"]["median_us"]
        r["a_over_c"] = r["a_transposed"]["median_us"] / r["c_index_select_then_plain"]["median_us"]
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="s32-band,s32-rand,c3-webgoogle,c5-rmat24")
    ap.add_argument("--ks", default="8,16,32,64")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    if not torch.cuda.is_available():
        sys.exit("multi_transposed_timing.py needs a GPU: a time taken anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# scripts/multi_transposed_timing.py: (a) TransposedMultiPlan.execute, (b) MultiPlan.execute on the materialised Apt / Ajt / "
             "Ax[perm], (c) torch.index_select(Ax, 0, perm) + (b), (d) torch.sparse.mm(A.t(), X); fp32, int32 offsets; one process, "
             "%d interleaved rounds, us per execute (median, fastest..slowest round); creates: wall clock, median of 3" % a.rounds]
    path = os.path.join(a.out, "multi_transposed_timing.txt")
    for workload in a.shapes.split(","):
        res = time_shape(sp, torch, workload, ks, a.rounds)
        r = res[0]
        lines.append("%-12s %9d x %9d %10d nnz | csr_transpose %.0f us | create_transposed %.0f us | device coo_to_csr of the same entries %.0f us" % (
            workload, r["n_rows"], r["n_cols"], r["nnz"], r["csr_transpose_us"], r["create_transposed_us"], r["coo_to_csr_us"]))
        for r in res:
            fmt = lambda s: "%9.1f us (%.1f..%.1f)" % (r[s]["median_us"], r[s]["min_us"], r[s]["max_us"])
            d = " | (d) " + fmt("d_torch_sparse_mm") if "d_torch_sparse_mm" in r else ""
            lines.append("%-12s k %2d %d pass | (a) %s | (b) %s | (c) %s%s | a / b %.3f | a / c %.3f | a == b bit for bit: %s" % (
                workload, r["k"], r["passes"], fmt("a_transposed"), fmt("b_plain_materialised"), fmt("c_index_select_then_plain"), d,
                r["a_over_b"], r["a_over_c"], r["a_equals_b_bit_for_bit"]))
        open(path, "w").write("\n".join(lines) + "\n")       # (after every workload: a later one may run out of time)
    sys.stdout.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
