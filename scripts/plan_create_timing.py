#!/usr/bin/env python3
"""Time plan creation — the host cost of a planner — for two or more builds of the library in one process, and record it
(profiles/rows_plan_timing.txt):

  s32  the S32-band target (2^22 rows x 32, band of +-4096, fp32, int32 offsets)
  c3   the C3 web-Google stand-in (916 428 rows, 5.1 M entries, fp32, int32 offsets)

for the kinds vector and merge.  MI355_SPMV_PLAN_CACHE=0 is set, so nothing is kept.  Each build is loaded by path
(--lib NAME=PATH, the first one is the baseline) and called through mi355_spmv_plan_create / mi355_spmv_plan_destroy alone.
After a warm-up the builds take turns, round by round; a round is a batch of create + destroy pairs under the host clock
(a create ends in a device-to-host copy, so it is complete when it returns).  Reported per build: the median round, the
fastest and the slowest (us per pair).  A build passes when its median is no slower than the baseline's slowest round.

  python scripts/plan_create_timing.py --out DIR --lib parent=PATH --lib change=PATH [--rounds 15] [--batch 20]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"s32": "s32-band", "c3": "c3-webgoogle"}
KINDS = {"vector": 0, "merge": 1}     # MI355_KIND_* (include/mi355_spmv.h)


def pairs(lib, kind, m, batch):
    """us per create + destroy pair over a batch."""
    h = C.c_void_p()
    t0 = time.perf_counter()
    for _ in range(batch):
        st = lib.mi355_spmv_plan_create(C.byref(h), kind, 0, 0, m.n_rows, m.n_cols, m.nnz, C.c_void_p(m.Ap.data_ptr()),
                                        C.c_void_p(m.Aj.data_ptr()), 0)
        if st != 0 or lib.mi355_spmv_plan_destroy(h) != 0:
            sys.exit("plan_create / plan_destroy failed: %s" % lib.mi355_spmv_last_error().decode())
    return (time.perf_counter() - t0) * 1e6 / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib", action="append", required=True, help="NAME=PATH; the first is the baseline")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    os.environ["MI355_SPMV_PLAN_CACHE"] = "0"
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    libs = {}
    for spec in a.lib:
        name, path = spec.split("=", 1)
        libs[name] = C.CDLL(os.path.abspath(path))
        libs[name].mi355_spmv_last_error.restype = C.c_char_p
        libs[name].mi355_spmv_plan_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int32,
                                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        libs[name].mi355_spmv_plan_destroy.argtypes = [C.c_void_p]
    base = next(iter(libs))
    lines = ["# scripts/plan_create_timing.py: mi355_spmv_plan_create + mi355_spmv_plan_destroy, MI355_SPMV_PLAN_CACHE=0, fp32, int32 "
             "offsets; one process, %d interleaved rounds of %d pairs per build, us per pair (median, fastest..slowest round)"
             % (a.rounds, a.batch)]
    ok = True
    for shape, workload in SHAPES.items():
        m = sp.synth.workload(workload, device=torch.device("cuda:0"))
        for kind, kind_id in KINDS.items():
            for lib in libs.values():
                pairs(lib, kind_id, m, a.batch)      # warm-up: code objects, the analysis buffer
            us = {name: [] for name in libs}
            for _ in range(a.rounds):
                for name, lib in libs.items():
                    us[name].append(pairs(lib, kind_id, m, a.batch))
            us = {name: sorted(v) for name, v in us.items()}
            line = "%-4s %-7s %9d rows %10d nnz |" % (shape, kind, m.n_rows, m.nnz)
            for name, v in us.items():
                not_slower = v[len(v) // 2] <= us[base][-1]
                ok = ok and not_slower
                line += " %s %8.1f us (%.1f..%.1f)%s |" % (name, v[len(v) // 2], v[0], v[-1], "" if name == base else
                                                         " %.3f of %s, not slower than its slowest round: %s" % (
                                                             v[len(v) // 2] / us[base][len(v) // 2], base, not_slower))
            print(line, flush=True)
            lines.append(line)
        del m
    os.makedirs(a.out, exist_ok=True)
    open(os.path.join(a.out, "rows_plan_timing.txt"), "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
