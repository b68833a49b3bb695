#!/usr/bin/env python3
"""Time COO -> CSR on the device (mi355_spmv_coo_to_csr) against the host ToCsr (host/load.hpp) on the same box, at
the sizes of two BASELINE configs, and record it (profiles/coo_csr_timing.txt + a rocprofv3 kernel trace):

  c4  the C4 stand-in (27-point stencil, 203^3 = 8.37 M rows, 224 M entries, int64 offsets, fp64 values) as a COO in
      column-major order, the order SuiteSparse files are stored in (the pattern is symmetric, so the column-major
      COO is rows = Aj, cols = the CSR row of each entry)
  c5  the C5 R-MAT-24 edge list (2^24 rows, 2^28 entries, hub rows, int32 offsets, fp32 values), in generation order,
      regenerated as synth.rmat makes it

Every case runs in a child process of its own under `timeout`; the trace is one more child under rocprofv3.  The
device result is compared with the host one entry for entry.

  python scripts/coo_csr_timing.py --out DIR [--reps 5]         everything; writes DIR/coo_csr_timing.txt,
                                                                DIR/coo_csr_kernel_trace.csv, DIR/trace/
  python scripts/coo_csr_timing.py --case c4|c5 [--reps N] [--no-host]     one case, one JSON line
"""
import argparse
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT = 600


def make_case(name, sp, torch, dev):
    if name == "c4":
        m = sp.synth.workload("c4-nlpkkt", device=dev)
        lens = (m.Ap[1:] - m.Ap[:-1]).long()
        rows = m.Aj
        cols = torch.repeat_interleave(torch.arange(m.n_rows, device=dev, dtype=torch.int32), lens)
        return m.n_rows, m.n_cols, rows, cols, m.Ax, torch.int64
    scale, E = 24, 16 << 24
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    a, b, c = 0.57, 0.19, 0.19
    rows = torch.zeros(E, dtype=torch.int32, device=dev)
    cols = torch.zeros(E, dtype=torch.int32, device=dev)
    for _bit in range(scale):
        r = torch.rand(E, generator=g, device=dev, dtype=torch.float32)
        rows.mul_(2).add_((r >= a + b).int())
        cols.mul_(2).add_((((r >= a) & (r < a + b)) | (r >= a + b + c)).int())
        del r
    vals = torch.rand(E, generator=g, device=dev, dtype=torch.float32) * 2 - 1
    return 1 << scale, 1 << scale, rows, cols, vals, torch.int32


def traffic(n_rows, nnz, passes, off_bytes, val_bytes):
    """Bytes the kernels move (each array read or written once per kernel that touches it): the validation pass, per
    radix pass a count (keys) and a scatter (keys + payload in, keys + payload out; the first pass makes its payload),
    the row offsets and the gather (payload, columns, values in; Aj, Ax out)."""
    b = 8 * nnz
    for p in range(passes):
        b += 4 * nnz + (4 if p == 0 else 8) * nnz + 8 * nnz
    b += (n_rows + 1) * off_bytes
    b += nnz * (4 + 4 + val_bytes) + nnz * (4 + val_bytes)
    return b


def run_case(name, reps, host):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    dev = torch.device("cuda:0")
    n_rows, n_cols, rows, cols, vals, off = make_case(name, sp, torch, dev)
    nnz = rows.numel()
    torch.cuda.synchronize()
    ms = []
    for i in range(reps + 1):   # the first call is the warm-up (code objects, allocator)
        t0 = time.perf_counter()
        csr = sp.coo_to_csr(n_rows, n_cols, rows, cols, vals, off)
        t1 = time.perf_counter()
        if i:
            ms.append((t1 - t0) * 1e3)
        if i < reps:
            del csr
    ms.sort()
    passes = (max(n_rows - 1, 0).bit_length() + 7) // 8
    vb, ob = vals.element_size(), (8 if off == torch.int64 else 4)
    moved = traffic(n_rows, nnz, passes, ob, vb)
    algorithmic = nnz * (8 + vb) + (n_rows + 1) * ob + nnz * (4 + vb)
    out = {"case": name, "n_rows": n_rows, "nnz": nnz, "off_bytes": ob, "val_bytes": vb, "passes": passes,
           "reps": reps, "gpu_ms_median": ms[len(ms) // 2], "gpu_ms_min": ms[0], "gpu_ms_max": ms[-1],
           "modelled_bytes": moved, "modelled_GBps": moved / (ms[len(ms) // 2] * 1e6),
           "algorithmic_bytes": algorithmic, "algorithmic_GBps": algorithmic / (ms[len(ms) // 2] * 1e6),
           "workspace_bytes": sp.capi.coo_to_csr_workspace_bytes(n_rows, nnz, off, vals.dtype)}
    if host:
        lib_dir = os.environ.get("COO_CSR_TIMING_TMP", "/tmp")   # where the host helper is built
        so = os.path.join(lib_dir, "libhosttocsr_%d.so" % os.getpid())
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", so,
                        os.path.join(ROOT, "scripts", "host_tocsr.cpp"), "-lpthread"], check=True)
        L = C.CDLL(so)
        L.host_tocsr.restype = C.c_double
        L.host_tocsr.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 6
        hr, hc, hv = rows.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
        Ap = np.empty(n_rows + 1, dtype=np.int64 if ob == 8 else np.int32)
        Aj = np.empty(nnz, dtype=np.int32)
        Ax = np.empty(nnz, dtype=hv.dtype)
        p = lambda a: C.c_void_p(a.ctypes.data)
        secs = L.host_tocsr(int(ob == 8), int(vb == 8), n_rows, n_cols, nnz, p(hr), p(hc), p(hv), p(Ap), p(Aj), p(Ax))
        os.remove(so)
        out["host_ToCsr_s"] = secs
        out["speedup"] = secs * 1e3 / out["gpu_ms_median"]
        out["equal_to_host"] = bool(np.array_equal(csr.Ap.cpu().numpy(), Ap) and np.array_equal(csr.Aj.cpu().numpy(), Aj)
                                    and np.array_equal(csr.Ax.cpu().numpy().view(np.uint8), Ax.view(np.uint8)))
        out["host_threads_used"] = 1
    print(json.dumps(out), flush=True)


def trace_lines(out):
    """The library's own kernels from the trace: their rows of the stats (into the record) and of the kernel trace
    (out/coo_csr_kernel_trace.csv)."""
    lines = []
    for kind in ("kernel_stats", "kernel_trace"):
        found = glob.glob(os.path.join(out, "trace", "**", "*%s.csv" % kind), recursive=True)
        if not found:
            continue
        rows = open(found[0]).read().splitlines()
        keep = rows[:1] + [r for r in rows[1:] if "coo::" in r]
        if kind == "kernel_stats":
            lines.append("# rocprofv3 --kernel-trace --stats, c4, 3 calls (the warm-up and 2 timed), mi355::coo kernels:")
            lines += keep
        else:
            open(os.path.join(out, "coo_csr_kernel_trace.csv"), "w").write("\n".join(keep) + "\n")
    return lines


def child(args, timeout):
    """One step in a child process under timeout; its last JSON line, or None (and the reason printed)."""
    cmd = ["timeout", "-k", "10", str(timeout)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        print("step failed (exit %d): %s" % (r.returncode, " ".join(args)), flush=True)
        return None
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1]) if lines else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["c4", "c5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.reps, not a.no_host)
    if not a.out:
        ap.error("--out DIR is needed to record a run")
    out = a.out
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    results = []
    for case in ("c4", "c5"):
        res = child(me + ["--case", case, "--reps", str(a.reps)], STEP_TIMEOUT)
        if res is None:
            break   # a failed step ends the run: nothing more goes to the device
        results.append(res)
        print(json.dumps(res), flush=True)
    trace_ok = False
    if len(results) == 2:
        tdir = os.path.join(out, "trace")
        shutil.rmtree(tdir, ignore_errors=True)
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", tdir, "-o", "coo_csr", "--"] + me + ["--case", "c4", "--reps", "2", "--no-host"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        trace_ok = r.returncode == 0
        if not trace_ok:
            print("trace step failed (exit %d)" % r.returncode, flush=True)
            sys.stderr.write(r.stderr[-4000:])
    lines = ["# scripts/coo_csr_timing.py: COO -> CSR, device (mi355_spmv_coo_to_csr, median of %d calls after one "
             "warm-up, host clock around the call, which ends in a stream synchronise) against the host ToCsr "
             "(host/load.hpp, one thread) on the same box" % a.reps]
    for r in results:
        lines.append("%s  %d rows  %d entries  off %dB val %dB  %d passes | GPU %.2f ms (min %.2f max %.2f)  "
                     "modelled %.2f GB -> %.0f GB/s, algorithmic %.2f GB -> %.0f GB/s | host ToCsr %.2f s | %.0fx | "
                     "equal to host: %s" % (
                         r["case"], r["n_rows"], r["nnz"], r["off_bytes"], r["val_bytes"], r["passes"],
                         r["gpu_ms_median"], r["gpu_ms_min"], r["gpu_ms_max"], r["modelled_bytes"] / 1e9,
                         r["modelled_GBps"], r["algorithmic_bytes"] / 1e9, r["algorithmic_GBps"],
                         r.get("host_ToCsr_s", float("nan")), r.get("speedup", float("nan")), r.get("equal_to_host")))
    if trace_ok:
        lines += trace_lines(out)
    text = "\n".join(lines) + "\n"
    open(os.path.join(out, "coo_csr_timing.txt"), "w").write(text)
    sys.stdout.write(text)
    return 0 if len(results) == 2 and trace_ok else 1


if __name__ == "__main__":
    sys.exit(main())
