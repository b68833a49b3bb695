#!/usr/bin/env python3
"""Time the symmetric COO -> CSR on the device (mi355_spmv_coo_to_csr_symmetric, on the STORED entries) against the
path it replaces and against the host, and record it (profiles/coo_sym_timing.txt):

  (a) the symmetric call on the stored entries; end to end = upload of the stored arrays + the count
      (mi355_spmv_coo_symmetric_nnz) + the call
  (b) the path before it: the host expansion loop (host/load.hpp, one thread, timed on its own) + the upload of the
      expanded arrays + mi355_spmv_coo_to_csr on them
  (c) the host alone: expansion + ToCsr (host/load.hpp, one thread)

Cases:
  c4   the lower triangle, diagonal included, of the C4 stand-in (27-point stencil, 203^3 rows; 116 M stored entries
       -> 224 M), stored column-major, int64 offsets, fp64 values
  mid  a random symmetric pattern, 2^20 rows, 8 M stored entries in shuffled order, int32 offsets, fp32 values

Host clock around each call including its synchronise, median of --reps after one warm-up, all legs interleaved in one
process.  Every case runs in a child process of its own under `timeout`, the kernel trace is one more child under
rocprofv3, and every exit status is checked: a failed step ends the run.

  python scripts/coo_sym_timing.py --out DIR [--reps 5]        everything; writes DIR/coo_sym_timing.txt
  python scripts/coo_sym_timing.py --case c4|mid [--reps N] [--device-only]     one case, one JSON line
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
STEP_TIMEOUT = 900


def make_case(name, sp, torch, dev):
    """Stored entries on the device: n, rows, cols, vals, offset dtype."""
    if name == "c4":
        m = sp.synth.workload("c4-nlpkkt", device=dev)
        lens = (m.Ap[1:] - m.Ap[:-1]).long()
        csr_row = torch.repeat_interleave(torch.arange(m.n_rows, device=dev, dtype=torch.int32), lens)
        keep = m.Aj >= csr_row                       # column-major COO of a symmetric pattern: (Aj[k], CSR row of k)
        return m.n_rows, m.Aj[keep].contiguous(), csr_row[keep].contiguous(), m.Ax[keep].contiguous(), torch.int64
    n, nnz = 1 << 20, 8 << 20
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    a = torch.randint(0, n, (nnz,), generator=g, device=dev, dtype=torch.int32)
    b = torch.randint(0, n, (nnz,), generator=g, device=dev, dtype=torch.int32)
    vals = torch.rand(nnz, generator=g, device=dev, dtype=torch.float32) * 2 - 1
    return n, torch.maximum(a, b), torch.minimum(a, b), vals, torch.int32


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def run_case(name, reps, device_only):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as g
    sp = g.load_package()
    dev = torch.device("cuda:0")
    n, rows, cols, vals, off = make_case(name, sp, torch, dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    nnz = rows.numel()
    expanded = sp.coo_symmetric_nnz(rows, cols)
    hr, hc, hv = rows.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy()
    ob, vb = (8 if off == torch.int64 else 4), vals.element_size()
    L = sp.capi.lib()
    ot, vt = sp.capi.OFF_TYPES[off][0], sp.capi.VAL_TYPES[vals.dtype][0]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    # outputs and workspaces once: the timed calls allocate nothing
    Ap = torch.empty(n + 1, dtype=off, device=dev)
    Aj = torch.empty(expanded, dtype=torch.int32, device=dev)
    Ax = torch.empty(expanded, dtype=vals.dtype, device=dev)
    ws_a = torch.empty(sp.capi.coo_to_csr_symmetric_workspace_bytes(n, nnz, expanded, off, vals.dtype),
                       dtype=torch.uint8, device=dev)
    ws_b = torch.empty(sp.capi.coo_to_csr_workspace_bytes(n, expanded, off, vals.dtype), dtype=torch.uint8, device=dev)

    def call_a(r, c, v):
        size = C.c_size_t(ws_a.numel())
        st = L.mi355_spmv_coo_to_csr_symmetric(ot, vt, n, n, nnz, expanded, p(r), p(c), p(v), p(Ap), p(Aj), p(Ax), None,
                                               p(ws_a), C.byref(size), stream)
        assert st == 0, L.mi355_spmv_last_error()

    def call_b(r, c, v):
        size = C.c_size_t(ws_b.numel())
        st = L.mi355_spmv_coo_to_csr(ot, vt, n, n, expanded, p(r), p(c), p(v), p(Ap), p(Aj), p(Ax), None, p(ws_b),
                                     C.byref(size), stream)
        assert st == 0, L.mi355_spmv_last_error()

    host = None
    if not device_only:
        lib_dir = os.environ.get("COO_SYM_TIMING_TMP", "/tmp")   # where the host helper is built
        so = os.path.join(lib_dir, "libhostsym_%d.so" % os.getpid())
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", so,
                        os.path.join(ROOT, "scripts", "host_expand.cpp"), os.path.join(ROOT, "scripts", "host_tocsr.cpp"),
                        "-lpthread"], check=True)
        host = C.CDLL(so)
        os.remove(so)
        host.host_expand.restype = C.c_double
        host.host_expand.argtypes = [C.c_int, C.c_int32, C.c_int64, C.c_int64] + [C.c_void_p] * 6
        host.host_tocsr.restype = C.c_double
        host.host_tocsr.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 6
    q = lambda a: C.c_void_p(a.ctypes.data)
    er, ec, ev = (np.empty(expanded, dtype=np.int32), np.empty(expanded, dtype=np.int32), np.empty(expanded, dtype=hv.dtype))
    hAp = np.empty(n + 1, dtype=np.int64 if ob == 8 else np.int32)
    hAj, hAx = np.empty(expanded, dtype=np.int32), np.empty(expanded, dtype=hv.dtype)
    t = {k: [] for k in ("a_device", "a_count", "a_upload", "b_device", "b_expand", "b_upload", "c_tocsr")}
    clock = time.perf_counter
    equal = {}
    for i in range(reps + 1):   # the first round is the warm-up (code objects, allocator, page faults)
        rec = {}
        t0 = clock(); call_a(rows, cols, vals); rec["a_device"] = clock() - t0
        if i == reps:
            got_a = [x.cpu().numpy() for x in (Ap, Aj, Ax)]
        t0 = clock(); sp.coo_symmetric_nnz(rows, cols); rec["a_count"] = clock() - t0
        if host is not None:
            t0 = clock()
            up = [torch.from_numpy(a).to(dev) for a in (hr, hc, hv)]
            torch.cuda.synchronize()
            rec["a_upload"] = clock() - t0
            del up
            rec["b_expand"] = host.host_expand(int(vb == 8), n, nnz, expanded, q(hr), q(hc), q(hv), q(er), q(ec), q(ev))
            assert rec["b_expand"] >= 0
            t0 = clock()
            d_er, d_ec, d_ev = [torch.from_numpy(a).to(dev) for a in (er, ec, ev)]
            torch.cuda.synchronize()
            rec["b_upload"] = clock() - t0
        elif i == 0:            # the expanded arrays made on the device, once (not timed)
            reps_ = 1 + (rows != cols).long()
            src = torch.repeat_interleave(torch.arange(nnz, device=dev), reps_)
            mirror = torch.zeros(expanded, dtype=torch.bool, device=dev)
            mirror[(torch.cumsum(reps_, 0) - 1)[reps_ == 2]] = True
            d_er = torch.where(mirror, cols[src], rows[src]).contiguous()
            d_ec = torch.where(mirror, rows[src], cols[src]).contiguous()
            d_ev = vals[src].contiguous()
            del reps_, src, mirror
        t0 = clock(); call_b(d_er, d_ec, d_ev); rec["b_device"] = clock() - t0
        if i == reps:
            equal["b_equals_a"] = all(np.array_equal(x.cpu().numpy().view(np.uint8), y.view(np.uint8))
                                      for x, y in zip((Ap, Aj, Ax), got_a))
        if host is not None:
            del d_er, d_ec, d_ev
            rec["c_tocsr"] = host.host_tocsr(int(ob == 8), int(vb == 8), n, n, expanded, q(er), q(ec), q(ev), q(hAp),
                                             q(hAj), q(hAx))
            if i == reps:
                equal["host_equals_a"] = all(np.array_equal(x.view(np.uint8), y.view(np.uint8))
                                             for x, y in zip((hAp, hAj, hAx), got_a))
        if i:
            for k, v in rec.items():
                t[k].append(v * 1e3)
    out = {"case": name, "n_rows": n, "nnz_stored": nnz, "nnz_expanded": expanded, "off_bytes": ob, "val_bytes": vb,
           "reps": reps, "stored_bytes": nnz * (8 + vb), "expanded_bytes": expanded * (8 + vb),
           "workspace_a": ws_a.numel(), "workspace_b": ws_b.numel()}
    out.update({k: stats(v) for k, v in t.items() if v})
    out.update(equal)
    print(json.dumps(out), flush=True)


def child(args, timeout):
    """One step in a child process under timeout; (its last JSON line or None, ok)."""
    cmd = ["timeout", "-k", "10", str(timeout)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        print("step failed (exit %d): %s" % (r.returncode, " ".join(args)), flush=True)
        return None, False
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return (json.loads(lines[-1]) if lines else None), True


def describe(r):
    f = lambda k: "%.2f (min %.2f max %.2f)" % (r[k]["median"], r[k]["min"], r[k]["max"])
    a_e2e = r["a_upload"]["median"] + r["a_count"]["median"] + r["a_device"]["median"]
    b_e2e = r["b_expand"]["median"] + r["b_upload"]["median"] + r["b_device"]["median"]
    c_all = r["b_expand"]["median"] + r["c_tocsr"]["median"]
    spread = max(r[k]["max"] - r[k]["min"] for k in ("a_device", "b_device"))
    return [
        "%s  %d rows  %d stored -> %d expanded entries  off %dB val %dB  (stored arrays %.2f GB, expanded %.2f GB; "
        "workspace (a) %.2f GB, (b) %.2f GB)" % (r["case"], r["n_rows"], r["nnz_stored"], r["nnz_expanded"], r["off_bytes"],
                                                 r["val_bytes"], r["stored_bytes"] / 1e9, r["expanded_bytes"] / 1e9,
                                                 r["workspace_a"] / 1e9, r["workspace_b"] / 1e9),
        "  (a) symmetric call, device   %s ms   | count query %s ms | upload of the stored arrays %s ms | end to end %.1f ms"
        % (f("a_device"), f("a_count"), f("a_upload"), a_e2e),
        "  (b) coo_to_csr on expanded   %s ms   | host expansion loop %s ms | upload of the expanded arrays %s ms | end to end %.1f ms"
        % (f("b_device"), f("b_expand"), f("b_upload"), b_e2e),
        "  (c) host expansion + host ToCsr  %.1f ms (ToCsr alone %s ms)" % (c_all, f("c_tocsr")),
        "  device (a) - (b) = %+.2f ms; largest min-max spread of the two = %.2f ms; end to end (b) / (a) = %.1fx, (c) / (a) = %.1fx; "
        "(b) equals (a): %s, host equals (a): %s" % (r["a_device"]["median"] - r["b_device"]["median"], spread, b_e2e / a_e2e,
                                                      c_all / a_e2e, r.get("b_equals_a"), r.get("host_equals_a")),
    ]


def trace_lines(tdir):
    found = glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return ["# (no kernel_stats.csv in the trace)"]
    rows = open(found[0]).read().splitlines()
    return (["# rocprofv3 --kernel-trace --stats, c4, 3 rounds of (a) then (b) on the device (the warm-up and 2 timed), "
             "mi355::coo kernels ((a) alone: validate_symmetric, offdiag_count, check_count, expand, gather_symmetric, "
             "offdiag_total; (b) alone: validate, gather; the sort's kernels serve both):"]
            + rows[:1] + [r for r in rows[1:] if "coo::" in r])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["c4", "mid"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.reps, a.device_only)
    if not a.out:
        ap.error("--out DIR is needed to record a run")
    os.makedirs(a.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    results = []
    for case in ("mid", "c4"):
        res, ok = child(me + ["--case", case, "--reps", str(a.reps)], STEP_TIMEOUT)
        if not ok or res is None:
            break   # a failed step ends the run: nothing more goes to the device
        results.append(res)
        print(json.dumps(res), flush=True)
    trace_ok = False
    tdir = os.path.join(a.out, "coo_sym_trace")
    if len(results) == 2:
        shutil.rmtree(tdir, ignore_errors=True)
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", tdir, "-o", "coo_sym", "--"] + me + ["--case", "c4", "--reps", "2", "--device-only"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        trace_ok = r.returncode == 0
        if not trace_ok:
            print("trace step failed (exit %d)" % r.returncode, flush=True)
            sys.stderr.write(r.stderr[-4000:])
    lines = ["# scripts/coo_sym_timing.py: stored entries of a symmetric matrix -> CSR.  Host clock around each call "
             "including its stream synchronise, median of %d after one warm-up, all legs interleaved in one process; "
             "host legs on one thread of the same box." % a.reps]
    for r in results:
        lines += describe(r)
    if trace_ok:
        lines += trace_lines(tdir)
        shutil.rmtree(tdir, ignore_errors=True)   # the stats rows above are the record
    text = "\n".join(lines) + "\n"
    open(os.path.join(a.out, "coo_sym_timing.txt"), "w").write(text)
    sys.stdout.write(text)
    return 0 if len(results) == 2 and trace_ok else 1


if __name__ == "__main__":
    sys.exit(main())
