"""GPU suite: the table of tests/coo_cases.py on the device — COO -> CSR, symmetric COO -> CSR and the CSR transpose
(csrc/coo_csr.hip) at every tile, quarter, step, scan-workgroup, digit and pass edge, the same inputs and the same check as
the host simulation (tests/test_coo_sim_cpu.py), which cannot show what only the lock step of a wave provides.

The families that only sort go through sp.coo_to_csr(..., symmetric=...) and sp.csr_transpose; refusals and the workspace
prefill go through the C entry points, with every output filled with a canary first and a workspace of exactly the
queried size.  The bar is equality with numpy's stable sort (coo_cases.expected): Ap, Aj, the bits of Ax, perm.  One test
per operation and family; nothing is larger than 70 000 entries except the 64 MB offsets of the two domains around 2^24."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__
import coo_cases as cc

pytestmark = pytest.mark.gpu
sp = __graft_entry__.load_package()
DEV = "cuda:0"
OFFS = {"i32": torch.int32, "i64": torch.int64}
VALS = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32}
TABLE = cc.table()
FAMILIES = sorted({(c.op, c.family) for c in TABLE})


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_values(c, n):
    """The case's values on the device in its type, from their bits."""
    bits = cc.values(n, c.val)
    if bits is None:
        return None
    return to_device(bits.view(np.int64 if c.val == "f64" else np.int32)).view(VALS[c.val])


def value_bits(t):
    if t is None:
        return None
    wide = t.element_size() == 8
    return t.view(torch.int64 if wide else torch.int32).cpu().numpy().view(np.uint64 if wide else np.uint32)


def through_the_package(c):
    x = cc.inputs(c)
    if c.op == "transpose":
        Apt, Ajt, perm = sp.csr_transpose(x["n_rows"], x["n_cols"], to_device(x["Ap"].astype(cc.NP[c.off])), to_device(x["Aj"]))
        torch.cuda.synchronize()
        return dict(status=0, message="", Ap=Apt.cpu().numpy(), Aj=Ajt.cpu().numpy(), Ax=None,
                    perm=perm.cpu().numpy().view(np.uint32).astype(np.int64))
    out = sp.coo_to_csr(x["n_rows"], x["n_cols"], to_device(x["rows"]), to_device(x["cols"]), device_values(c, len(x["rows"])), OFFS[c.off],
                        return_perm=c.perm, symmetric=c.op == "sym")
    torch.cuda.synchronize()
    csr, perm = out if c.perm else (out, None)
    assert (csr.n_rows, csr.n_cols, csr.nnz) == (x["n_rows"], x["n_cols"], cc.nnz_out(c)), c.name
    return dict(status=0, message="", Ap=csr.Ap.cpu().numpy(), Aj=csr.Aj.cpu().numpy(), Ax=value_bits(csr.Ax),
                perm=None if perm is None else perm.cpu().numpy())


def through_the_entry_point(c):
    """The C call on canary-filled outputs of exactly their sizes and a workspace of exactly the queried size holding the
    case's prefill."""
    L = sp.capi.lib()
    x = cc.inputs(c)
    n_out = cc.nnz_out(c)
    canary = lambda n, dtype: torch.full((n * torch.empty(0, dtype=dtype).element_size(),), cc.CANARY, dtype=torch.uint8, device=DEV).view(dtype)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Ap = canary(cc.domain(c) + 1, OFFS[c.off])
    Aj = canary(n_out, torch.int32)
    if c.op == "transpose":
        nbytes = sp.capi.csr_transpose_workspace_bytes(x["n_cols"], n_out, OFFS[c.off])
        ws = torch.full((nbytes,), c.prefill, dtype=torch.uint8, device=DEV)
        perm = canary(n_out, torch.int32)
        d_Ap, d_Aj = to_device(x["Ap"].astype(cc.NP[c.off])), to_device(x["Aj"])
        size = C.c_size_t(nbytes)
        st = L.mi355_spmv_csr_transpose(cc.OFF_TYPE[c.off], x["n_rows"], x["n_cols"], C.c_int64(n_out), ptr(d_Ap), ptr(d_Aj), ptr(Ap), ptr(Aj), ptr(perm),
                                        C.c_void_p(ws.data_ptr()), C.byref(size), stream)
        message = L.mi355_spmv_last_error().decode()
        torch.cuda.synchronize()
        p = perm.cpu().numpy().view(np.uint32)
        return dict(status=st, message=message, Ap=Ap.cpu().numpy(), Aj=Aj.cpu().numpy(), Ax=None, perm=p if c.bad else p.astype(np.int64))
    n_in = len(x["rows"])
    vals = device_values(c, n_in)
    Ax = canary(n_out, VALS[c.val]) if vals is not None else None
    perm = canary(n_out, torch.int64) if c.perm else None
    d_rows, d_cols = to_device(x["rows"]), to_device(x["cols"])
    val_dtype = VALS.get(c.val, torch.float32)
    val_type = max(cc.VAL_TYPE[c.val], 0)
    if c.op == "sym":
        nbytes = sp.capi.coo_to_csr_symmetric_workspace_bytes(x["n_rows"], n_in, n_out, OFFS[c.off], val_dtype)
        ws = torch.full((nbytes,), c.prefill, dtype=torch.uint8, device=DEV)
        size = C.c_size_t(nbytes)
        st = L.mi355_spmv_coo_to_csr_symmetric(cc.OFF_TYPE[c.off], val_type, x["n_rows"], x["n_cols"], C.c_int64(n_in), C.c_int64(n_out), ptr(d_rows),
                                               ptr(d_cols), ptr(vals), ptr(Ap), ptr(Aj), ptr(Ax), ptr(perm), C.c_void_p(ws.data_ptr()),
                                               C.byref(size), stream)
    else:
        nbytes = sp.capi.coo_to_csr_workspace_bytes(x["n_rows"], n_in, OFFS[c.off], val_dtype)
        ws = torch.full((nbytes,), c.prefill, dtype=torch.uint8, device=DEV)
        size = C.c_size_t(nbytes)
        st = L.mi355_spmv_coo_to_csr(cc.OFF_TYPE[c.off], val_type, x["n_rows"], x["n_cols"], C.c_int64(n_in), ptr(d_rows), ptr(d_cols), ptr(vals),
                                     ptr(Ap), ptr(Aj), ptr(Ax), ptr(perm), C.c_void_p(ws.data_ptr()), C.byref(size), stream)
    message = L.mi355_spmv_last_error().decode()
    torch.cuda.synchronize()
    return dict(status=st, message=message, Ap=Ap.cpu().numpy(), Aj=Aj.cpu().numpy(), Ax=value_bits(Ax),
                perm=None if perm is None else perm.cpu().numpy())


@pytest.mark.parametrize("op,family", [f for f in FAMILIES if f[1] not in ("bad", "workspace")])
def test_equals_the_stable_sort(op, family):
    cases = [c for c in TABLE if (c.op, c.family) == (op, family)]
    assert cases and all(cc.nnz_out(c) <= 2 * 70000 and len(cc.inputs(c)["Aj" if op == "transpose" else "rows"]) <= 70000 for c in cases)
    for c in cases:
        cc.check(c, through_the_package(c))


@pytest.mark.parametrize("op", cc.OPS)
def test_refusals_name_the_first_offender_and_write_nothing(op):
    cases = [c for c in TABLE if (c.op, c.family) == (op, "bad")]
    assert cases
    for c in cases:
        cc.check(c, through_the_entry_point(c))


@pytest.mark.parametrize("op", cc.OPS)
def test_the_result_does_not_depend_on_what_the_workspace_held(op):
    cases = [c for c in TABLE if (c.op, c.family) == (op, "workspace")]
    groups = {}
    for c in cases:
        groups.setdefault(c.args, []).append(c)
    assert len(groups) == 5
    for g in groups.values():
        assert {c.prefill for c in g} == set(cc.PREFILLS)
        got = [through_the_entry_point(c) for c in g]
        for c, r in zip(g, got):
            cc.check(c, r)
            for k in ("Ap", "Aj", "Ax", "perm"):
                assert (r[k] is None) == (got[0][k] is None) and (r[k] is None or r[k].tobytes() == got[0][k].tobytes()), (c.name, k)
