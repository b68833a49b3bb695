"""What the two device files of the heads of sparse attention share (tests/test_gpu_attention_heads.py,
tests/test_gpu_attention_bwd_heads.py): a case of tests/attention_heads_cases.py as device buffers — every operand of all
heads ONE buffer with a canary before and behind it — the 3-D views that the plans take, and the comparison of a heads
execute with the per-head executes on the same buffers' layout."""
import numpy as np
import torch

import attention_heads_cases as hd

DEV = torch.device("cuda:0")
TORCH = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
BITS = {2: (np.int16, torch.int16), 4: (np.int32, torch.int32), 8: (np.int64, torch.int64)}
GUARD = 8


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


class Buffer:
    """`heads` matrices of rows x width at (ld, stride) as one device buffer of stored bits, every element `fill_bits` first,
    its base `shift` elements past a 16-byte boundary, GUARD canary elements before and behind."""

    def __init__(self, c, heads, rows, width, ld, stride, dtype, fill_bits, shift, values=None):
        self.c, self.rows, self.width, self.ld, self.stride, self.dtype = c, rows, width, ld, stride, dtype
        self.heads = 1 if stride == 0 else heads
        es = torch.empty((), dtype=dtype).element_size()
        np_bits, torch_bits = BITS[es]
        self.elems = (self.heads - 1) * stride + (rows - 1) * ld + width if rows else 0
        fill = np.array(fill_bits).astype(np.int64).astype(np_bits)
        host = np.full(self.elems, fill, dtype=np_bits)
        if values is not None:
            stored = np.ascontiguousarray(values).view(np_bits).reshape(-1, rows, width)
            for h in range(self.heads):
                for r in range(rows):
                    host[h * stride + r * ld:h * stride + r * ld + width] = stored[h, r]
        self.host = host
        raw = torch.full((self.elems + 2 * GUARD + 32 // es + 1,), int(fill), dtype=torch_bits, device=DEV)
        base = ((16 - raw.data_ptr() % 16) % 16) // es + GUARD + 16 // es + shift
        self.guarded = raw[base - GUARD:base + self.elems + GUARD]
        self.flat = raw[base:base + self.elems]
        self.flat.copy_(torch.from_numpy(host))
        self.typed = self.flat.view(dtype)
        self.fill = fill

    def view3(self, H):
        """(rows, H, width): what a plan's execute takes."""
        return torch.as_strided(self.typed, (self.rows, H, self.width), (self.ld, self.stride, 1))

    def vectors(self, H):
        """(H, n) of a per-head vector operand (rows = 1, width = n), or (n,) where all heads share it."""
        return self.typed[:self.width] if self.stride == 0 else torch.as_strided(self.typed, (H, self.width), (self.stride, 1))

    def bits(self):
        return self.guarded.cpu().numpy()

    def lost(self):
        """The elements outside every head's rows x width that no longer hold the fill."""
        got = self.bits()
        inside = np.zeros(got.size, dtype=bool)
        for h in range(self.heads):
            for r in range(self.rows):
                b = GUARD + h * self.stride + r * self.ld
                inside[b:b + self.width] = True
        return int(np.sum(got[~inside] != self.fill))

    def head(self, h):
        """(rows, width) stored bits of head h as they are on the device now."""
        got = self.bits()[GUARD:GUARD + self.elems]
        return np.stack([got[h * self.stride + r * self.ld:h * self.stride + r * self.ld + self.width] for r in range(self.rows)]) if self.rows else got.reshape(0, self.width)


def structure_on_device(c):
    Ap, Aj = hd.csr(c)
    return torch.from_numpy(Ap).to(DEV), torch.from_numpy(Aj).to(DEV)


def inputs(c, names):
    """{name: Buffer} of a case's input matrices (NaN in the padding and between the heads), then bias and, backward, lse."""
    lay, vs, dat = hd.layout(c), hd.vector_strides(c), hd.data(c)
    E, S = TORCH[c.val], TORCH[hd.SIDE[c.val]]
    n_rows, _, nnz = hd.sizes(c)
    out = {}
    for name in names:
        rows, w = hd.matrices(c)[name]
        out[name] = Buffer(c, c.H, rows, w, *lay[name], E, hd.nan_bits(c.val), c.shift, hd.elem_bits(dat[name], c.val))
    side_nan = hd.ac.NAN_BITS[hd.SIDE[c.val]]
    out["bias"] = None if dat["bias"] is None else Buffer(c, c.H, 1, nnz, nnz, vs["bias"], S, side_nan, c.shift, dat["bias"][:, None, :])
    if "lse" in dat:
        out["lse"] = Buffer(c, c.H, 1, n_rows, n_rows, vs["lse"], S, side_nan, c.shift, dat["lse"][:, None, :])
    return out


def output(c, name):
    """A canary-filled output Buffer: a matrix of the case, or lse / dbias."""
    lay, vs = hd.layout(c), hd.vector_strides(c)
    n_rows, _, nnz = hd.sizes(c)
    if name in ("lse", "dbias"):
        n = n_rows if name == "lse" else nnz
        S = hd.SIDE[c.val]
        return Buffer(c, c.H, 1, n, n, vs[name], TORCH[S], hd.word_of(hd.CANARY, hd.NP[S]), c.shift)
    rows, w = hd.matrices(c)[name]
    return Buffer(c, c.H, rows, w, *lay[name], TORCH[c.val], hd.canary_bits(c.val), c.shift)


def assert_equal_heads(c, name, heads, single):
    assert heads.lost() == 0 and single.lost() == 0, "%s: a canary outside the heads of %s was written" % (c.name, name)
    for h in range(c.H):
        assert same_bits(heads.head(h), single.head(h)), "%s: head %d of %s differs from the single-head execute" % (c.name, h, name)
    assert same_bits(heads.bits(), single.bits()), "%s: %s" % (c.name, name)


def small(sp, val=torch.float32, H=3, d=16, dvv=24, seed=3):
    """A problem of H heads on the five-slice structure as contiguous (rows, H, width) device tensors, bias (H, nnz)."""
    c = hd._case("fwd", "five", "i32", "f32", 0)
    Ap, Aj = structure_on_device(c)
    n_rows, n_cols, nnz = hd.sizes(c)
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *shape: (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).to(val).to(DEV)
    P = dict(n_rows=n_rows, n_cols=n_cols, nnz=nnz, Ap=Ap, Aj=Aj, H=H, Q=rnd(n_rows, H, d) * 0.5, K=rnd(n_cols, H, d), V=rnd(n_cols, H, dvv),
             bias=rnd(H, nnz), val=val, d=d, dv=dvv)
    return P
