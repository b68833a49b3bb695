"""The table of cases for the heads of sparse attention in one call (mi355_spmv_attention_execute_heads and
mi355_spmv_attention_bwd_execute_heads), shared by the host simulations (tests/test_attention_heads_sim_cpu.py,
tests/test_attention_bwd_heads_sim_cpu.py) and the device files (tests/test_gpu_attention_heads.py,
tests/test_gpu_attention_bwd_heads.py).

The expected value of a case is never a formula: it is the single-head execute of the SAME object on head h's operands (the
pointers offset by h strides), compared bit for bit for every h.  That transfers every bound the single-head tables hold
(tests/attention_cases.py, tests/attention_bwd_cases.py and their 16-bit tables); no tolerance appears here.

Structures (slices per head = ceil((rows + nonzeros) / SLICE_LEN); a workgroup holds WAVES = 4 slices):
  one      1 slice: no fix-up                                   (slice_edges: items_1023)
  two      2 slices, empty rows at both ends                    (slice_edges: first_and_last_rows_empty)
  five     5 slices: the last workgroup of a head has three inactive waves, which must not run into the next head's
           slices; one row of 4400 entries crosses every slice, among them the workgroup edge between slices 3 and 4,
           and slices 1 .. 3 lie inside that one row                        (hub, its long row cut to 4400)
  eight    8 slices, an exact multiple of a workgroup: a row of 3000 entries over four slices, then runs of empty rows
           that fill whole slices and end them                            (hub's short rows and a long row, then empty_runs)
Every operand of all heads is ONE buffer; layouts name (leading dimension, head stride) per matrix:
  il       interleaved (n, H, w): ld = H w, stride = w          hm     head-major (H, n, w): ld = w, stride = n w
  il_pad   interleaved with a padding column behind every head: stride = w + 1, ld = H (w + 1) + 2
  odd      head-major with one element between the heads: ld = w, stride = n w + 1.  Where w * sizeof is a multiple of 16 the
           single-head execute on head 0 takes the 16-byte path and the heads execute the element path (the head stride in
           bytes is no multiple of 16): equal bits all the same
  k_hm     K head-major, the rest interleaved                   o_il   O (and, backward, dQ) interleaved, the rest head-major
  mqa      K and V shared by all heads (stride 0), the rest interleaved
  q0       Q shared by all heads, the rest head-major
bias: none; per head, with -inf masks that differ between the heads — in head 1 alone one row is masked whole, which must
give O = +0 and lse = -inf there and nowhere else; or one bias shared by all heads (stride 0).  Padding columns of inputs
and the gaps between heads hold NaN; outputs start as a canary that must survive outside every head's rows x width."""
import collections
import struct

import numpy as np

import attention_cases as ac
import attention_half_cases as hc
import row_softmax_cases as rc
from multi_cases import NP, SLICE_LEN, VAL_TYPE, word_of

WAVES = 4               # slices per workgroup (kSliceWaves)
CANARY = -777.25
HEADS = (1, 2, 3, 5)
LAYOUTS = ("il", "hm", "il_pad", "odd", "k_hm", "o_il", "mqa", "q0")
BIASES = ("none", "per_head", "shared")
# (offsets, the type of the matrices): fp32 and fp64 with both offset types, fp16 and bf16 with one each
TYPES = (("i32", "f32"), ("i64", "f32"), ("i32", "f64"), ("i64", "f64"), ("i32", "f16"), ("i64", "bf16"))
SIDE = {"f32": "f32", "f64": "f64", "f16": "f32", "bf16": "f32"}        # the type of bias, lse and dbias
WIDEST = {"f32": 32, "f64": 16, "f16": 64, "bf16": 64}
# (d, dv): one pass with 16-byte rows; dv above the widest tile (two passes) with a remainder of the loop over d; narrow
DIMS = {"f32": ((8, 8), (13, 40), (5, 3)), "f64": ((4, 4), (7, 20), (3, 2)), "f16": ((16, 16), (20, 70), (5, 3)), "bf16": ((16, 16), (20, 70), (5, 3))}
D_MAX, DV_MAX = 24, 72
NEEDS = ((True, True, True), (True, False, False), (False, True, True))

Matrix = ac.Matrix
Case = collections.namedtuple("Case", "name direction matrix off val H H_max d dv layout bias want_lse need want_dbias shift")


def _structures():
    edges = {m.name: m for m in rc.structures("slice_edges")}
    hub, runs = rc.structures("hub")[0], rc.structures("empty_runs")[0]
    long_row = max(hub.lens)
    five = tuple(4400 if n == long_row else n for n in hub.lens)
    short = tuple(3000 if n == long_row else n for n in hub.lens)
    room = 8 * SLICE_LEN - 40 - (len(short) + sum(short))          # items left for the runs of empty rows
    tail, items = [], 0
    for n in runs.lens:
        if items + 1 + n > room:
            break
        tail.append(n)
        items += 1 + n
    out = {"one": edges["items_1023"], "two": edges["first_and_last_rows_empty"],
           "five": Matrix("heads_five", "hub", five, hub.n_cols, hub.seed + 1),
           "eight": Matrix("heads_eight", "empty_runs", short + tuple(tail), hub.n_cols, hub.seed + 2)}
    for name, want in (("one", 1), ("two", 2), ("five", 5), ("eight", 8)):
        assert n_slices(out[name]) == want, (name, n_slices(out[name]))
    return out


def n_slices(m):
    return -(-(len(m.lens) + sum(m.lens)) // SLICE_LEN)


_structs = None


def structures():
    global _structs
    if _structs is None:
        _structs = _structures()
    return _structs


def crossing(m):
    """(rows that cross three or more slices, rows that cross the workgroup edge between slices WAVES - 1 and WAVES, slices
    that lie inside one row, slices that end with an empty row's end)."""
    ends = np.cumsum(np.asarray(m.lens) + 1)            # merge items up to and with each row's end
    begins = ends - np.asarray(m.lens) - 1
    first, last = begins // SLICE_LEN, (ends - 1) // SLICE_LEN
    lens = np.asarray(m.lens)
    inside = sum(1 for s in range(n_slices(m)) if np.any((begins <= s * SLICE_LEN) & (ends - 1 >= (s + 1) * SLICE_LEN)))
    empty_end = sum(1 for s in range(1, n_slices(m) + 1) if np.any((lens == 0) & (ends == s * SLICE_LEN)) or (s == n_slices(m) and lens[-1] == 0))
    return (int(np.sum(last - first >= 2)), int(np.sum((first <= WAVES - 1) & (last >= WAVES) & (lens > 0))), inside, empty_end)


def sizes(c):
    n_rows, n_cols = len(c.matrix.lens), c.matrix.n_cols
    return n_rows, n_cols, sum(c.matrix.lens)


def matrices(c):
    """{operand: (rows, width)} of a case's direction, inputs first."""
    n_rows, n_cols, _ = sizes(c)
    out = collections.OrderedDict(Q=(n_rows, c.d), K=(n_cols, c.d), V=(n_cols, c.dv), O=(n_rows, c.dv))
    if c.direction == "bwd":
        out.update(dO=(n_rows, c.dv), dQ=(n_rows, c.d), dK=(n_cols, c.d), dV=(n_cols, c.dv))
    return out


def layout(c):
    """{operand: (ld, head stride)} in elements."""
    H, out = c.H, {}
    il = lambda rows, w: (H * w, w)
    hm = lambda rows, w: (w, rows * w)
    for name, (rows, w) in matrices(c).items():
        if c.layout == "il":
            out[name] = il(rows, w)
        elif c.layout == "hm":
            out[name] = hm(rows, w)
        elif c.layout == "il_pad":
            out[name] = (H * (w + 1) + 2, w + 1)
        elif c.layout == "odd":
            out[name] = (w, rows * w + 1)
        elif c.layout == "k_hm":
            out[name] = hm(rows, w) if name == "K" else il(rows, w)
        elif c.layout == "o_il":
            out[name] = il(rows, w) if name in ("O", "dQ") else hm(rows, w)
        elif c.layout == "mqa":
            out[name] = (w, 0) if name in ("K", "V") else il(rows, w)
        elif c.layout == "q0":
            out[name] = (w, 0) if name == "Q" else hm(rows, w)
        else:
            raise ValueError(c.layout)
    return out


def vector_strides(c):
    """{bias, lse, dbias: head stride}: head-major vectors, one element between the heads under the odd layout."""
    n_rows, _, nnz = sizes(c)
    gap = 1 if c.layout == "odd" else 0
    return dict(bias=0 if c.bias == "shared" else nnz + gap, lse=n_rows + gap, dbias=nnz + gap)


def stored(c, stride):
    return 1 if stride == 0 else c.H


# ---- operands ---------------------------------------------------------------------------------------------------------
_data = {}


def whole_masked_row(c):
    """The row that head 1's bias masks whole: the longest row."""
    return int(np.argmax(c.matrix.lens))


def data(c):
    """{operand: array of (H, rows, width) in float32 / float64 (the 16-bit types: float32 values that the type holds
    exactly); bias (H, nnz) or None; backward: lse (H, n_rows)}.  Head h of a shared operand is head 0.  Made once per case
    and left unchanged."""
    if c.name in _data:
        return _data[c.name]
    n_rows, n_cols, nnz = sizes(c)
    T = NP[SIDE[c.val]] if c.val in ("f16", "bf16") else NP[c.val]
    rng = np.random.RandomState(c.matrix.seed * 17 + c.H * 5 + c.d * 3 + c.dv + len(c.name))
    exact = (lambda a: hc.from_bits(hc.to_bits(a.astype(np.float32), c.val), c.val)) if c.val in ("f16", "bf16") else (lambda a: a.astype(T))
    out = {}
    for name, (rows, w) in matrices(c).items():
        if name in ("dQ", "dK", "dV") or (name == "O" and c.direction == "fwd"):
            continue
        out[name] = exact((rng.rand(c.H, rows, w) * 2 - 1) * (0.5 if name == "Q" else 1.0))
    S = NP[SIDE[c.val]]
    if c.bias == "none":
        out["bias"] = None
    else:
        bias = (rng.rand(c.H, nnz) * 4 - 2).astype(S)
        bias[rng.rand(c.H, nnz) < 0.15] = -np.inf              # masks that differ between the heads
        if c.H > 1 and c.bias == "per_head":
            Ap = np.concatenate(([0], np.cumsum(c.matrix.lens)))
            r = whole_masked_row(c)
            keep = bias[:, Ap[r]:Ap[r + 1]]
            keep[np.isneginf(keep)] = 0.0                       # the other heads keep the row alive ...
            bias[1, Ap[r]:Ap[r + 1]] = -np.inf                  # ... head 1 masks it whole
        out["bias"] = bias
    if c.direction == "bwd":
        out["lse"] = (rng.rand(c.H, n_rows) * 3).astype(S)
    _data[c.name] = out
    return out


def csr(c):
    return ac.csr(c.matrix, c.off)


def elem_bits(a, val):
    """The stored bits of an array of a case's matrix type."""
    return hc.to_bits(a.astype(np.float32), val) if val in ("f16", "bf16") else np.ascontiguousarray(a.astype(NP[val]))


def nan_bits(val):
    return hc.NAN_BITS[val] if val in ("f16", "bf16") else ac.NAN_BITS[val]


def canary_bits(val):
    return int(hc.to_bits(np.float32(CANARY), val).reshape(-1)[0]) if val in ("f16", "bf16") else word_of(CANARY, NP[val])


def elem_dtype(val):
    return np.uint16 if val in ("f16", "bf16") else NP[val]


# ---- the table --------------------------------------------------------------------------------------------------------
def _case(direction, sname, off, val, n, dims=None, need=(True, True, True), want_dbias=False, H=None, lay=None, bias=None):
    """Case n of a direction: what the arguments leave open is drawn from a generator seeded with n (the coverage that the
    draws must reach is asserted by tests/test_attention_heads_cpu.py)."""
    rng = np.random.RandomState(7000 + n)
    pick = lambda seq: seq[rng.randint(len(seq))]
    m = structures()[sname]
    H = pick(HEADS) if H is None else H
    H_max = H + pick((0, 0, 2))
    d, dv = DIMS[val][n % len(DIMS[val])] if dims is None else dims
    lay = pick(LAYOUTS) if lay is None else lay
    bias = pick(BIASES) if bias is None else bias
    want_lse = pick((True, True, False))
    shift = 0 if lay == "odd" else pick((0, 1))     # (the odd layout: an aligned base under an unaligned head stride)
    name = "%s%d-%s-%s-%s-H%dof%d-d%d-dv%d-%s-%s-lse%d-need%s-db%d-sh%d" % (direction, n, sname, off, val, H, H_max, d, dv, lay, bias, int(want_lse),
                                                                         "".join(str(int(x)) for x in need), int(want_dbias), shift)
    return Case(name, direction, m, off, val, H, H_max, d, dv, lay, bias, want_lse, tuple(need), bool(want_dbias), shift)


STRUCTURES = ("one", "two", "five", "eight")


def forward_cases():
    """Every (type, widths) on every structure, the rest drawn; then, per type, the unaligned head stride under aligned rows
    and the masks that differ between heads, on the structure whose last workgroup has inactive waves."""
    out, n = [], 0
    for off, val in TYPES:
        for dims in DIMS[val]:
            for sname in STRUCTURES:
                out.append(_case("fwd", sname, off, val, n, dims))
                n += 1
    for off, val in TYPES:
        out.append(_case("fwd", "five", off, val, n, DIMS[val][0], H=3, lay="odd", bias="per_head"))
        out.append(_case("fwd", "eight", off, val, n + 1, DIMS[val][1], H=2, lay="mqa", bias="shared"))
        out.append(_case("fwd", "five", off, val, n + 2, DIMS[val][1], H=5, lay="q0", bias="per_head"))
        n += 3
    return out


def backward_cases():
    """Every (type, need) on two structures each, dbias on and off under dQ; then the forward's special cases."""
    out, n = [], 0
    for off, val in TYPES:
        for i, need in enumerate(NEEDS):
            for j in range(2):
                sname = STRUCTURES[(n // 2) % 4] if j == 0 else ("five", "eight")[(n + i) % 2]
                out.append(_case("bwd", sname, off, val, n, DIMS[val][(i + j) % 3], need, need[0] and j == 0))
                n += 1
    for off, val in TYPES:
        out.append(_case("bwd", "five", off, val, n, DIMS[val][0], NEEDS[0], True, H=3, lay="odd", bias="per_head"))
        out.append(_case("bwd", "eight", off, val, n + 1, DIMS[val][1], NEEDS[0], False, H=2, lay="o_il", bias="shared"))
        n += 2
    return out


def plan_key(c):
    return (c.direction, c.matrix.name, c.off, c.val)


def weight(g):
    return sum((len(c.matrix.lens) + sum(c.matrix.lens)) * c.H * (1 if c.direction == "fwd" else 3) * (2 + (c.d + c.dv) // 16) + 3000 for c in g)


# ---- the host programs' batch files (tests/cpp/attention_heads_sim.cpp, attention_bwd_heads_sim.cpp) ----------------------
def _words(*v):
    return struct.pack("<%dq" % len(v), *[int(x) for x in v])


def write_batch(path, cases, grid_probe=None):
    """Cases in plan order; returns them in the order their results come back."""
    last = None
    with open(path, "wb") as f:
        for c in cases:
            Ap, Aj = csr(c)
            n_rows, n_cols, nnz = sizes(c)
            if plan_key(c) != last:
                last = plan_key(c)
                f.write(_words(1, ("i32", "i64").index(c.off), VAL_TYPE[c.val], n_rows, n_cols, nnz, D_MAX, DV_MAX))
                f.write(Ap.tobytes())
                f.write(Aj.tobytes())
            lay, vs, dat = layout(c), vector_strides(c), data(c)
            bias_heads = 0 if dat["bias"] is None else stored(c, vs["bias"])
            side_canary = word_of(CANARY, NP[SIDE[c.val]])
            if c.direction == "fwd":
                f.write(_words(4, c.H, c.H_max, c.d, c.dv, int(c.want_lse), bias_heads, c.shift))
                for name in ("Q", "K", "V", "O"):
                    f.write(_words(*lay[name]))
                f.write(_words(vs["bias"], vs["lse"], nan_bits(c.val), canary_bits(c.val), side_canary))
                inputs, sides = ("Q", "K", "V"), ()
            else:
                f.write(_words(4, c.H, c.H_max, c.d, c.dv, bias_heads, *[int(x) for x in c.need], int(c.want_dbias), c.shift))
                for name in ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"):
                    f.write(_words(*lay[name]))
                f.write(_words(vs["bias"], vs["lse"], vs["dbias"], nan_bits(c.val), canary_bits(c.val), side_canary))
                inputs, sides = ("Q", "K", "V", "O", "dO"), ("lse",)
            f.write(struct.pack("<d", 0.25))
            for name in inputs:
                f.write(elem_bits(dat[name][:stored(c, lay[name][1])], c.val).tobytes())
            for name in sides:
                f.write(np.ascontiguousarray(dat[name]).tobytes())
            if bias_heads:
                f.write(np.ascontiguousarray(dat["bias"][:bias_heads]).tobytes())
        for probe in grid_probe or ():
            f.write(_words(9, *probe))
        f.write(_words(0))
    return list(cases)


Result = collections.namedtuple("Result", "statuses n_heads_max bad touched scratch_bytes held_bytes heads single")


def read_results(path, cases, n_probes=0):
    """[Result] per case — heads / single: {output: (H, rows, width) array of stored bits} of the heads execute and of the
    per-head executes — then the statuses of the grid probes.  Raises if the file is not complete."""
    out = []
    with open(path, "rb") as f:
        for c in cases:
            n_rows, n_cols, nnz = sizes(c)
            fwd = c.direction == "fwd"
            head = struct.unpack("<%dq" % (7 if fwd else 8), f.read(56 if fwd else 64))
            E, S = elem_dtype(c.val), NP[SIDE[c.val]]
            take = lambda dtype, rows, w: np.frombuffer(f.read(c.H * rows * w * np.dtype(dtype).itemsize), dtype=dtype).reshape(c.H, rows, w)
            heads, single = {}, {}
            if fwd:
                heads["O"], single["O"] = take(E, n_rows, c.dv), take(E, n_rows, c.dv)
                if c.want_lse:
                    heads["lse"], single["lse"] = take(S, 1, n_rows), take(S, 1, n_rows)
            else:
                for name, asked, rows, w, dtype in (("dQ", c.need[0], n_rows, c.d, E), ("dK", c.need[1], n_cols, c.d, E), ("dV", c.need[2], n_cols, c.dv, E),
                                                    ("dbias", c.want_dbias, 1, nnz, S)):
                    if asked:
                        heads[name], single[name] = take(dtype, rows, w), take(dtype, rows, w)
            out.append(Result(head[:3], head[3], head[4], head[5], head[6], head[7] if not fwd else 0, heads, single))
        probes = list(struct.unpack("<%dq" % n_probes, f.read(8 * n_probes))) if n_probes else []
        assert struct.unpack("<q", f.read(8))[0] == -1 and f.read() == b""
    return out, probes


# ---- refusals on a real object (record 8 of both programs): (what the text must name, the words of the record) ------------
def forward_refusals(c):
    """Bad execute_heads calls on the object of forward case c (which has reserved c.H_max >= 3 heads), three heads each."""
    n_rows, n_cols, nnz = sizes(c)
    d, dv, H = 8, 8, 3
    il = dict(q=d, k=d, v=dv, bias=nnz, o=dv, lse=n_rows)
    call = lambda lds=(H * d, H * d, H * dv, H * dv), want_lse=1, **hs: (H, *[dict(il, **hs)[k] for k in ("q", "k", "v", "bias", "o", "lse")], d, dv, *lds,
                                                                         want_lse)
    return [("stride o", call(o=dv - 1)),                                       # below the width
            ("stride o", call(o=0)),                                            # an output shared by all heads
            ("stride o", call(o=dv + 1)),                                       # interleaved, but ld holds only H * dv
            ("stride o", call(lds=(H * d, H * d, H * dv, dv), o=(n_rows - 1) * dv + dv - 1)),   # head-major, one element short
            ("stride lse", call(lse=n_rows - 1)),
            ("stride o", call(lds=(H * d, H * d, H * dv, 2 ** 62), o=2 ** 62)),     # (rows - 1) * ld would wrap: compared by division
            ("negative head stride k", call(k=-d)),
            ("n_heads = 3 above", None)]                                        # (asked of an object that reserves fewer: the test file)


def backward_refusals(c):
    n_rows, n_cols, nnz = sizes(c)
    d, dv, H = 8, 8, 3
    names = ("q", "k", "v", "bias", "o", "d_o", "lse", "dq", "dk", "dv", "dbias")
    il = dict(q=d, k=d, v=dv, bias=nnz, o=dv, d_o=dv, lse=n_rows, dq=d, dk=d, dv=dv, dbias=nnz)
    lds = [H * d, H * d, H * dv, H * dv, H * dv, H * d, H * d, H * dv]
    call = lambda need=(1, 1, 1), want_dbias=1, ld=None, **hs: (H, *[dict(il, **hs)[k] for k in names], d, dv, *(ld or lds), *need, want_dbias)
    short = list(lds)
    short[6] = d                                                                # dK head-major ...
    return [("stride dq", call(dq=d - 1)), ("stride dk", call(dk=d + 1)), ("stride dv", call(dv=0)),
            ("stride dk", call(ld=short, dk=(n_cols - 1) * d + d - 1)),         # ... one element short
            ("stride dbias", call(dbias=nnz - 1)), ("negative head stride d_o", call(d_o=-1)),
            ("dbias without dQ", call(need=(0, 1, 1)))]


def write_refusals(path, c, refusals):
    """The matrix record of c, a reserve through one run of c, then the refusal records."""
    cases = write_batch(path + ".run", [c])
    with open(path + ".run", "rb") as f:
        body = f.read()[:-8]
    with open(path, "wb") as f:
        f.write(body)
        for _, words in refusals:
            if words is not None:
                f.write(_words(8, *words))
        f.write(_words(0))
    return cases


def read_refusals(path, c, n):
    """[(status, text)] of the n refusal records behind the run of c."""
    with open(path, "rb") as f:
        blob = f.read()
    tail = blob[len(blob) - 8 - n * 264:]
    assert struct.unpack("<q", tail[-8:])[0] == -1
    return [(struct.unpack("<q", tail[i * 264:i * 264 + 8])[0], tail[i * 264 + 8:(i + 1) * 264].split(b"\0")[0].decode()) for i in range(n)]


def head_scratch_bytes(c):
    """The scratch of ONE head of a case's object, as csrc/attention.hip (attn_scratch_bytes) and csrc/attention_bwd.hip
    (attn_bwd_scratch_bytes) lay it out for D_MAX and DV_MAX: what get_info reports after create."""
    n_rows, n_cols, nnz = sizes(c)
    vb = 8 if c.val == "f64" else 4
    tiles = lambda w: -(-w // WIDEST[c.val]) * WIDEST[c.val]
    slices = lambda n: -(-(n + nnz) // SLICE_LEN)
    if c.direction == "fwd":
        return slices(n_rows) * 2 * (tiles(DV_MAX) * vb + 2 * vb + 4)
    return (n_rows * vb + 15) // 16 * 16 + max(slices(n_rows), slices(n_cols)) * 2 * (tiles(max(D_MAX, DV_MAX)) * vb + 4) + 16


def reserved_scratch_bytes(c):
    """scratch_bytes after reserve_heads(c.H_max): head h at h x (one head's bytes rounded up to whole 16), the last as it is."""
    one = head_scratch_bytes(c)
    return (c.H_max - 1) * ((one + 15) // 16 * 16) + one


def check_result(c, res, same_bits):
    """What both simulation files assert of a case's result."""
    assert res.scratch_bytes == reserved_scratch_bytes(c), "%s: scratch_bytes %d, not %d" % (c.name, res.scratch_bytes, reserved_scratch_bytes(c))
    assert res.statuses == (0, 0, 0), "%s: statuses of reserve_heads, execute_heads, execute: %s" % (c.name, res.statuses)
    assert res.n_heads_max == c.H_max, c.name
    assert res.bad == 0, "%s: %d elements outside the heads' rows x width lost their canary" % (c.name, res.bad)
    assert res.touched == 0, "%s: %d bytes of the scratch of heads that were not executed were written" % (c.name, res.touched)
    assert set(res.heads) == set(res.single) and res.heads, c.name
    for name in res.heads:
        for h in range(c.H):
            assert same_bits(res.heads[name][h], res.single[name][h]), "%s: head %d of %s differs from the single-head execute" % (c.name, h, name)
    if c.direction == "fwd" and c.H > 1 and c.bias == "per_head":
        r = whole_masked_row(c)
        O = res.heads["O"]
        assert not np.any(O[1, r].view(np.uint8)), "%s: the row masked whole in head 1 is not +0 there" % c.name
        if c.want_lse:
            lse = res.heads["lse"][:, 0, r]
            assert np.isneginf(lse[1]) and np.all(np.isfinite(np.delete(lse, 1))), "%s: lse of the row masked whole in head 1 alone: %s" % (c.name, lse)
