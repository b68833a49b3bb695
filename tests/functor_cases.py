"""The table of cases for the run-time functor kernels (csrc/functor_kernel.inc, launched in the shape of
csrc/functor_shape.hpp: DESIGN 3.6) that tests/test_gpu_functor_edges.py executes on the device, that
tests/test_functor_sim_cpu.py executes lane by lane on the host (tests/cpp/functor_sim.cpp) and whose reach
tests/test_functor_cases_cpu.py proves.

Geometry.  mean = nnz // n_rows picks T = 2 .. 64 lanes per row (T = 2 up to a mean of 8, doubling at 16, 32, 64, 128).
mi355_functor_rows_<T>: a workgroup of 256 threads takes 256 / T rows per ROUND of its grid loop (the grid is capped at
kCus * 32 workgroups); a lane takes the four nonzeros from k0 + 4 lane on, then 4 T further on (a STEP), into four
running values s[0..3]; the last, partial group of a row goes element by element into s[0] (the TAIL, on one lane); a
shuffle tree over the T lanes.  A row LONGER than long_len = max(2 048, 128 T) is left to mi355_functor_long_rows, which
launches only when nnz > long_len: every wave looks at 64 row lengths at a time (a GROUP; the grid is capped at kCus * 8
workgroups of 4 waves, so 256 rows per workgroup and round), ballots the long ones and takes them one after another
with all 64 lanes: element k0 + lane, four of them 64 apart per MAIN iteration while k + 192 < k1, the rest in steps of 64
into s[0].

census() restates that DECOMPOSITION only - T, the kernel that takes each row, the rounds, the groups and lanes of the
ballot, the walks' iterations, where a planted element lands - and never computes a y.  Its launch shape is compared
with the product's functor_shape by the tests.  Expected values come from expected(): a fold per row in float64 / int64.

Data.  Integer values without zeros ({+-1, +-2, +-3} x {+-1, +-2}): (+, x) is exact in any order and ONE missing or
doubled element changes its row.  For the min / max functors every row of two and more elements carries a unique
maximum and a unique minimum (PLANTS: columns C_BIG and C_SMALL of x), at a position that goes through the row's position
classes from row to row, so a skipped element is seen as well.  The columns of x that no row references hold NaN (the
16-bit and 32-bit integer x: 0x5A5A..), y is prefilled with bytes 0x5A, guard elements on both sides included."""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-samples_amd", "csrc")
TEXT_FILE = os.path.join(ROOT, "tests", "cpp", "functor_texts.inc")

# the literals the table was written with; source_constants() reads the same from the product's text
BLOCK = 256                              # kBlock
WAVE = 64                                # kWave
STEP = 4                                 # nonzeros (and running values) per lane and step
LANES = (2, 4, 8, 16, 32, 64)
T_MEANS = (8, 16, 32, 64, 128)           # T = LANES[i] up to a mean of T_MEANS[i]; beyond the last: 64
LONG_PER_LANE = 128                      # long_len = 128 T ...
LONG_MIN = 2048                          # ... at least this
CUS = 256
ROWS_CAP = CUS * 32                      # workgroups of the rows kernel
LONG_CAP = CUS * 8                       # workgroups of the long-row kernel
GUARD = 16                               # elements of y on either side of the rows
N_COLS = 2048
FILL = 0x5A


def text():
    """The functors' source: one text for hiprtc and for the host simulation."""
    with open(TEXT_FILE) as f:
        return f.read()


def source_constants():
    """The same constants from csrc/functor_kernel.inc and csrc/functor_shape.hpp, as text: a changed constant fails
    test_functor_cases_cpu instead of moving an edge."""
    read = lambda f: open(os.path.join(CSRC, f)).read()
    kern, shape = read("functor_kernel.inc"), read("functor_shape.hpp")
    const = lambda t, name: int(re.search(r"constexpr int %s = (\d+);" % name, t).group(1))
    first = int(re.search(r"while \(s\.choice < kFunctorLaneChoices - 1 && \(int64_t\((\d+)\) << s\.choice\) < mean\) \+\+s\.choice;", shape).group(1))
    choices = const(shape, "kFunctorLaneChoices")
    lane0 = int(re.search(r"s\.T = (\d+) << s\.choice;", shape).group(1))
    step = re.search(r"for \(long long k = k0 \+ (\d+) \* lane; k < k1; k \+= (\d+) \* T\) \{\s+if \(k \+ (\d+) < k1\) \{", kern)
    walk = re.search(r"for \(; k \+ (\d+) \* kWave < k1; k \+= (\d+) \* kWave\)", kern)
    return {
        "kBlock": const(kern, "kBlock"), "kWave": const(kern, "kWave"),
        "shape_block": const(shape, "kFunctorBlock"), "shape_wave": const(shape, "kFunctorWave"), "kCus": const(shape, "kFunctorCus"),
        "step": tuple(int(v) for v in step.groups()), "running_values": [int(v) for v in re.findall(r"mi355_y_t s\[(\d+)\];", kern)],
        "walk": tuple(int(v) for v in walk.groups()), "walk_tail_step_is_a_wave": "for (; k < k1; k += kWave) s[0] =" in kern,
        "rows_kernels": tuple(int(v) for v in re.findall(r"^MI355_FUNCTOR_ROWS\((\d+)\)$", kern, re.M)),
        "lanes": tuple(lane0 << i for i in range(choices)), "t_means": tuple(first << i for i in range(choices - 1)),
        "long_per_lane": int(re.search(r"s\.long_len = (\d+)ll \* s\.T;", shape).group(1)),
        "long_min": tuple(int(v) for v in re.search(r"if \(s\.long_len < (\d+)\) s\.long_len = (\d+);", shape).groups()),
        "rows_cap": tuple(int(v) for v in re.search(r"s\.rows_grid = unsigned\(want < int64_t\(kFunctorCus\) \* (\d+) \? want : int64_t\(kFunctorCus\) \* (\d+)\);", shape).groups()),
        "long_cap": tuple(int(v) for v in re.search(r"s\.long_grid = unsigned\(wgs < int64_t\(kFunctorCus\) \* (\d+) \? wgs : int64_t\(kFunctorCus\) \* (\d+)\);", shape).groups()),
        "mean_is_floor": "const int64_t mean = nnz / n_rows;" in shape,
        "long_launch_rule": "s.long_launch = nnz > s.long_len;" in shape,
        "long_row_rule": kern.count("if (k1 - k0 > long_len) continue;") == 1 and kern.count("__ballot(len > long_len)") == 1,
    }


# ---- the type sets -------------------------------------------------------------------------------------------------
TRI = np.dtype([("sum", np.int16), ("lo", np.int16), ("hi", np.int16)])
STAT12 = np.dtype([("hi", np.float32), ("lo", np.float32), ("count", np.int32)])
STAT16 = np.dtype([("sum", np.float64), ("hi", np.float32), ("count", np.int32)])
# functor: the C++ type; off / mat / x / y: C++ type names; np_*: the same in numpy; op: what expected() folds;
# plant: "times" | "plus" | "or" (how a planted element is made extreme); semiring: the oracle's number, where it has one
TypeSet = collections.namedtuple("TypeSet", "name functor off mat x y np_off np_mat np_x np_y op plant semiring")
TYPE_SETS = collections.OrderedDict((t.name, t) for t in (
    TypeSet("pt_f32", "PlusTimesFn<float, float, float>", "int", "float", "float", "float", np.int32, np.float32, np.float32, np.dtype(np.float32), "plus_times", "times", 0),
    TypeSet("pt_f64_i64", "PlusTimesFn<double, double, double>", "long long", "double", "double", "double", np.int64, np.float64, np.float64, np.dtype(np.float64), "plus_times", "times", 0),
    TypeSet("minplus_f32", "MinPlusFn<float, float, float>", "int", "float", "float", "float", np.int32, np.float32, np.float32, np.dtype(np.float32), "min_plus", "plus", 1),
    TypeSet("maxtimes_f32_i64", "MaxTimesFn<float, float, float>", "long long", "float", "float", "float", np.int64, np.float32, np.float32, np.dtype(np.float32), "max_times", "times", 2),
    TypeSet("maxplus_f64", "MaxPlusFn<double, double, double>", "int", "double", "double", "double", np.int32, np.float64, np.float64, np.dtype(np.float64), "max_plus", "plus", 3),
    TypeSet("or_u8", "OrAndFn<float, float, unsigned char>", "int", "float", "float", "unsigned char", np.int32, np.float32, np.float32, np.dtype(np.uint8), "or_and", "or", 4),
    TypeSet("min_i16", "MinI16Fn", "int", "short", "short", "short", np.int32, np.int16, np.int16, np.dtype(np.int16), "min_plus_i16", "plus", None),
    TypeSet("tri_i16_i64", "TriFn", "long long", "short", "short", "Tri", np.int64, np.int16, np.int16, TRI, "tri", "times", None),
    TypeSet("stat12", "Stat12Fn", "int", "float", "float", "Stat12", np.int32, np.float32, np.float32, STAT12, "stat12", "times", None),
    TypeSet("stat16_i64", "Stat16Fn", "long long", "float", "double", "Stat16", np.int64, np.float32, np.float64, STAT16, "stat16", "times", None),
    TypeSet("count_mix", "CountAbove", "long long", "double", "int", "long long", np.int64, np.float64, np.int32, np.dtype(np.int64), "count", "times", None),
))
Y_BYTES = (1, 2, 4, 6, 8, 12, 16)

# plant: whether rows carry planted extrema (not the two big stride matrices)
Matrix = collections.namedtuple("Matrix", "name lens seed plant")
# shift: elements that Aj, Ax and x lie behind a 64-byte boundary (0: aligned); grids: (rows grid, long grid) that the
# simulation runs instead of the shape's own (0: the shape's); sim: whether the host simulation runs the case
Case = collections.namedtuple("Case", "name family matrix typeset edge shift grids sim")
Shape = collections.namedtuple("Shape", "T long_len rows_grid long_launch long_grid")


def lanes_of(mean):
    for m, t in zip(T_MEANS, LANES):
        if mean <= m:
            return t
    return LANES[-1]


def band_of(T):
    """The means [lo, hi] that pick T."""
    i = LANES.index(T)
    return (T_MEANS[i - 1] + 1 if i else 0), (T_MEANS[i] if i < len(T_MEANS) else 1 << 40)


def long_len_of(T):
    return max(LONG_MIN, LONG_PER_LANE * T)


def shape_of(n_rows, nnz, grids=(0, 0)):
    """The launch shape, restated: the tests hold it against the product's functor_shape."""
    T = lanes_of(nnz // n_rows)
    long_len = long_len_of(T)
    rows_grid = min(-(-n_rows // (BLOCK // T)), ROWS_CAP)
    launch = nnz > long_len
    long_grid = min(-(-(-(-n_rows // WAVE)) // (BLOCK // WAVE)), LONG_CAP) if launch else 0
    return Shape(T, long_len, grids[0] or rows_grid, launch, (grids[1] or long_grid) if launch else 0)


# ---- planted extrema ---------------------------------------------------------------------------------------------------
def plant_positions(lens, T):
    """Per row of two and more nonzeros the positions (hi, lo) of its planted maximum and minimum (-1: none): from row to
    row through the row's first and last element, the elements of its first group of four, the group and the elements
    around the end of the first step, and the elements of the tail."""
    hi = np.full(len(lens), -1, dtype=np.int64)
    lo = np.full(len(lens), -1, dtype=np.int64)
    for r, L in enumerate(lens):
        if L < 2:
            continue
        t = L & ~3
        cand = [0, L - 1, 1, 2, 3, 4, 7, t, t + 1, t + 2, t - 1, t - 4, 4 * T - 1, 4 * T, 4 * T + 1, 4 * T + 2, 4 * T + 3, 8 * T - 1,
                WAVE, 3 * WAVE + 63, 4 * WAVE, 4 * WAVE + 1, L - 64, L - 65, L - 2]
        if L > LONG_MIN:                         # (a row of the long kernel: the four slots of a main iteration, the tail)
            cand = [0, L - 1, WAVE, 2 * WAVE + 5, 3 * WAVE + 63, 4 * WAVE, WAVE - 1, L - 64, L - 65, L - 2, 4 * WAVE + 1]
        cand = list(dict.fromkeys(c for c in cand if 0 <= c < L))
        i = r % len(cand)
        hi[r], lo[r] = cand[i], cand[(i + 1 + r // len(cand)) % len(cand)]
        if lo[r] == hi[r]:
            lo[r] = cand[(i + 1) % len(cand)]
    return hi, lo


# ---- the decomposition -------------------------------------------------------------------------------------------------
Census = collections.namedtuple("Census", "shape states long_rows")


def census(lens, grids=(0, 0), plant=False):
    """The launch shape, the rows of the long kernel and the states that the decomposition of these row lengths reaches,
    as a set of names."""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    nnz = int(lens.sum())
    Ap = np.concatenate(([0], np.cumsum(lens)))
    sh = shape_of(n, nnz, grids)
    T, LL = sh.T, sh.long_len
    s = set()
    mean = nnz // n
    # ---- lanes
    s.add("T=%d" % T)
    if mean in T_MEANS or mean - 1 in T_MEANS:
        s.add("mean=%d" % mean)
    if mean in T_MEANS and (nnz + 1) // n == mean + 1:
        s.add("floor_decides")
    # ---- the rows kernel
    is_long = lens > LL
    long_rows = np.nonzero(is_long)[0]
    short = lens[~is_long]
    present = set(np.unique(short).tolist())
    if present >= set(range(8 * T + 5)):
        s.add("T%d:lengths_0..8T+4" % T)
    for name, v in (("4T-1", 4 * T - 1), ("4T", 4 * T), ("4T+1", 4 * T + 1), ("8T-1", 8 * T - 1), ("8T", 8 * T), ("8T+1", 8 * T + 1)):
        if v in present:
            s.add("T%d:len=%s" % (T, name))
    for L in present:
        strides = -(-L // (4 * T))
        if L % 4 and strides in (2, 3):
            s.add("T%d:tail%d@strides%d" % (T, L % 4, strides))
        if L % 4:
            g = L // 4
            if g % T == T - 1:
                s.add("T%d:tail_on_last_lane" % T)
            if g % T == 0 and g >= T:
                s.add("T%d:tail_on_lane0_in_a_later_step" % T)
    k_rows = BLOCK // T
    empty = np.nonzero(lens == 0)[0]
    if len(empty):
        if (empty % k_rows == 0).any():
            s.add("empty_first_of_wg")
        if (empty % k_rows == k_rows - 1).any():
            s.add("empty_last_of_wg")
        if empty[0] == 0:
            s.add("empty_first_row")
        if empty[-1] == n - 1:
            s.add("empty_last_row")
    starts = Ap[:-1][lens >= 4]
    for ph in set((starts % 4).tolist()):
        s.add("phase%d" % ph)
    # the grid loop
    per_round = k_rows * sh.rows_grid
    rounds = -(-n // per_round)
    if rounds >= 2:
        s.add("rows_round2")
        if n % per_round:
            s.add("rows_last_round_partial")
        if (long_rows >= per_round).any():
            s.add("rows_kernel_skips_a_long_row_in_round2")
        if len(short) and (np.nonzero(~is_long & (lens > 0))[0] >= per_round).any():
            s.add("rows_kernel_takes_a_row_in_round2")
    # ---- the long edge
    for name, v in (("LL-1", LL - 1), ("LL", LL), ("LL+1", LL + 1)):
        if (lens == v).any():
            s.add("LL%d:len=%s" % (LL, name))
    if nnz == LL:
        s.add("LL%d:nnz=LL" % LL)
    if nnz == LL + 1:
        s.add("LL%d:nnz=LL+1" % LL)
    if n == 1:
        s.add("one_row")
    s.add("long_launch" if sh.long_launch else "no_long_launch")
    assert sh.long_launch or not len(long_rows)                  # a long row only exists when nnz allows it
    if sh.long_launch and not len(long_rows):
        s.add("long_launch_without_a_long_row")
    # ---- the long kernel
    if len(long_rows):
        for L in set(lens[long_rows].tolist()):
            s.add("walk_mod=%d" % (L % (4 * WAVE)))
            if (L - 1 - 3 * WAVE) // (4 * WAVE) + 1 >= 2:        # lane 0: k = 0, 256, ... while k + 192 < L
                s.add("walk_main_2plus")
        groups = {}
        for r in long_rows.tolist():
            groups.setdefault(r // WAVE, set()).add(r % WAVE)
        for g, lanes in groups.items():
            if len(lanes) == WAVE:
                s.add("ballot=all64")
            elif len(lanes) <= 2:
                s.add("ballot={%s}" % ",".join(str(v) for v in sorted(lanes)))
        if n % WAVE and is_long[n - 1]:
            s.add("last_group_rows=%d_last_row_long" % (n % WAVE))
        if is_long[n - 1]:
            s.add("long_row_is_last_row")
        n_waves = sh.long_grid * (BLOCK // WAVE)
        where = collections.defaultdict(set)                     # (round, workgroup) -> its waves that find a long row
        for g in groups:
            where[(g // n_waves, (g % n_waves) // (BLOCK // WAVE))].add(g % (BLOCK // WAVE))
        if any(len(w) >= 2 for w in where.values()):
            s.add("long_rows_in_two_waves_of_a_wg")
        per_round = n_waves * WAVE
        if (long_rows >= per_round).any():
            s.add("long_round2")
        for name, v in (("last_of_round1", per_round - 1), ("first_of_round2", per_round), ("lane63_of_round2", per_round + 63)):
            if v < n and is_long[v]:
                s.add("long_row_" + name)
    # ---- where the planted maxima land
    if plant:
        hi = plant_positions(lens, T)[0]
        for r in np.nonzero(hi >= 0)[0].tolist():
            L, p = int(lens[r]), int(hi[r])
            if L > LL:
                lane, q = p % WAVE, p // WAVE
                n_main = max(0, (L - 1 - 3 * WAVE - lane) // (4 * WAVE) + 1) if L - lane > 3 * WAVE else 0
                s.add("plant_long_main_slot%d" % (q % 4) if q < 4 * n_main else "plant_long_tail")
                if lane in (0, WAVE - 1):
                    s.add("plant_long_lane%d" % lane)
                continue
            g = p // 4
            if p == 0:
                s.add("plant_first")
            if p == L - 1:
                s.add("plant_last")
            if 4 * g + 3 < L:
                s.add("plant_slot%d" % (p % 4))
            else:
                s.add("plant_tail%d" % (p - 4 * g))
            if g % T == T - 1:
                s.add("plant_on_last_lane")
            if g >= T:
                s.add("plant_in_a_later_step")
    return Census(sh, s, long_rows)


_census = {}


def census_of(c):
    key = (c.matrix.name, c.grids)
    if key not in _census:
        _census[key] = census(c.matrix.lens, c.grids, c.matrix.plant)
    return _census[key]


def states_of(c):
    """The census states of the case's matrix and grids, and those of its type set and operand placement."""
    ts = TYPE_SETS[c.typeset]
    s = set(census_of(c).states)
    s |= {"y_bytes=%d" % ts.np_y.itemsize, "off=%s" % ("i64" if ts.np_off == np.int64 else "i32")}
    if ts.name == "count_mix":
        s.add("five_independent_types")
    if c.shift:
        s.add("shift=%d" % c.shift)
    return s


# ---- structures --------------------------------------------------------------------------------------------------------
def pad_mean(lens, T):
    """The same rows with empty rows (or rows of 4 T) appended until nnz // n_rows picks T."""
    lens = list(lens)
    lo, hi = band_of(T)
    while sum(lens) // len(lens) > hi:
        lens.append(0)
    while sum(lens) // len(lens) < lo:
        lens.append(4 * T)
    assert lanes_of(sum(lens) // len(lens)) == T, (T, sum(lens), len(lens))
    return lens


def steps_matrix(T):
    """Rows of every length 0 .. 8 T + 4 and of 12 T - 3, - 2, - 1 (the three tail lengths at three strides), behind an
    empty first row; empty rows at the last slot of workgroup 0 and the first of workgroup 1; empty rows behind."""
    lens = [0] + list(range(8 * T + 5)) + [12 * T - 3, 12 * T - 2, 12 * T - 1]
    k = BLOCK // T
    while len(lens) < k - 1:                                             # (T = 2, 4: rows of 1 up to the workgroup's end)
        lens.append(1)
    lens[k - 1:k - 1] = [0, 0]
    lens = pad_mean(lens, T)
    if lens[-1]:
        lens.append(0)
    return pad_mean(lens, T)


def lanes_matrices():
    """Per threshold m of the T rule: nnz // n_rows = m exactly, = m by the floor alone (one nonzero short of m + 1), and
    = m + 1; 300 rows of m - 3 and m + 3 (+ 1) nonzeros."""
    out = []
    n = 300
    for m in T_MEANS:
        at = [m - 3, m + 3] * (n // 2)
        above = [m - 2, m + 4] * (n // 2)
        floor = list(above)
        floor[7] -= 1
        out += [("mean_%d" % m, at, m, False), ("mean_%d_by_floor" % m, floor, m, True), ("mean_%d" % (m + 1), above, m + 1, False)]
    return out


def long_edge_matrix(T):
    LL = long_len_of(T)
    return pad_mean([LL - 1, 5, LL, 0, LL + 1, 7], T)


def nnz_edge_matrices():
    """nnz = long_len exactly (no long launch) and long_len + 1 in ONE row (launched, and found), per long_len."""
    out = []
    for T, n, n1 in ((8, 64, 64), (32, 48, 40), (64, 1, 1)):
        LL = long_len_of(T)
        base, extra = divmod(LL, n)
        eq = [base] * (n - 1) + [base + extra]
        one = [0] * n1
        one[n1 // 2] = LL + 1
        assert sum(eq) == LL and lanes_of(LL // n) == T and lanes_of((LL + 1) // n1) == T
        out += [("nnz_LL%d" % LL, eq, T), ("nnz_LL%d+1" % LL, one, T)]
    return out


WALK_MODS = (0, 1, 63, 64, 65, 191, 192, 193, 255)


def walk_matrix():
    lens = []
    for m in WALK_MODS:
        L = LONG_MIN + 1
        while L % (4 * WAVE) != m:
            L += 1
        lens += [3, L, 2]
    return pad_mean(lens, 4)


def ballot_matrices():
    LONG = LONG_MIN + 1
    a = [2] * (WAVE * 10 + 1)
    for g, lanes in enumerate(((0,), (63,), (0, 63), (31, 32))):        # the four waves of workgroup 0
        for l in lanes:
            a[g * WAVE + l] = LONG
    a[-1] = LONG                                                         # n_rows % 64 == 1, the last row long
    b = [0] * (WAVE * 32 + 63)
    for l in range(WAVE):
        b[5 * WAVE + l] = LONG
    b[-1] = LONG                                                         # n_rows % 64 == 63
    assert long_len_of(lanes_of(sum(a) // len(a))) == LONG_MIN and long_len_of(lanes_of(sum(b) // len(b))) == LONG_MIN
    return a, b


STRIDE_LONG = LONG_MIN + 1


def stride_matrix(rows_grid, long_grid, extra=300):
    """T = 2: n_rows = rows_grid * 128 * k + extra with k such that both kernels go a second round (k = 1 at the true
    caps), rows of r % 3 nonzeros, rows of 2 049 at the first group's lanes 0, 63 and the next group's 0, on both sides of
    the long kernel's first round end, at lane 63 of its second round's first group, and in the last row."""
    per_long = long_grid * BLOCK
    k = 1
    while rows_grid * 128 * k + extra <= per_long + 64 or (7 * STRIDE_LONG) // (rows_grid * 128 * k + extra) + 1 > T_MEANS[0]:
        k += 1
    n = rows_grid * 128 * k + extra
    lens = np.arange(n, dtype=np.int64) % 3
    for r in (0, 63, 64, per_long - 1, per_long, per_long + 63, n - 1):
        lens[r] = STRIDE_LONG
    assert int(lens.sum()) // n <= T_MEANS[0]
    return lens


# ---- the table ---------------------------------------------------------------------------------------------------------
FAMILIES = ("lanes", "steps", "long_edge", "long_walk", "ballot", "stride", "types", "unaligned")
LONG_LENS = (2048, 4096, 8192)
PLANT_STATES = ["plant_first", "plant_last", "plant_slot0", "plant_slot1", "plant_slot2", "plant_slot3", "plant_tail0", "plant_tail1",
                "plant_tail2", "plant_on_last_lane", "plant_in_a_later_step", "plant_long_main_slot0", "plant_long_main_slot1",
                "plant_long_main_slot2", "plant_long_main_slot3", "plant_long_tail", "plant_long_lane0", "plant_long_lane63"]
STRIDE_STATES = ["rows_round2", "rows_last_round_partial", "rows_kernel_skips_a_long_row_in_round2", "rows_kernel_takes_a_row_in_round2",
                 "long_round2", "long_row_last_of_round1", "long_row_first_of_round2", "long_row_lane63_of_round2", "long_row_is_last_row",
                 "ballot={0,63}", "ballot={0}", "ballot={63}", "T=2"]
STATES = {
    "lanes": ["T=%d" % t for t in LANES] + ["mean=%d" % (m + e) for m in T_MEANS for e in (0, 1)] + ["floor_decides"],
    "steps": ["T%d:%s" % (t, v) for t in LANES for v in (
        "lengths_0..8T+4", "len=4T-1", "len=4T", "len=4T+1", "len=8T-1", "len=8T", "len=8T+1", "tail_on_last_lane", "tail_on_lane0_in_a_later_step",
        "tail1@strides2", "tail2@strides2", "tail3@strides2", "tail1@strides3", "tail2@strides3", "tail3@strides3")] + [
        "empty_first_of_wg", "empty_last_of_wg", "empty_first_row", "empty_last_row"],
    "long_edge": ["LL%d:%s" % (v, e) for v in LONG_LENS for e in ("len=LL-1", "len=LL", "len=LL+1", "nnz=LL", "nnz=LL+1")] + [
        "one_row", "no_long_launch", "long_launch"],
    "long_walk": ["walk_mod=%d" % m for m in WALK_MODS] + ["walk_main_2plus"],
    "ballot": ["ballot={0}", "ballot={63}", "ballot={0,63}", "ballot={31,32}", "ballot=all64", "last_group_rows=1_last_row_long",
               "last_group_rows=63_last_row_long", "long_rows_in_two_waves_of_a_wg"],
    "stride": STRIDE_STATES,
    "types": ["y_bytes=%d" % b for b in Y_BYTES] + ["off=i32", "off=i64", "five_independent_types"] + PLANT_STATES,
    "unaligned": ["shift=1", "shift=3", "phase0", "phase1", "phase2", "phase3"],
}


def states():
    return set().union(*[set(v) for v in STATES.values()])


def _table():
    seed = [9000]
    matrices = {}

    def matrix(name, lens, plant=True):
        if name not in matrices:
            seed[0] += 1
            matrices[name] = Matrix(name, tuple(int(v) for v in lens), seed[0], plant)
        return matrices[name]

    def case(family, m, typeset, edge, shift=0, grids=(0, 0), sim=True, tag=""):
        return Case("%s-%s%s" % (m.name, typeset, tag), family, m, typeset, tuple(edge), shift, grids, sim)

    out = []
    # lanes
    for name, lens, mean, floor in lanes_matrices():
        edge = ["T=%d" % lanes_of(mean), "mean=%d" % mean] + (["floor_decides"] if floor else [])
        out.append(case("lanes", matrix(name, lens), "pt_f32", edge))
    # steps
    step_names = [v.split(":", 1)[1] for v in STATES["steps"] if v.startswith("T2:")]
    for T in LANES:
        edge = ["T%d:%s" % (T, v) for v in step_names] + ["T=%d" % T, "empty_first_of_wg", "empty_last_of_wg", "empty_first_row", "empty_last_row"]
        out.append(case("steps", matrix("steps_T%d" % T, steps_matrix(T)), "pt_f32", edge))
    # long edge
    for T in (8, 32, 64):
        LL = long_len_of(T)
        out.append(case("long_edge", matrix("long_edge_LL%d" % LL, long_edge_matrix(T)), "pt_f32",
                        ["LL%d:len=%s" % (LL, e) for e in ("LL-1", "LL", "LL+1")] + ["long_launch"]))
    for name, lens, T in nnz_edge_matrices():
        LL = long_len_of(T)
        plus = name.endswith("+1")
        edge = ["LL%d:nnz=%s" % (LL, "LL+1" if plus else "LL"), "long_launch" if plus else "no_long_launch"] + (["one_row"] if len(lens) == 1 else [])
        edge += ["LL%d:len=LL+1" % LL] if plus else []
        out.append(case("long_edge", matrix(name, lens), "pt_f32", edge))
    # long walk
    walk = matrix("long_walk", walk_matrix())
    out.append(case("long_walk", walk, "pt_f32", STATES["long_walk"]))
    # ballot
    a, b = ballot_matrices()
    ballot_a = matrix("ballot_lanes", a)
    out.append(case("ballot", ballot_a, "pt_f32", ["ballot={0}", "ballot={63}", "ballot={0,63}", "ballot={31,32}", "last_group_rows=1_last_row_long",
                                                   "long_rows_in_two_waves_of_a_wg"]))
    out.append(case("ballot", matrix("ballot_all64", b), "pt_f32", ["ballot=all64", "last_group_rows=63_last_row_long"]))
    # stride: the true caps on the device alone; the same shape at two and one workgroups in the simulation (and on the
    # device, where the grids are the shape's own and it is one more ragged matrix)
    out.append(case("stride", matrix("stride_true_caps", stride_matrix(ROWS_CAP, LONG_CAP), plant=False), "pt_f32", STRIDE_STATES, sim=False))
    out.append(case("stride", matrix("stride_small", stride_matrix(2, 1), plant=False), "pt_f32", STRIDE_STATES, grids=(2, 1), tag="-grids2x1"))
    # types: every type set on the steps of T = 2 and T = 8, a ragged matrix with two long rows, and the ballot lanes
    mix = matrix("types_mix", pad_mean(list(range(41)) + [LONG_MIN + 1, 0, 1, LONG_MIN + 65] + list(range(40, 0, -3)), 16))
    for ts in TYPE_SETS.values():
        edge = ["y_bytes=%d" % ts.np_y.itemsize, "off=%s" % ("i64" if ts.np_off == np.int64 else "i32")]
        edge += ["five_independent_types"] if ts.name == "count_mix" else []
        for m in (matrices["steps_T2"], matrices["steps_T8"], mix, ballot_a, walk):
            if ts.name == "pt_f32" and m is not mix:
                continue
            planted = sorted(census(m.lens, plant=True).states & set(PLANT_STATES)) if ts.op not in ("plus_times", "count") else []
            out.append(case("types", m, ts.name, edge + planted))
    # unaligned
    lens = pad_mean([5, 6, 7, 9, 0, 12, 4, 1, 2, 3, 8, 11] * 24 + [LONG_MIN + 1, 5, 6, 7, LONG_MIN + 3], 4)
    un = matrix("unaligned", lens)
    for shift in (1, 3):
        for ts in ("pt_f32", "pt_f64_i64", "min_i16"):
            out.append(case("unaligned", un, ts, ["shift=%d" % shift, "phase0", "phase1", "phase2", "phase3"], shift=shift, tag="-shift%d" % shift))
    return out


_tables = []


def table():
    if not _tables:
        _tables.append(_table())
    return _tables[0]


def family(name):
    return [c for c in table() if c.family == name]


def real_cases():
    """One real-valued (+, x) case per T: the steps matrices, for the parity bound."""
    return [c for c in family("steps") if c.typeset == "pt_f32"]


# ---- operands ------------------------------------------------------------------------------------------------------------
C_BIG, C_SMALL = N_COLS - 1, N_COLS - 3         # odd columns: no ordinary nonzero references them
_arrays = {}


def arrays(m, plant_kind, real=False):
    """(Ap int64, Aj int32, Ax float64, x float64, used columns) of a matrix; made once and left unchanged.  Ordinary
    nonzeros reference EVEN columns; plant_kind ("times" | "plus" | "or") says how the planted elements are extreme."""
    key = (m.name, plant_kind, real)
    if key in _arrays:
        return _arrays[key]
    rng = np.random.RandomState(m.seed)
    lens = np.asarray(m.lens, dtype=np.int64)
    n = len(lens)
    Ap = np.concatenate(([0], np.cumsum(lens)))
    nnz = int(Ap[-1])
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(nnz) - Ap[rows]
    half = (N_COLS - 4) // 2
    Aj = 2 * ((3 * rows + pos) % half)
    if real:
        Ax, x = rng.rand(nnz) * 2 - 1, rng.rand(N_COLS) * 2 - 1
    else:
        Ax = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=nnz)
        x = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=N_COLS)
        if plant_kind == "or":
            x[:] = 0.0
        x[C_BIG], x[C_SMALL] = (1.0, 0.0) if plant_kind == "or" else (5.0, -5.0)
        if m.plant:
            T = lanes_of(nnz // n)
            hi, lo = plant_positions(lens, T)
            r = np.nonzero(hi >= 0)[0]
            Aj[Ap[r] + hi[r]], Ax[Ap[r] + hi[r]] = C_BIG, 3.0
            Aj[Ap[r] + lo[r]], Ax[Ap[r] + lo[r]] = C_SMALL, (-3.0 if plant_kind == "plus" else 3.0)
    used = np.zeros(N_COLS, dtype=bool)
    used[Aj] = True
    _arrays[key] = (Ap, Aj.astype(np.int32), Ax, x, used)
    return _arrays[key]


def operands(c, real=False):
    """(Ap, Aj, Ax, x) in the case's types; x holds NaN (an integer x: bytes 0x5A) where no row references it."""
    ts = TYPE_SETS[c.typeset]
    Ap, Aj, Ax, x, used = arrays(c.matrix, ts.plant, real)
    xv = x.astype(ts.np_x)
    if np.issubdtype(ts.np_x, np.floating):
        xv[~used] = np.nan
    else:
        xv.view(np.uint8).reshape(len(xv), -1)[~used] = FILL
    return Ap.astype(ts.np_off), Aj, Ax.astype(ts.np_mat), xv


def _fold(ufunc, terms, Ap, init, dtype):
    out = np.full(len(Ap) - 1, init, dtype=dtype)
    lens = np.diff(Ap)
    rows = np.nonzero(lens > 0)[0]
    if rows.size:
        out[rows] = ufunc.reduceat(terms, Ap[:-1][rows])
    return out


def expected(c, real=False):
    """y of the case: per row a fold over combine(Ax[k], x[Aj[k]]) from initialize(), in float64 / int64 (every term and
    every partial result of the integer data is exact there, so the order of the fold does not matter), then in y's type."""
    ts = TYPE_SETS[c.typeset]
    Ap, Aj, Ax, x = operands(c, real)
    Ap = Ap.astype(np.int64)
    a, b = Ax.astype(np.float64), x.astype(np.float64)[Aj]
    assert not np.isnan(b).any()
    times, plus = a * b, a + b
    op = ts.op
    if op == "plus_times":
        if real:                                 # (the product type of the functor: Y(a * x), summed in Y)
            times = (Ax * x[Aj]).astype(np.float64)
        return _fold(np.add, times, Ap, 0.0, np.float64).astype(ts.np_y)
    if op == "min_plus":
        return _fold(np.minimum, plus, Ap, np.inf, np.float64).astype(ts.np_y)
    if op == "max_plus":
        return _fold(np.maximum, plus, Ap, -np.inf, np.float64).astype(ts.np_y)
    if op == "max_times":
        return _fold(np.maximum, times, Ap, -np.inf, np.float64).astype(ts.np_y)
    if op == "or_and":
        return _fold(np.maximum, ((a != 0) & (b != 0)).astype(np.int64), Ap, 0, np.int64).astype(ts.np_y)
    if op == "min_plus_i16":
        return _fold(np.minimum, plus.astype(np.int64), Ap, 32767, np.int64).astype(np.int16)
    if op == "count":
        return _fold(np.add, times.astype(np.int64) + 1000000 * (times > 2.5), Ap, 0, np.int64)
    y = np.zeros(len(Ap) - 1, dtype=ts.np_y)
    ones = np.ones(len(a), dtype=np.int64)
    if op == "tri":
        t = times.astype(np.int64)
        y["sum"] = _fold(np.add, t, Ap, 0, np.int64).astype(np.int16)
        y["lo"], y["hi"] = _fold(np.minimum, t, Ap, 32767, np.int64), _fold(np.maximum, t, Ap, -32768, np.int64)
    elif op == "stat12":
        y["hi"], y["lo"] = _fold(np.maximum, times, Ap, -np.inf, np.float64), _fold(np.minimum, times, Ap, np.inf, np.float64)
        y["count"] = _fold(np.add, ones, Ap, 0, np.int64)
    elif op == "stat16":
        y["sum"], y["hi"] = _fold(np.add, times, Ap, 0.0, np.float64), _fold(np.maximum, times, Ap, -np.inf, np.float64)
        y["count"] = _fold(np.add, ones, Ap, 0, np.int64)
    else:
        raise AssertionError(op)
    return y


def y_buffer(c):
    """y before the call, as bytes: n_rows + 2 GUARD elements of bytes 0x5A, which no result equals."""
    ts = TYPE_SETS[c.typeset]
    return np.full((len(c.matrix.lens) + 2 * GUARD) * ts.np_y.itemsize, FILL, dtype=np.uint8)


def weight(c):
    return len(c.matrix.lens) + sum(c.matrix.lens)
