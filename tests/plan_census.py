"""What a plan is, as plain data, and the shapes of the plan space as predicates over it — shared by the census of the
plans kept as A (tests/test_gpu_kept_plans.py) and the census of the whole plans whose row blocks were checked
(tests/test_gpu_block_shapes.py).  A census line is (label, predicate over (kind, info, extra)): `info` is Plan.info(),
`extra` the few fields of Plan.shape() that info() does not carry (describe() below)."""

REPORT = ("main_kernel", "block_threads", "lanes_per_row", "window_elems", "window_segments", "balanced_chunks",
          "grid_blocks", "n_chunks", "n_kernels")
PLAIN, TILE, RUNS = "csr_vector_kernel", "merge_tile_kernel", "merge_rows_kernel"
WINDOW = {"vector": "csr_vector_window_kernel", "light": "light_rows_window_kernel"}
SWEEP = {"vector": "csr_vector_sweep_kernel", "light": "light_rows_sweep_kernel"}


def describe(plan):
    """A plan's info, its shape as bytes, and the few shape fields the census reads."""
    info, sh = plan.info(), plan.shape()
    extra = {"window_from_band": sh.window_from_band, "window_sweep": sh.window_sweep, "small_plain": sh.small_plain,
             "band": int(sh.band_hi - sh.band_lo + 1), "probe_ok": sh.probe_ok}
    return info, bytes(sh), extra


def has_giant_list(kind, info):
    """VECTOR / LIGHT run one kernel, plus two for the slices of giant rows (rows_plan.hip, set_rows_launch); the merge
    kind has no such list."""
    return kind != "merge" and info["n_kernels"] == 3


def one_band(kind, threads):
    return lambda k, i, e: (k == kind and i["main_kernel"] == WINDOW[kind] and i["window_segments"] == 1 and
                            i["window_elems"] > 0 and e["window_from_band"] == 1 and i["balanced_chunks"] == 0 and
                            i["block_threads"] == threads)


def row_kind_lines():
    """The shapes of the row-local kinds, VECTOR and LIGHT."""
    lines = []
    for kind in ("vector", "light"):
        lines += [
            ("%s: one band-placed window, 256 threads" % kind, one_band(kind, 256)),
            ("%s: one band-placed window, 512 threads" % kind, one_band(kind, 512)),
            ("%s: one band-placed window, 1024 threads" % kind, one_band(kind, 1024)),
            ("%s: window kernel, window_segments >= 2" % kind,
             lambda k, i, e, kind=kind: k == kind and i["main_kernel"] == WINDOW[kind] and i["window_segments"] >= 2),
            ("%s: window kernel, window_elems == 0" % kind,
             lambda k, i, e, kind=kind: k == kind and i["main_kernel"] == WINDOW[kind] and i["window_elems"] == 0 and
             i["balanced_chunks"] == 0),
            ("%s: sweep kernel" % kind, lambda k, i, e, kind=kind: k == kind and i["main_kernel"] == SWEEP[kind]),
            ("%s: weight-cut chunks with a window" % kind,
             lambda k, i, e, kind=kind: k == kind and i["balanced_chunks"] == 1 and i["window_elems"] > 0),
            ("%s: weight-cut chunks without a window" % kind,
             lambda k, i, e, kind=kind: k == kind and i["balanced_chunks"] == 1 and i["window_elems"] == 0),
        ]
    lines += [
        ("light: grid_blocks < n_chunks", lambda k, i, e: k == "light" and i["grid_blocks"] < i["n_chunks"]),
        ("light: grid_blocks == n_chunks",
         lambda k, i, e: k == "light" and i["main_kernel"] != PLAIN and i["grid_blocks"] == i["n_chunks"]),
    ]
    return lines


def merge_lines():
    # merge: n_kernels = the main kernel, the carry fix-up when there is more than one run, and the search kernel in
    # front unless the main kernel searches its own coordinates (merge_plan.hip, shape_merge)
    searches_itself = lambda i: i["n_kernels"] == (2 if i["grid_blocks"] > 1 else 1)
    runs = lambda k, i: k == "merge" and i["main_kernel"] == RUNS
    sweeping = lambda i, e: i["block_threads"] == 1024 and 0 < i["window_elems"] < e["band"]
    return [
        ("merge: tile kernel, the search inside", lambda k, i, e: k == "merge" and i["main_kernel"] == TILE and searches_itself(i)),
        ("merge: tile kernel, the search kernel in front",
         lambda k, i, e: k == "merge" and i["main_kernel"] == TILE and not searches_itself(i)),
        ("merge: run kernel, 256 threads", lambda k, i, e: runs(k, i) and i["block_threads"] == 256),
        ("merge: run kernel, 512 threads", lambda k, i, e: runs(k, i) and i["block_threads"] == 512),
        ("merge: run kernel, 1024 threads, one band-placed window",
         lambda k, i, e: runs(k, i) and i["block_threads"] == 1024 and not sweeping(i, e)),
        ("merge: run kernel, window_segments >= 2", lambda k, i, e: runs(k, i) and i["window_segments"] >= 2),
        ("merge: run kernel, sweeping", lambda k, i, e: runs(k, i) and sweeping(i, e)),
    ]


def plain_lanes(kind, infos):
    """The lane widths of the plain kernel among `infos` of one kind."""
    return sorted({i["lanes_per_row"] for k, i in infos if k == kind and i["main_kernel"] == PLAIN})
