"""Non-finite operands for the group product (pygim_spmm_run_group, pygim_block_run, pygim_grande_run_group, pygim_spmv_run_group): the graph,
the poisoned features and values, the CPU loop's answer with the set of outputs the poison may reach, the comparison rule and the table of
kernel forms.  Host only; tests/test_group_nonfinite_cpu.py proves this fixture, tests/test_group_nonfinite_gpu.py runs the table.

Why non-finite operands: every form of the product has lanes, tokens or slots that do no useful work (masked lanes that load column 0 with
value 0, padding tokens that point at column 0, partly filled chunks, partial sums that are added back).  With finite X a `0 x garbage` term
or a sum that lands in the neighbouring row, feature or slice is invisible or tiny; with X[0, :] = NaN it is a NaN in an output that must
not hold one.  Only values change, never an index, so the probes cannot cause a memory fault.

The clean features are the reference driver's small integers, so every finite sum is exact in whatever order a form adds it, and ONE rule
(compare) serves all forms, the reordering ones included.  The one operand that would break this is the subnormal column: an integer plus a
subnormal rounds the subnormal away, and whether a row keeps it then depends on whether its integer partial sum passes through zero, i.e.
on the order.  So column 65 is kept out of every row but the two that are there for it (rows 6 and 8, whose other terms are zeros), and
the subnormal value sits on the single entry of row 3; mixing magnitudes in one sum is rounding, which is outside every form's contract.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle
from conftest import NP_DTYPES, coalesce, driver_features, random_csr

NROWS, NCOLS = 600, 500
DTYPES = ("FLT32", "DBL64")
WEIGHTS = ("unit", "valued")
# rows every graph of this file holds (-1 = the last column), sorted inside a row: unsorted rows would switch the panel plans off
FIXED_ROWS = ((1, (0,)), (2, (-1,)), (3, (63,)), (4, ()), (5, (64, 64, 64)), (6, (65, 65)), (7, (63, -1)), (8, (64, 65)))
COL_NEG_ZERO, COL_SUBNORMAL, COL_BOTH_INF, COL_SLICE = 64, 65, 255, 128
SUBNORMAL_ROWS = (6, 8)


def overwrite_rows(rowptr, col, ncols):
    """the CSR with FIXED_ROWS written over rows 1..8 and column 65 moved to 66 in every other row (see the module's docstring)"""
    nrows = len(rowptr) - 1
    assert nrows > 16 and ncols > COL_BOTH_INF + 1
    rows_of = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    keep = ~np.isin(rows_of, [r for r, _ in FIXED_ROWS])
    r_old, c_old = rows_of[keep], col[keep].astype(np.int64)
    c_old[c_old == COL_SUBNORMAL] = COL_SUBNORMAL + 1
    r_new = np.array([r for r, cs in FIXED_ROWS for _ in cs], dtype=np.int64)
    c_new = np.array([c % ncols for _, cs in FIXED_ROWS for c in cs], dtype=np.int64)
    r_all, c_all = np.concatenate([r_old, r_new]), np.concatenate([c_old, c_new])
    order = np.lexsort((c_all, r_all))
    out_ptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(r_all, minlength=nrows), out=out_ptr[1:])
    return _frozen(out_ptr.astype(np.int32)), _frozen(c_all[order].astype(np.int32))


def _frozen(a):
    a.flags.writeable = False
    return a


# name -> (seed, rows, columns, mean degree, empty fraction, long rows).  "base" is the graph of every form that engages on it; the others
# are the graphs of the existing finite tests of forms that need more (tests/test_parity_gpu.py, tests/test_lds_gpu.py, tests/test_codegen_gpu.py)
GRAPHS = {
    "base": (1, NROWS, NCOLS, 12, 0.15, ((0, 3000), (77, 257), (599, 1200))),
    "deg3": (2, 300, 400, 3, 0.1, ((9, 5000),)),            # test_csr_vector_kernel_for_rows_of_one_to_four_elements: the 4-lane groups
    "deg60": (3, 300, 400, 60, 0.1, ((9, 5000),)),          # ... and the 32-lane groups
    "spmv_lds": (4, 2600, 2600, 160, 0.03, ((9, 3000), (2598, 900))),   # test_lds_staged_spmv_kernel
    "wide": (5, 2500, 30000, 150, 0.1, ((9, 9000),)),       # test_short_row_shares_split_their_tiles_into_column_ranges
    "tail": (6, 16 * 1824 + 200, 40000, 40, 0.05, ((16 * 1824 + 193, 3000), (11, 5000), (16 * 1824 + 50, 0))),   # test_a_share_that_all_but_fits_...
    "half": (7, 5000, 30001, 60, 0.1, ((9, 9000), (4999, 4000))),       # test_half_split_plans_for_products_of_at_most_32_lanes
}


@functools.lru_cache(maxsize=None)
def graph(name="base"):
    """(rowptr, col, ncols) of a named graph with the fixed rows written in; built once, read-only"""
    seed, nrows, ncols, deg, empty, long_rows = GRAPHS[name]
    rowptr, col = random_csr(np.random.default_rng(seed), nrows, ncols, deg, empty_frac=empty, long_rows=list(long_rows))
    rowptr, col = overwrite_rows(rowptr, col, ncols)
    return rowptr, col, ncols


@functools.lru_cache(maxsize=None)
def coalesced(name="base"):
    """the same graph as COO input: (row, col, counts, rowptr, ncols), sorted and free of duplicates (a duplicate becomes a count)"""
    rowptr, col, ncols = graph(name)
    r, c, n = coalesce(rowptr, col, np.float64)
    rp = np.zeros(len(rowptr), dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=len(rowptr) - 1), out=rp[1:])
    return _frozen(r), _frozen(c), _frozen(n), _frozen(rp.astype(np.int32)), ncols


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr.astype(np.int64)))


def subnormal(npdt):
    return np.nextafter(npdt(0), npdt(1))


# what one case multiplies: the poisoned operands, the clean ones they were laid over, and where the poison sits
Operands = namedtuple("Operands", "x x_clean vals vals_clean poisons entries")


def poison_features(x_clean, edge_cols=()):
    """(X, [(column, features)]): the table of poisons laid over clean features.  edge_cols: the last column of one panel or chunk
    and the first of the next (+inf in feature 0)"""
    x = x_clean.copy()
    ncols, h = x.shape
    npdt, poisons = x.dtype.type, []

    def put(c, feats, value):
        feats = np.unique(np.asarray(feats, dtype=np.int64))
        x[c, feats] = value
        poisons.append((int(c), feats))

    every = np.arange(h)
    for c in edge_cols:
        if 0 < c < ncols and c not in (COL_NEG_ZERO, COL_SUBNORMAL):
            put(c, [0], np.inf)
    per_slice = 256 // x.itemsize
    if h > per_slice:   # the last feature of the first 256-byte slice and the first of the second
        put(COL_SLICE, [per_slice - 1], -np.inf)
        put(COL_SLICE, [per_slice], np.inf)
    put(COL_BOTH_INF, [0], np.inf)
    put(COL_BOTH_INF, [h - 1], -np.inf)
    put(0, every, np.nan)                       # where masked lanes and padding tokens point
    put(ncols - 1, [0, h - 1], np.inf)
    put(63, [h // 2], -np.inf)
    put(COL_NEG_ZERO, every, npdt(-0.0))
    put(COL_SUBNORMAL, every, ((every % 7) - 3).astype(npdt) * subnormal(npdt))
    return x, poisons


def poison_values(rowptr, vals_clean, small_subnormal=None):
    """(values, [entry]): a stored 0 on the single entry of row 2 (its column holds +inf), +inf, NaN and -0.0 on entries of the first three
    non-empty rows from row 10 on, a subnormal on the single entry of row 3.  small_subnormal: that subnormal, when the type's own will not do"""
    vals = vals_clean.copy()
    npdt = vals.dtype.type
    deg = np.diff(rowptr.astype(np.int64))
    free = [r for r in range(10, len(deg)) if 0 < deg[r] < 200][:3]
    assert len(free) == 3 and deg[2] == 1 and deg[3] == 1
    entries = [int(rowptr[2]), int(rowptr[free[0]]), int(rowptr[free[1] + 1]) - 1, int(rowptr[free[2]]) + int(deg[free[2]]) // 2, int(rowptr[3])]
    vals[entries[0]] = 0.0
    vals[entries[1]] = np.inf
    vals[entries[2]] = np.nan
    vals[entries[3]] = npdt(-0.0)
    vals[entries[4]] = npdt(3) * (subnormal(npdt) if small_subnormal is None else npdt(small_subnormal))
    return vals, entries


def operands(seed, rowptr, ncols, h, npdt, weights, nnz=None, edge_cols=(), counts=None, small_subnormal=None):
    """clean features (conftest.driver_features) and, for "valued", integer values in [-3, 3], with the poison laid over both.
    counts: the multiplicities of a coalesced graph -- its weights when the case is "unit" (a COO group always carries values) """
    rng = np.random.default_rng(seed)
    x_clean = driver_features(rng, ncols, h, npdt)
    x, poisons = poison_features(x_clean, edge_cols)
    nnz = int(rowptr[-1]) if nnz is None else nnz
    if weights == "unit":
        v = None if counts is None else counts.astype(npdt)
        return Operands(x, x_clean, v, v, poisons, [])
    vals_clean = rng.integers(-3, 4, size=nnz).astype(npdt)
    vals, entries = poison_values(rowptr, vals_clean, small_subnormal)
    return Operands(x, x_clean, vals, vals_clean, poisons, entries)


def affected_mask(rowptr, col, h, poisons, entries=()):
    """from the structure alone: rows that hold a poisoned column x that column's poisoned features, and the rows of the poisoned values"""
    nrows = len(rowptr) - 1
    r_of = rows_of(rowptr)
    mask = np.zeros((nrows, h), dtype=bool)
    for c, feats in poisons:
        mask[np.ix_(np.unique(r_of[col == c]), feats)] = True
    for e in entries:
        mask[r_of[e], :] = True
    return mask


def expected(rowptr, col, ops, fmt="CSR", parts=None):
    """(the CPU loop's product, the affected mask).  fmt "CSR" / "COO" (rowptr is the coalesced graph's) / "GROUP" (parts: the column blocks
    [(rowptr, local col, vals, ncols)] the group was created from, multiplied and added block by block like the reference's group driver)"""
    nrows, h = len(rowptr) - 1, ops.x.shape[1]
    if fmt == "CSR":
        want = oracle.spmm_csr(rowptr, col, ops.vals, ops.x)
    elif fmt == "COO":
        want = oracle.spmm_coo(rows_of(rowptr), col, ops.vals, ops.x, nrows)
    else:
        want = oracle.group(False, [p[0] for p in parts], [p[1] for p in parts], None if ops.vals is None else [p[2] for p in parts],
                            [nrows] * len(parts), [p[3] for p in parts], [ops.x], h)
    return want, affected_mask(rowptr, col, h, ops.poisons, ops.entries)


def column_blocks(rowptr, col, vals, bounds):
    """the column blocks [bounds[i], bounds[i + 1]) as CSR parts with local column ids: [(rowptr, col, vals or None, ncols)]"""
    nrows, r_of = len(rowptr) - 1, rows_of(rowptr)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        k = (col >= lo) & (col < hi)
        rp = np.zeros(nrows + 1, dtype=np.int64)
        np.cumsum(np.bincount(r_of[k], minlength=nrows), out=rp[1:])
        parts.append((rp.astype(np.int32), (col[k] - lo).astype(np.int32), None if vals is None else np.ascontiguousarray(vals[k]), hi - lo))
    return parts


def classes(a):
    """how many elements of each kind an array holds"""
    tiny = np.finfo(a.dtype).tiny
    return {"nan": int(np.isnan(a).sum()), "+inf": int(np.isposinf(a).sum()), "-inf": int(np.isneginf(a).sum()),
            "subnormal": int(((a != 0) & (np.abs(a) < tiny)).sum()), "-0.0": int(((a == 0) & np.signbit(a)).sum())}


def compare(got, want, what=""):
    """the rule of every case, no tolerance: NaN exactly where the CPU loop has NaN (payload and sign of a NaN are not compared), every other
    element the CPU loop's bits -- the sign of an infinity, every subnormal, the sign of zero -- and no -0.0 anywhere"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g_nan, w_nan = np.isnan(got), np.isnan(want)
    bad = (g_nan != w_nan) | (~w_nan & ~g_nan & (np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)))
    if bad.any():
        where = np.argwhere(bad)
        rows = np.unique(where[:, 0])
        first = [(int(r), int(f), got[r, f].item(), want[r, f].item()) for r, f in where[:12]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ from the CPU loop in {len(rows)} rows "
                             f"(rows {rows[:20].tolist()}); (row, feature, got, want): {first}; got {classes(got)}, want {classes(want)}")
    assert classes(got)["-0.0"] == 0, (what, "a product returned -0.0")


# ---- the forms ---------------------------------------------------------------------------------------------------------------------------------
# One row per kernel form.  knobs: tunables set for the whole case; create_knobs: only while the group is created (the finite test of the form
# does the same); entry: how the product is called (tests/test_group_nonfinite_gpu.py, RUNNERS); proof: what the group's own queries must say
# -- (query, field or None, "==" | ">=" | "has" | "lacks", value) -- and forced: the words "forced by knob only" with the reason, where no
# query tells the form from its neighbour; edge: the query field whose value W puts +inf into feature 0 of columns W - 1 and W.
Case = namedtuple("Case", "form graph fmt entry knobs create_knobs hs dtypes weights proof forced edge")


def case(form, knobs, hs, proof=(), forced="", graph="base", fmt="CSR", entry="spmm", create_knobs=None, dtypes=DTYPES, weights=WEIGHTS, edge=None):
    return Case(form, graph, fmt, entry, dict(knobs), dict(create_knobs or {}), tuple(hs), tuple(dtypes), tuple(weights), tuple(proof), forced, edge)


ROW_PER_WAVE = {"panel_mode": 2, "lds_mode": 0}
NO_PANEL_PLAN = (("plan", "n_panels", "==", 0), ("lds_runs", None, "==", 0))
SWEEP = {"panel_mode": 1, "lds_mode": 0, "panel_bytes": 128 * 40}
MANY_PANELS = (("plan", "n_panels", ">=", 10), ("lds_runs", None, "==", 0))
LDS = {"lds_mode": 1}
GEO_KNOBS = ("lds_code_waves", "lds_code_nbuf", "lds_code_kc", "lds_code_gsize", "lds_code_nsets", "lds_code_boundary")
CODE_STREAM = (("lds_plan", "tiles", ">=", 1), ("lds_code", "active", "==", 1), ("lds_runs", None, ">=", 1))
HYBRID_KNOBS = {"lds_mode": 0, "lds_min_reuse_x100": 10 ** 6, "panel_locality": 2, "lds_hybrid_min": 32, "lds_hybrid": 2}   # tests/test_hybrid_gpu.py TUNE


def token(waves):
    return (("lds_plan", "tiles", ">=", 1), ("lds_code", "active", "==", 0), ("lds_geometry", "waves", "==", waves), ("lds_runs", None, ">=", 1))


CASES = [
    # -- one row per wave
    case("row per wave, wide (k_csr_wide)", {**ROW_PER_WAVE, "csr_kernel": 1}, (64, 100, 300), NO_PANEL_PLAN,
         "forced by knob only: no query tells k_csr_wide from k_csr_sub"),
    case("row per wave, sub-wave (k_csr_sub)", {**ROW_PER_WAVE, "csr_kernel": 2}, (3, 9, 32), NO_PANEL_PLAN,
         "forced by knob only: no query tells k_csr_sub from k_csr_wide"),
    case("long rows (k_long_segments, k_long_reduce)", {**ROW_PER_WAVE, "long_row_threshold": 256}, (64, 100, 300),
         NO_PANEL_PLAN + (("info", "n_long_rows", "==", 3),)),
    case("long rows in short segments", {**ROW_PER_WAVE, "long_row_threshold": 256, "long_segment": 64}, (9, 100),
         NO_PANEL_PLAN + (("info", "n_long_rows", "==", 3),)),
    case("long rows beside the sweep", {"panel_mode": 1, "lds_mode": 0, "long_row_threshold": 64}, (64,), (("plan", "n_segment_tasks", ">=", 2), ("lds_runs", None, "==", 0))),
    # -- COO: rows 0 and 599 straddle several chunks of 64 entries (left-open, right-open and whole-chunk carries)
    case("native COO (k_coo_wide, k_coo_fixup)", {**ROW_PER_WAVE, "coo_via_rowptr": 0, "coo_chunk": 64}, (100, 300), NO_PANEL_PLAN,
         "forced by knob only: the native kernel takes COO groups of more than 16 lanes when no sweep is planned", fmt="COO"),
    case("COO through the derived row pointers", {**ROW_PER_WAVE, "coo_via_rowptr": 1}, (100, 300), NO_PANEL_PLAN, "forced by knob only: coo_via_rowptr", fmt="COO"),
    # -- the SpMV end
    case("k_csr_vec, 4-lane groups", {"vec_kernel": 1, "vec_lds": 0}, (1, 2, 3, 4), (("lds_runs", None, "==", 0),),
         "forced by knob only: vec_lds = 0 leaves k_csr_vec, and the lane group follows the mean degree", graph="deg3"),
    case("k_csr_vec, 32-lane groups", {"vec_kernel": 1, "vec_lds": 0}, (1, 2, 3, 4), (("lds_runs", None, "==", 0),),
         "forced by knob only: vec_lds = 0 leaves k_csr_vec, and the lane group follows the mean degree", graph="deg60"),
    case("k_csr_vec through pygim_spmv_run_group", {"vec_kernel": 1, "vec_lds": 0}, (3,), (("lds_runs", None, "==", 0),),
         "forced by knob only: vec_lds = 0", graph="deg60", entry="spmv", weights=("unit",)),
    case("k_spmv_lds", {"vec_kernel": 1, "vec_lds": 1, "panel_bytes": 128 * 900, "merge_parts": 0}, (1, 4), (("info", "n_panels", ">=", 3), ("plan", "col16", "==", 1)),
         "forced by knob only: vec_lds = 1 on a plan that meets the kernel's rule (160 / 3 entries per row and panel)", graph="spmv_lds", edge=("plan", "panel_cols")),
    # -- the L2 panel sweep
    case("panel sweep, every row continues from C", {**SWEEP, "panel_coop": 1 << 20}, (64, 100), MANY_PANELS + (("plan", "n_coop_items", "==", 0),), edge=("plan", "panel_cols")),
    case("panel sweep, cooperative items", {**SWEEP, "panel_coop": 64}, (64,), MANY_PANELS + (("plan", "n_coop_items", ">=", 1),), edge=("plan", "panel_cols")),
    case("panel sweep, 16-bit column ids", {**SWEEP, "panel_col16": 1}, (64,), MANY_PANELS + (("plan", "col16", "==", 1),), edge=("plan", "panel_cols")),
    case("panel sweep, 32-bit column ids", {**SWEEP, "panel_col16": 0}, (64,), MANY_PANELS + (("plan", "col16", "==", 0),), edge=("plan", "panel_cols")),
] + [
    case(f"panel sweep, {gs} slice(s) a launch, {'slice-major copy' if pack else 'row-major gathers'}",
         {"panel_mode": 1, "lds_mode": 0, "panel_bytes": 128 * 200, "slice_group_bytes": NCOLS * 128 * gs, "panel_pack": pack}, (100, 264),
         (("plan", "n_panels", ">=", 2), ("lds_runs", None, "==", 0)), "forced by knob only: slice_group_bytes, panel_pack", edge=("plan", "panel_cols"))
    for gs in (1, 3) for pack in (1, 0)
] + [
    case("panel sweep, misaligned widths", {"panel_mode": 1, "lds_mode": 0, "panel_bytes": 128 * 150, "merge_parts": 0}, (41, 255),
         (("plan", "n_panels", ">=", 2), ("lds_runs", None, "==", 0)), edge=("plan", "panel_cols")),
    case("panel sweep, strided block run adding twice onto a poisoned C", {"panel_mode": 1, "lds_mode": 0, "panel_bytes": 128 * 150, "merge_parts": 0}, (41, 255),
         (("plan", "n_panels", ">=", 2), ("lds_runs", None, "==", 0)), entry="block2", edge=("plan", "panel_cols")),
    # -- the LDS-staged product
    case("LDS code stream", LDS, (64, 100, 264), CODE_STREAM, edge=("lds_geometry", "chunk_cols")),
    case("LDS code stream, 8 waves and 5 buffers", {**LDS, **dict(zip(GEO_KNOBS, (8, 5, 0, 0, 0, 0)))}, (64, 100),
         CODE_STREAM + (("lds_geometry", "waves", "==", 8), ("lds_geometry", "buffers", "==", 5)), dtypes=("FLT32",), edge=("lds_geometry", "chunk_cols")),
    case("LDS code stream, 512-byte rows in a ring of 4 x 64 columns", {**LDS, "lds_code_nbuf": 4, "lds_code_kc": 64, "lds_code_gsize": 5, "lds_code_nsets": 2}, (64, 100),
         CODE_STREAM + (("lds_geometry", "waves", "==", 8), ("lds_geometry", "buffers", "==", 4), ("lds_geometry", "chunk_cols", "==", 64)), dtypes=("DBL64",),
         edge=("lds_geometry", "chunk_cols")),   # (tests/test_lds_gpu.py test_8_byte_elements_on_their_code_stream)
    case("LDS code stream, 16 waves, 3 buffers, groups of 8", {**LDS, **dict(zip(GEO_KNOBS, (16, 3, 0, 8, 2, 1)))}, (64, 100),
         CODE_STREAM + (("lds_geometry", "waves", "==", 16), ("lds_geometry", "buffers", "==", 3)), dtypes=("FLT32",), edge=("lds_geometry", "chunk_cols")),
    case("LDS token kernel, 16 waves", {**LDS, "lds_code": 0, "lds_waves": 16, "lds_long_slots": 0}, (64, 100), token(16), dtypes=("FLT32",), edge=("lds_geometry", "chunk_cols")),
    case("LDS token kernel, 8 waves", {**LDS, "lds_code": 0, "lds_waves": 8, "lds_long_slots": 0}, (64, 100), token(8), dtypes=("FLT32",), weights=("unit",),
         edge=("lds_geometry", "chunk_cols")),
    case("LDS token kernel, long slots", {**LDS, "lds_code": 0, "lds_waves": 16, "lds_long_slots": 1}, (64, 100), token(16), dtypes=("FLT32",), weights=("unit",),
         edge=("lds_geometry", "chunk_cols")),
    case("LDS ladder: generation fails, token form", LDS, (64,), token(16) + (("lds_note", None, "has", "token form"),), create_knobs={"lds_fail": 1}, dtypes=("FLT32",)),
    case("LDS ladder: no executable memory, token form", LDS, (64,), token(16) + (("lds_note", None, "has", "token form"),), create_knobs={"lds_fail": 2}, dtypes=("FLT32",)),
    case("LDS ladder: no schedule, the sweep", LDS, (64,), (("lds_plan", "tiles", "==", 0), ("lds_note", None, "has", "sweep"), ("lds_runs", None, "==", 0)),
         create_knobs={"lds_fail": 4}, dtypes=("FLT32",)),
    case("LDS one-slice product reads the caller's X", {**LDS, "lds_direct_x": 1}, (64,), CODE_STREAM, "forced by knob only: lds_direct_x", entry="device",
         edge=("lds_geometry", "chunk_cols")),
    case("LDS one-slice product reads a staged copy", {**LDS, "lds_direct_x": 0}, (64,), CODE_STREAM, "forced by knob only: lds_direct_x", entry="device",
         edge=("lds_geometry", "chunk_cols")),
    case("LDS column-split tiles, 2 ranges", {**LDS, "lds_col_split": 2, "lds_col_split_f32": 2}, (64, 264), CODE_STREAM + (("lds_geometry", "col_splits", "==", 2),),
         graph="wide", dtypes=("FLT32",), weights=("unit",), edge=("lds_geometry", "chunk_cols")),
    case("LDS column-split tiles, 3 ranges", {**LDS, "lds_col_split": 3, "lds_col_split_f32": 2}, (64, 264), CODE_STREAM + (("lds_geometry", "col_splits", "==", 3),),
         graph="wide", dtypes=("FLT32",), weights=("unit",), edge=("lds_geometry", "chunk_cols")),
    case("LDS column split asked for, FLT32 rule at its default", {**LDS, "lds_col_split": 2}, (64,), CODE_STREAM,
         "forced by knob only: whether a FLT32 part of this size is split is the library's rule; the case holds whichever form it picks to the CPU loop",
         graph="wide", dtypes=("FLT32",), weights=("unit",), edge=("lds_geometry", "chunk_cols")),
    case("LDS column split asked for, DBL64", {**LDS, "lds_col_split": 2}, (64,), (("lds_plan", "tiles", ">=", 1),),
         "forced by knob only: the 8-byte code stream serves whole-X tiles; a DBL64 share asked to split must still give the CPU loop's product",
         graph="wide", dtypes=("DBL64",), weights=("unit",)),
    case("LDS row tail (k_lds_tail)", {"lds_col_split_f32": 2}, (256,), (("lds_geometry", "col_splits", "==", 4), ("lds_note", None, "has", "k_lds_tail"), ("lds_runs", None, ">=", 1)),
         graph="tail", dtypes=("FLT32",), weights=("unit",), edge=("lds_geometry", "chunk_cols")),
    case("LDS half-split plan", {"lds_col_split_f32": 2, "lds_col_split": 0, "lds_mode": 0, "lds_half_split": 1}, (17, 32),
         (("lds_note", None, "has", "half-split"), ("lds_code", "active", "==", 1), ("lds_runs", None, "==", 1)), graph="half", dtypes=("FLT32",), weights=("unit",)),
    case("hybrid density split, floats asked for", HYBRID_KNOBS, (256,), (("lds_note", None, "has", "density split"), ("lds_runs", None, ">=", 1)),
         graph="hybrid", entry="device", dtypes=("FLT32",), weights=("unit",)),
    # -- several parts, windows, host operands
    case("three column blocks, merged", {"merge_parts": 1}, (64, 100), (("info", "n_parts", "==", 3), ("plan", "merged", "==", 1)), entry="parts"),
    case("three column blocks, the later parts add onto C", {"merge_parts": 0}, (64, 100), (("info", "n_parts", "==", 3), ("plan", "merged", "==", 0)), entry="parts"),
    case("three feature windows, fused into one product", {"fuse_windows": 1}, (100,), (), "forced by knob only: fuse_windows", entry="windows"),
    case("three feature windows, one product each", {"fuse_windows": 0}, (100,), (), "forced by knob only: fuse_windows", entry="windows"),
    case("grande windows with padded strides", {}, (100,), (), "forced by knob only: the entry point (pygim_grande_run_group)", entry="grande"),
] + [
    case(f"host operands, {hw} window(s), {'page-locked' if pinned else 'pageable'} result", {"host_windows": hw}, (264,), (("host_windows", None, "==", hw),),
         entry="pinned" if pinned else "spmm")
    for hw in (1, 3) for pinned in (False, True)
] + [
    case(f"DBL64 values streamed {'narrow' if nv else 'wide'}", {"narrow_vals": nv, "panel_mode": 1, "lds_mode": 0}, (64,), (("info", "all_ones", "==", 0), ("lds_runs", None, "==", 0)),
         "forced by knob only: narrow_vals", entry="narrow", dtypes=("DBL64",), weights=("valued",))
    for nv in (1, 0)
] + [
    case("transposed group of the backward", {}, (20, 64), (("info", "total_rows", "==", NROWS), ("info", "total_cols", "==", NCOLS), ("info", "n_parts", "==", 1)), entry="transposed"),
]


def params():
    """(case, type, weights) of every case of the table, with the ids pytest shows"""
    out, ids = [], []
    for c in CASES:
        for dt in c.dtypes:
            for w in c.weights:
                out.append((c, dt, w))
                ids.append(f"{c.form}-{dt}-{w}".replace(" ", "_"))
    return out, ids


__all__ = ["CASES", "Case", "DTYPES", "NP_DTYPES", "WEIGHTS", "affected_mask", "classes", "coalesced", "column_blocks", "compare", "expected", "graph",
           "operands", "overwrite_rows", "params", "poison_features", "poison_values", "rows_of", "subnormal"]
