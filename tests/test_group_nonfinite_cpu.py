"""The fixture of tests/test_group_nonfinite_gpu.py, proven on the CPU before anything is launched (tests/group_nonfinite.py): the set of
outputs the poison may reach is complete, the CPU loop yields every class of result inside it, the finite sums are exact in any order, the
comparison rule rejects what it must, and the table of kernel forms is well formed."""
import numpy as np
import pytest

import oracle
from group_nonfinite import (CASES, DTYPES, GRAPHS, NCOLS, NP_DTYPES, NROWS, SUBNORMAL_ROWS, WEIGHTS, classes, coalesced, column_blocks, compare,
                             expected, graph, operands, params, rows_of, subnormal)

HS = (3, 64, 100, 264)


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def clean_of(ops):
    return ops._replace(x=ops.x_clean, vals=ops.vals_clean, poisons=[], entries=[])


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("dt", DTYPES)
def test_the_mask_is_complete_and_every_class_occurs(dt, h, weights):
    npdt = NP_DTYPES[dt]
    rowptr, col, ncols = graph("base")
    ops = operands(h, rowptr, ncols, h, npdt, weights, edge_cols=(38, 39))
    want, mask = expected(rowptr, col, ops)
    clean, _ = expected(rowptr, col, clean_of(ops))
    assert np.isfinite(clean).all() and classes(clean)["-0.0"] == 0
    # outside the mask the poisoned product has the clean product's bits: nothing else may change on the GPU either
    assert np.array_equal(bits(want)[~mask], bits(clean)[~mask])
    inside = want[mask]
    k = classes(inside)
    assert k["nan"] > 0 and k["+inf"] > 0 and k["-inf"] > 0 and k["subnormal"] > 0, k
    assert np.isfinite(inside).any(), "no affected element stays finite"
    assert classes(want)["-0.0"] == 0
    assert mask.sum() < mask.size // 4, "the poison reaches too much of the output to show a leak"
    # rows of -0.0 features alone give +0.0, the subnormal rows keep their subnormals, 0 x inf from a stored 0 is NaN
    assert not want[5].any() and not np.signbit(want[5]).any()
    for r in SUBNORMAL_ROWS:
        assert (np.abs(want[r][want[r] != 0]) < np.finfo(npdt).tiny).all() and ((want[r] != 0).any() or weights == "valued")   # (values may cancel)
    if weights == "valued":
        nan2 = np.isnan(want[2])
        assert nan2[0] and nan2[h - 1] and nan2.sum() == len({0, h - 1}), "a stored 0 on an infinite feature must give NaN, there and nowhere else"
        assert ops.vals[ops.entries[0]] == 0 and not np.signbit(ops.vals[ops.entries[0]])


def test_most_rows_do_not_hold_column_zero():
    for name in GRAPHS:
        rowptr, col, _ = graph(name)
        with_zero = np.unique(rows_of(rowptr)[col == 0])
        assert 1 in with_zero and len(with_zero) * 2 <= len(rowptr) - 1, (name, len(with_zero))
    rowptr, col, _ = graph("base")
    assert len(rowptr) - 1 == NROWS and col.max() == NCOLS - 1
    assert len(np.unique(rows_of(rowptr)[col == 0])) < 30


@pytest.mark.parametrize("dt", DTYPES)
def test_no_clean_partial_sum_can_overflow_or_round(dt):
    """max |A| . |x| over the finite terms is far below the first integer a float32 cannot hold: every finite sum is exact in any order"""
    npdt = NP_DTYPES[dt]
    for name in GRAPHS:
        rowptr, col, ncols = graph(name)
        ops = operands(3, rowptr, ncols, 8, npdt, "valued")
        x = np.where(np.isfinite(ops.x), np.abs(ops.x), 0).astype(np.float64)
        v = np.where(np.isfinite(ops.vals), np.abs(ops.vals), 0).astype(np.float64)
        assert oracle.spmm_csr(rowptr, col, v, x).max() < 1e6, name


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_the_cpu_loop_gives_the_same_bits_in_any_order(dt, weights):
    """what lets one rule serve the reordering forms: every row's entries reversed, shuffled, and summed as two halves added afterwards give the
    bits of the stored order (column 65 stays out of the rows that hold integers, tests/group_nonfinite.py)"""
    npdt = NP_DTYPES[dt]
    rng = np.random.default_rng(5)
    rowptr, col, ncols = graph("base")
    ops = operands(9, rowptr, ncols, 64, npdt, weights)
    want, _ = expected(rowptr, col, ops)
    r_of = rows_of(rowptr)
    for perm in (np.lexsort((-np.arange(len(col)), r_of)), np.lexsort((rng.random(len(col)), r_of))):
        v = None if ops.vals is None else ops.vals[perm]
        compare(oracle.spmm_csr(rowptr, col[perm], v, ops.x), want, "permuted rows")
    parts = column_blocks(rowptr, col, ops.vals, [0, 170, 171, ncols])
    halves, _ = expected(rowptr, col, ops, fmt="GROUP", parts=parts)
    compare(halves, want, "column blocks added afterwards")


@pytest.mark.parametrize("weights", WEIGHTS)
def test_the_coalesced_graph_is_the_same_product(weights):
    r, c, n, rp, ncols = coalesced("base")
    assert np.all(np.diff(r.astype(np.int64) * ncols + c) > 0), "COO input must be sorted and free of duplicates"
    ops = operands(7, rp, ncols, 100, np.float32, weights, nnz=len(c), counts=n)
    want, mask = expected(rp, c, ops, fmt="COO")
    compare(oracle.spmm_csr(rp, c, ops.vals, ops.x), want, "COO loop against CSR loop")
    clean, _ = expected(rp, c, clean_of(ops), fmt="COO")
    assert np.array_equal(bits(want)[~mask], bits(clean)[~mask])
    if weights == "unit":   # the counts are the multigraph's weights
        rowptr, col, _ = graph("base")
        compare(oracle.spmm_csr(rowptr, col, None, ops.x), want, "multigraph against its coalesced form")
    deg = np.diff(rp)
    assert deg[0] > 6 * 64 and deg[NROWS - 1] > 6 * 64, "rows 0 and 599 must straddle several chunks of 64 entries"


def test_compare_rejects_what_it_must():
    want = np.array([[np.nan, np.inf, -np.inf, 0.0, 3 * subnormal(np.float32), 5.0]], dtype=np.float32)
    other_nan = want.copy()
    other_nan.view(np.uint32)[0, 0] = 0xFFC00001          # another payload and sign: still a NaN in the same place
    compare(other_nan, want)
    for f, value in ((0, 1.0), (1, np.nan), (1, -np.inf), (2, np.inf), (3, -0.0), (3, subnormal(np.float32)), (4, 0.0), (4, 2 * subnormal(np.float32)),
                     (5, np.nextafter(np.float32(5), np.float32(6)))):
        got = want.copy()
        got[0, f] = value
        with pytest.raises(AssertionError):
            compare(got, want)
    with pytest.raises(AssertionError):
        compare(want.astype(np.float64), want)


def test_the_table_of_forms_is_well_formed():
    from pygim_amd import _lib

    forms = [c.form for c in CASES]
    assert len(forms) == len(set(forms)), "a form is listed twice"
    entries = {"spmm", "spmv", "block2", "device", "parts", "windows", "grande", "pinned", "narrow", "transposed"}
    for c in CASES:
        assert c.proof or c.forced.startswith("forced by knob only"), c.form
        assert set(c.dtypes) <= set(DTYPES) and len(set(c.dtypes)) == len(c.dtypes) >= 1, c.form
        assert set(c.weights) <= set(WEIGHTS) and len(set(c.weights)) == len(c.weights) >= 1, c.form
        assert c.hs and c.entry in entries and (c.graph in GRAPHS or c.graph == "hybrid") and c.fmt in ("CSR", "COO"), c.form
        for query, field, op, value in c.proof:
            assert query in ("info", "plan", "lds_plan", "lds_code", "lds_geometry", "lds_note", "lds_runs", "host_windows") and op in ("==", ">=", "has", "lacks"), c.form
        for name in list(c.knobs) + list(c.create_knobs):     # a misspelt knob would leave the form unforced
            old = _lib.set_tunable(name, 0)
            assert old != -1, (c.form, name)
            _lib.set_tunable(name, old)
    ps, ids = params()
    assert len(ids) == len(set(ids)) and len(ps) >= 100
    text = " ".join(forms)
    for word in ("k_csr_wide", "k_csr_sub", "k_long_segments", "k_coo_wide", "k_csr_vec", "k_spmv_lds", "cooperative", "16-bit", "slice", "misaligned", "strided",
                 "code stream", "token", "ladder", "one-slice", "column-split", "k_lds_tail", "half-split", "hybrid", "column blocks", "feature windows", "host operands",
                 "narrow", "transposed"):
        assert word in text, f"the table lacks a form: {word}"
