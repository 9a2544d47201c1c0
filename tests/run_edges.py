"""Hand-built graphs for the entry-run walker (row_gather_dev.hpp and its four siblings: 512 entries per run, two slots per run, a
fix-up over the runs) and the masked entries of the non-finite tests; shared by test_run_edges_gpu.py, test_nonfinite_gpu.py and
test_nonfinite_cpu.py.  Host only: numpy in, numpy out."""
import numpy as np

RUN = 512          # RG_EPW: entries per run of the gather kernels
NCOLS = 97
EDGES_DEG = [0, 0, 0, 512, 0, 1024, 511, 2, 300, 700, 351, 1300, 0, 1, 63, 64, 65, 0, 0, 7, 128, 72, 21, 0, 0]


def csr_of(deg, ncols, seed):
    """columns drawn with a fixed seed and sorted per row, as conftest.random_csr does"""
    r = np.random.default_rng(seed)
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = r.integers(0, ncols, size=int(rowptr[-1]), dtype=np.int64)
    for i in range(len(deg)):
        col[rowptr[i]:rowptr[i + 1]].sort()
    return rowptr.astype(np.int32), col.astype(np.int32)


def run_of(e):
    return int(e) // RUN


def edges_graph():
    """25 rows, 97 columns, nnz = 10 * 512 + 1; every assertion names the walker case the graph exists for"""
    n, m = len(EDGES_DEG), NCOLS
    rowptr, col = csr_of(EDGES_DEG, m, 41)
    rp = rowptr.astype(np.int64)
    nnz = len(col)
    deg = np.diff(rp)
    assert nnz == 5121 and nnz % RUN == 1 and nnz % 64 == 1 and nnz % 256 == 1 and nnz % 1024 == 1
    assert (nnz + RUN - 1) // RUN == 11, "11 runs: the fix-up launches 3 blocks of 4 waves"
    assert (deg[:3] == 0).all() and (deg[-2:] == 0).all(), "three leading empty rows, two trailing ones"
    assert (rp[3], rp[4]) == (0, RUN), "row 3 is exactly run 0"
    assert deg[4] == 0 and rp[4] == RUN, "an empty row sits on the boundary 512"
    assert rp[5] == RUN and rp[6] - 1 == 3 * RUN - 1, "row 5 starts on a run boundary, is cut, and ends on a run's last entry: run 3 starts clean"
    assert (rp[7], rp[8] - 1) == (4 * RUN - 1, 4 * RUN), "row 7: one entry on each side of the boundary 2048"
    assert rp[10] < 6 * RUN < rp[11] < 7 * RUN < rp[12], "run 6 is the tail of row 10 and the head of row 11, nothing complete between them"
    assert run_of(rp[11]) == 6 and run_of(rp[12] - 1) == 9 and rp[12] - 1 < 10 * RUN - 1, "row 11: from inside run 6 to inside run 9, runs 7 and 8 whole"
    assert np.flatnonzero(deg)[-1] == 22 and rp[23] == nnz and rp[22] < 10 * RUN == nnz - 1, \
        "row 22, the last non-empty one, is cut: its last entry 5120 is alone in run 10, and only empty rows follow"
    row = np.repeat(np.arange(n), deg)
    assert len(np.unique(col)) == m and ((col[1:] == col[:-1]) & (row[1:] == row[:-1])).any(), "every column is used, with duplicates"
    return n, m, rowptr, col


def one_row_graph():
    """nrows == 1: one row over four runs, the last run with a single entry"""
    rowptr, col = csr_of([3 * RUN + 1], NCOLS, 42)
    assert len(col) == 1537 and (len(col) + RUN - 1) // RUN == 4 and len(col) % RUN == 1
    return 1, NCOLS, rowptr, col


def whole_batches_graph():
    """eight rows of 64: nnz == 512, a single run (no fix-up launch), every row exactly one 64-entry batch"""
    rowptr, col = csr_of([64] * 8, NCOLS, 43)
    assert len(col) == RUN and (rowptr % 64 == 0).all()
    return 8, NCOLS, rowptr, col


def transpose_csr(n, m, rowptr, col):
    """the CSR of A^T (stable: a column's entries keep their stored order), built with numpy -> (m, n, rowptr_t, col_t, perm) with
    perm[j] the entry of A that entry j of A^T is"""
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    perm = np.argsort(col, kind="stable")
    rowptr_t = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=m), out=rowptr_t[1:])
    return m, n, rowptr_t.astype(np.int32), row[perm].astype(np.int32), perm


def edges_transposed_graph():
    """97 rows of about 53 entries whose columns are the rows of `edges`: the backward kernels get the edge structure on the gathered side"""
    mt, nt, rowptr_t, col_t, _ = transpose_csr(*edges_graph())
    return mt, nt, rowptr_t, col_t


GRAPHS = {"edges": edges_graph, "edges-T": edges_transposed_graph, "one-row": one_row_graph, "whole-batches": whole_batches_graph}
_cache = {}


def graph(name):
    """(n, m, rowptr, col), built once; fresh copies of the arrays, so a test may write to them"""
    if name not in _cache:
        _cache[name] = GRAPHS[name]()
    n, m, rowptr, col = _cache[name]
    return n, m, rowptr.copy(), col.copy()


FULLY_MASKED_ROWS = (13, 19)


def masked_entries(rowptr):
    """the masked entries of `edges` as a bool array over the entries"""
    rp = rowptr.astype(np.int64)
    deg = np.diff(rp)
    mask = np.zeros(int(rp[-1]), dtype=bool)
    mask[rp[:-1][deg >= 2]] = True                   # the first entry of every row with at least two entries
    mask[7 * RUN:8 * RUN] = True                     # a whole middle run of row 11
    mask[RUN:2 * RUN] = True                         # the first run of row 5
    mask[rp[9]:rp[9] + 64] = True                    # the first 64 entries of row 9: whole lane groups, a whole batch of the walk
    mask[10 * RUN] = True                            # entry 5120: the single entry of the last run
    for r in FULLY_MASKED_ROWS:
        mask[rp[r]:rp[r + 1]] = True
    assert rp[11] < 7 * RUN and 8 * RUN < rp[12] and (rp[5], rp[6]) == (RUN, 3 * RUN)
    row = np.repeat(np.arange(len(deg)), deg)
    left = np.bincount(row[~mask], minlength=len(deg))
    assert tuple(np.flatnonzero((deg > 0) & (left == 0))) == FULLY_MASKED_ROWS, "rows 13 and 19 are the only fully masked ones"
    return mask


MASKED_COLS = np.array([3, 40, 41, 77, 96])


def masked_columns(col, mask):
    """a copy of col in which exactly the masked entries point at MASKED_COLS (stored order is the contract: the columns of a row need
    not stay sorted)"""
    out = col.copy()
    hit = np.isin(out, MASKED_COLS) & ~mask
    out[hit] += 1                                    # 4, 41 -> 42 (see below), 78, 97 -> wrapped
    out[hit & (out == 41)] = 42
    out[hit & (out >= NCOLS)] = 0
    out[mask] = MASKED_COLS[np.arange(int(mask.sum())) % len(MASKED_COLS)]
    assert np.array_equal(np.isin(out, MASKED_COLS), mask)
    return out


def pruned_csr(rowptr, col, mask):
    """the graph without the masked entries: a masked entry has probability exactly 0, so the softmax over the rest is the reference of
    every partially masked row (the fully masked rows are empty here)"""
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row[~mask], minlength=n), out=rp[1:])
    return rp.astype(np.int32), np.ascontiguousarray(col[~mask])
