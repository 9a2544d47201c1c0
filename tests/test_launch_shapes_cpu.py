"""tests/launch_shapes.py is complete and has no redundant case, proven from pygim_gather_launch_shape alone (no device): the query is
swept over the domain of every family, every answer is reduced to its class, and the family's table has to hit every reachable class and
every storage type under every kind of misalignment, with no case that could be removed.  Also here: the query against the limits of
the entry points, and the sharpness of the bounds the deep GPU cases of test_launch_shapes_gpu.py rely on, from the float64 reference
alone."""
import numpy as np
import pytest
import torch

import launch_shapes as ls
from pygim_amd import _lib

FAMILY_NAMES = list(ls.FAMILIES)


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_every_case_states_the_shape_the_launcher_picks(family):
    """what a docstring could only claim: the stated shape of a case is what the launch function computes for it, for every entry point
    that shares the family's table"""
    assert ls.TABLES[family], family
    for case in ls.TABLES[family]:
        assert case.dtype in ls.FAMILIES[family]["dtypes"] and case.mis in ls.FAMILIES[family]["mis"], case
        for kind in ls.FAMILIES[family]["kinds"]:
            shape = ls.query(family, case.h, case.heads, case.dtype, case.mis is None, kind)
            assert tuple(shape[k] for k in _lib.SHAPE_FIELDS) == case.shape, (case, shape)
        assert case.why == ls.describe(dict(zip(_lib.SHAPE_FIELDS, case.shape))), case


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_table_covers_every_reachable_class_and_no_case_is_redundant(family):
    need = ls.requirements(family)
    classes = [r for r in need if r[0] == "class"]
    covered = [ls.satisfies(family, case) for case in ls.TABLES[family]]
    missing = need - set().union(*covered)
    print(f"{family}: {len(classes)} reachable classes, {len(need) - len(classes)} (type, misalignment) pairs, {len(covered)} cases")
    assert not missing, f"{family}: no case for {sorted(missing, key=str)}"
    assert len(set(ls.TABLES[family])) == len(ls.TABLES[family]), "a case is listed twice"
    for i, case in enumerate(ls.TABLES[family]):
        others = set().union(*(covered[:i] + covered[i + 1:]))
        assert covered[i] - others, f"{family}: {case} covers nothing the other cases do not cover: it does not belong in the table"


def test_the_kinds_of_a_family_share_their_shape_function():
    """one table serves spmm_values and gat_aggregate, and one sparse_attention and both GATv2 entry points"""
    for family in ("walker", "head"):
        kinds = ls.FAMILIES[family]["kinds"]
        for h, heads in ls.domain(family)[::7] + ls.domain(family)[-1:]:
            for dtype in ("f32", "bf16"):
                for aligned in (True, False):
                    first = ls.query(family, h, heads, dtype, aligned, kinds[0])
                    assert all(ls.query(family, h, heads, dtype, aligned, k) == first for k in kinds[1:])


def test_the_classes_named_in_the_kernels_comments_are_reachable():
    """spot checks of the class definition against the launch code, read by hand"""
    q = ls.query
    s = q("head", 99, 1, "f32", True)       # hd = 99: scalar, two pieces per lane, the second one on lanes 0 .. 34 only
    assert (s["vec"], s["pieces"], s["LH"], s["L"], s["per"]) == (1, 2, 64, 64, 1) and s["flags"] & _lib.SHAPE_PART_PIECE
    s = q("head", 75, 3, "f32", True)       # hd = 25, three heads: 32 lanes per head, two heads per block, the last block holds one
    assert (s["LH"], s["L"], s["per"], s["chunks"]) == (32, 64, 2, 2) and s["flags"] & _lib.SHAPE_PART_CHUNK and s["flags"] & _lib.SHAPE_PART_HEADS
    s = q("head", 130, 130, "f32", True)    # hd = 1: 64 heads per block, three chunks, the last one with two heads
    assert (s["LH"], s["L"], s["per"], s["chunks"]) == (1, 64, 64, 3) and s["flags"] & _lib.SHAPE_PART_CHUNK
    s = q("head", *ls.TWO_LAUNCHES, "f32", True)
    assert (s["vec"], s["per"], s["chunks"], s["launches"]) == (1, 1, 65537, 2)
    s = q("walker", 520, 1, "f32", True)    # 130 pieces of 16 bytes: two per lane, two chunks, the second one with two pieces
    assert (s["vec"], s["pieces"], s["L"], s["chunks"]) == (4, 2, 64, 2) and s["flags"] & _lib.SHAPE_PART_CHUNK
    s = q("sddmm", 8, 1, "f32", True)
    assert (s["vec"], s["L"]) == (4, 2)
    s = q("edge_softmax", 8, 8, "f32", False)
    assert s["vec"] == 1 and s["flags"] == _lib.SHAPE_SCALAR_ALIGN and s["chunks"] == 8
    assert q("edge_softmax", 3, 3, "f32", True)["flags"] == _lib.SHAPE_SCALAR_SIZE


def test_widths_one_launch_cannot_hold_are_rejected_by_the_query_and_the_workspace_functions():
    """the row walkers put ceil(pieces / 128) into gridDim.y: a row of more than 65535 * 128 features is rejected, by the workspace
    functions (-1) as by the entry points (tested with a device in test_launch_shapes_gpu.py), and the query reports the same limit"""
    top = _lib.GATHER_MAX_H
    assert top == 65535 * 128
    for kind in (_lib.SHAPE_SPMM_VALUES, _lib.SHAPE_SPMM_REDUCE, _lib.SHAPE_GAT_AGGREGATE, _lib.SHAPE_SPMM_REDUCE_BACKWARD):
        for aligned in (True, False):
            assert _lib.gather_launch_shape(kind, _lib.FLT32, top, 1, aligned)["chunks"] == (65535 if not aligned else 16384)
            with pytest.raises(_lib.PygimError):
                _lib.gather_launch_shape(kind, _lib.FLT32, top + 1, 1, aligned)
    assert _lib.spmm_values_workspace(_lib.FLT32, 1, 1, top, 1) > 0 and _lib.gat_aggregate_workspace(_lib.FLT32, 1, 1, top, 1) > 0
    assert _lib.spmm_reduce_workspace(_lib.FLT32, _lib.REDUCE_MAX, 1, 1, top) > 0
    for call in (lambda: _lib.spmm_values_workspace(_lib.FLT32, 1, 1, top + 1, 1), lambda: _lib.gat_aggregate_workspace(_lib.FLT32, 1, 1, top + 1, 1),
                 lambda: _lib.spmm_reduce_workspace(_lib.FLT32, _lib.REDUCE_MAX, 1, 1, top + 1),
                 lambda: _lib.spmm_reduce_workspace(_lib.BF16, _lib.REDUCE_MEAN, 1, 1, top + 1)):
        with pytest.raises(_lib.PygimError):
            call()
    # the head-wise kernels loop over launches instead: no such limit
    assert _lib.gather_launch_shape(_lib.SHAPE_SPARSE_ATTENTION, _lib.FLT32, 65536 * 256, 65536, True)["launches"] == 2


def test_the_query_rejects_what_the_entry_points_reject():
    for kind, dtype, h, heads in ((99, _lib.FLT32, 8, 1), (_lib.SHAPE_SPMM_VALUES, _lib.INT32, 8, 1), (_lib.SHAPE_SPMM_REDUCE_BACKWARD, _lib.BF16, 8, 1),
                                 (_lib.SHAPE_EDGE_SOFTMAX, _lib.FLT16, 8, 8), (_lib.SHAPE_SPARSE_ATTENTION, _lib.FLT32, 257, 1),
                                 (_lib.SHAPE_GATV2_BACKWARD, _lib.FLT32, 9, 2), (_lib.SHAPE_SDDMM, _lib.FLT32, 0, 1), (_lib.SHAPE_GAT_AGGREGATE, _lib.FLT32, 8, 0)):
        with pytest.raises(_lib.PygimError):
            _lib.gather_launch_shape(kind, dtype, h, heads, True)
    assert _lib.gather_launch_shape(_lib.SHAPE_SPMM_REDUCE, _lib.INT8, 32, 1, True)["vec"] == 16


# ---- the deep GPU cases can fail: shown on the float64 reference alone ----
@pytest.mark.parametrize("runs,h,heads", ls.DATT_CASES)
def test_a_datt_without_any_one_run_violates_the_bound(runs, h, heads):
    """what a dropped partial, a wrong buffer or a lost ragged block of k_gatv2_datt_reduce would return is the reference without the
    part of one or more runs: for every run of every graph, leaving its part out moves some feature of datt by more than
    test_gatv2_backward_parity's bound (GRAD_TOL, the one test_gatv2_datt_reduction_depth asserts) allows"""
    import test_gatv2_gpu as t_v2

    for dtype in (torch.float32, torch.float64):
        if runs == 65537 and dtype == torch.float32:
            continue   # not run on the GPU either (see test_gatv2_datt_reduction_depth)
        n, m, rowptr, col = ls.datt_graph(runs)
        Xd, Xs, G, att = ls.datt_operands(runs, h, heads, dtype)
        ref, _, _, parts = ls.datt_reference(rowptr, col, Xd, Xs, att, G, h, heads, slope=t_v2.SLOPE, per_run=True)
        assert parts.shape == (runs, h) and torch.allclose(parts.sum(0), ref, rtol=1e-12, atol=0)
        tol = t_v2.GRAD_TOL[dtype]
        bound = tol["atol"] + tol["rtol"] * ref.abs()
        margin = (parts.abs() / bound).max(1).values   # per run: its largest part of a feature, in units of the bound
        print(f"datt runs={runs} {dtype}: |ref| = {ref.abs().min().item():.3e} .. {ref.abs().max().item():.3e}, the smallest run moves datt by "
              f"{margin.min().item():.3e} bounds (run {margin.argmin().item()})")
        assert (margin > 1).all(), f"run {margin.argmin().item()} could be lost unnoticed"


def _head_slice_reference(kind, rowptr, col, A, B, V, att, hd, scale):
    """float64 out, sum_e p |v| and Delta of one head-wise forward on a handful of entries: sparse attention (kind 'sa': A = Q, B = K)
    or GATv2 (kind 'gatv2': A = x_dst, B = V = x_src), as include/pygim_hip.h states them; [rows, heads * hd] operands"""
    n = len(rowptr) - 1
    heads = A.shape[1] // hd
    out, mag, delta = (np.zeros((n, A.shape[1])) for _ in range(3))
    for r in range(n):
        es = col[rowptr[r]:rowptr[r + 1]]
        if len(es) == 0:
            continue
        if kind == "sa":
            terms = scale * A[r][None, :] * B[es]
        else:
            z = A[r][None, :] + B[es]
            terms = att[None, :] * np.where(z > 0, z, ls.SLOPE * z)
        s = terms.reshape(len(es), heads, hd).sum(-1)
        d = np.abs(terms).reshape(len(es), heads, hd).sum(-1).max(0)
        p = np.exp(s - s.max(0))
        p = np.repeat(p / p.sum(0), hd, axis=1)
        out[r], mag[r], delta[r] = (p * V[es]).sum(0), (p * np.abs(V[es])).sum(0), np.repeat(d, hd)
    return out, mag, delta


def test_an_out_without_the_second_launch_violates_the_bound():
    """the 65 537-head case: a result whose heads 65535 and 65536 (the second launch) were never computed is the reference with those
    heads zero, and that violates out's bound (2 EPS + 2 Delta) sum_e p |v| of the sparse-attention and GATv2 files, EPS = 1e-5, in
    every non-empty row.  Heads are independent, so the reference of the last two heads is computed on their 66 features alone"""
    h, heads = ls.TWO_LAUNCHES
    hd = h // heads
    assert ls.query("head", h, heads, "f32", True)["launches"] == 2 and 65535 * 1 == heads - 2
    n, m, rowptr, col = ls.two_launch_graph()
    Q, K, V, att = (t.astype(np.float64)[..., 65535 * hd:] for t in ls.two_launch_operands())
    for kind, values in (("sa", V), ("gatv2", K)):
        ref, mag, delta = _head_slice_reference(kind, rowptr, col, Q, K, values, att, hd, hd ** -0.5)
        bound = (2e-5 + 2 * 1e-5 * delta) * mag
        rows_with_entries = np.diff(rowptr) > 0
        print(f"{kind}: |ref| / bound over the second launch's features: min {np.min(np.abs(ref[rows_with_entries]) / bound[rows_with_entries]):.3e}")
        assert (np.abs(ref) > bound)[rows_with_entries].any(axis=1).all()
