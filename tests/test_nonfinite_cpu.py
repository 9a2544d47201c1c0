"""Masked scores on the CPU: the C-ABI doubles (tests/fake_abi.py extended in test_attention_cpu.py, test_gat_fused_cpu.py and
test_sparse_attention_cpu.py) and the per-entry torch references give, for the masked inputs of test_nonfinite_gpu.py on the same
`edges` graph, what the kernels are held to there: a masked entry has probability exactly 0, a partially masked row is the softmax
over the rest (the reference on the graph without the masked entries), a fully masked (row, head) is NaN with lse = -inf, and the
gradients through the wrappers are finite and zero on what is masked."""
import numpy as np
import pytest
import torch

import run_edges
from pygim_amd import pim_ops
from pygim_amd.attention import edge_softmax, gat_aggregate, sparse_attention
from test_attention_cpu import graph_of, ref_softmax
from test_gat_fused_cpu import ref_gat_aggregate
from test_sparse_attention_cpu import FakeLibS, ref_sparse_attention

MASKED = torch.from_numpy(run_edges.MASKED_COLS)
DEAD = list(run_edges.FULLY_MASKED_ROWS)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibS()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    pim_ops._variant = None
    pim_ops._groups.clear()


def masked_edges(fully=True):
    """-> n, m, rowptr, col with the masked entries on the masked nodes, the entry mask, and the graph without those entries"""
    n, m, rowptr, col = run_edges.graph("edges")
    mask = run_edges.masked_entries(rowptr)
    if not fully:
        for r in DEAD:
            mask[rowptr[r]:rowptr[r + 1]] = False
    col_m = run_edges.masked_columns(col, mask)
    return n, m, rowptr, col_m, mask, run_edges.pruned_csr(rowptr, col_m, mask)


def test_the_graph_helpers():
    for name in run_edges.GRAPHS:
        n, m, rowptr, col = run_edges.graph(name)
        assert rowptr[0] == 0 and rowptr[-1] == len(col) and len(rowptr) == n + 1 and 0 <= col.min() and col.max() < m
    n, m, rowptr, col = run_edges.graph("edges")
    mt, nt, rowptr_t, col_t, perm = run_edges.transpose_csr(n, m, rowptr, col)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    assert (mt, nt) == (m, n) and np.array_equal(col[perm], np.repeat(np.arange(m), np.diff(rowptr_t))) and np.array_equal(row[perm], col_t)
    assert (np.diff(perm)[np.diff(col[perm]) == 0] > 0).all(), "a column's entries keep their stored order"
    n, m, rowptr, col_m, mask, (rowptr_p, col_p) = masked_edges()
    assert mask.sum() == len(col_m) - len(col_p) and not np.isin(col_p, run_edges.MASKED_COLS).any()
    assert tuple(np.flatnonzero((np.diff(rowptr) > 0) & (np.diff(rowptr_p) == 0))) == run_edges.FULLY_MASKED_ROWS


@pytest.mark.parametrize("heads", [1, 3, 4])
def test_edge_softmax_double_and_reference(fake, heads):
    n, m, rowptr, col_m, mask, (rowptr_p, _) = masked_edges()
    g = graph_of(rowptr, col_m, n, m)
    row = g.row.long()
    mk = torch.from_numpy(mask)
    torch.manual_seed(11)
    base = torch.randn(len(col_m), heads, dtype=torch.float64) * 3
    for which in ("all heads", "head 0"):
        s = base.clone()
        if which == "all heads":
            s[mk] = -float("inf")
        else:
            s[mk, 0] = -float("inf")
        P = edge_softmax(g, s)
        ref = ref_softmax(rowptr, s, n)
        dead = torch.zeros(n, heads, dtype=torch.bool)
        dead[DEAD] = True if which == "all heads" else torch.tensor([True] + [False] * (heads - 1))
        assert torch.equal(torch.isnan(P), dead[row]) and torch.equal(torch.isnan(ref), dead[row])
        live = ~dead[row]
        assert (P[torch.isinf(s) & live] == 0).all()
        assert torch.allclose(P[live], ref[live], rtol=1e-12, atol=1e-300)
        # the rest of a partially masked row: the softmax on the graph without the masked entries
        keep = ~mk
        want = ref_softmax(rowptr_p, base[keep], n)
        cols = slice(None) if which == "all heads" else slice(0, 1)
        sub = live[keep][:, cols]
        assert torch.allclose(P[keep][:, cols][sub], want[:, cols][sub], rtol=1e-12, atol=1e-300)
    assert "edge_softmax" in fake.calls


def test_gat_aggregate_double_reference_and_gradients(fake):
    heads, h = 4, 8
    torch.manual_seed(12)
    # fully masked rows 13 and 19: NaN and lse = -inf from the double, NaN from the reference; the other rows as on the pruned graph
    n, m, rowptr, col_m, mask, (rowptr_p, col_p) = masked_edges()
    a_dst, a_fin, X = (torch.randn(r, w, dtype=torch.float64) for r, w in ((n, heads), (m, heads), (m, h)))
    for masked_heads in ([True] * heads, [True] + [False] * (heads - 1)):
        a_src = a_fin.clone()
        a_src[MASKED.unsqueeze(1), torch.tensor(masked_heads).nonzero().squeeze(1)] = -float("inf")
        out = torch.full((n, h), 7.0, dtype=torch.float64)
        lse = torch.full((n, heads), 7.0, dtype=torch.float64)
        rp, cc = torch.from_numpy(rowptr), torch.from_numpy(col_m)
        fake.gat_aggregate(fake.DBL64, n, rp.data_ptr(), cc.data_ptr(), len(col_m), a_dst.data_ptr(), a_src.data_ptr(), heads, 0.2, X.data_ptr(), h, h,
                           out.data_ptr(), h, lse.data_ptr(), 0, 96)
        ref = ref_gat_aggregate(rowptr, col_m, a_dst, a_src, X, 0.2, n)
        pick = torch.tensor(masked_heads)
        dead = torch.zeros(n, heads, dtype=torch.bool)
        dead[DEAD] = pick
        dead_f = dead.repeat_interleave(h // heads, dim=1)
        assert torch.equal(torch.isnan(out), dead_f) and torch.equal(torch.isnan(ref), dead_f)
        assert torch.equal(torch.isneginf(lse), dead) and torch.isfinite(lse[~dead]).all()
        assert torch.allclose(out[~dead_f], ref[~dead_f], rtol=1e-12, atol=1e-12)
        want = torch.where(pick.repeat_interleave(h // heads), ref_gat_aggregate(rowptr_p, col_p, a_dst, a_fin, X, 0.2, n),
                           ref_gat_aggregate(rowptr, col_m, a_dst, a_fin, X, 0.2, n))
        assert torch.allclose(out[~dead_f], want[~dead_f], rtol=1e-11, atol=1e-12)
        empty = torch.from_numpy(np.diff(rowptr) == 0)
        assert (out[empty] == 0).all() and (lse[empty] == 0).all()
    # no fully masked row: forward and gradients through the wrapper against autograd of the reference
    n, m, rowptr, col_m, mask, _ = masked_edges(fully=False)
    g = graph_of(rowptr, col_m, n, m)
    a_src = a_fin.clone()
    a_src[MASKED] = -float("inf")
    G = torch.randn(n, h, dtype=torch.float64)
    ours = [t.clone().requires_grad_() for t in (a_dst, a_src, X)]
    theirs = [t.clone().requires_grad_() for t in (a_dst, a_src, X)]
    out = gat_aggregate(g, *ours, 0.2)
    ref = ref_gat_aggregate(rowptr, col_m, *theirs, 0.2, n)
    assert torch.isfinite(out).all() and torch.allclose(out, ref, rtol=1e-12, atol=1e-12)
    out.backward(G)
    ref.backward(G)
    for name, a, b in zip(("a_dst", "a_src", "X"), ours, theirs):
        assert torch.isfinite(a.grad).all() and torch.allclose(a.grad, b.grad, rtol=1e-9, atol=1e-11), name
    assert (ours[1].grad[MASKED] == 0).all() and (ours[2].grad[MASKED] == 0).all()
    # the unfused composition of GATConv(fused=False) and the probabilities' own gradient
    row, col = g.row.long(), g.col.long()
    score = torch.nn.functional.leaky_relu(a_dst[row] + a_src[col], 0.2).requires_grad_()
    P = edge_softmax(g, score)
    P.backward(torch.randn_like(P))
    mk = torch.from_numpy(mask)
    assert torch.isfinite(P).all() and (P[mk] == 0).all() and torch.isfinite(score.grad).all() and (score.grad[mk] == 0).all()


@pytest.mark.parametrize("h,heads", [(8, 4), (6, 1)])
def test_sparse_attention_double_and_reference(fake, h, heads):
    n, m, rowptr, col_m, mask, (rowptr_p, col_p) = masked_edges()
    hd = h // heads
    torch.manual_seed(13)
    Q = torch.rand(n, h, dtype=torch.float64) * 1.5 + 0.5
    K_fin, V = torch.randn(m, h, dtype=torch.float64), torch.randn(m, h, dtype=torch.float64)
    K = K_fin.clone()
    K[MASKED] = -float("inf")
    out = torch.full((n, h), 7.0, dtype=torch.float64)
    lse = torch.full((n, heads), 7.0, dtype=torch.float64)
    rp, cc = torch.from_numpy(rowptr), torch.from_numpy(col_m)
    fake.sparse_attention(fake.DBL64, n, rp.data_ptr(), cc.data_ptr(), len(col_m), Q.data_ptr(), h, K.data_ptr(), h, V.data_ptr(), h, h, heads, hd ** -0.5,
                          out.data_ptr(), h, lse.data_ptr(), 0, 112)
    ref = ref_sparse_attention(rowptr, col_m, Q, K, V, heads, n)
    dead = torch.zeros(n, dtype=torch.bool)
    dead[DEAD] = True
    assert torch.equal(torch.isnan(out), dead.unsqueeze(1).expand(n, h)) and torch.equal(torch.isnan(ref), torch.isnan(out))
    assert torch.equal(torch.isneginf(lse), dead.unsqueeze(1).expand(n, heads)) and torch.isfinite(lse[~dead]).all()
    want = ref_sparse_attention(rowptr_p, col_p, Q, K_fin, V, heads, n)
    assert torch.allclose(out[~dead], ref[~dead], rtol=1e-12, atol=1e-12) and torch.allclose(out[~dead], want[~dead], rtol=1e-11, atol=1e-12)
    # through the wrapper, no fully masked row: finite, and the masked keys and values get no gradient
    n, m, rowptr, col_m, mask, _ = masked_edges(fully=False)
    g = graph_of(rowptr, col_m, n, m)
    ours = [t.clone().requires_grad_() for t in (Q, K, V)]
    theirs = [t.clone().requires_grad_() for t in (Q, K, V)]
    o = sparse_attention(g, *ours, heads=heads)
    r = ref_sparse_attention(rowptr, col_m, *theirs, heads, n)
    assert torch.isfinite(o).all() and torch.allclose(o, r, rtol=1e-12, atol=1e-12)
    G = torch.randn(n, h, dtype=torch.float64)
    o.backward(G)
    assert torch.isfinite(ours[2].grad).all() and (ours[2].grad[MASKED] == 0).all()
