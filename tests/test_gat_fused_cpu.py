"""The fused GAT aggregation on CPU: pygim_amd.gat_aggregate and gnn.GATConv(fused=True) driven with the C-ABI test double of
test_attention_cpu.py, extended here with numpy float64 statements of pygim_gat_aggregate and pygim_gat_aggregate_workspace."""
import numpy as np
import pytest
import torch

import pygim_amd
from fake_abi import NP_OF, _view
from pygim_amd import gnn, pim_ops
from pygim_amd.attention import gat_aggregate
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import FakeLibA, _rows, gat_reference, graph_of, multigraph, softmax_shift
from conftest import random_csr


class FakeLibG(FakeLibA):
    """FakeLibA with the two entry points of the fused aggregation"""

    def gat_aggregate_workspace(self, dtype, nrows, nnz, h, heads):
        return 96

    def gat_aggregate(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr, ldo, lse_ptr,
                      ws_ptr, ws_bytes, stream=0):
        self.calls.append("gat_aggregate")
        assert h % heads == 0 and ws_bytes >= 96
        npdt = NP_OF[dtype]
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        out = _rows(out_ptr, nrows, ldo, h, npdt)
        acc = np.zeros((nrows, h))
        lse = np.zeros((nrows, heads))
        if nnz:
            row = np.repeat(np.arange(nrows), np.diff(rowptr))
            ncols = int(col.max()) + 1
            a_dst = _view(a_dst_ptr, nrows * heads, npdt).reshape(nrows, heads).astype(np.float64)
            a_src = _view(a_src_ptr, ncols * heads, npdt).reshape(ncols, heads).astype(np.float64)
            X = _rows(x_ptr, ncols, ldx, h, npdt).astype(np.float64)
            z = a_dst[row] + a_src[col]
            s = np.where(z >= 0, z, negative_slope * z)
            m = np.full((nrows, heads), -np.inf)
            np.maximum.at(m, row, s)
            e = np.exp(s - softmax_shift(m)[row])
            l = np.zeros((nrows, heads))
            np.add.at(l, row, e)
            full = np.diff(rowptr) > 0
            with np.errstate(invalid="ignore", divide="ignore"):   # a fully masked row: 0 / 0 = NaN, lse = -inf + log(0) = -inf
                np.add.at(acc, row, np.repeat(e / l[row], h // heads, axis=1) * X[col])
                lse[full] = m[full] + np.log(l[full])
        out[:] = acc.astype(npdt)
        if lse_ptr:
            _view(lse_ptr, nrows * heads, npdt).reshape(nrows, heads)[:] = lse.astype(npdt)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibG()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    pim_ops._variant = None
    pim_ops._groups.clear()


def ref_gat_aggregate(rowptr, col, a_dst, a_src, X, slope, n):
    """per-entry reference in plain torch (differentiable)"""
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    heads = a_src.size(1)
    s = torch.nn.functional.leaky_relu(a_dst[row] + a_src[cc], slope)
    m = torch.full((n, heads), -float("inf"), dtype=X.dtype).index_reduce_(0, row, s.detach(), "amax", include_self=True)
    e = torch.exp(s - m[row])
    p = e / torch.zeros(n, heads, dtype=X.dtype).index_add(0, row, e)[row]
    return torch.zeros(n, X.size(1), dtype=X.dtype).index_add(0, row, p.repeat_interleave(X.size(1) // heads, dim=1) * X[cc])


def test_public_name():
    assert pygim_amd.gat_aggregate is gat_aggregate


@pytest.mark.parametrize("heads", [1, 3])
def test_forward_and_gradients_match_the_per_entry_reference(rng, fake, heads):
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    a_dst = (torch.randn(n, heads, dtype=torch.float64) * 2).requires_grad_()
    a_src = (torch.randn(m, heads, dtype=torch.float64) * 2).requires_grad_()
    X = torch.randn(m, h, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, h, dtype=torch.float64)
    if heads == 1:   # 1-D node terms mean one head
        out = gat_aggregate(g, a_dst[:, 0], a_src[:, 0], X, 0.3)
    else:
        out = gat_aggregate(g, a_dst, a_src, X, 0.3)
    want = ref_gat_aggregate(rowptr, col, a_dst, a_src, X, 0.3, n)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert (out[np.diff(rowptr) == 0] == 0).all()
    out.backward(G)
    got = [t.grad.clone() for t in (a_dst, a_src, X)]
    for t in (a_dst, a_src, X):
        t.grad = None
    want.backward(G)
    for a, t in zip(got, (a_dst, a_src, X)):
        assert torch.allclose(a, t.grad, rtol=1e-9, atol=1e-11)
    assert torch.autograd.gradcheck(lambda a, b, c: gat_aggregate(g, a, b, c, 0.3), (a_dst, a_src, X))
    assert "edge_softmax" not in fake.calls and "gat_aggregate" in fake.calls


def test_lse_is_requested_only_when_a_gradient_is_needed(rng, fake, monkeypatch):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    asked = []
    inner = fake.gat_aggregate

    def spy(*a, **k):
        asked.append(bool(a[14]))   # lse_ptr
        return inner(*a, **k)

    monkeypatch.setattr(fake, "gat_aggregate", spy)
    a_dst, a_src, X = torch.randn(n, 2), torch.randn(m, 2), torch.randn(m, 4)
    gat_aggregate(g, a_dst, a_src, X)
    gat_aggregate(g, a_dst, a_src, X.clone().requires_grad_())
    assert asked == [False, True]


@pytest.mark.parametrize("heads,concat", [(1, True), (3, True), (2, False)])
def test_fused_gatconv_matches_per_entry_reference(rng, fake, heads, concat):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(3)
    conv = gnn.GATConv(7, 4, heads=heads, concat=concat, fused=True).double()
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 7, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, 4 * heads if concat else 4, dtype=torch.float64)
    out = conv(x, adj)
    assert out.shape == G.shape
    assert fake.calls == ["gat_aggregate"], "the fused forward is one call: no edge_softmax, no spmm_values"
    out.backward(G)
    got = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    want_out = gat_reference(conv, x, rowptr, col, n)
    want_out.backward(G)
    want = [x.grad] + [p.grad for p in conv.parameters()]
    assert torch.allclose(out, want_out, rtol=1e-10, atol=1e-12)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    assert "edge_softmax" not in fake.calls and "edge_softmax_backward" not in fake.calls


def test_the_default_layer_is_the_unfused_one(rng, fake):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    conv = gnn.GATConv(7, 4, heads=2).double()
    assert conv.fused is False
    conv(torch.randn(n, 7, dtype=torch.float64), adj)
    assert fake.calls == ["edge_softmax", "spmm_values"]
    model = gnn.GAT(5, 8, 3, num_layers=2, dropout=0.0, heads=2, fused=True)
    assert all(c.fused for c in model.convs) and not any(c.fused for c in gnn.GAT(5, 8, 3, heads=2).convs)


def test_nothing_of_size_nnz_is_saved_for_the_backward(rng, fake):
    """a multigraph with more entries than any node-sized tensor has elements: the fused forward saves none of that size, the
    unfused one does (scores, probabilities, gathered node terms)"""
    n, heads, fo = 12, 2, 3
    h = heads * fo
    rowptr, col = random_csr(rng, n, n, 90, empty_frac=0.1)
    nnz = len(col)
    assert nnz > n * max(h, 7)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    x = torch.randn(n, 7, dtype=torch.float64, requires_grad=True)

    def largest_saved(fused):
        torch.manual_seed(1)
        conv = gnn.GATConv(7, fo, heads=heads, fused=fused).double()
        sizes = []

        def pack(t):
            sizes.append(t.numel())
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = conv(x, adj)
        out.sum().backward()
        return max(sizes)

    assert largest_saved(True) < nnz
    assert largest_saved(False) >= nnz


def test_argument_validation(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    a_dst, a_src, X = torch.randn(n, 2, dtype=torch.float64), torch.randn(m, 2, dtype=torch.float64), torch.randn(m, 6, dtype=torch.float64)
    with pytest.raises(TypeError):
        gat_aggregate(g, a_dst.float(), a_src, X)              # dtype mismatch
    with pytest.raises(TypeError):
        gat_aggregate(g, a_dst.int(), a_src.int(), X.int())    # not a float type
    with pytest.raises(ValueError):
        gat_aggregate(g, a_dst[:-1], a_src, X)                 # a_dst does not cover the rows
    with pytest.raises(ValueError):
        gat_aggregate(g, a_dst, a_src[:-1], X)                 # a_src does not cover the columns
    with pytest.raises(ValueError):
        gat_aggregate(g, a_dst, a_src[:, :1], X)               # heads differ
    with pytest.raises(ValueError):
        gat_aggregate(g, a_dst[:, 0], a_src, X)                # one 1-D, one 2-D
    with pytest.raises(ValueError):
        gat_aggregate(g, a_dst, a_src, X[:-1])                 # X does not cover the columns
    with pytest.raises(ValueError):
        gat_aggregate(g, torch.randn(n, 4, dtype=torch.float64), torch.randn(m, 4, dtype=torch.float64), X)   # 6 % 4 != 0
    assert fake.calls == []
