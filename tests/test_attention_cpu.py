"""Per-call edge values on CPU: pygim_amd.attention (EdgeGraph, spmm_values, edge_softmax), SparseGroupBase.mul_values and gnn.GATConv
driven with the C-ABI test double of tests/fake_abi.py, extended here with numpy float64 statements of pygim_spmm_values,
pygim_edge_softmax, pygim_edge_softmax_backward (and a stride-aware pygim_sddmm)."""
import types

import numpy as np
import pytest
import torch

import pygim_amd
from conftest import random_csr
from fake_abi import NP_OF, FakeLib, PygimError, _view
from pygim_amd import attention, gnn, pim_ops
from pygim_amd.attention import EdgeGraph, edge_softmax, spmm_values
from pygim_amd.backend_pim import spmm as spmm_mod
from pygim_amd.sparse_tensor import SparseTensorShim


def softmax_shift(m):
    """what the kernels subtract from the scores under a maximum m: m, or 0 when every score is -inf (masked), so that a masked score
    gives exp(-inf) = 0 and a fully masked row 0 / 0 = NaN with a log-sum-exp of -inf"""
    return np.where(np.isneginf(m), 0.0, m)


def _rows(ptr, rows, ld, width, npdt):
    """a [rows, width] window of a row-major buffer with row stride ld (elements)"""
    if rows == 0:
        return np.zeros((0, width), dtype=npdt)
    flat = _view(ptr, (rows - 1) * ld + width, npdt)
    es = np.dtype(npdt).itemsize
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, width), strides=(ld * es, es), writeable=True)


class FakeLibA(FakeLib):
    """the fake ABI with the entry points of pygim_amd.attention"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def group_serial(self, handle):
        if int(handle) not in self.groups:
            raise PygimError(1, "unknown group handle")
        return int(handle)

    def spmm_values_workspace(self, dtype, nrows, nnz, h, heads):
        return 64

    def edge_softmax_workspace(self, dtype, nrows, nnz, heads):
        return 0

    def spmm_values(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, heads, x_ptr, ldx, h, out_ptr, ldo, ws_ptr, ws_bytes, stream=0):
        self.calls.append("spmm_values")
        assert h % heads == 0 and ws_bytes >= 64
        npdt = NP_OF[dtype]
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        out = _rows(out_ptr, nrows, ldo, h, npdt)
        acc = np.zeros((nrows, h), dtype=np.float64)
        if nnz:
            val = _view(val_ptr, nnz * heads, npdt).reshape(nnz, heads).astype(np.float64)
            X = _rows(x_ptr, int(col.max()) + 1, ldx, h, npdt).astype(np.float64)
            row = np.repeat(np.arange(nrows), np.diff(rowptr))
            np.add.at(acc, row, np.repeat(val, h // heads, axis=1) * X[col])
        out[:] = acc.astype(npdt)

    def sddmm(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, g_ptr, ldg, x_ptr, ldx, h, out_ptr, stream=0):
        self.calls.append("sddmm")
        npdt = NP_OF[dtype]
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        G = _rows(g_ptr, nrows, ldg, h, npdt).astype(np.float64)
        X = _rows(x_ptr, int(col.max()) + 1, ldx, h, npdt).astype(np.float64)
        row = np.repeat(np.arange(nrows), np.diff(rowptr))
        _view(out_ptr, nnz, npdt)[:] = np.einsum("ef,ef->e", G[row], X[col]).astype(npdt)

    def _row_of(self, nrows, rowptr_ptr):
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        return np.repeat(np.arange(nrows), np.diff(rowptr))

    def edge_softmax(self, dtype, nrows, rowptr_ptr, nnz, s_ptr, heads, out_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("edge_softmax")
        npdt = NP_OF[dtype]
        row = self._row_of(nrows, rowptr_ptr)
        s = _view(s_ptr, nnz * heads, npdt).reshape(nnz, heads).astype(np.float64)
        m = np.full((nrows, heads), -np.inf)
        np.maximum.at(m, row, s)
        e = np.exp(s - softmax_shift(m)[row])
        z = np.zeros((nrows, heads))
        np.add.at(z, row, e)
        with np.errstate(invalid="ignore"):   # a fully masked row: 0 / 0
            _view(out_ptr, nnz * heads, npdt).reshape(nnz, heads)[:] = (e / z[row]).astype(npdt)

    def edge_softmax_backward(self, dtype, nrows, rowptr_ptr, nnz, p_ptr, dp_ptr, heads, out_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("edge_softmax_backward")
        npdt = NP_OF[dtype]
        row = self._row_of(nrows, rowptr_ptr)
        P = _view(p_ptr, nnz * heads, npdt).reshape(nnz, heads).astype(np.float64)
        dP = _view(dp_ptr, nnz * heads, npdt).reshape(nnz, heads).astype(np.float64)
        t = np.zeros((nrows, heads))
        np.add.at(t, row, P * dP)
        _view(out_ptr, nnz * heads, npdt).reshape(nnz, heads)[:] = (P * (dP - t[row])).astype(npdt)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibA()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    if pim_ops._library is not None:
        assert pim_ops._library != "native"
        pim_ops._library._destroy()
        pim_ops._library = None
    pim_ops._variant = None
    pim_ops._groups.clear()


def multigraph(rng, n=24, m=19, deg=4, used_cols=None):
    """duplicate entries, empty rows, a long row, and (used_cols < m) an empty trailing column range"""
    rowptr, col = random_csr(rng, n, used_cols or m, deg, empty_frac=0.2, long_rows=((5, 4 * deg),))
    col[rowptr[5] + 1] = col[rowptr[5]]   # a certain duplicate
    assert (np.diff(rowptr) == 0).any()
    return rowptr, col


def graph_of(rowptr, col, n, m):
    return EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))


def ref_spmm(rowptr, col, value, X, heads, n):
    """per-entry reference in plain torch (differentiable)"""
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    h = X.size(1)
    msg = value.reshape(-1, heads).repeat_interleave(h // heads, dim=1) * X[torch.from_numpy(col).long()]
    return torch.zeros(n, h, dtype=X.dtype).index_add(0, row, msg)


def ref_softmax(rowptr, scores, n):
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    s2 = scores.reshape(scores.size(0), -1)
    m = torch.full((n, s2.size(1)), -float("inf"), dtype=s2.dtype).index_reduce_(0, row, s2.detach(), "amax", include_self=True)
    e = torch.exp(s2 - m[row])
    z = torch.zeros(n, s2.size(1), dtype=s2.dtype).index_add(0, row, e)
    return (e / z[row]).reshape(scores.shape)


def test_public_names():
    assert pygim_amd.spmm_values is spmm_values and pygim_amd.edge_softmax is edge_softmax and pygim_amd.EdgeGraph is EdgeGraph
    assert hasattr(gnn, "GATConv") and hasattr(gnn, "GAT")


def test_edge_graph_structure_and_transpose(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    assert g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32 and g.nnz == len(col)
    assert np.array_equal(g.row.numpy(), np.repeat(np.arange(n), np.diff(rowptr)))
    gt, perm = g.transposed()
    order = np.argsort(col, kind="stable")
    assert np.array_equal(perm.numpy(), order)
    assert gt.nrows == m and gt.ncols == n
    assert np.array_equal(gt.rowptr.numpy(), np.concatenate([[0], np.cumsum(np.bincount(col, minlength=m))]))
    assert np.array_equal(gt.col.numpy(), np.repeat(np.arange(n), np.diff(rowptr))[order])
    assert g.transposed()[0] is gt, "the transposed structure is built once"
    assert EdgeGraph.of(g) is g
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, m))
    assert EdgeGraph.of(adj) is EdgeGraph.of(adj) and EdgeGraph.of(adj).nnz == len(col)


def test_argument_validation(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    nnz = len(col)
    v, X = torch.rand(nnz, dtype=torch.float64), torch.randn(m, 6, dtype=torch.float64)
    with pytest.raises(TypeError):
        spmm_values(g, v.float(), X)                      # dtype mismatch
    with pytest.raises(TypeError):
        spmm_values(g, v.int(), X.int())                   # not a float type
    with pytest.raises(ValueError):
        spmm_values(g, torch.rand(nnz, 4, dtype=torch.float64), X, heads=4)   # 6 % 4 != 0
    with pytest.raises(ValueError):
        spmm_values(g, v[:-1], X)                         # value of the wrong length
    with pytest.raises(ValueError):
        spmm_values(g, torch.rand(nnz, 2, dtype=torch.float64), X, heads=3)
    with pytest.raises(ValueError):
        spmm_values(g, v, X[:-1])                         # X does not cover the columns
    with pytest.raises(ValueError):
        edge_softmax(g, v[:-1])
    with pytest.raises(TypeError):
        edge_softmax(g, v.long())
    bad = col.copy()
    bad[0] = m
    with pytest.raises(ValueError):
        graph_of(rowptr, bad, n, m)                        # a column outside sparse_sizes
    rp = rowptr.copy()
    rp[3], rp[4] = rp[4] + 1, rp[3]
    with pytest.raises(ValueError):
        graph_of(rp, col, n, m)                            # rowptr not monotone
    with pytest.raises(ValueError):
        graph_of(rowptr[:-1], col, n, m)
    with pytest.raises(TypeError):
        EdgeGraph.of(object())
    assert fake.calls == []


@pytest.mark.parametrize("heads", [1, 3])
def test_spmm_values_forward_and_gradcheck(rng, fake, heads):
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    v = torch.rand(len(col), heads, dtype=torch.float64).add_(0.5).requires_grad_()
    X = torch.randn(m, h, dtype=torch.float64, requires_grad=True)
    out = spmm_values(g, v if heads > 1 else v[:, 0], X, heads=heads)
    assert torch.allclose(out, ref_spmm(rowptr, col, v, X, heads, n), rtol=1e-12, atol=1e-12)
    assert (out[np.diff(rowptr) == 0] == 0).all()
    assert torch.autograd.gradcheck(lambda a, b: spmm_values(g, a, b, heads=heads), (v, X))
    assert "sddmm" in fake.calls and fake.calls.count("spmm_values") >= 2


def test_spmm_values_float32_matches_reference(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    v = torch.rand(len(col), 2).requires_grad_()
    X = torch.randn(m, 8, requires_grad=True)
    G = torch.randn(n, 8)
    spmm_values(g, v, X, heads=2).backward(G)
    gv, gx = v.grad.clone(), X.grad.clone()
    v.grad = X.grad = None
    ref_spmm(rowptr, col, v, X, 2, n).backward(G)
    assert torch.allclose(gv, v.grad, rtol=1e-5, atol=1e-5) and torch.allclose(gx, X.grad, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("heads", [None, 3])
def test_edge_softmax_forward_and_gradcheck(rng, fake, heads):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    shape = (len(col),) if heads is None else (len(col), heads)
    s = (torch.randn(*shape, dtype=torch.float64) * 3).requires_grad_()
    p = edge_softmax(g, s)
    assert p.shape == s.shape and torch.allclose(p, ref_softmax(rowptr, s, n), rtol=1e-12, atol=1e-300)
    sums = torch.zeros(n, p.reshape(len(col), -1).size(1), dtype=torch.float64).index_add(0, g.row.long(), p.detach().reshape(len(col), -1))
    assert torch.allclose(sums[np.diff(rowptr) > 0], torch.ones(1, dtype=torch.float64))
    assert torch.autograd.gradcheck(lambda a: edge_softmax(g, a), (s,))
    assert "edge_softmax_backward" in fake.calls


def gat_reference(conv, x, rowptr, col, n):
    """PyG's GATConv arithmetic per stored entry in plain torch"""
    H, Fo = conv.heads, conv.out_channels
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    xp = (x @ conv.lin.weight.t()).view(-1, H, Fo)
    a_src, a_dst = (xp * conv.att_src).sum(-1), (xp * conv.att_dst).sum(-1)
    score = torch.nn.functional.leaky_relu(a_dst[row] + a_src[cc], conv.negative_slope)
    m = torch.full((n, H), -float("inf"), dtype=x.dtype).index_reduce_(0, row, score.detach(), "amax", include_self=True)
    e = torch.exp(score - m[row])
    p = e / torch.zeros(n, H, dtype=x.dtype).index_add(0, row, e)[row]
    out = torch.zeros(n, H, Fo, dtype=x.dtype).index_add(0, row, p.unsqueeze(-1) * xp[cc])
    out = out.reshape(n, H * Fo) if conv.concat else out.mean(1)
    return out if conv.bias is None else out + conv.bias


@pytest.mark.parametrize("heads,concat", [(1, True), (3, True), (2, False)])
def test_gatconv_matches_per_entry_reference(rng, fake, heads, concat):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(3)
    conv = gnn.GATConv(7, 4, heads=heads, concat=concat).double()
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 7, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, 4 * heads if concat else 4, dtype=torch.float64)
    out = conv(x, adj)
    assert out.shape == G.shape
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
    assert {"edge_softmax", "edge_softmax_backward", "spmm_values", "sddmm"} <= set(fake.calls)


def test_gat_stack_trains(rng, fake):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(0)
    model = gnn.GAT(5, 8, 3, num_layers=2, dropout=0.0, heads=2).double()
    x, y = torch.randn(n, 5, dtype=torch.float64), torch.randn(n, 3, dtype=torch.float64)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((model(x, adj) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert losses[-1] < losses[0]


def test_mul_values_follows_the_values_and_mul_does_not(rng, fake):
    """the contract: a group multiplies by the values it was created with; mul_values by the values of the call"""
    pim_ops.load("spmm")
    n, m, h = 30, 21, 4
    rowptr, col = multigraph(rng, n, m)
    v0 = torch.rand(len(col), dtype=torch.float64) + 0.5
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), value=v0.clone(), sparse_sizes=(n, m))
    torch.ops.pim_ops.dpu_init_ranks(1)
    A = spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=torch.float64, sp_format="CSR", sp_parts=1, ds_parts=1, hidden_size=h))
    x = torch.randn(m, h, dtype=torch.float64)
    old = ref_spmm(rowptr, col, v0, x, 1, n)
    assert torch.allclose(A.mul(x), old, rtol=1e-12, atol=1e-12)
    assert torch.allclose(A.mul_values(v0, x), old, rtol=1e-12, atol=1e-12)
    v1 = v0 * 2 + 1
    adj.storage.value().copy_(v1)   # what an optimizer step does
    assert torch.allclose(A.mul_values(v1, x), ref_spmm(rowptr, col, v1, x, 1, n), rtol=1e-12, atol=1e-12)
    assert torch.allclose(A.mul(x), old, rtol=1e-12, atol=1e-12), "mul uses the values the group was created with"
    assert EdgeGraph.of(A) is EdgeGraph.of(A), "the structure is cached on the wrapper"
    vv = torch.rand(len(col), 2, dtype=torch.float64)
    assert torch.allclose(A.mul_values(vv, x, heads=2), ref_spmm(rowptr, col, vv, x, 2, n), rtol=1e-12, atol=1e-12)
