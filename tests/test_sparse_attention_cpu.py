"""Sparse dot-product attention on CPU: pygim_amd.sparse_attention, gnn.TransformerConv and gnn.GraphTransformer driven with the C-ABI
test double of test_gat_fused_cpu.py, extended here with numpy float64 statements of pygim_sparse_attention and
pygim_sparse_attention_workspace (heads wider than 256 features rejected, as the library rejects them)."""
import numpy as np
import pytest
import torch

import pygim_amd
from fake_abi import NP_OF, PygimError, _view
from pygim_amd import gnn, pim_ops
from pygim_amd.attention import sparse_attention
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import _rows, graph_of, multigraph, softmax_shift
from test_gat_fused_cpu import FakeLibG


class FakeLibS(FakeLibG):
    """FakeLibG with the two entry points of the fused dot-product attention"""

    def sparse_attention_workspace(self, dtype, nrows, nnz, h, heads):
        if h < 1 or heads < 1 or h % heads != 0 or h // heads > 256:
            raise PygimError(1, "bad sparse_attention_workspace arguments")
        return 112

    def sparse_attention(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, h, heads, scale, out_ptr, ldo, lse_ptr,
                         ws_ptr, ws_bytes, stream=0):
        self.calls.append("sparse_attention")
        if h % heads != 0 or h // heads > 256:
            raise PygimError(1, "sparse_attention: a head is at most 256 features wide")
        assert ws_bytes >= 112
        npdt = NP_OF[dtype]
        hd = h // heads
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        out = _rows(out_ptr, nrows, ldo, h, npdt)
        acc = np.zeros((nrows, h))
        lse = np.zeros((nrows, heads))
        if nnz:
            row = np.repeat(np.arange(nrows), np.diff(rowptr))
            ncols = int(col.max()) + 1
            Q = _rows(q_ptr, nrows, ldq, h, npdt).astype(np.float64).reshape(nrows, heads, hd)
            K = _rows(k_ptr, ncols, ldk, h, npdt).astype(np.float64).reshape(ncols, heads, hd)
            V = _rows(v_ptr, ncols, ldv, h, npdt).astype(np.float64)
            s = scale * np.einsum("ekf,ekf->ek", Q[row], K[col])
            m = np.full((nrows, heads), -np.inf)
            np.maximum.at(m, row, s)
            e = np.exp(s - softmax_shift(m)[row])
            l = np.zeros((nrows, heads))
            np.add.at(l, row, e)
            full = np.diff(rowptr) > 0
            with np.errstate(invalid="ignore", divide="ignore"):   # a fully masked row: 0 / 0 = NaN, lse = -inf + log(0) = -inf
                np.add.at(acc, row, np.repeat(e / l[row], hd, axis=1) * V[col])
                lse[full] = m[full] + np.log(l[full])
        out[:] = acc.astype(npdt)
        if lse_ptr:
            _view(lse_ptr, nrows * heads, npdt).reshape(nrows, heads)[:] = lse.astype(npdt)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibS()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    pim_ops._variant = None
    pim_ops._groups.clear()


def ref_sparse_attention(rowptr, col, Q, K, V, heads, n, scale=None):
    """per-entry reference in plain torch (differentiable)"""
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    h = Q.size(1)
    hd = h // heads
    scale = hd ** -0.5 if scale is None else scale
    s = scale * (Q.view(-1, heads, hd)[row] * K.view(-1, heads, hd)[cc]).sum(-1)
    m = torch.full((n, heads), -float("inf"), dtype=Q.dtype).index_reduce_(0, row, s.detach(), "amax", include_self=True)
    e = torch.exp(s - m[row])
    p = e / torch.zeros(n, heads, dtype=Q.dtype).index_add(0, row, e)[row]
    return torch.zeros(n, h, dtype=Q.dtype).index_add(0, row, p.repeat_interleave(hd, dim=1) * V[cc])


def transformer_reference(conv, x, rowptr, col, n):
    """PyG's TransformerConv arithmetic (no edge features, no beta) per stored entry in plain torch"""
    H, Fo = conv.heads, conv.out_channels
    q, k, v = conv.lin_query(x), conv.lin_key(x), conv.lin_value(x)
    out = ref_sparse_attention(rowptr, col, q, k, v, H, n, scale=Fo ** -0.5)
    if not conv.concat:
        out = out.view(n, H, Fo).mean(1)
    return out if conv.lin_skip is None else out + conv.lin_skip(x)


def test_public_names():
    assert pygim_amd.sparse_attention is sparse_attention
    assert hasattr(gnn, "TransformerConv") and hasattr(gnn, "GraphTransformer")


def operands(n, m, h, dtype=torch.float64):
    return [torch.randn(n, h, dtype=dtype), torch.randn(m, h, dtype=dtype), torch.randn(m, h, dtype=dtype)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
def test_forward_and_gradients_match_the_per_entry_reference(rng, fake, heads, fused):
    """a multigraph with empty rows and an empty trailing column range; the default scale and a given one"""
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    torch.manual_seed(5)
    Q, K, V = (t.mul_(1.5).requires_grad_() for t in operands(n, m, h))
    G = torch.randn(n, h, dtype=torch.float64)
    for scale in (None, 0.7):
        out = sparse_attention(g, Q, K, V, heads=heads, scale=scale, fused=fused)
        want = ref_sparse_attention(rowptr, col, Q, K, V, heads, n, scale)
        assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
        assert (out[np.diff(rowptr) == 0] == 0).all()
        out.backward(G)
        got = [t.grad.clone() for t in (Q, K, V)]
        for t in (Q, K, V):
            t.grad = None
        want.backward(G)
        for a, t in zip(got, (Q, K, V)):
            assert a.dtype == t.dtype and torch.allclose(a, t.grad, rtol=1e-9, atol=1e-11)
            t.grad = None
    assert torch.autograd.gradcheck(lambda a, b, c: sparse_attention(g, a, b, c, heads=heads, fused=fused), (Q, K, V))
    if fused:
        assert "edge_softmax" not in fake.calls and "sparse_attention" in fake.calls
    else:
        assert "sparse_attention" not in fake.calls and {"sddmm", "edge_softmax", "edge_softmax_backward", "spmm_values"} <= set(fake.calls)


def test_the_fused_forward_is_one_call_and_float32_works(rng, fake):
    n, m, h, heads = 24, 19, 8, 2
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    Q, K, V = operands(n, m, h, torch.float32)
    out = sparse_attention(g, Q, K, V, heads=heads)
    assert fake.calls == ["sparse_attention"] and out.dtype == torch.float32
    want = ref_sparse_attention(rowptr, col, Q.double(), K.double(), V.double(), heads, n)
    assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-6)
    unfused = sparse_attention(g, Q, K, V, heads=heads, fused=False)
    assert torch.allclose(unfused, out, rtol=1e-5, atol=1e-6)
    assert fake.calls == ["sparse_attention"] + ["sddmm"] * heads + ["edge_softmax", "spmm_values"]


def test_lse_is_requested_only_when_a_gradient_is_needed(rng, fake, monkeypatch):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    asked = []
    inner = fake.sparse_attention

    def spy(*a, **k):
        asked.append(bool(a[16]))   # lse_ptr
        return inner(*a, **k)

    monkeypatch.setattr(fake, "sparse_attention", spy)
    Q, K, V = operands(n, m, 4, torch.float32)
    sparse_attention(g, Q, K, V, heads=2)
    sparse_attention(g, Q, K.clone().requires_grad_(), V, heads=2)
    assert asked == [False, True]


def test_heads_wider_than_256_run_unfused(rng, fake):
    """hd = 300: the library rejects it (so does the double), the wrapper takes the composition without saying so; hd = 256 is fused"""
    n, m = 12, 10
    rowptr, col = multigraph(rng, n, m, deg=3)
    g = graph_of(rowptr, col, n, m)
    with pytest.raises(PygimError):
        fake.sparse_attention_workspace(5, n, len(col), 600, 2)
    assert fake.sparse_attention_workspace(5, n, len(col), 512, 2) > 0
    Q, K, V = (t.mul_(0.3).requires_grad_() for t in operands(n, m, 600))
    out = sparse_attention(g, Q, K, V, heads=2)
    assert "sparse_attention" not in fake.calls and "edge_softmax" in fake.calls
    want = ref_sparse_attention(rowptr, col, Q, K, V, 2, n)
    assert torch.allclose(out, want, rtol=1e-11, atol=1e-12)
    G = torch.randn(n, 600, dtype=torch.float64)
    out.backward(G)
    got = [t.grad.clone() for t in (Q, K, V)]
    for t in (Q, K, V):
        t.grad = None
    want.backward(G)
    for a, t in zip(got, (Q, K, V)):
        assert torch.allclose(a, t.grad, rtol=1e-9, atol=1e-11)
    fake.calls.clear()
    sparse_attention(g, Q.detach()[:, :512], K.detach()[:, :512], V.detach()[:, :512], heads=2)
    assert fake.calls == ["sparse_attention"]


def test_nothing_of_size_nnz_is_saved_for_the_backward(rng, fake):
    n, m, h, heads = 12, 12, 6, 2
    from conftest import random_csr

    rowptr, col = random_csr(rng, n, m, 90, empty_frac=0.1)
    nnz = len(col)
    assert nnz > n * h
    g = graph_of(rowptr, col, n, m)
    Q, K, V = (t.requires_grad_() for t in operands(n, m, h))

    def largest_saved(fused):
        sizes = []

        def pack(t):
            sizes.append(t.numel())
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = sparse_attention(g, Q, K, V, heads=heads, fused=fused)
        out.sum().backward()
        return max(sizes)

    assert largest_saved(True) < nnz
    assert largest_saved(False) >= nnz


def test_argument_validation(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    Q, K, V = operands(n, m, 6)
    with pytest.raises(TypeError):
        sparse_attention(g, Q.float(), K, V)                     # dtype mismatch
    with pytest.raises(TypeError):
        sparse_attention(g, Q, K, V.bfloat16())                  # one 16-bit operand among float64 ones
    with pytest.raises(TypeError):
        sparse_attention(g, Q.int(), K.int(), V.int())           # not a float type
    with pytest.raises(TypeError):
        sparse_attention(g, Q.bfloat16(), K.half(), V.half())    # two 16-bit types
    with pytest.raises(ValueError):
        sparse_attention(g, Q[:-1], K, V)                        # Q does not cover the rows
    with pytest.raises(ValueError):
        sparse_attention(g, Q, K[:-1], V)                        # K does not cover the columns
    with pytest.raises(ValueError):
        sparse_attention(g, Q, K, V[:, :-1])                     # V has another width
    with pytest.raises(ValueError):
        sparse_attention(g, Q[:, 0], K[:, 0], V[:, 0])           # 1-D
    with pytest.raises(ValueError):
        sparse_attention(g, Q, K, V, heads=4)                    # 6 % 4 != 0
    with pytest.raises(ValueError):
        sparse_attention(g, Q, K, V, heads=0)
    assert fake.calls == []


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads,concat,root_weight", [(1, True, True), (3, True, False), (2, False, True), (2, False, False)])
def test_transformerconv_matches_per_entry_reference(rng, fake, heads, concat, root_weight, fused):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(3)
    conv = gnn.TransformerConv(7, 4, heads=heads, concat=concat, root_weight=root_weight, fused=fused).double()
    assert (conv.lin_skip is not None) == root_weight and all(lin.bias is not None for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
    x = torch.randn(n, 7, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, 4 * heads if concat else 4, dtype=torch.float64)
    out = conv(x, adj)
    assert out.shape == G.shape
    if fused:
        assert fake.calls == ["sparse_attention"], "the fused forward is one call: no sddmm, no edge_softmax, no spmm_values"
    out.backward(G)
    got = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    want_out = transformer_reference(conv, x, rowptr, col, n)
    want_out.backward(G)
    want = [x.grad] + [p.grad for p in conv.parameters()]
    assert torch.allclose(out, want_out, rtol=1e-10, atol=1e-12)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    assert ("edge_softmax" in fake.calls) == (not fused)


def test_transformerconv_without_bias(fake):
    conv = gnn.TransformerConv(5, 3, heads=2, bias=False)
    assert all(lin.bias is None for lin in (conv.lin_query, conv.lin_key, conv.lin_value, conv.lin_skip))


@pytest.mark.parametrize("fused", [True, False])
def test_graph_transformer_trains(rng, fake, fused):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(0)
    model = gnn.GraphTransformer(5, 8, 3, num_layers=2, dropout=0.0, heads=2, fused=fused).double()
    assert all(c.fused is fused for c in model.convs)
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
