"""Edge terms on CPU: gat_aggregate(a_edge=), sparse_attention(bias=) and gnn.GATConv(edge_dim=) driven with the C-ABI test double of
test_sparse_attention_cpu.py, extended here with numpy float64 statements of pygim_gat_aggregate_edge, pygim_sparse_attention_bias and
pygim_attention_dropout_mask (the mask from the numpy mirror of attn_dropout_ref.py); and, on the float64 reference of edge_term_ref.py
alone, the proof that the GPU parity cases of test_edge_term_gpu.py can fail: a term that is left out, or shifted by one entry, moves
every row with two or more entries by more than the asserted bound."""
import numpy as np
import pytest
import torch

import attn_dropout_ref as ad
import edge_term_ref as er
from fake_abi import NP_OF, PygimError, _view
from pygim_amd import gnn, pim_ops
from pygim_amd.attention import gat_aggregate, sparse_attention
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import _rows, graph_of, multigraph, softmax_shift
from test_sparse_attention_cpu import FakeLibS

SEED = ad.SEED


class FakeLibE(FakeLibS):
    """FakeLibS with the two entry points that take an edge term, and the dropout mask the composed backwards and compositions ask for"""

    @staticmethod
    def _finish(nrows, rowptr, col, s, V, h, heads, p, seed, out, lse_ptr, npdt):
        row = np.repeat(np.arange(nrows), np.diff(rowptr))
        m = np.full((nrows, heads), -np.inf)
        np.maximum.at(m, row, s)
        e = np.exp(s - softmax_shift(m)[row])
        l = np.zeros((nrows, heads))
        np.add.at(l, row, e)
        w = ad.weights(len(col), heads, p, seed) if p > 0.0 else 1.0
        acc = np.zeros((nrows, h))
        lse = np.zeros((nrows, heads))
        full = np.diff(rowptr) > 0
        with np.errstate(invalid="ignore", divide="ignore"):   # a fully masked row: 0 / 0 = NaN, lse = -inf
            np.add.at(acc, row, np.repeat(e / l[row] * w, h // heads, axis=1) * V[col])
            lse[full] = m[full] + np.log(l[full])
        out[:] = acc.astype(npdt)
        if lse_ptr:
            _view(lse_ptr, nrows * heads, npdt).reshape(nrows, heads)[:] = lse.astype(npdt)

    def gat_aggregate_edge(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr, ldo,
                           lse_ptr, ws_ptr, ws_bytes, stream, a_edge_ptr, p=0.0, seed=0):
        self.calls.append("gat_aggregate_edge")
        assert h % heads == 0 and ws_bytes >= 96 and 0.0 <= p < 1.0
        if nnz and not a_edge_ptr:
            raise PygimError(1, "gat_aggregate_edge: a_edge is NULL")
        npdt = NP_OF[dtype]
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        out = _rows(out_ptr, nrows, ldo, h, npdt)
        if not nnz:
            out[:] = 0
            if lse_ptr:
                _view(lse_ptr, nrows * heads, npdt)[:] = 0
            return
        row = np.repeat(np.arange(nrows), np.diff(rowptr))
        ncols = int(col.max()) + 1
        a_dst = _view(a_dst_ptr, nrows * heads, npdt).reshape(nrows, heads).astype(np.float64)
        a_src = _view(a_src_ptr, ncols * heads, npdt).reshape(ncols, heads).astype(np.float64)
        a_edge = _view(a_edge_ptr, nnz * heads, npdt).reshape(nnz, heads).astype(np.float64)
        X = _rows(x_ptr, ncols, ldx, h, npdt).astype(np.float64)
        z = a_dst[row] + a_src[col] + a_edge
        s = np.where(z >= 0, z, negative_slope * z)
        self._finish(nrows, rowptr, col, s, X, h, heads, p, seed, out, lse_ptr, npdt)

    def sparse_attention_bias(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, h, heads, scale, out_ptr, ldo,
                              lse_ptr, ws_ptr, ws_bytes, stream, bias_ptr, p=0.0, seed=0):
        self.calls.append("sparse_attention_bias")
        if h % heads != 0 or h // heads > 256:
            raise PygimError(1, "sparse_attention: a head is at most 256 features wide")
        assert ws_bytes >= 112 and 0.0 <= p < 1.0
        if nnz and not bias_ptr:
            raise PygimError(1, "sparse_attention_bias: bias is NULL")
        npdt = NP_OF[dtype]
        hd = h // heads
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        out = _rows(out_ptr, nrows, ldo, h, npdt)
        if not nnz:
            out[:] = 0
            if lse_ptr:
                _view(lse_ptr, nrows * heads, npdt)[:] = 0
            return
        row = np.repeat(np.arange(nrows), np.diff(rowptr))
        ncols = int(col.max()) + 1
        Q = _rows(q_ptr, nrows, ldq, h, npdt).astype(np.float64).reshape(nrows, heads, hd)
        K = _rows(k_ptr, ncols, ldk, h, npdt).astype(np.float64).reshape(ncols, heads, hd)
        V = _rows(v_ptr, ncols, ldv, h, npdt).astype(np.float64)
        bias = _view(bias_ptr, nnz * heads, npdt).reshape(nnz, heads).astype(np.float64)
        s = scale * np.einsum("ekf,ekf->ek", Q[row], K[col]) + bias
        self._finish(nrows, rowptr, col, s, V, h, heads, p, seed, out, lse_ptr, npdt)

    def attention_dropout_mask(self, dtype, nnz, heads, entry_ids_ptr, p, seed, mask_ptr, stream=0):
        self.calls.append("attention_dropout_mask")
        ids = _view(entry_ids_ptr, nnz, np.int32) if entry_ids_ptr else None
        _view(mask_ptr, nnz * heads, NP_OF[dtype]).reshape(nnz, heads)[:] = ad.weights(nnz, heads, p, seed, ids)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibE()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    pim_ops._variant = None
    pim_ops._groups.clear()


def softmax_product(rowptr, s, V, cc, heads, n, w=None):
    """per-entry softmax of the scores s [nnz, heads] over every row and the product with V[cc], in plain torch (differentiable)"""
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    m = torch.full((n, heads), -float("inf"), dtype=V.dtype).index_reduce_(0, row, s.detach(), "amax", include_self=True)
    e = torch.exp(s - m[row])
    p = e / torch.zeros(n, heads, dtype=V.dtype).index_add(0, row, e)[row]
    if w is not None:
        p = p * w
    return torch.zeros(n, V.size(1), dtype=V.dtype).index_add(0, row, p.repeat_interleave(V.size(1) // heads, dim=1) * V[cc])


def ref_gat_edge(rowptr, col, a_dst, a_src, a_edge, X, slope, n, w=None):
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    heads = a_src.size(1)
    s = torch.nn.functional.leaky_relu(a_dst[row] + a_src[cc] + a_edge.reshape(-1, heads), slope)
    return softmax_product(rowptr, s, X, cc, heads, n, w)


def ref_sa_bias(rowptr, col, Q, K, V, bias, heads, n, scale=None, w=None):
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    hd = Q.size(1) // heads
    scale = hd ** -0.5 if scale is None else scale
    s = scale * (Q.view(-1, heads, hd)[row] * K.view(-1, heads, hd)[cc]).sum(-1) + bias.reshape(-1, heads)
    return softmax_product(rowptr, s, V, cc, heads, n, w)


def grads_of(out, G, leaves):
    out.backward(G)
    got = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    return got


def dropout_weights(nnz, heads, p):
    return None if p == 0.0 else torch.from_numpy(ad.weights(nnz, heads, p, SEED))


@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("heads", [1, 2, 3])
def test_gat_forward_and_gradients_match_the_per_entry_reference(rng, fake, heads, p):
    """a multigraph with empty rows and an empty trailing column range; one head also with a 1-D term"""
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    nnz = len(col)
    torch.manual_seed(heads)
    a_dst = (torch.randn(n, heads, dtype=torch.float64) * 2).requires_grad_()
    a_src = (torch.randn(m, heads, dtype=torch.float64) * 2).requires_grad_()
    a_edge = (torch.randn(nnz, heads, dtype=torch.float64) * 2).requires_grad_()
    X = torch.randn(m, h, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, h, dtype=torch.float64)
    leaves = (a_dst, a_src, a_edge, X)
    if heads == 1:
        out = gat_aggregate(g, a_dst[:, 0], a_src[:, 0], X, 0.3, dropout=p, seed=SEED, a_edge=a_edge[:, 0])
    else:
        out = gat_aggregate(g, a_dst, a_src, X, 0.3, dropout=p, seed=SEED, a_edge=a_edge)
    want = ref_gat_edge(rowptr, col, a_dst, a_src, a_edge, X, 0.3, n, dropout_weights(nnz, heads, p))
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert (out[np.diff(rowptr) == 0] == 0).all()
    got = grads_of(out, G, leaves)
    for a, b, t in zip(got, grads_of(want, G, leaves), leaves):
        assert a.dtype == t.dtype and a.shape == t.shape and torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    assert "gat_aggregate_edge" in fake.calls and "gat_aggregate" not in fake.calls and "edge_softmax" not in fake.calls
    # a term that does not require grad gets none, and the others do not change
    out = gat_aggregate(g, a_dst, a_src, X, 0.3, dropout=p, seed=SEED, a_edge=a_edge.detach())
    again = grads_of(out, G, (a_dst, a_src, X))
    for a, b in zip(again, (got[0], got[1], got[3])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads", [1, 2, 3])
def test_sparse_attention_forward_and_gradients_match_the_per_entry_reference(rng, fake, heads, fused, p):
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    nnz = len(col)
    torch.manual_seed(5 + heads)
    Q, K, V = ((torch.randn(r, h, dtype=torch.float64) * 1.5).requires_grad_() for r in (n, m, m))
    bias = (torch.randn(nnz, heads, dtype=torch.float64) * 2).requires_grad_()
    G = torch.randn(n, h, dtype=torch.float64)
    leaves = (Q, K, V, bias)
    for scale in (None, 0.7):
        out = sparse_attention(g, Q, K, V, heads=heads, scale=scale, fused=fused, dropout=p, seed=SEED, bias=bias[:, 0] if heads == 1 else bias)
        want = ref_sa_bias(rowptr, col, Q, K, V, bias, heads, n, scale, dropout_weights(nnz, heads, p))
        assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
        assert (out[np.diff(rowptr) == 0] == 0).all()
        for a, b, t in zip(grads_of(out, G, leaves), grads_of(want, G, leaves), leaves):
            assert a.dtype == t.dtype and a.shape == t.shape and torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    if fused:
        assert "sparse_attention_bias" in fake.calls and "sparse_attention" not in fake.calls and "edge_softmax" not in fake.calls
    else:
        assert "sparse_attention_bias" not in fake.calls and {"sddmm", "edge_softmax", "edge_softmax_backward", "spmm_values"} <= set(fake.calls)
    # the bias alone: only its gradient is formed
    out = sparse_attention(g, Q.detach(), K.detach(), V.detach(), heads=heads, fused=fused, dropout=p, seed=SEED, bias=bias)
    want = ref_sa_bias(rowptr, col, Q.detach(), K.detach(), V.detach(), bias, heads, n, None, dropout_weights(nnz, heads, p))
    assert torch.allclose(grads_of(out, G, (bias,))[0], grads_of(want, G, (bias,))[0], rtol=1e-9, atol=1e-11)


def test_wide_heads_add_the_bias_to_the_composed_scores(rng, fake):
    n, m, h = 9, 8, 260
    rowptr, col = multigraph(rng, n, m, deg=2)
    g = graph_of(rowptr, col, n, m)
    torch.manual_seed(2)
    Q, K, V = (torch.randn(r, h, dtype=torch.float64) * 0.3 for r in (n, m, m))
    bias = torch.randn(len(col), dtype=torch.float64)
    out = sparse_attention(g, Q, K, V, heads=1, bias=bias)
    assert "sparse_attention_bias" not in fake.calls and "edge_softmax" in fake.calls
    assert torch.allclose(out, ref_sa_bias(rowptr, col, Q, K, V, bias, 1, n), rtol=1e-12, atol=1e-12)


def test_gradcheck(rng, fake):
    n, m, h, heads = 20, 17, 4, 2
    rowptr, col = multigraph(rng, n, m, deg=3)
    g = graph_of(rowptr, col, n, m)
    nnz = len(col)
    torch.manual_seed(9)
    a_dst, a_src, X = (torch.randn(r, c, dtype=torch.float64, requires_grad=True) for r, c in ((n, heads), (m, heads), (m, h)))
    term = torch.randn(nnz, heads, dtype=torch.float64, requires_grad=True)
    Q = torch.randn(n, h, dtype=torch.float64, requires_grad=True)
    for p in (0.0, 0.3):
        assert torch.autograd.gradcheck(lambda a, b, e, x: gat_aggregate(g, a, b, x, 0.3, dropout=p, seed=SEED, a_edge=e), (a_dst, a_src, term, X))
        for fused in (True, False):
            assert torch.autograd.gradcheck(lambda q, k, v, b: sparse_attention(g, q, k, v, heads=heads, fused=fused, dropout=p, seed=SEED, bias=b),
                                            (Q, X, X.detach().clone().requires_grad_(), term))


def masked_setup(rng, heads):
    """a multigraph and a mask that leaves every row at least its first entry"""
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    nnz = len(col)
    gone = rng.random(nnz) < 0.4
    gone[rowptr[:-1][np.diff(rowptr) > 0]] = False
    assert gone.sum() > 5 and gone[rowptr[5]:rowptr[6]].sum() >= 2, "entries of the long row are masked too"
    rp2, col2 = er.remove_entries(n, rowptr, col, gone)
    return n, m, rowptr, col, gone, rp2, col2


@pytest.mark.parametrize("heads", [1, 3])
def test_minus_infinity_masks_gat_entries(rng, fake, heads):
    n, m, rowptr, col, gone, rp2, col2 = masked_setup(rng, heads)
    h = 6
    g, g2 = graph_of(rowptr, col, n, m), graph_of(rp2, col2, n, m)
    torch.manual_seed(4)
    a_dst, a_src = (torch.randn(r, heads, dtype=torch.float64, requires_grad=True) for r in (n, m))
    X = torch.randn(m, h, dtype=torch.float64, requires_grad=True)
    term = torch.randn(len(col), heads, dtype=torch.float64)
    term[torch.from_numpy(gone)] = -float("inf")
    term.requires_grad_()
    G = torch.randn(n, h, dtype=torch.float64)
    out = gat_aggregate(g, a_dst, a_src, X, 0.3, a_edge=term)
    got = grads_of(out, G, (a_dst, a_src, X, term))
    kept = term.detach()[torch.from_numpy(~gone)].clone().requires_grad_()
    want = gat_aggregate(g2, a_dst, a_src, X, 0.3, a_edge=kept)
    ref = grads_of(want, G, (a_dst, a_src, X, kept))
    assert not torch.isnan(out).any() and all(not torch.isnan(t).any() for t in got)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    for a, b in zip(got[:3], ref[:3]):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    assert (got[3][torch.from_numpy(gone)] == 0).all(), "a masked entry has a gradient of exactly 0"
    assert torch.allclose(got[3][torch.from_numpy(~gone)], ref[3], rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
def test_minus_infinity_masks_attention_entries(rng, fake, heads, fused):
    n, m, rowptr, col, gone, rp2, col2 = masked_setup(rng, heads)
    h = 6
    g, g2 = graph_of(rowptr, col, n, m), graph_of(rp2, col2, n, m)
    torch.manual_seed(6)
    Q, K, V = (torch.randn(r, h, dtype=torch.float64, requires_grad=True) for r in (n, m, m))
    bias = torch.randn(len(col), heads, dtype=torch.float64)
    bias[torch.from_numpy(gone)] = -float("inf")
    bias.requires_grad_()
    G = torch.randn(n, h, dtype=torch.float64)
    out = sparse_attention(g, Q, K, V, heads=heads, fused=fused, bias=bias)
    got = grads_of(out, G, (Q, K, V, bias))
    kept = bias.detach()[torch.from_numpy(~gone)].clone().requires_grad_()
    want = sparse_attention(g2, Q, K, V, heads=heads, fused=fused, bias=kept)
    ref = grads_of(want, G, (Q, K, V, kept))
    assert not torch.isnan(out).any() and all(not torch.isnan(t).any() for t in got)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    for a, b in zip(got[:3], ref[:3]):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    assert (got[3][torch.from_numpy(gone)] == 0).all(), "a masked entry has a gradient of exactly 0"
    assert torch.allclose(got[3][torch.from_numpy(~gone)], ref[3], rtol=1e-9, atol=1e-11)


def test_no_term_reaches_the_old_entry_points(rng, fake, monkeypatch):
    n, m, h, heads = 24, 19, 6, 2
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    for name in ("gat_aggregate_edge", "sparse_attention_bias"):
        monkeypatch.setattr(fake, name, lambda *a, **k: pytest.fail("a call without a term reached the entry point with one"))
    a_dst, a_src = torch.randn(n, heads, dtype=torch.float64), torch.randn(m, heads, dtype=torch.float64, requires_grad=True)
    X = torch.randn(m, h, dtype=torch.float64, requires_grad=True)
    gat_aggregate(g, a_dst, a_src, X).sum().backward()
    gat_aggregate(g, a_dst, a_src, X, a_edge=None).sum().backward()
    sparse_attention(g, torch.randn(n, h, dtype=torch.float64), X, X, heads=heads).sum().backward()
    sparse_attention(g, torch.randn(n, h, dtype=torch.float64), X, X, heads=heads, bias=None).sum().backward()
    assert fake.calls.count("gat_aggregate") == 2 and fake.calls.count("sparse_attention") == 2
    conv = gnn.GATConv(7, 3, heads=2, fused=True, edge_dim=4).double()
    conv(torch.randn(n, 7, dtype=torch.float64), graph_of(*multigraph(rng, n, n), n, n))   # edge_attr=None: the layer as without edge_dim
    assert fake.calls.count("gat_aggregate") == 3


def test_the_forward_saves_the_term_and_nothing_else_of_size_nnz(rng, fake):
    """more entries than any node-sized tensor has elements: what the fused forward saves of that size is the term itself (the caller's
    storage), and nothing has h * nnz elements"""
    from conftest import random_csr

    n, heads, h = 12, 2, 6
    rowptr, col = random_csr(rng, n, n, 90, empty_frac=0.1)
    nnz = len(col)
    assert nnz > n * h
    g = graph_of(rowptr, col, n, n)
    term = torch.randn(nnz, heads, dtype=torch.float64, requires_grad=True)
    a = torch.randn(n, heads, dtype=torch.float64, requires_grad=True)
    X = torch.randn(n, h, dtype=torch.float64, requires_grad=True)
    for call in (lambda: gat_aggregate(g, a, a, X, a_edge=term), lambda: sparse_attention(g, X, X, X, heads=heads, bias=term)):
        saved = []

        def pack(t):
            saved.append(t)
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = call()
        out.sum().backward()
        big = [t for t in saved if t.numel() >= nnz]
        assert len(big) == 1 and big[0].data_ptr() == term.data_ptr() and big[0].numel() == nnz * heads
        assert max(t.numel() for t in saved) < h * nnz


def gatconv_edge_reference(conv, x, edge_attr, rowptr, col, n):
    """PyG's GATConv(edge_dim=) arithmetic per stored entry in plain torch, with the [nnz, H, C] tensor of lin_edge(edge_attr)"""
    H, C = conv.heads, conv.out_channels
    cc = torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    xp = (x @ conv.lin.weight.t()).view(-1, H, C)
    a_src, a_dst = (xp * conv.att_src).sum(-1), (xp * conv.att_dst).sum(-1)
    a_edge = (conv.lin_edge(edge_attr).view(-1, H, C) * conv.att_edge).sum(-1)
    s = torch.nn.functional.leaky_relu(a_dst[row] + a_src[cc] + a_edge, conv.negative_slope)
    out = softmax_product(rowptr, s, xp.reshape(-1, H * C), cc, H, n)
    if not conv.concat:
        out = out.view(n, H, C).mean(1)
    return out if conv.bias is None else out + conv.bias


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads,concat", [(1, True), (3, True), (2, False)])
def test_gatconv_with_edge_features_matches_the_formula_of_pyg(rng, fake, heads, concat, fused):
    n, d = 22, 5
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(3)
    conv = gnn.GATConv(7, 4, heads=heads, concat=concat, fused=fused, edge_dim=d).double()
    assert conv.lin_edge.weight.shape == (heads * 4, d) and conv.lin_edge.bias is None and conv.att_edge.shape == (1, heads, 4)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 7, dtype=torch.float64, requires_grad=True)
    edge_attr = torch.randn(len(col), d, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, 4 * heads if concat else 4, dtype=torch.float64)
    leaves = [x, edge_attr] + list(conv.parameters())
    out = conv(x, adj, edge_attr)
    assert fake.calls == (["gat_aggregate_edge"] if fused else ["edge_softmax", "spmm_values"])
    got = grads_of(out, G, leaves)
    want_out = gatconv_edge_reference(conv, x, edge_attr, rowptr, col, n)
    want = grads_of(want_out, G, leaves)
    assert out.shape == G.shape and torch.allclose(out, want_out, rtol=1e-10, atol=1e-12)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    # train() with attention dropout runs; eval() drops nothing
    drop = gnn.GATConv(7, 4, heads=heads, concat=concat, fused=fused, edge_dim=d, dropout=0.5).double()
    drop.load_state_dict(conv.state_dict())
    assert not torch.allclose(drop(x, adj, edge_attr), out) and torch.allclose(drop.eval()(x, adj, edge_attr), out, rtol=1e-12, atol=1e-12)


def test_gatconv_without_edge_dim_is_the_layer_as_before(rng, fake):
    torch.manual_seed(8)
    plain = gnn.GATConv(7, 4, heads=2)
    torch.manual_seed(8)
    edged = gnn.GATConv(7, 4, heads=2, edge_dim=3)
    assert not hasattr(plain, "lin_edge") and plain.edge_dim is None
    for k, v in plain.state_dict().items():
        assert torch.equal(v, edged.state_dict()[k]), "the existing parameters draw what they drew before"
    assert set(edged.state_dict()) - set(plain.state_dict()) == {"lin_edge.weight", "att_edge"}
    n = 22
    g = graph_of(*multigraph(rng, n, n), n, n)
    with pytest.raises(ValueError, match="GATConv"):
        plain(torch.randn(n, 7), g, torch.randn(g.nnz, 3))             # edge_attr without edge_dim
    with pytest.raises(ValueError, match="GATConv"):
        edged(torch.randn(n, 7), g, torch.randn(g.nnz, 4))             # the wrong edge_dim
    with pytest.raises(ValueError, match="GATConv"):
        edged(torch.randn(n, 7), g, torch.randn(g.nnz - 1, 3))         # not one row per entry
    with pytest.raises(ValueError, match="GATConv"):
        gnn.GATConv(7, 4, edge_dim=0)


def test_float32_terms_and_gradient_dtypes(rng, fake):
    n, m, h, heads = 24, 19, 8, 2
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    torch.manual_seed(1)
    a_dst, a_src, X = torch.randn(n, heads), torch.randn(m, heads), torch.randn(m, h)
    term = torch.randn(len(col), heads, requires_grad=True)
    out = gat_aggregate(g, a_dst, a_src, X, a_edge=term)
    want = ref_gat_edge(rowptr, col, a_dst.double(), a_src.double(), term.detach().double(), X.double(), 0.2, n)
    assert out.dtype == torch.float32 and torch.allclose(out.double(), want, rtol=1e-5, atol=1e-5)
    out.sum().backward()
    assert term.grad.dtype == torch.float32 and term.grad.shape == term.shape
    Q = torch.randn(n, h)
    out = sparse_attention(g, Q, X, X, heads=heads, bias=term)
    assert out.dtype == torch.float32 and torch.allclose(out.double(), ref_sa_bias(rowptr, col, Q.double(), X.double(), X.double(), term.detach().double(),
                                                                                    heads, n), rtol=1e-5, atol=1e-5)


def test_argument_validation(rng, fake):
    n, m, h, heads = 24, 19, 6, 2
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    nnz = len(col)
    f64 = dict(dtype=torch.float64)
    a_dst, a_src, X, Q = torch.randn(n, heads, **f64), torch.randn(m, heads, **f64), torch.randn(m, h, **f64), torch.randn(n, h, **f64)
    term = torch.randn(nnz, heads, **f64)
    gat = lambda t: gat_aggregate(g, a_dst, a_src, X, a_edge=t)
    sa = lambda t: sparse_attention(g, Q, X, X, heads=heads, bias=t)
    for call, name in ((gat, "gat_aggregate"), (sa, "sparse_attention")):
        with pytest.raises(TypeError, match=name):
            call(term.float())                                  # not the dtype of the other operands
        with pytest.raises(TypeError, match=name):
            call(term.long())                                   # not a floating type
        with pytest.raises(TypeError, match=name):
            call(term.numpy())                                  # not a tensor
        with pytest.raises(ValueError, match=name):
            call(term[:-1])                                     # not one row per stored entry
        with pytest.raises(ValueError, match=name):
            call(term[:, :1])                                   # not one column per head
        with pytest.raises(ValueError, match=name):
            call(term[:, 0])                                    # 1-D is one head only
        with pytest.raises(ValueError, match=name):
            call(term.unsqueeze(-1))
    with pytest.raises(TypeError, match="gat_aggregate"):
        gat_aggregate(g, a_dst.float(), a_src.float(), X.bfloat16(), a_edge=term)   # beside 16-bit features: float32 or that type
    with pytest.raises(TypeError, match="sparse_attention"):
        sparse_attention(g, Q.bfloat16(), X.bfloat16(), X.bfloat16(), heads=heads, bias=term.half())
    with pytest.raises(ValueError, match="gat_aggregate"):
        gat_aggregate(g, a_dst, a_src, X, dropout=1.0, a_edge=term)
    assert fake.calls == []


# ---- the GPU parity cases can fail: on the float64 reference alone

def sensitivity(kind, gname, h, heads):
    """for every row with two or more entries: does leaving the term out / shifting it by one entry move some output of the row (out or
    lse) by more than the bound the GPU test asserts for FLT32 (the wider of its two)?  -> (rows with >= 2 entries, moved by leaving out,
    moved by the shift)"""
    n, m, rowptr, col = er.graph(gname)
    ops = er.as_float64(er.operands(kind, n, m, len(col), h, heads, torch.float32), "cpu")
    base = er.reference(kind, torch.float32, n, rowptr, col, ops, h, heads, "cpu")
    bound, lbound = er.out_bound(kind, torch.float32, base, h, heads), er.lse_bound(kind, torch.float32, base)
    many = torch.from_numpy(np.diff(rowptr.astype(np.int64)) >= 2)
    moved = []
    for other in (None, torch.from_numpy(np.roll(ops["term"].numpy(), 1, 0))):
        r = er.reference(kind, torch.float32, n, rowptr, col, ops, h, heads, "cpu", term=other)
        moved.append((((r["ref"] - base["ref"]).abs() > bound).any(1) | ((r["lse"] - base["lse"]).abs() > lbound).any(1))[many])
    return int(many.sum()), moved[0], moved[1]


@pytest.mark.parametrize("gname", er.GRAPH_NAMES)
def test_the_gat_parity_cases_tell_a_term_that_is_ignored_or_misplaced(gname):
    for h, heads in er.gat_cases():
        rows, left_out, shifted = sensitivity("gat", gname, h, heads)
        assert rows > 0 and left_out.all() and shifted.all(), (gname, h, heads)
    n, m, rowptr, col = er.graph(gname)
    ops = er.operands("gat", n, m, len(col), 32, 4, torch.float32)
    assert ops["term"].abs().max() <= 2 and (ops["A"].abs().max() + ops["B"].abs().max() + 2) <= 8, "|z| <= 8"


@pytest.mark.parametrize("gname", er.GRAPH_NAMES)
def test_the_attention_parity_cases_tell_a_bias_that_is_ignored_or_misplaced(gname):
    for h, heads in er.SA_SHAPES:
        rows, left_out, shifted = sensitivity("sa", gname, h, heads)
        assert rows > 0 and left_out.all() and shifted.all(), (gname, h, heads)
