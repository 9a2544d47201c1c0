"""The GATv2 aggregation on CPU: pygim_amd.gatv2_aggregate, gnn.GATv2Conv and gnn.GATv2 driven with the C-ABI test double of
test_sparse_attention_cpu.py, extended here with numpy float64 statements of pygim_gatv2_aggregate, pygim_gatv2_backward and their
workspace functions (heads wider than 256 features rejected, as the library rejects them)."""
import copy

import numpy as np
import pytest
import torch

import pygim_amd
from conftest import random_csr
from fake_abi import NP_OF, PygimError, _view
from pygim_amd import gnn, pim_ops
from pygim_amd.attention import gatv2_aggregate
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import _rows, graph_of, multigraph
from test_sparse_attention_cpu import FakeLibS


class FakeLibV2(FakeLibS):
    """FakeLibS with the four entry points of the GATv2 aggregation"""

    def _gatv2_check(self, h, heads):
        if h < 1 or heads < 1 or h % heads != 0 or h // heads > 256:
            raise PygimError(1, "gatv2: heads must divide h and a head is at most 256 features wide")

    def gatv2_aggregate_workspace(self, dtype, nrows, nnz, h, heads):
        self._gatv2_check(h, heads)
        return 128

    def gatv2_backward_workspace(self, dtype, nrows, nnz, h, heads):
        self._gatv2_check(h, heads)
        return 144

    @staticmethod
    def _scores(xd, xs, att, r, c, heads, slope):
        """z, leaky_relu(z) [nnz, h] and the scores [nnz, heads] of the entries (r, c)"""
        z = xd[r] + xs[c]
        lz = np.where(z > 0, z, slope * z)
        return z, lz, (lz * att).reshape(len(r), heads, -1).sum(-1)

    def gatv2_aggregate(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, xd_ptr, ld_dst, xs_ptr, ld_src, att_ptr, h, heads, negative_slope, out_ptr, ldo,
                        lse_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("gatv2_aggregate")
        self._gatv2_check(h, heads)
        assert ws_bytes >= 128
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
            xd = _rows(xd_ptr, nrows, ld_dst, h, npdt).astype(np.float64)
            xs = _rows(xs_ptr, ncols, ld_src, h, npdt).astype(np.float64)
            att = _view(att_ptr, h, npdt).astype(np.float64)
            _, _, s = self._scores(xd, xs, att, row, col, heads, negative_slope)
            m = np.full((nrows, heads), -np.inf)
            np.maximum.at(m, row, s)
            e = np.exp(s - m[row])
            l = np.zeros((nrows, heads))
            np.add.at(l, row, e)
            np.add.at(acc, row, np.repeat(e / l[row], hd, axis=1) * xs[col])
            full = np.diff(rowptr) > 0
            lse[full] = m[full] + np.log(l[full])
        out[:] = acc.astype(npdt)
        if lse_ptr:
            _view(lse_ptr, nrows * heads, npdt).reshape(nrows, heads)[:] = lse.astype(npdt)

    def gatv2_backward(self, dtype, transposed, nrows, rowptr_ptr, col_ptr, nnz, own_ptr, ld_own, oth_ptr, ld_oth, att_ptr, h, heads, negative_slope,
                       g_ptr, ldg, lse_ptr, delta_ptr, d_own_ptr, ldd, datt_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("gatv2_backward")
        self._gatv2_check(h, heads)
        if transposed and datt_ptr:
            raise PygimError(1, "gatv2_backward: datt belongs to the call on the CSR of A")
        assert ws_bytes >= 144
        npdt = NP_OF[dtype]
        hd = h // heads
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        d_own = np.zeros((nrows, h))
        datt = np.zeros(h)
        if nnz:
            i = np.repeat(np.arange(nrows), np.diff(rowptr))
            noth = int(col.max()) + 1
            own = _rows(own_ptr, nrows, ld_own, h, npdt).astype(np.float64)
            oth = _rows(oth_ptr, noth, ld_oth, h, npdt).astype(np.float64)
            att = _view(att_ptr, h, npdt).astype(np.float64)
            r, c, xd, xs, na = (col, i, oth, own, noth) if transposed else (i, col, own, oth, nrows)   # the rows and columns of A
            G = _rows(g_ptr, na, ldg, h, npdt).astype(np.float64)
            lse = _view(lse_ptr, na * heads, npdt).reshape(na, heads).astype(np.float64)
            delta = _view(delta_ptr, na * heads, npdt).reshape(na, heads).astype(np.float64)
            z, lz, s = self._scores(xd, xs, att, r, c, heads, negative_slope)
            p = np.exp(s - lse[r])
            dp = (G[r] * xs[c]).reshape(nnz, heads, hd).sum(-1)
            ds = np.repeat(p * (dp - delta[r]), hd, axis=1)
            t = ds * att * np.where(z > 0, 1.0, negative_slope)
            if transposed:
                np.add.at(d_own, c, np.repeat(p, hd, axis=1) * G[r] + t)
            else:
                np.add.at(d_own, r, t)
                datt = (ds * lz).sum(0)
        _rows(d_own_ptr, nrows, ldd, h, npdt)[:] = d_own.astype(npdt)
        if datt_ptr:
            _view(datt_ptr, h, npdt)[:] = datt.astype(npdt)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibV2()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    pim_ops._variant = None
    pim_ops._groups.clear()


def ref_gatv2(rowptr, col, x_dst, x_src, att, heads, n, slope=0.2):
    """per-entry reference in plain torch (differentiable); torch's leaky_relu, so its convention at z == 0"""
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    h = x_src.size(1)
    hd = h // heads
    z = x_dst[row] + x_src[cc]
    s = (torch.nn.functional.leaky_relu(z, slope) * att.reshape(1, h)).view(-1, heads, hd).sum(-1)
    m = torch.full((n, heads), -float("inf"), dtype=s.dtype).index_reduce_(0, row, s.detach(), "amax", include_self=True)
    e = torch.exp(s - m[row])
    p = e / torch.zeros(n, heads, dtype=s.dtype).index_add(0, row, e)[row]
    return torch.zeros(n, h, dtype=s.dtype).index_add(0, row, p.repeat_interleave(hd, dim=1) * x_src[cc])


def gatv2_reference(conv, x, rowptr, col, n):
    """PyG's GATv2Conv arithmetic (no self loops, no edge features) per stored entry in plain torch"""
    H, Fo = conv.heads, conv.out_channels
    x_l, x_r = conv.lin_l(x), conv.lin_r(x)
    out = ref_gatv2(rowptr, col, x_r, x_l, conv.att, H, n, conv.negative_slope)
    if not conv.concat:
        out = out.view(n, H, Fo).mean(1)
    return out if conv.bias is None else out + conv.bias


def test_public_names():
    assert pygim_amd.gatv2_aggregate is gatv2_aggregate
    assert hasattr(gnn, "GATv2Conv") and hasattr(gnn, "GATv2")
    assert hasattr(pygim_amd.attention, "GatV2Aggregate")
    for name in ("pygim_gatv2_aggregate", "pygim_gatv2_aggregate_workspace", "pygim_gatv2_backward", "pygim_gatv2_backward_workspace"):
        assert name in pygim_amd._lib.EXPORTS


def operands(rowptr, col, n, m, h, min_gap=0.0):
    """x_dst, x_src, att in float64.  min_gap > 0: every z[e, f] = x_dst[row(e), f] + x_src[col[e], f] is at least that far from 0, the kink
    of leaky_relu -- seeds are tried in order until one gives such operands (each of the few hundred z misses a band of 2e-3 with
    probability 0.9994, so one of the first seeds does)"""
    row, cc = torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))).long(), torch.from_numpy(col).long()
    for seed in range(5, 200):
        gen = torch.Generator().manual_seed(seed)
        xd, xs = torch.randn(n, h, dtype=torch.float64, generator=gen) * 1.5, torch.randn(m, h, dtype=torch.float64, generator=gen) * 1.5
        att = torch.randn(h, dtype=torch.float64, generator=gen)
        if min_gap == 0.0 or (xd[row] + xs[cc]).abs().min() >= min_gap:
            return [xd, xs, att]
    raise AssertionError("no seed keeps z away from 0")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
def test_forward_and_gradients_match_the_per_entry_reference(rng, fake, heads, fused):
    """a multigraph with empty rows and an empty trailing column range; att as [h] and as [heads, hd].  gradcheck compares with finite
    differences of step 1e-6, which are wrong across the kink of leaky_relu: its operands keep every z at least 1e-3 from 0 (operands())"""
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m, used_cols=15)
    g = graph_of(rowptr, col, n, m)
    xd, xs, att = (t.requires_grad_() for t in operands(rowptr, col, n, m, h))
    G = torch.randn(n, h, dtype=torch.float64)
    for slope, shape in ((0.2, (h,)), (0.35, (heads, h // heads))):
        out = gatv2_aggregate(g, xd, xs, att.view(shape), heads=heads, negative_slope=slope, fused=fused)
        want = ref_gatv2(rowptr, col, xd, xs, att, heads, n, slope)
        assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
        assert (out[np.diff(rowptr) == 0] == 0).all()
        out.backward(G)
        got = [t.grad.clone() for t in (xd, xs, att)]
        for t in (xd, xs, att):
            t.grad = None
        want.backward(G)
        for a, t in zip(got, (xd, xs, att)):
            assert a.dtype == t.dtype and a.shape == t.shape and torch.allclose(a, t.grad, rtol=1e-9, atol=1e-11)
            t.grad = None
    assert (got[1][15:] == 0).all(), "columns without entries get zero gradient rows"
    away = [t.requires_grad_() for t in operands(rowptr, col, n, m, h, min_gap=1e-3)]
    assert torch.autograd.gradcheck(lambda a, b, c: gatv2_aggregate(g, a, b, c, heads=heads, fused=fused), away)
    if fused:
        assert set(fake.calls) == {"gatv2_aggregate", "gatv2_backward"}
    else:
        assert "gatv2_aggregate" not in fake.calls and "gatv2_backward" not in fake.calls
        assert {"edge_softmax", "edge_softmax_backward", "spmm_values"} <= set(fake.calls)


def test_the_fused_path_is_one_forward_and_at_most_two_backward_calls(rng, fake):
    n, m, h, heads = 24, 19, 8, 2
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    xd, xs, att = operands(rowptr, col, n, m, h)
    out = gatv2_aggregate(g, xd, xs, att, heads=heads)
    assert fake.calls == ["gatv2_aggregate"]
    leaves = [t.clone().requires_grad_() for t in (xd, xs, att)]
    gatv2_aggregate(g, *leaves, heads=heads).sum().backward()
    assert fake.calls == ["gatv2_aggregate"] * 2 + ["gatv2_backward"] * 2, "no sddmm, no spmm_values, no edge_softmax"
    assert all(t.grad is not None for t in leaves)
    # only x_dst and att need a gradient: the row-side call alone
    fake.calls.clear()
    a, c = xd.clone().requires_grad_(), att.clone().requires_grad_()
    gatv2_aggregate(g, a, xs, c, heads=heads).sum().backward()
    assert fake.calls == ["gatv2_aggregate", "gatv2_backward"]
    assert torch.allclose(a.grad, leaves[0].grad) and torch.allclose(c.grad, leaves[2].grad)
    # only x_src: the transposed call alone
    fake.calls.clear()
    b = xs.clone().requires_grad_()
    gatv2_aggregate(g, xd, b, att, heads=heads).sum().backward()
    assert fake.calls == ["gatv2_aggregate", "gatv2_backward"] and torch.allclose(b.grad, leaves[1].grad)
    # float32 works and agrees with the composition
    fake.calls.clear()
    o32 = gatv2_aggregate(g, xd.float(), xs.float(), att.float(), heads=heads)
    assert o32.dtype == torch.float32 and torch.allclose(o32.double(), out, rtol=1e-5, atol=1e-6)
    u32 = gatv2_aggregate(g, xd.float(), xs.float(), att.float(), heads=heads, fused=False)
    assert torch.allclose(u32, o32, rtol=1e-5, atol=1e-6)
    assert fake.calls == ["gatv2_aggregate", "edge_softmax", "spmm_values"]


def test_lse_is_requested_only_when_a_gradient_is_needed(rng, fake, monkeypatch):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    asked = []
    inner = fake.gatv2_aggregate

    def spy(*a, **k):
        asked.append(bool(a[15]))   # lse_ptr
        return inner(*a, **k)

    monkeypatch.setattr(fake, "gatv2_aggregate", spy)
    xd, xs, att = operands(rowptr, col, n, m, 4)
    gatv2_aggregate(g, xd, xs, att, heads=2)
    gatv2_aggregate(g, xd, xs, att.clone().requires_grad_(), heads=2)
    assert asked == [False, True]


def test_nothing_of_size_nnz_is_saved_for_the_backward(rng, fake):
    n, m, h, heads = 12, 12, 6, 2
    rowptr, col = random_csr(rng, n, m, 90, empty_frac=0.1)
    nnz = len(col)
    assert nnz > n * h
    g = graph_of(rowptr, col, n, m)
    leaves = [t.requires_grad_() for t in operands(rowptr, col, n, m, h)]

    def largest_saved(fused):
        sizes = []

        def pack(t):
            sizes.append(t.numel())
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = gatv2_aggregate(g, *leaves, heads=heads, fused=fused)
        out.sum().backward()
        return max(sizes)

    assert largest_saved(True) < nnz
    assert largest_saved(False) >= nnz * h


def test_heads_wider_than_256_run_unfused(rng, fake):
    """hd = 300: the library rejects it (so does the double), the wrapper takes the composition without saying so; hd = 256 is fused"""
    n, m = 12, 10
    rowptr, col = multigraph(rng, n, m, deg=3)
    g = graph_of(rowptr, col, n, m)
    for ws in (fake.gatv2_aggregate_workspace, fake.gatv2_backward_workspace):
        with pytest.raises(PygimError):
            ws(5, n, len(col), 600, 2)
        assert ws(5, n, len(col), 512, 2) > 0
    with pytest.raises(PygimError):
        fake.gatv2_aggregate(5, n, 0, 0, 0, 0, 600, 0, 600, 0, 600, 2, 0.2, 0, 600, 0, 0, 1 << 20)
    with pytest.raises(PygimError):
        fake.gatv2_backward(5, 0, n, 0, 0, 0, 0, 600, 0, 600, 0, 600, 2, 0.2, 0, 600, 0, 0, 0, 600, 0, 0, 1 << 20)
    fake.calls.clear()
    xd, xs, att = (t.mul_(0.3).requires_grad_() for t in operands(rowptr, col, n, m, 600))
    out = gatv2_aggregate(g, xd, xs, att, heads=2)
    assert "gatv2_aggregate" not in fake.calls and "edge_softmax" in fake.calls
    want = ref_gatv2(rowptr, col, xd, xs, att, 2, n)
    assert torch.allclose(out, want, rtol=1e-11, atol=1e-12)
    G = torch.randn(n, 600, dtype=torch.float64)
    out.backward(G)
    got = [t.grad.clone() for t in (xd, xs, att)]
    for t in (xd, xs, att):
        t.grad = None
    want.backward(G)
    for a, t in zip(got, (xd, xs, att)):
        assert torch.allclose(a, t.grad, rtol=1e-9, atol=1e-11)
    fake.calls.clear()
    gatv2_aggregate(g, xd.detach()[:, :512], xs.detach()[:, :512], att.detach()[:512], heads=2)
    assert fake.calls == ["gatv2_aggregate"]


def test_argument_validation(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = graph_of(rowptr, col, n, m)
    xd, xs, att = operands(rowptr, col, n, m, 6)
    with pytest.raises(TypeError):
        gatv2_aggregate(g, xd.float(), xs, att)                          # dtype mismatch
    with pytest.raises(TypeError):
        gatv2_aggregate(g, xd, xs, att.float())                          # float32 att beside float64 features
    with pytest.raises(TypeError):
        gatv2_aggregate(g, xd.int(), xs.int(), att.int())                # not a float type
    with pytest.raises(TypeError):
        gatv2_aggregate(g, xd.bfloat16(), xs.half(), att.float())        # two 16-bit types
    with pytest.raises(TypeError):
        gatv2_aggregate(g, xd.bfloat16(), xs.bfloat16(), att.half())     # att neither float32 nor the feature type
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd[:-1], xs, att)                             # x_dst does not cover the rows
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd, xs[:-1], att)                             # x_src does not cover the columns
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd, xs[:, :-1], att)                          # x_src has another width
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd[:, 0], xs[:, 0], att[:1])                  # 1-D
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd, xs, att[:-1])                             # att too short
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd, xs, att.view(3, 2), heads=2)              # att [3, 2] beside heads = 2
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd, xs, att, heads=4)                         # 6 % 4 != 0
    with pytest.raises(ValueError):
        gatv2_aggregate(g, xd, xs, att, heads=0)
    assert fake.calls == []


def layer_case(rng, n=22):
    rowptr, col = multigraph(rng, n, n)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    return n, rowptr, col, adj


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("heads,concat,share", [(1, True, False), (3, True, False), (2, False, False), (2, True, True), (2, False, True)])
def test_gatv2conv_matches_per_entry_reference(rng, fake, heads, concat, share, fused):
    """concat and mean over heads; share_weights: lin_r is lin_l, one parameter set, and its gradient is the sum of both sides'"""
    n, rowptr, col, adj = layer_case(rng)
    torch.manual_seed(3)
    conv = gnn.GATv2Conv(7, 4, heads=heads, concat=concat, share_weights=share, fused=fused).double()
    assert (conv.lin_r is conv.lin_l) == share and tuple(conv.att.shape) == (heads, 4)
    assert len(list(conv.parameters())) == (4 if share else 6)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 7, dtype=torch.float64, requires_grad=True)
    G = torch.randn(n, 4 * heads if concat else 4, dtype=torch.float64)
    out = conv(x, adj)
    assert out.shape == G.shape
    if fused:
        assert fake.calls == ["gatv2_aggregate"], "the fused forward is one call"
    out.backward(G)
    if fused:
        assert fake.calls == ["gatv2_aggregate", "gatv2_backward", "gatv2_backward"]
    got = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    want_out = gatv2_reference(conv, x, rowptr, col, n)
    want_out.backward(G)
    want = [x.grad] + [p.grad for p in conv.parameters()]
    assert torch.allclose(out, want_out, rtol=1e-10, atol=1e-12)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)


def test_gatv2conv_without_bias(fake):
    conv = gnn.GATv2Conv(5, 3, heads=2, bias=False)
    assert conv.bias is None and conv.lin_l.bias is None and conv.lin_r.bias is None and conv.fused


@pytest.mark.parametrize("fused", [True, False])
def test_gatv2_stack_sgd_steps_match_the_reference_layer(rng, fake, fused):
    """a 2-layer GATv2, 4 SGD steps in float64: losses and parameter gradients as with the per-entry plain-torch layer"""
    n, rowptr, col, adj = layer_case(rng)
    torch.manual_seed(0)
    base = gnn.GATv2(5, 8, 3, num_layers=2, dropout=0.0, heads=2, fused=fused).double()
    assert all(isinstance(c, gnn.GATv2Conv) and c.fused is fused for c in base.convs)
    x, y = torch.randn(n, 5, dtype=torch.float64), torch.randn(n, 3, dtype=torch.float64)

    def run(model):
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        losses, grads = [], []
        for _ in range(4):
            opt.zero_grad()
            loss = ((model(x, adj) - y) ** 2).mean()
            loss.backward()
            losses.append(loss.item())
            grads.append([p.grad.clone() for p in model.parameters()])
            opt.step()
        return losses, grads

    ref_model = copy.deepcopy(base)
    for conv in ref_model.convs:
        conv.forward = (lambda c: lambda x_, adj_t: gatv2_reference(c, x_, rowptr, col, n))(conv)
    l_got, g_got = run(copy.deepcopy(base))
    l_ref, g_ref = run(ref_model)
    assert np.allclose(l_got, l_ref, rtol=1e-10, atol=1e-12) and l_got[-1] < l_got[0]
    for a, b in zip(g_got, g_ref):
        for p, q in zip(a, b):
            assert torch.allclose(p, q, rtol=1e-9, atol=1e-11)
