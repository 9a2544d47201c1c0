"""16-bit features (bfloat16, float16) on CPU: the dtype rules of spmm_values, gat_aggregate, spmm_reduce(mean), autograd.sddmm and the
layers on top of them, driven with a test double of the C ABI that knows PYGIM_FLT16 / PYGIM_BF16 as include/pygim_hip.h states them:
X / G / out are 16-bit, values, a_dst, a_src, lse and the sddmm result are float32.  The double reads every buffer in the type the ABI
gives it, so a wrapper that hands 16-bit values to a float32 argument (or the other way round) produces numbers far from the reference."""
import numpy as np
import pytest
import torch

from fake_abi import NP_OF, PygimError, _view
from pygim_amd import attention, autograd, gnn, pim_ops
from pygim_amd.attention import EdgeGraph, edge_softmax, gat_aggregate, spmm_values
from pygim_amd.reduce import spmm_reduce
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import _rows, multigraph, ref_spmm
from test_gat_fused_cpu import FakeLibG, ref_gat_aggregate
from test_reduce_cpu import MEAN, FakeLibR

FLT16, BF16 = 6, 7
TORCH_OF = {FLT16: torch.float16, BF16: torch.bfloat16}
HALF = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def load16(ptr, rows, ld, width, code):
    """a [rows, width] window of 16-bit elements (row stride ld) as float64"""
    bits = np.ascontiguousarray(_rows(ptr, rows, ld, width, np.uint16))
    if code == BF16:
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float16).astype(np.float64)


def store16(ptr, rows, ld, width, code, values):
    """values (float64) rounded once to the 16-bit type of `code`"""
    rounded = torch.from_numpy(np.ascontiguousarray(values)).to(TORCH_OF[code]).view(torch.int16).numpy()
    _rows(ptr, rows, ld, width, np.int16)[:] = rounded


class FakeLibH(FakeLibG, FakeLibR):
    """the doubles of the attention, fused-GAT and reduce entry points, with the two 16-bit feature codes"""

    def __init__(self):
        super().__init__()
        self.seen = []   # (entry point, dtype code)

    def _csr(self, nrows, rowptr_ptr, col_ptr, nnz):
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        return rowptr, col, np.repeat(np.arange(nrows), np.diff(rowptr))

    def spmm_values_workspace(self, dtype, nrows, nnz, h, heads):
        assert dtype in (self.FLT32, self.DBL64, FLT16, BF16)
        return 64

    def spmm_values(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, heads, x_ptr, ldx, h, out_ptr, ldo, ws_ptr, ws_bytes, stream=0):
        self.seen.append(("spmm_values", dtype))
        if dtype in NP_OF:
            return super().spmm_values(dtype, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, heads, x_ptr, ldx, h, out_ptr, ldo, ws_ptr, ws_bytes, stream)
        self.calls.append("spmm_values")
        rowptr, col, row = self._csr(nrows, rowptr_ptr, col_ptr, nnz)
        acc = np.zeros((nrows, h))
        if nnz:
            val = _view(val_ptr, nnz * heads, np.float32).reshape(nnz, heads).astype(np.float64)   # float32, whatever X is
            X = load16(x_ptr, int(col.max()) + 1, ldx, h, dtype)
            np.add.at(acc, row, np.repeat(val, h // heads, axis=1) * X[col])
        store16(out_ptr, nrows, ldo, h, dtype, acc)

    def sddmm(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, g_ptr, ldg, x_ptr, ldx, h, out_ptr, stream=0):
        self.seen.append(("sddmm", dtype))
        if dtype in NP_OF:
            return super().sddmm(dtype, nrows, rowptr_ptr, col_ptr, nnz, g_ptr, ldg, x_ptr, ldx, h, out_ptr, stream)
        self.calls.append("sddmm")
        rowptr, col, row = self._csr(nrows, rowptr_ptr, col_ptr, nnz)
        G, X = load16(g_ptr, nrows, ldg, h, dtype), load16(x_ptr, int(col.max()) + 1, ldx, h, dtype)
        _view(out_ptr, nnz, np.float32)[:] = np.einsum("ef,ef->e", G[row], X[col]).astype(np.float32)   # float32 out

    def gat_aggregate_workspace(self, dtype, nrows, nnz, h, heads):
        assert dtype in (self.FLT32, self.DBL64, FLT16, BF16)
        return 96

    def gat_aggregate(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr, ldo, lse_ptr,
                      ws_ptr, ws_bytes, stream=0):
        self.seen.append(("gat_aggregate", dtype))
        if dtype in NP_OF:
            return super().gat_aggregate(dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr,
                                         ldo, lse_ptr, ws_ptr, ws_bytes, stream)
        self.calls.append("gat_aggregate")
        rowptr, col, row = self._csr(nrows, rowptr_ptr, col_ptr, nnz)
        acc, lse = np.zeros((nrows, h)), np.zeros((nrows, heads))
        if nnz:
            ncols = int(col.max()) + 1
            a_dst = _view(a_dst_ptr, nrows * heads, np.float32).reshape(nrows, heads).astype(np.float64)   # float32 node terms
            a_src = _view(a_src_ptr, ncols * heads, np.float32).reshape(ncols, heads).astype(np.float64)
            X = load16(x_ptr, ncols, ldx, h, dtype)
            z = a_dst[row] + a_src[col]
            s = np.where(z >= 0, z, negative_slope * z)
            m = np.full((nrows, heads), -np.inf)
            np.maximum.at(m, row, s)
            e = np.exp(s - m[row])
            l = np.zeros((nrows, heads))
            np.add.at(l, row, e)
            np.add.at(acc, row, np.repeat(e / l[row], h // heads, axis=1) * X[col])
            full = np.diff(rowptr) > 0
            lse[full] = m[full] + np.log(l[full])
        store16(out_ptr, nrows, ldo, h, dtype, acc)
        if lse_ptr:
            _view(lse_ptr, nrows * heads, np.float32).reshape(nrows, heads)[:] = lse.astype(np.float32)   # float32 lse

    def spmm_reduce_workspace(self, dtype, op, nrows, nnz, h):
        if dtype in (FLT16, BF16):
            if op != MEAN:
                raise PygimError(1, "bad spmm_reduce_workspace arguments")
            return 48
        return super().spmm_reduce_workspace(dtype, op, nrows, nnz, h)

    def spmm_reduce(self, dtype, op, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, x_ptr, ldx, h, out_ptr, ldo, arg_ptr, ws_ptr, ws_bytes, stream=0):
        self.seen.append(("spmm_reduce", dtype))
        if dtype in NP_OF:
            return super().spmm_reduce(dtype, op, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, x_ptr, ldx, h, out_ptr, ldo, arg_ptr, ws_ptr, ws_bytes, stream)
        self.calls.append("spmm_reduce")
        if op != MEAN or arg_ptr:
            raise PygimError(1, "spmm_reduce: max / min take no 16-bit type")
        rowptr, col, row = self._csr(nrows, rowptr_ptr, col_ptr, nnz)
        acc = np.zeros((nrows, h))
        if nnz:
            val = _view(val_ptr, nnz, np.float32).astype(np.float64) if val_ptr else np.ones(nnz)
            np.add.at(acc, row, val[:, None] * load16(x_ptr, int(col.max()) + 1, ldx, h, dtype)[col])
        store16(out_ptr, nrows, ldo, h, dtype, acc / np.maximum(np.diff(rowptr), 1)[:, None])

    def edge_softmax(self, dtype, *a, **k):
        self.seen.append(("edge_softmax", dtype))
        if dtype not in (self.FLT32, self.DBL64):
            raise PygimError(1, "edge_softmax: type must be FLT32 or DBL64")
        return super().edge_softmax(dtype, *a, **k)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibH()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    pim_ops._variant = None
    pim_ops._groups.clear()


N, M = 24, 19


def make_graph(rng):
    rowptr, col = multigraph(rng, N, M, used_cols=15)
    return rowptr, col, EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (N, M))


def once_rounded(got, want, dtype):
    """got is `want` (float64) rounded once to dtype: half an ulp, and a little for results below the normal range"""
    return bool(torch.all((got.double() - want).abs() <= 1.001 * U[dtype] * want.abs() + 2.0 ** -24))


def test_the_codes_belong_to_the_gather_family_alone():
    assert attention.HALF_CODE == {torch.float16: FLT16, torch.bfloat16: BF16}
    assert not set(attention.HALF_CODE) & set(pim_ops.DTYPE_CODE), "DTYPE_CODE is the list of group types: no 16-bit groups"
    assert attention._compute_dtype(torch.bfloat16) == torch.float32 and attention._compute_dtype(torch.float64) == torch.float64


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("value_in_x_dtype", [False, True])
def test_spmm_values_dtype_rules_and_gradients(rng, fake, dtype, value_in_x_dtype):
    rowptr, col, g = make_graph(rng)
    heads, h = 2, 8
    val = torch.rand(len(col), heads) + 0.5
    if value_in_x_dtype:
        val = val.to(dtype)
    X, G = torch.randn(M, h).to(dtype), torch.randn(N, h).to(dtype)
    v, x = val.clone().requires_grad_(), X.clone().requires_grad_()
    out = spmm_values(g, v, x, heads=heads)
    out.backward(G)
    assert out.dtype == dtype and v.grad.dtype == val.dtype and x.grad.dtype == dtype
    vc, xc = val.double().requires_grad_(), X.double().requires_grad_()
    ref = ref_spmm(rowptr, col, vc, xc, heads, N)
    ref.backward(G.double())
    assert once_rounded(out.detach(), ref.detach(), dtype) and once_rounded(x.grad, xc.grad, dtype)
    if value_in_x_dtype:
        assert once_rounded(v.grad, vc.grad, dtype)
    else:
        assert torch.allclose(v.grad.double(), vc.grad, rtol=1e-6, atol=1e-6), "dvalue is float32 and unrounded"
    code = attention.HALF_CODE[dtype]
    assert set(fake.seen) == {("spmm_values", code), ("sddmm", code)}


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("terms_in_x_dtype", [False, True])
def test_gat_aggregate_dtype_rules_and_gradients(rng, fake, dtype, terms_in_x_dtype):
    rowptr, col, g = make_graph(rng)
    heads, h = 2, 8
    tdt = dtype if terms_in_x_dtype else torch.float32
    a_dst, a_src = torch.randn(N, heads).to(tdt), torch.randn(M, heads).to(tdt)
    X, G = torch.randn(M, h).to(dtype), torch.randn(N, h).to(dtype)
    ops = [t.clone().requires_grad_() for t in (a_dst, a_src, X)]
    out = gat_aggregate(g, *ops, 0.2)
    out.backward(G)
    assert out.dtype == dtype and [t.grad.dtype for t in ops] == [tdt, tdt, dtype]
    ref_ops = [t.double().requires_grad_() for t in (a_dst, a_src, X)]
    ref = ref_gat_aggregate(rowptr, col, *ref_ops, 0.2, N)
    ref.backward(G.double())
    assert once_rounded(out.detach(), ref.detach(), dtype)
    # the recomputed probabilities, delta and ds are float32: the node-term gradients carry float32 errors, not 16-bit ones
    for got, want in zip(ops[:2], ref_ops[:2]):
        if terms_in_x_dtype:
            assert torch.allclose(got.grad.double(), want.grad, rtol=2 * U[dtype], atol=1e-4)
        else:
            assert torch.allclose(got.grad.double(), want.grad, rtol=1e-4, atol=1e-5)
    p_err = 1e-5   # of the float32 probabilities the dX product is made with
    assert torch.all((ops[2].grad.double() - ref_ops[2].grad).abs() <= 1.001 * U[dtype] * ref_ops[2].grad.abs() + p_err * G.double().abs().max() * 16)
    code = attention.HALF_CODE[dtype]
    assert ("gat_aggregate", code) in fake.seen and ("sddmm", code) in fake.seen
    assert ("spmm_values", fake.FLT32) in fake.seen, "the per-head sums of the backward are FLT32 calls on float32 ones"
    with pytest.raises(TypeError):
        gat_aggregate(g, a_dst.float(), a_src.to(dtype), X)       # mixed node terms
    with pytest.raises(TypeError):
        gat_aggregate(g, a_dst.double(), a_src.double(), X)       # float64 beside 16-bit features
    with pytest.raises(TypeError):
        gat_aggregate(g, a_dst.to(dtype), a_src.to(dtype), X.float())   # 16-bit terms beside float32 features


@pytest.mark.parametrize("dtype", HALF)
def test_mean_dtype_rules_and_gradients(rng, fake, dtype):
    rowptr, col, g = make_graph(rng)
    h = 8
    cnt = torch.from_numpy(np.maximum(np.diff(rowptr), 1)).double().unsqueeze(1)
    X, G = torch.randn(M, h).to(dtype), torch.randn(N, h).to(dtype)
    for val in (None, torch.rand(len(col)) + 0.5, (torch.rand(len(col)) + 0.5).to(dtype)):
        v = None if val is None else val.clone().requires_grad_()
        x = X.clone().requires_grad_()
        out = spmm_reduce(g, x, "mean", value=v)
        out.backward(G)
        vc = torch.ones(len(col), dtype=torch.float64) if val is None else val.double()
        vc, xc = vc.requires_grad_(), X.double().requires_grad_()
        ref = ref_spmm(rowptr, col, vc, xc, 1, N) / cnt
        ref.backward(G.double())
        assert out.dtype == dtype and x.grad.dtype == dtype
        assert once_rounded(out.detach(), ref.detach(), dtype) and once_rounded(x.grad, xc.grad, dtype)
        if val is not None:
            assert v.grad.dtype == val.dtype
            if val.dtype == torch.float32:
                assert torch.allclose(v.grad.double(), vc.grad, rtol=1e-6, atol=1e-6), "G / count must not be rounded to 16 bits on the way"
    code = attention.HALF_CODE[dtype]
    assert set(fake.seen) == {("spmm_reduce", code), ("spmm_values", code), ("sddmm", code)}


def test_sddmm_returns_float32(rng, fake):
    rowptr, col, g = make_graph(rng)
    for dtype in HALF:
        G, X = torch.randn(N, 8).to(dtype), torch.randn(M, 8).to(dtype)
        out = autograd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(col), G, X)
        want = (G.double()[g.row.long()] * X.double()[g.col.long()]).sum(1)
        assert out.dtype == torch.float32 and torch.allclose(out.double(), want, rtol=1e-6, atol=1e-6)
    with pytest.raises(TypeError):
        autograd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(col), G.float(), X)


def test_the_old_rejections_still_raise(rng, fake):
    rowptr, col, g = make_graph(rng)
    nnz = len(col)
    v, X = torch.rand(nnz, dtype=torch.float64), torch.randn(M, 6, dtype=torch.float64)
    with pytest.raises(TypeError):
        spmm_values(g, v.int(), X.int())                          # integer X
    with pytest.raises(TypeError):
        spmm_values(g, v.float(), X)                              # float32 value beside float64 X
    with pytest.raises(TypeError):
        spmm_values(g, v.bfloat16(), X.float())                   # 16-bit value beside float32 X
    with pytest.raises(TypeError):
        spmm_values(g, v, X.bfloat16())                           # float64 value beside 16-bit X
    with pytest.raises(TypeError):
        spmm_values(g, v.half(), X.bfloat16())                    # the other 16-bit type
    for dtype in HALF:
        with pytest.raises(TypeError):
            spmm_reduce(g, X.to(dtype), "max")
        with pytest.raises(TypeError):
            spmm_reduce(g, X.to(dtype), "min", return_arg=True)
        with pytest.raises(TypeError):
            spmm_reduce(g, X.to(dtype), "mean", value=v)           # float64 value beside 16-bit X
        with pytest.raises(TypeError):
            edge_softmax(g, v.to(dtype))
    with pytest.raises(TypeError):
        spmm_reduce(g, X.int(), "mean")
    assert fake.seen == []


def square(rng):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    return n, SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))


@pytest.mark.parametrize("mode", ["to", "autocast"])
@pytest.mark.parametrize("layer", ["gat-fused", "gat", "sage-mean"])
def test_layers_in_bfloat16(rng, fake, layer, mode):
    n, adj = square(rng)
    torch.manual_seed(2)
    conv = gnn.SAGEConv(7, 8, aggr="mean") if layer == "sage-mean" else gnn.GATConv(7, 4, heads=2, fused=layer == "gat-fused")
    x = torch.randn(n, 7)
    if mode == "to":
        conv, x = conv.to(torch.bfloat16), x.to(torch.bfloat16)
        out = conv(x.requires_grad_(), adj)
        assert out.dtype == torch.bfloat16
    else:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = conv(x.requires_grad_(), adj)
    out.float().square().mean().backward()
    assert out.shape == (n, 8) and torch.isfinite(out).all() and x.grad.dtype == x.dtype and torch.isfinite(x.grad).all()
    for p in conv.parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and torch.isfinite(p.grad).all()
    if layer == "gat":   # 16-bit scores go up to float32 before the softmax; the product takes float32 probabilities beside bfloat16 features
        assert ("edge_softmax", fake.FLT32) in fake.seen and ("spmm_values", BF16) in fake.seen
    elif layer == "gat-fused":
        assert ("gat_aggregate", BF16) in fake.seen
    elif mode == "to":
        assert ("spmm_reduce", BF16) in fake.seen
