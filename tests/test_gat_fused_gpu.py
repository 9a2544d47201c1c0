"""The fused GAT aggregation on the GPU: pygim_gat_aggregate through the C ABI against float64 on the device, and
pygim_amd.gat_aggregate / gnn.GATConv(fused=True) (autograd, training) against the per-entry CPU reference.

Bound: |out - ref| <= TOL * sum_e p_ref[e] * |x[e]| with TOL = 2e-5 (FLT32) / 2e-12 (DBL64): the two contracts of the unfused path
added -- 1e-5 relative on each probability (pygim_edge_softmax) and 1e-5 of the magnitude sum (pygim_spmm_values); with |z| <= 8 the
rounding of a float32 score adds under 5e-7.  lse within TOL * (1 + |lse|)."""
import copy

import numpy as np
import pytest
import torch

from conftest import random_csr
from pygim_amd import _lib, gnn, pim_ops
from pygim_amd.attention import EdgeGraph, gat_aggregate
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import gat_reference
from test_attention_gpu import GRAPHS, dev_csr, hub_graph, small_graph
from test_gat_fused_cpu import ref_gat_aggregate

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.float64: 2e-12}
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def call_gat(dtype, n, rp, cc, a_dst, a_src, heads, slope, X, h, out=None, want_lse=True):
    """X: [rows, ldx] device tensor whose first h columns are the operand; -> (out, lse or None), both filled with NaN before the call"""
    code = pim_ops.DTYPE_CODE[dtype]
    nnz = cc.numel()
    ws = torch.empty(max(_lib.gat_aggregate_workspace(code, n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((n, heads), float("nan"), dtype=dtype, device=DEV) if want_lse else None
    _lib.gat_aggregate(code, n, rp.data_ptr(), cc.data_ptr(), nnz, a_dst.data_ptr(), a_src.data_ptr(), heads, slope, X.data_ptr(), X.stride(0), h,
                       out.data_ptr(), out.stride(0), lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, lse


def gat_reference_dev(n, rowptr, col, a_dst, a_src, heads, slope, X, h):
    """float64 on the device: (exact out, sum_e p * |x| per output, lse with 0 for empty rows, the row of every entry, its column)"""
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(torch.from_numpy(rowptr).long().to(DEV)))
    cc = torch.from_numpy(col).long().to(DEV)
    z = a_dst.double()[row] + a_src.double()[cc]
    s = torch.where(z >= 0, z, slope * z)
    m = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - m[row])
    l = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, e)
    msg = (e / l[row]).repeat_interleave(h // heads, dim=1) * X[:, :h].double()[cc]
    ref = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg)
    mag = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg.abs())
    lse = torch.where(l > 0, m + torch.log(l), torch.zeros_like(l))
    return ref, mag, lse, row, cc


def check_against_reference(tag, dtype, n, rowptr, col, rp, cc, a_dst, a_src, heads, slope, X, h):
    out, lse = call_gat(dtype, n, rp, cc, a_dst, a_src, heads, slope, X, h)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), "a row was not written"
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert (out[empty] == 0).all() and (lse[empty] == 0).all()
    ref, mag, lse_ref, row, col_l = gat_reference_dev(n, rowptr, col, a_dst, a_src, heads, slope, X, h)
    err = (out.double() - ref).abs()
    lerr = (lse.double() - lse_ref).abs()
    lbound = TOL[dtype] * (1 + lse_ref.abs())
    print(f"gat_aggregate {tag}: max err / bound = {(err / (TOL[dtype] * mag).clamp_min(1e-300)).max().item():.3e}, "
          f"lse max err / bound = {(lerr / lbound).max().item():.3e}")
    assert torch.all(err <= TOL[dtype] * mag)
    assert torch.all(lerr <= lbound)
    out2, lse2 = call_gat(dtype, n, rp, cc, a_dst, a_src, heads, slope, X, h)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "two launches differ"
    return out, ref, mag, row, col_l


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", [1, 9, 32, 100, 256, 300, 512])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_gat_aggregate_parity(rng, dtype, h, graph):
    """h = 1, 9, 32, 100: lane groups; 256: the whole wave (FLT32, 16-byte pieces); 512: two pieces per lane (and two blockIdx.y chunks
    in DBL64); 300 with the misaligned stride: 300 one-element pieces, three blockIdx.y chunks, the last one partly empty"""
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    for heads in [k for k in (1, 4, 8) if h % k == 0]:
        a_dst = torch.from_numpy(rng.uniform(-4, 4, size=(n, heads))).to(DEV, dtype)
        a_src = torch.from_numpy(rng.uniform(-4, 4, size=(m, heads))).to(DEV, dtype)
        # a contiguous X, a wider row stride that keeps 16-byte alignment, and one that breaks it
        for ldx in ((h, h + 2 * vec, h + 1) if graph == "small" else (h,)):
            X = torch.from_numpy(rng.uniform(-1, 1, size=(m, ldx))).to(DEV, dtype)
            check_against_reference(f"{graph} {dtype} h={h} heads={heads} ldx={ldx}", dtype, n, rowptr, col, rp, cc, a_dst, a_src, heads, 0.2, X, h)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gat_aggregate_is_stable_for_large_scores(rng, dtype):
    """integer-valued node terms in [-5000, 5000] and slope 0.25: every float32 score and difference is exact, only exp and the sums
    round.  The output is finite, meets the same bound, and is a convex combination of the row's gathered x within that bound."""
    n, m, rowptr, col = hub_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h, heads = 64, 4
    a_dst = torch.from_numpy(rng.integers(-5000, 5001, size=(n, heads))).to(DEV, dtype)
    a_src = torch.from_numpy(rng.integers(-5000, 5001, size=(m, heads))).to(DEV, dtype)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(DEV, dtype)
    out, ref, mag, row, col_l = check_against_reference(f"large scores {dtype}", dtype, n, rowptr, col, rp, cc, a_dst, a_src, heads, 0.25, X, h)
    assert torch.isfinite(out).all()
    xg = X.double()[col_l]
    lo = torch.full((n, h), float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, xg, "amin", include_self=True)
    hi = torch.full((n, h), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, xg, "amax", include_self=True)
    full = torch.from_numpy(np.diff(rowptr) > 0).to(DEV)
    bound = TOL[dtype] * mag
    assert torch.all(out.double()[full] >= (lo - bound)[full]) and torch.all(out.double()[full] <= (hi + bound)[full])


def test_gat_aggregate_strided_out_no_lse_nnz0_and_bad_arguments(rng):
    n, m, rowptr, col = small_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h, heads = 32, 4
    a_dst = torch.from_numpy(rng.uniform(-4, 4, size=(n, heads))).to(DEV, torch.float32)
    a_src = torch.from_numpy(rng.uniform(-4, 4, size=(m, heads))).to(DEV, torch.float32)
    X = torch.randn(m, h, device=DEV)
    wide = torch.full((n, h + 5), float("nan"), device=DEV)
    call_gat(torch.float32, n, rp, cc, a_dst, a_src, heads, 0.2, X, h, out=wide)
    ref, mag, _, _, _ = gat_reference_dev(n, rowptr, col, a_dst, a_src, heads, 0.2, X, h)
    assert torch.all((wide[:, :h].double() - ref).abs() <= 2e-5 * mag) and torch.isnan(wide[:, h:]).all(), "stores outside out[:, :h]"
    # out does not depend on whether lse is asked for
    with_lse, _ = call_gat(torch.float32, n, rp, cc, a_dst, a_src, heads, 0.2, X, h)
    without, none = call_gat(torch.float32, n, rp, cc, a_dst, a_src, heads, 0.2, X, h, want_lse=False)
    assert none is None and torch.equal(with_lse, without)
    # nnz = 0: every row is empty, out and lse are zero
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    out, lse = call_gat(torch.float32, n, rp0, cc[:0], a_dst, a_src, heads, 0.2, X, h)
    assert (out == 0).all() and (lse == 0).all()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    o = torch.empty(n, h, device=DEV)
    args = (n, rp.data_ptr(), cc.data_ptr(), len(col), a_dst.data_ptr(), a_src.data_ptr())
    with pytest.raises(_lib.PygimError):   # integer types have no such aggregation
        _lib.gat_aggregate(_lib.INT32, *args, heads, 0.2, X.data_ptr(), h, h, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # heads must divide h
        _lib.gat_aggregate(_lib.FLT32, *args, 5, 0.2, X.data_ptr(), h, h, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # a workspace smaller than pygim_gat_aggregate_workspace says
        _lib.gat_aggregate(_lib.FLT32, *args, heads, 0.2, X.data_ptr(), h, h, o.data_ptr(), h, 0, ws.data_ptr(), 16)
    with pytest.raises(_lib.PygimError):   # ... or misaligned
        _lib.gat_aggregate(_lib.FLT32, *args, heads, 0.2, X.data_ptr(), h, h, o.data_ptr(), h, 0, ws.data_ptr() + 4, ws.numel() - 4)
    with pytest.raises(_lib.PygimError):
        _lib.gat_aggregate_workspace(_lib.FLT32, n, len(col), h, 5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_autograd_on_device_matches_the_cpu_reference(rng, dtype):
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert g.rowptr.is_cuda
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-11)
    heads, h = 4, 32
    a_dst, a_src = torch.randn(n, heads, dtype=dtype), torch.randn(m, heads, dtype=dtype)
    X = torch.randn(m, h, dtype=dtype)
    G = torch.randn(n, h, dtype=dtype)
    dev = [t.to(DEV).requires_grad_() for t in (a_dst, a_src, X)]
    out = gat_aggregate(g, *dev, 0.2)
    assert out.is_cuda
    out.backward(G.to(DEV))
    cpu = [t.double().requires_grad_() for t in (a_dst, a_src, X)]
    ref = ref_gat_aggregate(rowptr, col, *cpu, 0.2, n)
    ref.backward(G.double())
    assert torch.allclose(out.detach().cpu().double(), ref.detach(), **tol)
    for name, d, c in zip(("a_dst", "a_src", "X"), dev, cpu):
        print(f"gat_aggregate autograd {dtype} d{name}: max abs err = {(d.grad.cpu().double() - c.grad).abs().max().item():.3e}")
        assert torch.allclose(d.grad.cpu().double(), c.grad, **tol), name
    # CPU tensors are staged to the device and come home
    out_host = gat_aggregate(g, a_dst, a_src, X, 0.2)
    assert not out_host.is_cuda and torch.equal(out_host, out.detach().cpu())


def test_fused_gat_sgd_steps_match_the_cpu_reference(rng):
    """test_attention_gpu.test_gat_sgd_steps_match_the_cpu_reference with fused=True: a 2-layer GAT, 4 SGD steps in float64, losses and
    parameter gradients as with the per-entry plain-torch layer on the CPU; then one float32 forward, fused against unfused"""
    n, f_in, hid, f_out, heads = 1500, 16, 32, 8, 4
    rowptr, col = random_csr(rng, n, n, 9)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.GAT(f_in, hid, f_out, num_layers=2, dropout=0.0, heads=heads, fused=True).double()

    def run(model, dev):
        model = model.to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        losses, grads = [], []
        for _ in range(4):
            opt.zero_grad()
            loss = ((model(feats.to(dev), adj) - target.to(dev)) ** 2).mean()
            loss.backward()
            losses.append(loss.item())
            grads.append([p.grad.cpu().clone() for p in model.parameters()])
            opt.step()
        return losses, grads

    cpu_model = copy.deepcopy(base)
    for conv in cpu_model.convs:
        conv.forward = (lambda c: lambda x, adj_t: gat_reference(c, x, rowptr, col, n))(conv)
    l_gpu, g_gpu = run(copy.deepcopy(base), DEV)
    l_cpu, g_cpu = run(cpu_model, "cpu")
    assert np.allclose(l_gpu, l_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_gpu, g_cpu):
        for x, y in zip(a, b):
            assert torch.allclose(x, y, rtol=1e-9, atol=1e-11)
    fused = copy.deepcopy(base).float().to(DEV).eval()
    plain = copy.deepcopy(fused)
    for conv in plain.convs:
        conv.fused = False
    with torch.no_grad():
        a, b = fused(feats.float().to(DEV), adj), plain(feats.float().to(DEV), adj)
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)
