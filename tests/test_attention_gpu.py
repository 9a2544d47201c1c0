"""Per-call edge values on the GPU: pygim_spmm_values, pygim_edge_softmax and pygim_edge_softmax_backward through the C ABI against
float64 references, and pygim_amd.attention / gnn.GATConv (autograd) against the per-entry CPU reference of test_attention_cpu.py.

Tolerances are the project's own (include/pygim_hip.h on pygim_sddmm): 1e-5 (FLT32) / 1e-12 (DBL64) relative to the sum of the
magnitudes a result is made of."""
import copy

import numpy as np
import pytest
import torch

from conftest import random_csr
from pygim_amd import _lib, attention, gnn, pim_ops, synth
from pygim_amd.attention import EdgeGraph, edge_softmax, spmm_values
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import gat_reference, ref_softmax, ref_spmm

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float64: 1e-12}
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def small_graph(rng):
    """duplicates, 10 % empty rows, rows around and across the 64-entry batches"""
    n, m = 700, 500
    rowptr, col = random_csr(rng, n, m, 12, empty_frac=0.1, long_rows=((11, 64), (12, 128), (300, 700)))
    return n, m, rowptr, col


def hub_graph(rng):
    """one row of 21 000 entries, one of 1 500, short rows and empty rows around them, and a hub column"""
    n, m = 400, 3000
    rowptr, col = random_csr(rng, n, m, 6, empty_frac=0.1, long_rows=((0, 3), (7, 21000), (150, 1500), (399, 0)))
    col[::3] = 3
    return n, m, rowptr, col


GRAPHS = {"small": small_graph, "hub": hub_graph}


def dev_csr(rowptr, col):
    return torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV)


def call_spmm_values(dtype, n, rp, cc, val, heads, X, h, out=None):
    """X: [rows, ldx] device tensor whose first h columns are the operand (row stride X.stride(0))"""
    code = pim_ops.DTYPE_CODE[dtype]
    nnz = cc.numel()
    nbytes = _lib.spmm_values_workspace(code, n, nnz, h, heads)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    _lib.spmm_values(code, n, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), heads, X.data_ptr(), X.stride(0), h, out.data_ptr(), out.stride(0),
                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def spmm_reference(n, rowptr, col, val, heads, X, h):
    """(exact value, sum of |value . x|) per output, float64 on the device"""
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(torch.from_numpy(rowptr).long().to(DEV)))
    msg = val.double().reshape(-1, heads).repeat_interleave(h // heads, dim=1) * X[:, :h].double()[torch.from_numpy(col).long().to(DEV)]
    ref = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg)
    mag = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg.abs())
    return ref, mag


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", [1, 9, 32, 100, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_spmm_values_parity(rng, dtype, h, graph):
    check_spmm_values_parity(rng, dtype, h, graph)


def test_spmm_values_parity_over_three_feature_chunks(rng):
    """h = 300: the misaligned stride gives 300 one-element pieces, three blockIdx.y chunks of 128, the last one partly empty"""
    check_spmm_values_parity(rng, torch.float32, 300, "small")


def check_spmm_values_parity(rng, dtype, h, graph, head_counts=(1, 4, 8), ldxs=None):
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    nnz = len(col)
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    for heads in [k for k in head_counts if h % k == 0]:
        val = torch.from_numpy(rng.uniform(-2, 2, size=(nnz, heads))).to(DEV, dtype)
        # a contiguous X, a wider row stride that keeps 16-byte alignment, and one that breaks it
        for ldx in ldxs or ((h, h + 2 * vec, h + 1) if graph == "small" else (h,)):
            X = torch.from_numpy(rng.uniform(-1, 1, size=(m, ldx))).to(DEV, dtype)
            out = call_spmm_values(dtype, n, rp, cc, val, heads, X, h)
            assert not torch.isnan(out).any(), "a row was not written"
            assert (out[torch.from_numpy(np.diff(rowptr) == 0).to(DEV)] == 0).all()
            ref, mag = spmm_reference(n, rowptr, col, val, heads, X, h)
            err = (out.double() - ref).abs()
            print(f"spmm_values {graph} {dtype} h={h} heads={heads} ldx={ldx}: max err / mag = {(err / mag.clamp_min(1e-300)).max().item():.3e}")
            assert torch.all(err <= TOL[dtype] * mag)
            assert torch.equal(out, call_spmm_values(dtype, n, rp, cc, val, heads, X, h)), "two launches differ"


def test_spmm_values_strided_out_nnz0_and_bad_arguments(rng):
    n, m, rowptr, col = small_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h, heads = 32, 4
    val = torch.rand(len(col), heads, device=DEV)
    X = torch.randn(m, h, device=DEV)
    wide = torch.full((n, h + 5), float("nan"), device=DEV)
    call_spmm_values(torch.float32, n, rp, cc, val, heads, X, h, out=wide)
    ref, mag = spmm_reference(n, rowptr, col, val, heads, X, h)
    assert torch.all((wide[:, :h].double() - ref).abs() <= 1e-5 * mag) and torch.isnan(wide[:, h:]).all(), "stores outside out[:, :h]"
    # nnz = 0: every row is empty, the result is zero
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    out = call_spmm_values(torch.float32, n, rp0, cc[:0], val[:0], heads, X, h)
    assert (out == 0).all()
    for dtype in (torch.float32, torch.float64):
        s0 = torch.empty(0, heads, dtype=dtype, device=DEV)
        assert edge_softmax(EdgeGraph(rp0, cc[:0], (n, m)), s0).shape == (0, heads)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    o = torch.empty(n, h, device=DEV)
    args = (n, rp.data_ptr(), cc.data_ptr(), len(col), val.data_ptr())
    with pytest.raises(_lib.PygimError):   # integer types have no such product
        _lib.spmm_values(_lib.INT32, *args, heads, X.data_ptr(), h, h, o.data_ptr(), h, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # heads must divide h
        _lib.spmm_values(_lib.FLT32, *args, 5, X.data_ptr(), h, h, o.data_ptr(), h, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # a workspace smaller than pygim_spmm_values_workspace says
        _lib.spmm_values(_lib.FLT32, *args, heads, X.data_ptr(), h, h, o.data_ptr(), h, ws.data_ptr(), 16)
    with pytest.raises(_lib.PygimError):
        _lib.edge_softmax(_lib.INT8, n, rp.data_ptr(), len(col), val.data_ptr(), heads, o.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):
        _lib.edge_softmax(_lib.FLT32, n, rp.data_ptr(), len(col), val.data_ptr(), heads, o.data_ptr(), ws.data_ptr(), 16)


def call_softmax(dtype, n, rp, nnz, a, heads, b=None, out=None):
    """a, b, out: [nnz, heads] contiguous (out: NaN-filled before the call)"""
    code = pim_ops.DTYPE_CODE[dtype]
    ws = torch.empty(max(_lib.edge_softmax_workspace(code, n, nnz, heads), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((nnz, heads), float("nan"), dtype=dtype, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if b is None:
        _lib.edge_softmax(code, n, rp.data_ptr(), nnz, a.data_ptr(), heads, out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    else:
        _lib.edge_softmax_backward(code, n, rp.data_ptr(), nnz, a.data_ptr(), b.data_ptr(), heads, out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return out


def softmax_reference(n, row, s):
    s = s.double()
    mx = torch.full((n, s.size(1)), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - mx[row])
    return e / torch.zeros(n, s.size(1), dtype=torch.float64, device=DEV).index_add_(0, row, e)[row]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("heads", [1, 3, 4, 8])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_edge_softmax_parity(rng, dtype, heads, graph):
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, _ = dev_csr(rowptr, col)
    nnz = len(col)
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(rp.long()))
    tiny = float(np.finfo(np.float32).tiny)
    for scale in (3.0, 30.0):
        s = torch.from_numpy(rng.normal(0, scale, size=(nnz, heads))).to(DEV, dtype)
        P = call_softmax(dtype, n, rp, nnz, s, heads)
        assert not torch.isnan(P).any()
        ref = softmax_reference(n, row, s)
        err = (P.double() - ref).abs()
        print(f"edge_softmax {graph} {dtype} heads={heads} scale={scale}: max rel err = {(err / ref.clamp_min(tiny)).max().item():.3e}")
        assert torch.all(err <= TOL[dtype] * ref + tiny)
        assert torch.equal(P, call_softmax(dtype, n, rp, nnz, s, heads)), "two launches differ"
        # backward on the exact probabilities rounded to the type
        Pin = ref.to(dtype)
        dP = torch.from_numpy(rng.normal(0, 1, size=(nnz, heads))).to(DEV, dtype)
        got = call_softmax(dtype, n, rp, nnz, Pin, heads, dP)
        assert not torch.isnan(got).any()
        t = Pin.double() * dP.double()
        tsum = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, t)
        tabs = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, t.abs())
        want = Pin.double() * (dP.double() - tsum[row])
        berr = (got.double() - want).abs()
        bound = TOL[dtype] * (tabs[row] + t.abs())
        print(f"edge_softmax_backward {graph} {dtype} heads={heads}: max err / bound = {(berr / bound.clamp_min(1e-300)).max().item():.3e}")
        assert torch.all(berr <= bound)
        assert torch.equal(got, call_softmax(dtype, n, rp, nnz, Pin, heads, dP)), "two launches differ"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_edge_softmax_is_stable_for_large_scores(rng, dtype):
    n, m, rowptr, col = hub_graph(rng)
    rp, _ = dev_csr(rowptr, col)
    nnz, heads = len(col), 4
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(rp.long()))
    s = torch.from_numpy(rng.choice([-1e4, 1e4], size=(nnz, heads))).to(DEV, dtype)
    s[::5] += torch.from_numpy(rng.normal(0, 1, size=(len(range(0, nnz, 5)), heads))).to(DEV, dtype)
    P = call_softmax(dtype, n, rp, nnz, s, heads)
    assert torch.isfinite(P).all() and (P >= 0).all()
    sums = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, P.double())
    nonempty = torch.from_numpy(np.diff(rowptr) > 0).to(DEV)
    # every probability is within TOL of its exact value, so a row's sum is within TOL of 1
    assert torch.all((sums[nonempty] - 1).abs() <= TOL[dtype])
    ref = softmax_reference(n, row, s)
    assert torch.all((P.double() - ref).abs() <= TOL[dtype] * ref + float(np.finfo(np.float32).tiny))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_autograd_on_device_matches_the_cpu_reference(rng, dtype):
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert g.rowptr.is_cuda
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-11)
    heads, h = 4, 32
    v = torch.rand(len(col), heads, dtype=dtype)
    X = torch.randn(m, h, dtype=dtype)
    G = torch.randn(n, h, dtype=dtype)
    vd, Xd = v.to(DEV).requires_grad_(), X.to(DEV).requires_grad_()
    out = spmm_values(g, vd, Xd, heads=heads)
    assert out.is_cuda
    out.backward(G.to(DEV))
    vc, Xc = v.double().requires_grad_(), X.double().requires_grad_()
    ref = ref_spmm(rowptr, col, vc, Xc, heads, n)
    ref.backward(G.double())
    assert torch.allclose(out.detach().cpu().double(), ref.detach(), **tol)
    assert torch.allclose(vd.grad.cpu().double(), vc.grad, **tol) and torch.allclose(Xd.grad.cpu().double(), Xc.grad, **tol)
    # CPU tensors are staged to the device and come home
    out_host = spmm_values(g, v, X, heads=heads)
    assert not out_host.is_cuda and torch.equal(out_host, out.detach().cpu())
    s = torch.randn(len(col), heads, dtype=dtype) * 2
    dP = torch.randn(len(col), heads, dtype=dtype)
    sd = s.to(DEV).requires_grad_()
    edge_softmax(g, sd).backward(dP.to(DEV))
    sc = s.double().requires_grad_()
    ref_softmax(rowptr, sc, n).backward(dP.double())
    assert torch.allclose(sd.grad.cpu().double(), sc.grad, **tol)


def test_gat_sgd_steps_match_the_cpu_reference(rng):
    """a 2-layer GAT, a few SGD steps in float64: losses and parameter gradients as with the per-entry plain-torch layer on the CPU
    (the tolerances of test_autograd_gpu.test_sgd_steps_match_the_cpu_path)"""
    n, f_in, hid, f_out, heads = 1500, 16, 32, 8, 4
    rowptr, col = random_csr(rng, n, n, 9)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.GAT(f_in, hid, f_out, num_layers=2, dropout=0.0, heads=heads).double()

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


def test_full_size_reddit_f32_h256_heads8():
    dev = torch.device("cuda", 0)
    n, nnz, d_max = synth.SHAPES["reddit"]
    h, heads = 256, 8
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    g = EdgeGraph(rowptr, col, (n, n))
    row = g.row.long()
    gen = torch.Generator(device=dev).manual_seed(5)
    scores = torch.randn(nnz, heads, device=dev, generator=gen) * 4
    P = edge_softmax(g, scores)
    # a seeded sample of 2^20 probabilities against float64 (the maxima and sums of all rows in float64, in blocks of entries)
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=dev)
    z = torch.zeros(n, heads, dtype=torch.float64, device=dev)
    step = 1 << 23
    for s in range(0, nnz, step):
        mx.index_reduce_(0, row[s:s + step], scores[s:s + step].double(), "amax", include_self=True)
    for s in range(0, nnz, step):
        z.index_add_(0, row[s:s + step], torch.exp(scores[s:s + step].double() - mx[row[s:s + step]]))
    pick = torch.from_numpy(np.random.default_rng(7).integers(0, nnz, size=(1 << 20) // heads)).to(dev)
    ref = torch.exp(scores[pick].double() - mx[row[pick]]) / z[row[pick]]
    tiny = float(np.finfo(np.float32).tiny)
    assert torch.all((P[pick].double() - ref).abs() <= 1e-5 * ref + tiny)
    del mx, z, scores
    # the product with those probabilities: 4096 seeded rows x 256 features = 2^20 outputs against float64
    X = synth.features(n, h, torch.float32, seed=3, device=dev, kind="uniform")
    out = spmm_values(g, P, X, heads=heads)
    rows = torch.from_numpy(np.random.default_rng(8).choice(n, size=4096, replace=False)).to(dev)
    slot = torch.full((n,), -1, dtype=torch.int64, device=dev)
    slot[rows] = torch.arange(4096, device=dev)
    for lo in range(0, 4096, 512):   # 512 rows at a time: their entries' messages in float64
        e = torch.nonzero((slot[row] >= lo) & (slot[row] < lo + 512)).squeeze(1)
        msg = P[e].double().repeat_interleave(h // heads, dim=1) * X[g.col[e].long()].double()
        ref = torch.zeros(512, h, dtype=torch.float64, device=dev).index_add_(0, slot[row[e]] - lo, msg)
        mag = torch.zeros(512, h, dtype=torch.float64, device=dev).index_add_(0, slot[row[e]] - lo, msg.abs())
        got = out[rows[lo:lo + 512]].double()
        assert torch.all((got - ref).abs() <= 1e-5 * mag)
