"""Sparse dot-product attention on the GPU: pygim_sparse_attention through the C ABI against float64 on the device, and
pygim_amd.sparse_attention / gnn.TransformerConv / gnn.GraphTransformer (autograd, training) against the per-entry CPU reference.

Bounds (include/pygim_hip.h), with EPS = 1e-5 (FLT32, FLT16, BF16) / 1e-12 (DBL64) and
Delta[r, k] = EPS * |scale| * max_e sum_{f in head k} |Q[r, f] * K[col[e], f]| -- the pygim_sddmm bound on a score:
    |out - ref| <= (2 EPS + 2 Delta[r, k]) * sum_e p_ref[e] * |v[e]|     (a score error of Delta moves a probability by at most e^(2 Delta) - 1)
    |lse - ref| <= 2 EPS * (1 + |lse_ref|) + Delta[r, k]
and for the 16-bit types u * |ref| more on out, u = 2^-8 (BF16) / 2^-11 (FLT16), ref computed in float64 from the 16-bit inputs."""
import copy

import numpy as np
import pytest
import torch

from conftest import random_csr
from pygim_amd import _lib, gnn, pim_ops
from pygim_amd.attention import EdgeGraph, sparse_attention
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_gpu import dev_csr, hub_graph, small_graph
from test_sparse_attention_cpu import ref_sparse_attention, transformer_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRAPHS = {"small": small_graph, "hub": hub_graph}
EPS = {torch.float32: 1e-5, torch.float64: 1e-12, torch.float16: 1e-5, torch.bfloat16: 1e-5}
U = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CODE = {torch.float32: _lib.FLT32, torch.float64: _lib.DBL64, torch.bfloat16: _lib.BF16, torch.float16: _lib.FLT16}
SHAPES = [(4, 4), (9, 3), (32, 1), (32, 4), (32, 8), (100, 4), (256, 1), (256, 8), (512, 2), (1024, 16)]


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def lse_type(dtype):
    return torch.float32 if dtype in (torch.float16, torch.bfloat16) else dtype


def call_sa(dtype, n, rp, cc, Q, K, V, h, heads, scale, out=None, want_lse=True):
    """Q, K, V: [rows, ld] device tensors whose first h columns are the operands; -> (out, lse or None), NaN-filled before the call"""
    nnz = cc.numel()
    ws = torch.empty(max(_lib.sparse_attention_workspace(CODE[dtype], n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((n, heads), float("nan"), dtype=lse_type(dtype), device=DEV) if want_lse else None
    _lib.sparse_attention(CODE[dtype], n, rp.data_ptr(), cc.data_ptr(), nnz, Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(),
                          V.stride(0), h, heads, scale, out.data_ptr(), out.stride(0), lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, lse


def sa_reference_dev(dtype, n, rowptr, col, Q, K, V, h, heads, scale):
    """float64 on the device, from the operands as stored: (exact out, sum_e p |v| per output, lse with 0 for empty rows, Delta per row
    and head, the row of every entry, its column)"""
    hd = h // heads
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(torch.from_numpy(rowptr).long().to(DEV)))
    cc = torch.from_numpy(col).long().to(DEV)
    prod = (Q[:, :h].double()[row] * K[:, :h].double()[cc]).view(-1, heads, hd)
    s = scale * prod.sum(-1)
    sabs = abs(scale) * prod.abs().sum(-1)
    del prod
    delta = EPS[dtype] * torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_reduce_(0, row, sabs, "amax", include_self=True)
    m = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - m[row])
    l = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, e)
    msg = (e / l[row]).repeat_interleave(hd, dim=1) * V[:, :h].double()[cc]
    ref = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg)
    mag = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg.abs())
    lse = torch.where(l > 0, m + torch.log(l), torch.zeros_like(l))
    return ref, mag, lse, delta, row, cc


def out_bound(dtype, ref, mag, delta, h, heads):
    return (2 * EPS[dtype] + 2 * delta.repeat_interleave(h // heads, dim=1)) * mag + U[dtype] * ref.abs()


def check(tag, dtype, n, rowptr, rp, cc, Q, K, V, h, heads, scale, reference):
    """one call under the bounds, every row written, empty rows zero, a second launch bit-equal"""
    ref, mag, lse_ref, delta, _, _ = reference
    out, lse = call_sa(dtype, n, rp, cc, Q, K, V, h, heads, scale)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), "a row was not written"
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert (out[empty] == 0).all() and (lse[empty] == 0).all()
    err = (out.double() - ref).abs()
    bound = out_bound(dtype, ref, mag, delta, h, heads)
    lerr = (lse.double() - lse_ref).abs()
    lbound = 2 * EPS[dtype] * (1 + lse_ref.abs()) + delta
    print(f"sparse_attention {tag}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3e}, "
          f"lse max err / bound = {(lerr / lbound).max().item():.3e}")
    assert torch.all(err <= bound)
    assert torch.all(lerr <= lbound)
    out2, lse2 = call_sa(dtype, n, rp, cc, Q, K, V, h, heads, scale)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "two launches differ"
    return out


def strided(t, ld):
    """the same values in a buffer of row stride ld (the padding NaN: nothing may read it)"""
    if ld == t.size(1):
        return t
    buf = torch.full((t.size(0), ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.size(1)] = t
    return buf


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", SHAPES)
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_sparse_attention_parity(rng, dtype, h, heads, graph):
    """(4, 4): hd = 1, sixteen lane groups; (9, 3): scalar pieces, a head count that is no power of two; (32, *): 16-byte pieces, one to
    eight heads side by side; (100, 4): hd = 25 (FLT32: 16-byte pieces do not fit, DBL64: hd is odd); (256, 1): the whole wave one head;
    (512, 2): hd = 256, the cap (DBL64: two pieces per lane); (1024, 16): heads across blockIdx.y.  On the small graph every operand
    also with a padded aligned row stride and with a misaligned one (one element per lane, up to four pieces per lane at hd = 256)."""
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    scale = (h // heads) ** -0.5
    Q = torch.from_numpy(rng.uniform(-2, 2, size=(n, h))).to(DEV, dtype)
    K = torch.from_numpy(rng.uniform(-2, 2, size=(m, h))).to(DEV, dtype)
    V = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(DEV, dtype)
    reference = sa_reference_dev(dtype, n, rowptr, col, Q, K, V, h, heads, scale)
    lds = [(h, h, h)]
    if graph == "small":
        for ld in (h + 2 * vec, h + 1):
            lds += [(ld, h, h), (h, ld, h), (h, h, ld)]
    for ldq, ldk, ldv in lds:
        check(f"{graph} {dtype} h={h} heads={heads} ld={ldq},{ldk},{ldv}", dtype, n, rowptr, rp, cc, strided(Q, ldq), strided(K, ldk), strided(V, ldv),
              h, heads, scale, reference)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h,heads", [(32, 4), (256, 8), (100, 4)])
def test_sparse_attention_16_bit(rng, dtype, h, heads):
    """16-bit Q, K, V and out, float32 lse; the reference is float64 on the 16-bit inputs.  |v| in [0.5, 2) with random signs, as in
    test_half_gpu's GAT test: the bound has no absolute term, so a result far below every |v| must be a cancellation that the
    sum p |v| term covers"""
    for graph in GRAPHS:
        n, m, rowptr, col = GRAPHS[graph](rng)
        rp, cc = dev_csr(rowptr, col)
        scale = (h // heads) ** -0.5
        Q = torch.from_numpy(rng.uniform(-2, 2, size=(n, h))).to(DEV, dtype)
        K = torch.from_numpy(rng.uniform(-2, 2, size=(m, h))).to(DEV, dtype)
        V = torch.from_numpy(rng.uniform(0.5, 2, size=(m, h)) * rng.choice([-1.0, 1.0], size=(m, h))).to(DEV, dtype)
        reference = sa_reference_dev(dtype, n, rowptr, col, Q, K, V, h, heads, scale)
        for ld in ((h, h + 16, h + 1) if graph == "small" else (h,)):
            q, k, v = strided(Q, ld), strided(K, ld), strided(V, ld)
            out = check(f"{graph} {dtype} h={h} heads={heads} ld={ld}", dtype, n, rowptr, rp, cc, q, k, v, h, heads, scale, reference)
            without, none = call_sa(dtype, n, rp, cc, q, k, v, h, heads, scale, want_lse=False)
            assert none is None and torch.equal(out, without)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sparse_attention_is_stable_for_large_scores(rng, dtype):
    """integer-valued Q and K in [-8, 8], hd = 16, scale = 1: every product, dot product and score difference is exact in float32 and
    the scores reach +-1024; only exp and the sums round.  The output is finite, meets the bound, and is a convex combination of the
    row's gathered V within that bound."""
    n, m, rowptr, col = hub_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h, heads = 64, 4
    Q = torch.from_numpy(rng.integers(-8, 9, size=(n, h))).to(DEV, dtype)
    K = torch.from_numpy(rng.integers(-8, 9, size=(m, h))).to(DEV, dtype)
    V = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(DEV, dtype)
    reference = sa_reference_dev(dtype, n, rowptr, col, Q, K, V, h, heads, 1.0)
    out = check(f"large scores {dtype}", dtype, n, rowptr, rp, cc, Q, K, V, h, heads, 1.0, reference)
    ref, mag, lse_ref, delta, row, col_l = reference
    assert lse_ref.abs().max() > 300, "the scores of this test are meant to be large"
    assert torch.isfinite(out).all()
    vg = V.double()[col_l]
    lo = torch.full((n, h), float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, vg, "amin", include_self=True)
    hi = torch.full((n, h), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, vg, "amax", include_self=True)
    full = torch.from_numpy(np.diff(rowptr) > 0).to(DEV)
    bound = out_bound(dtype, ref, mag, delta, h, heads)
    assert torch.all(out.double()[full] >= (lo - bound)[full]) and torch.all(out.double()[full] <= (hi + bound)[full])


def test_sparse_attention_strided_out_no_lse_nnz0_and_bad_arguments(rng):
    n, m, rowptr, col = small_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h, heads = 32, 4
    scale = 8 ** -0.5
    Q, K, V = torch.randn(n, h, device=DEV), torch.randn(m, h, device=DEV), torch.randn(m, h, device=DEV)
    ref, mag, _, delta, _, _ = sa_reference_dev(torch.float32, n, rowptr, col, Q, K, V, h, heads, scale)
    bound = out_bound(torch.float32, ref, mag, delta, h, heads)
    for pad in (5, 8):   # a misaligned and an aligned stride of out, NaN guard columns behind every row
        wide = torch.full((n, h + pad), float("nan"), device=DEV)
        call_sa(torch.float32, n, rp, cc, Q, K, V, h, heads, scale, out=wide)
        assert torch.all((wide[:, :h].double() - ref).abs() <= bound) and torch.isnan(wide[:, h:]).all(), "stores outside out[:, :h]"
    # out does not depend on whether lse is asked for
    with_lse, _ = call_sa(torch.float32, n, rp, cc, Q, K, V, h, heads, scale)
    without, none = call_sa(torch.float32, n, rp, cc, Q, K, V, h, heads, scale, want_lse=False)
    assert none is None and torch.equal(with_lse, without)
    # nnz = 0: every row is empty, out and lse are zero
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    out, lse = call_sa(torch.float32, n, rp0, cc[:0], Q, K, V, h, heads, scale)
    assert (out == 0).all() and (lse == 0).all()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    o = torch.empty(n, h, device=DEV)
    head = (n, rp.data_ptr(), cc.data_ptr(), len(col), Q.data_ptr(), h, K.data_ptr(), h, V.data_ptr(), h)
    with pytest.raises(_lib.PygimError):   # integer types have no such aggregation
        _lib.sparse_attention(_lib.INT32, *head, h, heads, scale, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # heads must divide h
        _lib.sparse_attention(_lib.FLT32, *head, h, 5, scale, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # a workspace smaller than pygim_sparse_attention_workspace says
        _lib.sparse_attention(_lib.FLT32, *head, h, heads, scale, o.data_ptr(), h, 0, ws.data_ptr(), 16)
    with pytest.raises(_lib.PygimError):   # ... or misaligned
        _lib.sparse_attention(_lib.FLT32, *head, h, heads, scale, o.data_ptr(), h, 0, ws.data_ptr() + 4, ws.numel() - 4)
    # a head wider than 256 features: h = 514, heads = 2 (the operands are never read: the call is rejected before any launch)
    wq, wk = torch.zeros(n, 514, device=DEV), torch.zeros(m, 514, device=DEV)
    big = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.PygimError):
        _lib.sparse_attention(_lib.FLT32, n, rp.data_ptr(), cc.data_ptr(), len(col), wq.data_ptr(), 514, wk.data_ptr(), 514, wk.data_ptr(), 514, 514, 2,
                              scale, wq.data_ptr(), 514, 0, big.data_ptr(), big.numel())
    assert _lib.sparse_attention_workspace(_lib.FLT32, n, len(col), 512, 2) == _lib.gat_aggregate_workspace(_lib.FLT32, n, len(col), 512, 2)
    for bad in ((_lib.FLT32, h, 5), (_lib.FLT32, 514, 2), (_lib.INT32, h, heads)):
        with pytest.raises(_lib.PygimError):
            _lib.sparse_attention_workspace(bad[0], n, len(col), bad[1], bad[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_autograd_on_device_matches_the_cpu_reference(rng, dtype):
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert g.rowptr.is_cuda
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-11)
    heads, h = 4, 32
    torch.manual_seed(21)
    Q, K, V = torch.randn(n, h, dtype=dtype), torch.randn(m, h, dtype=dtype), torch.randn(m, h, dtype=dtype)
    G = torch.randn(n, h, dtype=dtype)
    cpu = [t.clone().double().requires_grad_() for t in (Q, K, V)]   # clone: .double() of a float64 tensor is the tensor itself
    ref = ref_sparse_attention(rowptr, col, *cpu, heads, n)
    ref.backward(G.double())
    for fused in (True, False):
        dev = [t.to(DEV).requires_grad_() for t in (Q, K, V)]
        out = sparse_attention(g, *dev, heads=heads, fused=fused)
        assert out.is_cuda
        out.backward(G.to(DEV))
        assert torch.allclose(out.detach().cpu().double(), ref.detach(), **tol)
        for name, d, c in zip("QKV", dev, cpu):
            print(f"sparse_attention autograd {dtype} fused={fused} d{name}: max abs err = {(d.grad.cpu().double() - c.grad).abs().max().item():.3e}")
            assert d.grad.dtype == dtype and torch.allclose(d.grad.cpu().double(), c.grad, **tol), name
        # CPU tensors are staged to the device and come home
        out_host = sparse_attention(g, Q, K, V, heads=heads, fused=fused)
        assert not out_host.is_cuda and torch.equal(out_host, out.detach().cpu())


def test_wide_heads_run_unfused_on_the_device(rng):
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    Q, K, V = torch.randn(n, 300, device=DEV), torch.randn(m, 300, device=DEV), torch.randn(m, 300, device=DEV)
    out = sparse_attention(g, Q, K, V, heads=1)
    ref = ref_sparse_attention(rowptr, col, Q.cpu().double(), K.cpu().double(), V.cpu().double(), 1, n)
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_gradients_in_bfloat16(rng):
    """bfloat16 Q, K, V and G; every gradient comes back in bfloat16, rounded once from float32 sums, against float64 on the CPU from the
    same 16-bit operands.  With A[e] = sum_f |G[r, f] V[c, f]| per head (the pygim_sddmm magnitude of dP) and
    rel = 2 Delta + 2 EPS (1 + |lse|) + EPS, the relative error of a recomputed probability exp(s - lse) (score, lse, exp):
      dV = sum_e P G:   u |ref| + (rel + EPS) * sum_e P |G|                            (the probabilities, then the float32 sum)
      dS = scale P (dP - delta[r]),  delta = sum_e P dP:  the factor P is off by rel, dP by EPS A, delta by (rel + 2 EPS) sum_e P A, so
           |dS - ref| <= (2 rel + 3 EPS + 1e-6) * W,  W[e] = |scale| P (A[e] + sum_{e' in row} P A)      (1e-6: the three float32 products)
      dQ = sum_e dS K,  dK = sum_e dS Q:   u |ref| + (2 rel + 4 EPS + 1e-6) * sum_e W |K|  (resp. |Q|)"""
    dtype, u, eps = torch.bfloat16, 2.0 ** -8, 1e-5
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    h, heads = 64, 4
    hd = h // heads
    scale = hd ** -0.5
    torch.manual_seed(22)
    Q, K, V, G = (torch.randn(r, h).to(dtype) for r in (n, m, m, n))
    dev = [t.to(DEV).requires_grad_() for t in (Q, K, V)]
    out = sparse_attention(g, *dev, heads=heads)
    out.backward(G.to(DEV))
    assert out.dtype == dtype and [t.grad.dtype for t in dev] == [dtype] * 3
    cpu = [t.double().requires_grad_() for t in (Q, K, V)]
    ref_sparse_attention(rowptr, col, *cpu, heads, n).backward(G.double())
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    q3, k3, v3, g3 = (t.double().view(-1, heads, hd) for t in (Q, K, V, G))
    s = scale * (q3[row] * k3[cc]).sum(-1)
    sabs = scale * (q3[row] * k3[cc]).abs().sum(-1)
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - mx[row])
    l = torch.zeros(n, heads, dtype=torch.float64).index_add_(0, row, e)
    P = e / l[row]
    lse = torch.where(l > 0, mx + torch.log(l.clamp_min(1e-300)), torch.zeros_like(l))
    rel = 2 * eps * sabs.max().item() + 2 * eps * (1 + lse.abs().max().item()) + eps
    A = (g3[row] * v3[cc]).abs().sum(-1)
    W = scale * P * (A + torch.zeros(n, heads, dtype=torch.float64).index_add_(0, row, P * A)[row])
    wide = lambda t: t.repeat_interleave(hd, dim=1)
    mag_v = torch.zeros(m, h, dtype=torch.float64).index_add_(0, cc, wide(P) * G.double()[row].abs())
    mag_q = torch.zeros(n, h, dtype=torch.float64).index_add_(0, row, wide(W) * K.double()[cc].abs())
    mag_k = torch.zeros(m, h, dtype=torch.float64).index_add_(0, cc, wide(W) * Q.double()[row].abs())
    for name, d, c, mag, tol in (("Q", dev[0], cpu[0], mag_q, 2 * rel + 4 * eps + 1e-6), ("K", dev[1], cpu[1], mag_k, 2 * rel + 4 * eps + 1e-6),
                                 ("V", dev[2], cpu[2], mag_v, rel + eps)):
        err = (d.grad.cpu().double() - c.grad).abs()
        bound = u * c.grad.abs() + tol * mag + 2.0 ** -24
        print(f"sparse_attention bfloat16 d{name}: max err / bound = {(err / bound).max().item():.3f}")
        assert torch.all(err <= bound), name


@pytest.mark.parametrize("mode", ["to", "autocast"])
@pytest.mark.parametrize("fused", [True, False])
def test_transformerconv_in_bfloat16(rng, mode, fused):
    """after conv.to(torch.bfloat16) and under torch.autocast: forward and backward run, everything is finite and of the expected dtype"""
    n = 600
    rowptr, col = random_csr(rng, n, n, 9, empty_frac=0.1)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(0)
    conv = gnn.TransformerConv(24, 8, heads=4, fused=fused).to(DEV)
    x = torch.randn(n, 24, device=DEV)
    if mode == "to":
        conv, x = conv.to(torch.bfloat16), x.to(torch.bfloat16)
        out = conv(x.requires_grad_(), adj)
        assert out.dtype == torch.bfloat16
    else:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = conv(x.requires_grad_(), adj)
        assert out.dtype in (torch.bfloat16, torch.float32)
    out.float().square().mean().backward()
    assert out.shape == (n, 32) and torch.isfinite(out).all()
    assert x.grad.dtype == x.dtype and torch.isfinite(x.grad).all()
    for p in conv.parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and torch.isfinite(p.grad).all()


def test_graph_transformer_sgd_steps_match_the_cpu_reference(rng):
    """a 2-layer GraphTransformer, 4 SGD steps in float64: losses and parameter gradients as with the per-entry plain-torch layer on the
    CPU; then one float32 forward, fused against unfused"""
    n, f_in, hid, f_out, heads = 1500, 16, 32, 8, 4
    rowptr, col = random_csr(rng, n, n, 9)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.GraphTransformer(f_in, hid, f_out, num_layers=2, dropout=0.0, heads=heads, fused=True).double()

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
        conv.forward = (lambda c: lambda x, adj_t: transformer_reference(c, x, rowptr, col, n))(conv)
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
