"""Attention dropout on the GPU: pygim_gat_aggregate_dropout, pygim_sparse_attention_dropout, pygim_gatv2_aggregate_dropout,
pygim_gatv2_backward_dropout and pygim_attention_dropout_mask through the C ABI against float64 on the device with the mask from the numpy
mirror (attn_dropout_ref.py), then the autograd functions and the layers.

Forward bound (include/pygim_hip.h, the kernels' own with p[e] read as pr * w):
    |out - ref| <= (2 EPS + 2 Delta[r, k]) * sum_e pr w |v| + u |ref|,   EPS = 1e-5 (FLT32, BF16) / 1e-12 (DBL64), u = 2^-8 (BF16)
The one extra float32 multiply by w (exact for p = 0.5, half an ulp = 6e-8 for p = 0.3) sits far inside EPS.  test_attn_dropout_cpu.py
shows on the reference alone that a kernel which ignored the mask would violate this bound in every row with a dropped entry.
Graphs: `edges` of run_edges.py (5121 entries, rows cut across runs, a last run of one entry) and small_graph of test_attention_gpu.py.
Gradients: the tolerances of the functions' own GPU files, rtol = atol = 1e-4 (FLT32), 1e-10 / 1e-11 (DBL64)."""
import copy

import numpy as np
import pytest
import torch

import attn_dropout_ref as ad
import launch_shapes as ls
import run_edges
from conftest import random_csr
from pygim_amd import _lib, gnn
from pygim_amd.attention import EdgeGraph, dropout_mask, gat_aggregate, gatv2_aggregate, sparse_attention
from pygim_amd.sparse_tensor import SparseTensorShim
from test_gatv2_gpu import GRAD_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda"
CODE = {torch.float32: _lib.FLT32, torch.float64: _lib.DBL64, torch.bfloat16: _lib.BF16}
TYPED_CASES = [(d, h, k) for d in (torch.float32, torch.float64) for h, k in ad.CASES] + [(torch.bfloat16, h, k) for h, k in ad.HALF_CASES]


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def compute_type(dtype):
    return torch.float32 if dtype == torch.bfloat16 else dtype


def stream():
    return torch.cuda.current_stream().cuda_stream


def on_device(ops):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in ops.items()}


def dev_csr(rowptr, col):
    return torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV)


def call(kind, dtype, n, rp, cc, ops, h, heads, p=0.0, seed=0, base=False):
    """one forward call, through the *_dropout entry point or (base) the entry point without the argument; operands on the device;
    -> (out, lse), NaN-filled before the call"""
    nnz, code = cc.numel(), CODE[dtype]
    out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((n, heads), float("nan"), dtype=compute_type(dtype), device=DEV)
    head = (code, n, rp.data_ptr(), cc.data_ptr(), nnz)
    A, B, V = ops["A"], ops["B"], ops["V"]
    if kind == "gat":
        ws = torch.empty(max(_lib.gat_aggregate_workspace(code, n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
        args = head + (A.data_ptr(), B.data_ptr(), heads, ops["scalar"], V.data_ptr(), V.stride(0), h, out.data_ptr(), h, lse.data_ptr(), ws.data_ptr(),
                       ws.numel(), stream())
        fn = _lib.gat_aggregate if base else _lib.gat_aggregate_dropout
    elif kind == "sa":
        ws = torch.empty(max(_lib.sparse_attention_workspace(code, n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
        args = head + (A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), V.data_ptr(), V.stride(0), h, heads, ops["scalar"], out.data_ptr(), h,
                       lse.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        fn = _lib.sparse_attention if base else _lib.sparse_attention_dropout
    else:
        ws = torch.empty(max(_lib.gatv2_aggregate_workspace(code, n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
        args = head + (A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), ops["att"].data_ptr(), h, heads, ops["scalar"], out.data_ptr(), h,
                       lse.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        fn = _lib.gatv2_aggregate if base else _lib.gatv2_aggregate_dropout
    fn(*args) if base else fn(*args, p, seed)
    torch.cuda.synchronize()
    return out, lse


def check_forward(kind, dtype, gname, n, rowptr, col, ops, h, heads, rates=ad.PS):
    rp, cc = dev_csr(rowptr, col)
    dev = on_device(ops)
    ops64 = ad.as_float64(ops, DEV)
    nnz = len(col)
    plain_out, plain_lse = call(kind, dtype, n, rp, cc, dev, h, heads, base=True)
    zero_out, zero_lse = call(kind, dtype, n, rp, cc, dev, h, heads, 0.0, ad.SEED)
    assert torch.equal(plain_out, zero_out) and torch.equal(plain_lse, zero_lse), "p = 0 through the dropout entry point differs from the base entry point"
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    for p in rates:
        r = ad.reference(kind, dtype, n, rowptr, col, ops64, h, heads, ad.weights(nnz, heads, p, ad.SEED), DEV)
        out, lse = call(kind, dtype, n, rp, cc, dev, h, heads, p, ad.SEED)
        assert not torch.isnan(out).any() and not torch.isnan(lse).any(), "a row was not written"
        assert (out[empty] == 0).all() and (lse[empty] == 0).all()
        err = (out.double() - r["ref"]).abs()
        bound = ad.out_bound(dtype, r, h, heads)
        print(f"{kind} dropout {gname} {dtype} h={h} heads={heads} p={p}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3e}")
        assert torch.all(err <= bound)
        assert torch.equal(lse, plain_lse), "lse must have the bits of the call without dropout"
        out2, lse2 = call(kind, dtype, n, rp, cc, dev, h, heads, p, ad.SEED)
        assert torch.equal(out, out2) and torch.equal(lse, lse2), "two launches differ"
        other, _ = call(kind, dtype, n, rp, cc, dev, h, heads, p, ad.SEED ^ 1)
        assert not torch.equal(out, other), "the seed is not read"


@pytest.mark.parametrize("dtype,h,heads", TYPED_CASES)
@pytest.mark.parametrize("kind", ad.KINDS)
def test_forward_with_dropout(kind, dtype, h, heads):
    """(4, 4): one lane per head; (9, 3): scalar, partly filled heads; (32, 8), (100, 4), (256, 8); (512, 2): two chunks (the row walker's
    two pieces per lane, DBL64 head-wise two pieces).  Per kernel and graph: under the bound for p = 0.3 and 0.5, lse bit-equal to the call
    without dropout, two launches bit-equal, p = 0 through the new entry point bit-equal to the base entry point"""
    for gname in ad.GRAPHS:
        n, m, rowptr, col = ad.graph(gname)
        check_forward(kind, dtype, gname, n, rowptr, col, ad.operands(kind, n, m, h, heads, dtype), h, heads)


@pytest.mark.parametrize("kind", ["sa", "gatv2"])
def test_forward_with_dropout_two_launches(kind):
    """65 537 heads of 33 features: the second launch starts at head0 = 65535, and the mask must be that of heads 65535 and 65536"""
    n, m, rowptr, col = ls.two_launch_graph()
    h, heads = ad.TWO_LAUNCH
    check_forward(kind, torch.float32, "two-launch", n, rowptr, col, ad.two_launch_operands(kind), h, heads)


@pytest.mark.parametrize("kind", ad.KINDS)
def test_heads_whose_entries_are_all_dropped_store_zeros(kind):
    n, m, rowptr, col = ad.graph("small")
    h, heads, p, dtype = 32, 8, 0.9, torch.float32
    keep = ad.keep_mirror(np.arange(len(col)), heads, p, ad.SEED)
    row = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    kept = np.zeros((n, heads), dtype=np.int64)
    np.add.at(kept, row, keep.astype(np.int64))
    nonempty = (np.diff(rowptr) > 0)[:, None]
    all_dropped = nonempty & (kept == 0)
    assert all_dropped.any() and (nonempty & (kept > 0)).any(), "the case needs both kinds of (row, head)"
    rp, cc = dev_csr(rowptr, col)
    ops = ad.operands(kind, n, m, h, heads, dtype)
    out, lse = call(kind, dtype, n, rp, cc, on_device(ops), h, heads, p, ad.SEED)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    per_head = out.view(n, heads, h // heads)
    assert (per_head[torch.from_numpy(all_dropped).to(DEV)] == 0).all(), "an all-dropped head is exact zeros"
    assert (per_head[torch.from_numpy(nonempty & (kept > 0)).to(DEV)] != 0).any()
    r = ad.reference(kind, dtype, n, rowptr, col, ad.as_float64(ops, DEV), h, heads, ad.weights(len(col), heads, p, ad.SEED), DEV)
    assert torch.all((out.double() - r["ref"]).abs() <= ad.out_bound(dtype, r, h, heads))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mask_entry_point_equals_the_mirror(dtype):
    n, m, rowptr, col = ad.graph("edges")
    nnz = len(col)
    perm = run_edges.transpose_csr(n, m, rowptr, col)[4]
    ids = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    for heads in (1, 3, 8):
        for p in (0.0, 0.3, 0.5, 0.9):
            for entries, ptr in ((None, 0), (perm, ids.data_ptr())):
                mask = torch.full((nnz, heads), float("nan"), dtype=dtype, device=DEV)
                _lib.attention_dropout_mask(CODE[dtype], nnz, heads, ptr, p, ad.SEED, mask.data_ptr(), stream())
                torch.cuda.synchronize()
                want = torch.from_numpy(ad.weights(nnz, heads, p, ad.SEED, entries)).to(dtype)
                assert torch.equal(mask.cpu(), want), f"heads {heads} p {p} entry_ids {entries is not None}"
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert torch.equal(dropout_mask(g, 3, 0.5, ad.SEED, dtype).cpu(), torch.from_numpy(ad.weights(nnz, 3, 0.5, ad.SEED)).to(dtype))
    assert torch.equal(dropout_mask(g, 3, 0.5, ad.SEED, dtype, transposed=True).cpu(), torch.from_numpy(ad.weights(nnz, 3, 0.5, ad.SEED, perm)).to(dtype))
    assert torch.equal(g.transposed()[1].cpu(), torch.from_numpy(perm)), "EdgeGraph.transposed and run_edges.transpose_csr state one permutation"


# ---- the GATv2 backward ----
def call_bwd(dtype, transposed, gr, own, oth, att, h, heads, G, lse, delta, entry_ids, p, seed):
    """one pygim_gatv2_backward_dropout call -> (d_own, datt or None), NaN-filled before the call"""
    code = CODE[dtype]
    ws = torch.empty(max(_lib.gatv2_backward_workspace(code, gr.nrows, gr.nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    d_own = torch.full((gr.nrows, h), float("nan"), dtype=dtype, device=DEV)
    datt = None if transposed else torch.full((h,), float("nan"), dtype=compute_type(dtype), device=DEV)
    _lib.gatv2_backward_dropout(code, int(transposed), gr.nrows, gr.rowptr.data_ptr(), gr.col.data_ptr(), gr.nnz, own.data_ptr(), own.stride(0),
                                oth.data_ptr(), oth.stride(0), att.data_ptr(), h, heads, ad.SLOPE, G.data_ptr(), G.stride(0), lse.data_ptr(),
                                delta.data_ptr(), d_own.data_ptr(), h, 0 if transposed else datt.data_ptr(), ws.data_ptr(), ws.numel(), stream(),
                                0 if entry_ids is None else entry_ids.data_ptr(), p, seed)
    torch.cuda.synchronize()
    return d_own, datt


def backward_reference(dtype, n, rowptr, col, Xd, Xs, att, G, h, heads, p):
    """float64 autograd of the per-entry reference with w as a constant -> ((dx_dst, dx_src, datt), lse, delta in the compute type)"""
    xd, xs, a = (t.double().detach().clone().requires_grad_() for t in (Xd, Xs, att))
    r = ad.reference("gatv2", dtype, n, rowptr, col, dict(A=xd, B=xs, V=xs, att=a, scalar=ad.SLOPE), h, heads,
                     ad.weights(len(col), heads, p, ad.SEED), DEV)
    r["ref"].backward(G.double())
    delta = (G.double() * r["ref"].detach()).view(n, heads, h // heads).sum(-1)
    ct = compute_type(dtype)
    return (xd.grad, xs.grad, a.grad), r["lse"].to(ct).contiguous(), delta.to(ct).contiguous()


def check_backward(dtype, gname, n, m, rowptr, col, h, heads, p, wrong_ids_must_fail=False):
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    gt, _ = g.transposed()
    ids = g.entry_ids_t()
    assert ids.dtype == torch.int32 and ids is g.entry_ids_t(), "the int32 copy of perm is cached on the graph"
    torch.manual_seed(21)
    Xd, Xs, G = (torch.randn(r, h, dtype=dtype, device=DEV) for r in (n, m, n))
    att = torch.randn(h, dtype=dtype, device=DEV) * (h // heads) ** -0.5
    want, lse, delta = backward_reference(dtype, n, rowptr, col, Xd, Xs, att, G, h, heads, p)
    tol = GRAD_TOL[dtype]
    d_dst, datt = call_bwd(dtype, False, g, Xd, Xs, att, h, heads, G, lse, delta, None, p, ad.SEED)
    d_src, none = call_bwd(dtype, True, gt, Xs, Xd, att, h, heads, G, lse, delta, ids, p, ad.SEED)
    assert none is None
    for name, got, ref in (("dx_dst", d_dst, want[0]), ("dx_src", d_src, want[1]), ("datt", datt, want[2])):
        assert not torch.isnan(got).any(), f"{name}: not written"
        err = (got.double() - ref).abs()
        print(f"gatv2_backward dropout {gname} {dtype} h={h} heads={heads} p={p} {name}: max err / (atol + rtol |ref|) = "
              f"{(err / (tol['atol'] + tol['rtol'] * ref.abs())).max().item():.3e}")
        assert torch.allclose(got.double(), ref, **tol), name
    again, _ = call_bwd(dtype, True, gt, Xs, Xd, att, h, heads, G, lse, delta, ids, p, ad.SEED)
    assert torch.equal(d_src, again), "two launches differ"
    if wrong_ids_must_fail:
        # identity ids on the transposed CSR are the wrong ids (duplicates, unsorted transposition): the test sees a wrong id
        wrong, _ = call_bwd(dtype, True, gt, Xs, Xd, att, h, heads, G, lse, delta, None, p, ad.SEED)
        assert not torch.allclose(wrong.double(), want[1], **tol), "identity entry ids on the transposed CSR went unnoticed"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", ad.CASES)
def test_gatv2_backward_with_dropout(dtype, h, heads):
    """both directions against float64 autograd of the per-entry reference with w as a constant, GRAD_TOL of test_gatv2_gpu.py; the
    transposed call takes perm, and with identity ids it must miss the bound on `edges`"""
    n, m, rowptr, col = ad.graph("edges")
    for p in ad.PS:
        check_backward(dtype, "edges", n, m, rowptr, col, h, heads, p, wrong_ids_must_fail=True)
    n, m, rowptr, col = ad.graph("small")
    check_backward(dtype, "small", n, m, rowptr, col, h, heads, 0.5)


def test_gatv2_backward_with_dropout_two_launches():
    n, m, rowptr, col = ls.two_launch_graph()
    h, heads = ad.TWO_LAUNCH
    check_backward(torch.float32, "two-launch", n, m, rowptr, col, h, heads, 0.5)


def test_gatv2_backward_rate_zero_is_the_base_call():
    n, m, rowptr, col = ad.graph("small")
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    gt, _ = g.transposed()
    h, heads, dtype = 32, 8, torch.float32
    torch.manual_seed(3)
    Xd, Xs, G = (torch.randn(r, h, device=DEV) for r in (n, m, n))
    att = torch.randn(h, device=DEV) / 2
    lse, delta = torch.randn(n, heads, device=DEV), torch.randn(n, heads, device=DEV)
    from test_gatv2_gpu import call_bwd as base_bwd

    for transposed, gr, own, oth in ((False, g, Xd, Xs), (True, gt, Xs, Xd)):
        a, da = base_bwd(dtype, transposed, gr.nrows, gr.rowptr, gr.col, own, oth, att, h, heads, G, lse, delta, ad.SLOPE)
        b, db = call_bwd(dtype, transposed, gr, own, oth, att, h, heads, G, lse, delta, None, 0.0, ad.SEED)
        assert torch.equal(a, b) and (transposed or torch.equal(da, db))


# ---- the autograd functions ----
FN_TOL = {torch.float32: dict(rtol=1e-4, atol=1e-4), torch.float64: dict(rtol=1e-10, atol=1e-11)}


def run_function(kind, g, tensors, heads, **kw):
    if kind == "gat":
        return gat_aggregate(g, *tensors, ad.SLOPE, **{k: v for k, v in kw.items() if k != "fused"})
    if kind == "sa":
        return sparse_attention(g, *tensors, heads=heads, **kw)
    return gatv2_aggregate(g, *tensors, heads=heads, negative_slope=ad.SLOPE, **kw)


def function_operands(kind, n, m, h, heads, dtype):
    torch.manual_seed(11)
    if kind == "gat":
        return [torch.randn(n, heads, dtype=dtype), torch.randn(m, heads, dtype=dtype), torch.randn(m, h, dtype=dtype)]
    if kind == "sa":
        return [torch.randn(n, h, dtype=dtype), torch.randn(m, h, dtype=dtype), torch.randn(m, h, dtype=dtype)]
    return [torch.randn(n, h, dtype=dtype), torch.randn(m, h, dtype=dtype), torch.randn(h, dtype=dtype) * (h // heads) ** -0.5]


def function_reference(kind, n, rowptr, col, tensors, h, heads, p, dtype):
    """float64 autograd of the reference with the mirror's w -> (out, grads)"""
    t64 = [t.to(DEV).double().requires_grad_() for t in tensors]
    if kind == "gat":
        ops = dict(A=t64[0], B=t64[1], V=t64[2], att=None, scalar=ad.SLOPE)
    elif kind == "sa":
        ops = dict(A=t64[0], B=t64[1], V=t64[2], att=None, scalar=(h // heads) ** -0.5)
    else:
        ops = dict(A=t64[0], B=t64[1], V=t64[1], att=t64[2], scalar=ad.SLOPE)
    r = ad.reference(kind, dtype, n, rowptr, col, ops, h, heads, ad.weights(len(col), heads, p, ad.SEED), DEV)
    return r["ref"], t64


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ad.KINDS)
def test_autograd_with_dropout(kind, dtype):
    """fused gradients against float64 autograd of the reference; with one seed fused and unfused drop the same entries; the same
    torch.manual_seed gives the same bits twice"""
    n, m, rowptr, col = ad.graph("small")
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    h, heads, p = 32, 4, 0.5
    tol = FN_TOL[dtype]
    tensors = function_operands(kind, n, m, h, heads, dtype)
    G = torch.randn(n, h, dtype=dtype, device=DEV)
    ref, t64 = function_reference(kind, n, rowptr, col, tensors, h, heads, p, dtype)
    ref.backward(G.double())
    results = {}
    for fused in ((True,) if kind == "gat" else (True, False)):
        dev = [t.to(DEV).requires_grad_() for t in tensors]
        out = run_function(kind, g, dev, heads, dropout=p, seed=ad.SEED, fused=fused)
        out.backward(G)
        results[fused] = (out.detach(), [t.grad for t in dev])
        assert torch.allclose(out.detach().double(), ref.detach(), **tol), f"fused={fused}"
        for i, (d, c) in enumerate(zip(dev, t64)):
            print(f"{kind} dropout autograd {dtype} fused={fused} operand {i}: max abs err = {(d.grad.double() - c.grad).abs().max().item():.3e}")
            assert d.grad.dtype == dtype and torch.allclose(d.grad.double(), c.grad, **tol), f"fused={fused} operand {i}"
    if False in results:
        assert torch.allclose(results[True][0], results[False][0], **tol)
        for a, b in zip(results[True][1], results[False][1]):
            assert torch.allclose(a, b, **tol)
    # without dropout the result is another one, and dropout = 0 is the call without the argument
    with torch.no_grad():
        dev = [t.to(DEV) for t in tensors]
        plain = run_function(kind, g, dev, heads)
        assert torch.equal(run_function(kind, g, dev, heads, dropout=0.0, seed=ad.SEED), plain)
        assert not torch.allclose(results[True][0], plain, **tol)
    # seed = None: drawn from torch's default generator
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        dev = [t.to(DEV).requires_grad_() for t in tensors]
        out = run_function(kind, g, dev, heads, dropout=p)
        out.backward(G)
        runs.append([out.detach()] + [t.grad for t in dev])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the same torch.manual_seed gives the same bits"
    other = run_function(kind, g, [t.to(DEV) for t in tensors], heads, dropout=p)
    assert not torch.equal(other, runs[0][0]), "the next call draws the next seed"


# ---- the layers ----
def layer_graph(rng, n=600):
    rowptr, col = random_csr(rng, n, n, 9, empty_frac=0.1)
    return SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))


def test_gatv2conv_drops_in_training_only(rng):
    adj = layer_graph(rng)
    x = torch.randn(600, 24, device=DEV)
    torch.manual_seed(0)
    conv = gnn.GATv2Conv(24, 8, heads=4, dropout=0.5).to(DEV)
    torch.manual_seed(0)
    plain = gnn.GATv2Conv(24, 8, heads=4, dropout=0.0).to(DEV)
    with torch.no_grad():
        trained = conv.train()(x, adj)
        evaluated = conv.eval()(x, adj)
        assert not torch.allclose(trained, evaluated, rtol=1e-3, atol=1e-3), "train() applies attention dropout"
        assert torch.equal(evaluated, plain.eval()(x, adj)) and torch.equal(evaluated, plain.train()(x, adj)), "eval() is the layer without dropout"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("layer", [gnn.GATConv, gnn.TransformerConv, gnn.GATv2Conv])
def test_one_optimiser_step_with_attention_dropout(rng, layer, fused, dtype):
    """float32, and the layer after .to(torch.bfloat16): the composed backwards then take delta as the row sum of pr * dpr"""
    adj = layer_graph(rng)
    torch.manual_seed(1)
    conv = layer(24, 8, heads=4, dropout=0.6, fused=fused).to(DEV, dtype).train()
    before = copy.deepcopy(conv.state_dict())
    opt = torch.optim.SGD(conv.parameters(), lr=0.1)
    x = torch.randn(600, 24, device=DEV).to(dtype).requires_grad_()
    out = conv(x, adj)
    out.float().square().mean().backward()
    opt.step()
    assert out.shape == (600, 32) and torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    for name, prm in conv.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    assert any(not torch.equal(before[k], v) for k, v in conv.state_dict().items())


def test_gatconv_fused_and_unfused_drop_the_same_entries(rng):
    """both paths draw one seed per forward: after the same torch.manual_seed they apply one mask"""
    adj = layer_graph(rng)
    x = torch.randn(600, 24, device=DEV)
    torch.manual_seed(2)
    fused = gnn.GATConv(24, 8, heads=4, dropout=0.5, fused=True).to(DEV).train()
    plain = copy.deepcopy(fused)
    plain.fused = False
    with torch.no_grad():
        torch.manual_seed(5)
        a = fused(x, adj)
        torch.manual_seed(5)
        b = plain(x, adj)
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)
        assert not torch.allclose(a, fused.eval()(x, adj), rtol=1e-3, atol=1e-3)
