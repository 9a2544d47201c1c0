"""The GATv2 aggregation on the GPU: pygim_gatv2_aggregate and pygim_gatv2_backward through the C ABI against float64 on the device, and
pygim_amd.gatv2_aggregate / gnn.GATv2Conv / gnn.GATv2 (autograd, training) against the per-entry CPU reference.

Forward bounds (include/pygim_hip.h): those of pygim_sparse_attention with EPS = 1e-5 (FLT32, FLT16, BF16) / 1e-12 (DBL64) and
Delta[r, k] = EPS * max_e sum_{f in head k} |att[f] * lrelu(z[e, f])| -- the pygim_sddmm bound on a score:
    |out - ref| <= (2 EPS + 2 Delta[r, k]) * sum_e p_ref[e] * |x_src[e]|
    |lse - ref| <= 2 EPS * (1 + |lse_ref|) + Delta[r, k]
and for the 16-bit types u * |ref| more on out, u = 2^-8 (BF16) / 2^-11 (FLT16), ref computed in float64 from the 16-bit inputs.
Gradients: the project's tolerances, rtol = atol = 1e-4 (FLT32), 1e-10 / 1e-11 (DBL64), against float64 autograd of the per-entry reference."""
import copy

import numpy as np
import pytest
import torch

from conftest import random_csr
from pygim_amd import _lib, gnn
from pygim_amd.attention import EdgeGraph, gatv2_aggregate
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_gpu import dev_csr, hub_graph, small_graph
from test_gatv2_cpu import gatv2_reference, ref_gatv2

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRAPHS = {"small": small_graph, "hub": hub_graph}
EPS = {torch.float32: 1e-5, torch.float64: 1e-12, torch.float16: 1e-5, torch.bfloat16: 1e-5}
U = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CODE = {torch.float32: _lib.FLT32, torch.float64: _lib.DBL64, torch.bfloat16: _lib.BF16, torch.float16: _lib.FLT16}
GRAD_TOL = {torch.float32: dict(rtol=1e-4, atol=1e-4), torch.float64: dict(rtol=1e-10, atol=1e-11)}
SHAPES = [(4, 4), (9, 3), (32, 1), (32, 4), (32, 8), (100, 4), (256, 1), (256, 8), (512, 2), (1024, 16)]
SLOPE = 0.2


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def compute_type(dtype):
    return torch.float32 if dtype in (torch.float16, torch.bfloat16) else dtype


def stream():
    return torch.cuda.current_stream().cuda_stream


def call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads, slope=SLOPE, out=None, want_lse=True):
    """Xd, Xs: [rows, ld] device tensors whose first h columns are the operands; -> (out, lse or None), NaN-filled before the call"""
    nnz = cc.numel()
    ws = torch.empty(max(_lib.gatv2_aggregate_workspace(CODE[dtype], n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((n, heads), float("nan"), dtype=compute_type(dtype), device=DEV) if want_lse else None
    _lib.gatv2_aggregate(CODE[dtype], n, rp.data_ptr(), cc.data_ptr(), nnz, Xd.data_ptr(), Xd.stride(0), Xs.data_ptr(), Xs.stride(0), att.data_ptr(), h,
                         heads, slope, out.data_ptr(), out.stride(0), lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out, lse


def call_bwd(dtype, transposed, nrows, rp, cc, own, oth, att, h, heads, G, lse, delta, slope=SLOPE, d_own=None, want_datt=None):
    """one pygim_gatv2_backward call; own, oth, G: [rows, ld] device tensors; -> (d_own, datt or None), NaN-filled before the call"""
    nnz = cc.numel()
    want_datt = (not transposed) if want_datt is None else want_datt
    ws = torch.empty(max(_lib.gatv2_backward_workspace(CODE[dtype], nrows, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    if d_own is None:
        d_own = torch.full((nrows, h), float("nan"), dtype=dtype, device=DEV)
    datt = torch.full((h,), float("nan"), dtype=compute_type(dtype), device=DEV) if want_datt else None
    _lib.gatv2_backward(CODE[dtype], int(transposed), nrows, rp.data_ptr(), cc.data_ptr(), nnz, own.data_ptr(), own.stride(0), oth.data_ptr(), oth.stride(0),
                        att.data_ptr(), h, heads, slope, G.data_ptr(), G.stride(0), lse.data_ptr(), delta.data_ptr(), d_own.data_ptr(), d_own.stride(0),
                        datt.data_ptr() if want_datt else 0, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return d_own, datt


def reference_dev(dtype, n, rowptr, col, Xd, Xs, att, h, heads, slope=SLOPE):
    """float64 on the device, from the operands as stored: (exact out, sum_e p |x_src| per output, lse with 0 for empty rows, Delta per
    row and head)"""
    hd = h // heads
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(torch.from_numpy(rowptr).long().to(DEV)))
    cc = torch.from_numpy(col).long().to(DEV)
    xs = Xs[:, :h].double()
    terms = (torch.nn.functional.leaky_relu(Xd[:, :h].double()[row] + xs[cc], slope) * att.double()).view(-1, heads, hd)
    s = terms.sum(-1)
    sabs = terms.abs().sum(-1)
    del terms
    delta = EPS[dtype] * torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_reduce_(0, row, sabs, "amax", include_self=True)
    m = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - m[row])
    l = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, e)
    msg = (e / l[row]).repeat_interleave(hd, dim=1) * xs[cc]
    ref = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg)
    mag = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add_(0, row, msg.abs())
    lse = torch.where(l > 0, m + torch.log(l), torch.zeros_like(l))
    return ref, mag, lse, delta


def out_bound(dtype, ref, mag, delta, h, heads):
    return (2 * EPS[dtype] + 2 * delta.repeat_interleave(h // heads, dim=1)) * mag + U[dtype] * ref.abs()


def check_fwd(tag, dtype, n, rowptr, rp, cc, Xd, Xs, att, h, heads, reference, slope=SLOPE):
    """one call under the bounds, every row written, empty rows zero, a second launch bit-equal, out the same without lse"""
    ref, mag, lse_ref, delta = reference
    out, lse = call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads, slope)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), "a row was not written"
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert (out[empty] == 0).all() and (lse[empty] == 0).all()
    err = (out.double() - ref).abs()
    bound = out_bound(dtype, ref, mag, delta, h, heads)
    lerr = (lse.double() - lse_ref).abs()
    lbound = 2 * EPS[dtype] * (1 + lse_ref.abs()) + delta
    print(f"gatv2_aggregate {tag}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3e}, "
          f"lse max err / bound = {(lerr / lbound).max().item():.3e}")
    assert torch.all(err <= bound)
    assert torch.all(lerr <= lbound)
    out2, lse2 = call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads, slope)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "two launches differ"
    without, none = call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads, slope, want_lse=False)
    assert none is None and torch.equal(out, without), "out depends on lse"
    return out


def strided(t, ld):
    """the same values in a buffer of row stride ld (the padding NaN: nothing may read it)"""
    if ld == t.size(1):
        return t
    buf = torch.full((t.size(0), ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.size(1)] = t
    return buf


def make_att(rng, h, heads, dtype):
    """uniform in [-1, 1] / sqrt(hd): scores of order 1 at every head width"""
    return torch.from_numpy(rng.uniform(-1, 1, size=h) * (h // heads) ** -0.5).to(DEV, compute_type(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", SHAPES)
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_gatv2_forward_parity(rng, dtype, h, heads, graph):
    """(4, 4): hd = 1, sixteen lane groups; (9, 3): scalar pieces, a head count that is no power of two; (32, *): 16-byte pieces, one to
    eight heads side by side; (100, 4): hd = 25 (FLT32: 16-byte pieces do not fit, DBL64: hd is odd); (256, 1): the whole wave one head;
    (512, 2): hd = 256, the cap (DBL64: two pieces per lane); (1024, 16): heads across blockIdx.y.  On the small graph every operand
    also with a padded aligned row stride and with a misaligned one (one element per lane, up to four pieces per lane at hd = 256)."""
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    Xd = torch.from_numpy(rng.uniform(-2, 2, size=(n, h))).to(DEV, dtype)
    Xs = torch.from_numpy(rng.uniform(-2, 2, size=(m, h))).to(DEV, dtype)
    att = make_att(rng, h, heads, dtype)
    reference = reference_dev(dtype, n, rowptr, col, Xd, Xs, att, h, heads)
    lds = [(h, h)]
    if graph == "small":
        for ld in (h + 2 * vec, h + 1):
            lds += [(ld, h), (h, ld)]
    for ldd, ldsrc in lds:
        check_fwd(f"{graph} {dtype} h={h} heads={heads} ld={ldd},{ldsrc}", dtype, n, rowptr, rp, cc, strided(Xd, ldd), strided(Xs, ldsrc), att, h, heads,
                  reference)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h,heads", [(32, 4), (256, 8), (100, 4)])
def test_gatv2_forward_16_bit(rng, dtype, h, heads):
    """16-bit x_dst, x_src and out, float32 att and lse; the reference is float64 on the 16-bit inputs.  |x_src| in [0.5, 2) with random
    signs, as in the existing 16-bit tests: the bound has no absolute term, so a result far below every |x_src| must be a cancellation
    that the sum p |x_src| term covers"""
    for graph in GRAPHS:
        n, m, rowptr, col = GRAPHS[graph](rng)
        rp, cc = dev_csr(rowptr, col)
        Xd = torch.from_numpy(rng.uniform(-2, 2, size=(n, h))).to(DEV, dtype)
        Xs = torch.from_numpy(rng.uniform(0.5, 2, size=(m, h)) * rng.choice([-1.0, 1.0], size=(m, h))).to(DEV, dtype)
        att = make_att(rng, h, heads, dtype)
        reference = reference_dev(dtype, n, rowptr, col, Xd, Xs, att, h, heads)
        for ld in ((h, h + 16, h + 1) if graph == "small" else (h,)):
            check_fwd(f"{graph} {dtype} h={h} heads={heads} ld={ld}", dtype, n, rowptr, rp, cc, strided(Xd, ld), strided(Xs, ld), att, h, heads, reference)


def test_gatv2_strided_out_nnz0_and_bad_arguments(rng):
    n, m, rowptr, col = small_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h, heads = 32, 4
    Xd, Xs, att = torch.randn(n, h, device=DEV), torch.randn(m, h, device=DEV), torch.randn(h, device=DEV) / 8 ** 0.5
    ref, mag, lse_ref, delta = reference_dev(torch.float32, n, rowptr, col, Xd, Xs, att, h, heads)
    bound = out_bound(torch.float32, ref, mag, delta, h, heads)
    for pad in (5, 8):   # a misaligned and an aligned stride of out, NaN guard columns behind every row
        wide = torch.full((n, h + pad), float("nan"), device=DEV)
        call_fwd(torch.float32, n, rp, cc, Xd, Xs, att, h, heads, out=wide)
        assert torch.all((wide[:, :h].double() - ref).abs() <= bound) and torch.isnan(wide[:, h:]).all(), "stores outside out[:, :h]"
    # nnz = 0: every row is empty; the forward is zeros, the backward is zeros, datt included
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    out, lse = call_fwd(torch.float32, n, rp0, cc[:0], Xd, Xs, att, h, heads)
    assert (out == 0).all() and (lse == 0).all()
    G, zl = torch.randn(n, h, device=DEV), torch.zeros(n, heads, device=DEV)
    d, datt = call_bwd(torch.float32, False, n, rp0, cc[:0], Xd, Xs, att, h, heads, G, zl, zl)
    assert (d == 0).all() and (datt == 0).all()
    rpt0 = torch.zeros(m + 1, dtype=torch.int32, device=DEV)
    d, none = call_bwd(torch.float32, True, m, rpt0, cc[:0], Xs, Xd, att, h, heads, G, zl, zl)
    assert none is None and (d == 0).all()
    # bad arguments
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    o = torch.empty(n, h, device=DEV)
    da = torch.empty(h, device=DEV)
    nnz = len(col)
    fwd_head = (n, rp.data_ptr(), cc.data_ptr(), nnz, Xd.data_ptr(), h, Xs.data_ptr(), h, att.data_ptr())
    bwd_head = (n, rp.data_ptr(), cc.data_ptr(), nnz, Xd.data_ptr(), h, Xs.data_ptr(), h, att.data_ptr())
    bwd_tail = (SLOPE, G.data_ptr(), h, zl.data_ptr(), zl.data_ptr(), o.data_ptr(), h)
    with pytest.raises(_lib.PygimError):   # integer types have no such aggregation
        _lib.gatv2_aggregate(_lib.INT32, *fwd_head, h, heads, SLOPE, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # heads must divide h
        _lib.gatv2_aggregate(_lib.FLT32, *fwd_head, h, 5, SLOPE, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # a workspace smaller than pygim_gatv2_aggregate_workspace says
        _lib.gatv2_aggregate(_lib.FLT32, *fwd_head, h, heads, SLOPE, o.data_ptr(), h, 0, ws.data_ptr(), 16)
    with pytest.raises(_lib.PygimError):   # ... or misaligned
        _lib.gatv2_aggregate(_lib.FLT32, *fwd_head, h, heads, SLOPE, o.data_ptr(), h, 0, ws.data_ptr() + 4, ws.numel() - 4)
    with pytest.raises(_lib.PygimError):
        _lib.gatv2_backward(_lib.INT32, 0, *bwd_head, h, heads, *bwd_tail, da.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):
        _lib.gatv2_backward(_lib.FLT32, 0, *bwd_head, h, 5, *bwd_tail, da.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):
        _lib.gatv2_backward(_lib.FLT32, 0, *bwd_head, h, heads, *bwd_tail, da.data_ptr(), ws.data_ptr(), 16)
    with pytest.raises(_lib.PygimError):
        _lib.gatv2_backward(_lib.FLT32, 0, *bwd_head, h, heads, *bwd_tail, da.data_ptr(), ws.data_ptr() + 4, ws.numel() - 4)
    with pytest.raises(_lib.PygimError):   # datt belongs to the call on the CSR of A (rejected before the CSR is looked at)
        _lib.gatv2_backward(_lib.FLT32, 1, *bwd_head, h, heads, *bwd_tail, da.data_ptr(), ws.data_ptr(), ws.numel())
    # a head wider than 256 features: h = 514, heads = 2 (the operands are never read: the call is rejected before any launch)
    wd, wsrc, wa = torch.zeros(n, 514, device=DEV), torch.zeros(m, 514, device=DEV), torch.zeros(514, device=DEV)
    big = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    wide_head = (n, rp.data_ptr(), cc.data_ptr(), nnz, wd.data_ptr(), 514, wsrc.data_ptr(), 514, wa.data_ptr(), 514, 2, SLOPE)
    with pytest.raises(_lib.PygimError):
        _lib.gatv2_aggregate(_lib.FLT32, *wide_head, wd.data_ptr(), 514, 0, big.data_ptr(), big.numel())
    with pytest.raises(_lib.PygimError):
        _lib.gatv2_backward(_lib.FLT32, 0, *wide_head, wd.data_ptr(), 514, zl.data_ptr(), zl.data_ptr(), wd.data_ptr(), 514, 0, big.data_ptr(), big.numel())
    assert _lib.gatv2_aggregate_workspace(_lib.FLT32, n, nnz, 512, 2) == _lib.gat_aggregate_workspace(_lib.FLT32, n, nnz, 512, 2)
    assert _lib.gatv2_backward_workspace(_lib.FLT32, n, nnz, 512, 2) > _lib.spmm_values_workspace(_lib.FLT32, n, nnz, 512, 2)
    for wsf in (_lib.gatv2_aggregate_workspace, _lib.gatv2_backward_workspace):
        for bad in ((_lib.FLT32, h, 5), (_lib.FLT32, 514, 2), (_lib.INT32, h, heads)):
            with pytest.raises(_lib.PygimError):
                wsf(bad[0], n, nnz, bad[1], bad[2])


def backward_case(dtype, n, m, rowptr, col, Xd, Xs, att, G, h, heads, slope=SLOPE):
    """float64 autograd of the per-entry reference on the device, from the operands as stored: (dx_dst, dx_src, datt) and, in the compute
    type of ``dtype``, the lse and delta = head sums of G * out that the backward takes"""
    hd = h // heads
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(torch.from_numpy(rowptr).long().to(DEV)))
    cc = torch.from_numpy(col).long().to(DEV)
    xd, xs, a = (t.double().detach().clone().requires_grad_() for t in (Xd, Xs, att))
    s = (torch.nn.functional.leaky_relu(xd[row] + xs[cc], slope) * a).view(-1, heads, hd).sum(-1)
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=DEV).index_reduce_(0, row, s.detach(), "amax", include_self=True)
    e = torch.exp(s - mx[row])
    l = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add(0, row, e)
    out = torch.zeros(n, h, dtype=torch.float64, device=DEV).index_add(0, row, (e / l[row]).repeat_interleave(hd, dim=1) * xs[cc])
    out.backward(G.double())
    lse = torch.where(l > 0, mx + torch.log(l.detach().clamp_min(1e-300)), torch.zeros_like(mx)).detach()
    delta = (G.double() * out.detach()).view(n, heads, hd).sum(-1)
    ct = compute_type(dtype)
    return (xd.grad, xs.grad, a.grad), lse.to(ct).contiguous(), delta.to(ct).contiguous()


def check_bwd(tag, dtype, g, gt, Xd, Xs, att, G, lse, delta, h, heads, want, lds=None, slope=SLOPE):
    """both directions under the tolerance, every row written, rows / columns without entries zero, a second launch bit-equal"""
    ld_own, ld_oth, ldg, ldd = lds or (h, h, h, h)
    tol = GRAD_TOL[dtype]
    results = []
    for transposed, gr, own, oth in ((False, g, Xd, Xs), (True, gt, Xs, Xd)):
        d_buf = torch.full((gr.nrows, ldd), float("nan"), dtype=dtype, device=DEV)
        args = (dtype, transposed, gr.nrows, gr.rowptr, gr.col, strided(own, ld_own), strided(oth, ld_oth), att, h, heads, strided(G, ldg), lse, delta, slope)
        d, datt = call_bwd(*args, d_own=d_buf)
        assert not torch.isnan(d[:, :h]).any() and torch.isnan(d[:, h:]).all(), "a row was not written, or a store went outside d_own[:, :h]"
        empty = (gr.rowptr[1:] == gr.rowptr[:-1])
        assert (d[empty][:, :h] == 0).all(), "rows / columns without entries get zero gradient rows"
        d2, datt2 = call_bwd(*args, d_own=torch.full_like(d_buf, float("nan")))
        assert torch.equal(d[:, :h], d2[:, :h]), "two launches differ"
        if transposed:
            assert datt is None
        else:
            assert not torch.isnan(datt).any() and torch.equal(datt, datt2), "datt: two launches differ"
            results.append(("datt", datt, want[2]))
        results.append(("dx_src" if transposed else "dx_dst", d[:, :h], want[1] if transposed else want[0]))
    for name, got, ref in results:
        err = (got.double() - ref).abs()
        print(f"gatv2_backward {tag} {name}: max abs err = {err.max().item():.3e}, max err / (atol + rtol |ref|) = "
              f"{(err / (tol['atol'] + tol['rtol'] * ref.abs())).max().item():.3e}")
        assert torch.allclose(got.double(), ref, **tol), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", [(9, 3), (32, 4), (100, 4), (256, 8), (512, 2)])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_gatv2_backward_parity(rng, dtype, h, heads, graph):
    """pygim_gatv2_backward, both directions, against float64 autograd.  Operands are randn, att randn / sqrt(hd) (scores of order 1 at
    every head width, what the default scale does for the sparse-attention test).  On the small graph also with misaligned strides of
    every operand and of d_own (one element per lane; NaN padding that nothing may read, NaN guard columns that nothing may write)."""
    n, m, rowptr, col = GRAPHS[graph](rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    gt, _ = g.transposed()
    torch.manual_seed(21)
    Xd, Xs, G = (torch.randn(r, h, dtype=dtype, device=DEV) for r in (n, m, n))
    att = torch.randn(h, dtype=dtype, device=DEV) * (h // heads) ** -0.5
    want, lse, delta = backward_case(dtype, n, m, rowptr, col, Xd, Xs, att, G, h, heads)
    check_bwd(f"{graph} {dtype} h={h} heads={heads}", dtype, g, gt, Xd, Xs, att, G, lse, delta, h, heads, want)
    if graph == "small":
        check_bwd(f"{graph} {dtype} h={h} heads={heads} misaligned", dtype, g, gt, Xd, Xs, att, G, lse, delta, h, heads, want, lds=(h + 1, h + 3, h + 1, h + 5))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gatv2_integer_valued_operands(rng, dtype):
    """integer-valued x_dst, x_src in [-4, 4] and att in [-1, 1], slope 0.25, hd = 4: one z in nine is exactly 0, every z, leaky_relu(z)
    and score (at most 32) is exact in float32, only lse, exp and the sums round.  The forward meets its bound and the gradients match float64 autograd through
    torch.nn.functional.leaky_relu, whose derivative at 0 is the slope: a kernel that took 1 there would miss by att * ds on one entry
    in nine"""
    n, m, rowptr, col = small_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    gt, _ = g.transposed()
    h, heads, slope = 32, 8, 0.25
    Xd = torch.from_numpy(rng.integers(-4, 5, size=(n, h))).to(DEV, dtype)
    Xs = torch.from_numpy(rng.integers(-4, 5, size=(m, h))).to(DEV, dtype)
    att = torch.from_numpy(rng.integers(-1, 2, size=h)).to(DEV, dtype)
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(rp.long()))
    assert ((Xd[row] + Xs[cc.long()]) == 0).float().mean() > 0.05, "this test is about z == 0"
    reference = reference_dev(dtype, n, rowptr, col, Xd, Xs, att, h, heads, slope)
    check_fwd(f"integers {dtype}", dtype, n, rowptr, rp, cc, Xd, Xs, att, h, heads, reference, slope)
    torch.manual_seed(23)
    G = torch.randn(n, h, dtype=dtype, device=DEV)
    want, lse, delta = backward_case(dtype, n, m, rowptr, col, Xd, Xs, att, G, h, heads, slope)
    check_bwd(f"integers {dtype}", dtype, g, gt, Xd, Xs, att, G, lse, delta, h, heads, want, slope=slope)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_autograd_on_device_matches_the_cpu_reference(rng, dtype):
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert g.rowptr.is_cuda
    tol = GRAD_TOL[dtype]
    heads, h = 4, 32
    torch.manual_seed(21)
    Xd, Xs, att = torch.randn(n, h, dtype=dtype), torch.randn(m, h, dtype=dtype), torch.randn(heads, h // heads, dtype=dtype) * (h // heads) ** -0.5
    G = torch.randn(n, h, dtype=dtype)
    cpu = [t.clone().double().requires_grad_() for t in (Xd, Xs, att)]   # clone: .double() of a float64 tensor is the tensor itself
    ref = ref_gatv2(rowptr, col, *cpu, heads, n)
    ref.backward(G.double())
    for fused in (True, False):
        dev = [t.to(DEV).requires_grad_() for t in (Xd, Xs, att)]
        out = gatv2_aggregate(g, *dev, heads=heads, fused=fused)
        assert out.is_cuda
        out.backward(G.to(DEV))
        assert torch.allclose(out.detach().cpu().double(), ref.detach(), **tol)
        for name, d, c in zip(("x_dst", "x_src", "att"), dev, cpu):
            print(f"gatv2_aggregate autograd {dtype} fused={fused} d{name}: max abs err = {(d.grad.cpu().double() - c.grad).abs().max().item():.3e}")
            assert d.grad.dtype == dtype and d.grad.shape == c.shape and torch.allclose(d.grad.cpu().double(), c.grad, **tol), name
        # CPU tensors are staged to the device and come home
        out_host = gatv2_aggregate(g, Xd, Xs, att, heads=heads, fused=fused)
        assert not out_host.is_cuda and torch.equal(out_host, out.detach().cpu())


def test_wide_heads_run_unfused_on_the_device(rng):
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    Xd, Xs, att = torch.randn(n, 300, device=DEV), torch.randn(m, 300, device=DEV), torch.randn(300, device=DEV) / 300 ** 0.5
    out = gatv2_aggregate(g, Xd, Xs, att, heads=1)
    ref = ref_gatv2(rowptr, col, Xd.cpu().double(), Xs.cpu().double(), att.cpu().double(), 1, n)
    assert torch.allclose(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_gradients_in_bfloat16(rng):
    """bfloat16 x_dst, x_src and G, float32 att; the feature gradients come back in bfloat16, rounded once from float32 sums, datt in
    float32, against float64 on the CPU from the same 16-bit operands.  Per entry, with B[e] = sum_f |att lrelu(z)| per head (the
    magnitude of a score), A[e] = sum_f |G[r, f] x_src[c, f]| per head (the magnitude of dp) and
    rel = 2 EPS max B + 2 EPS (1 + max |lse|) + EPS, the relative error of a recomputed probability exp(s - lse) (score, lse, exp):
      delta[r] = sum_f G out is taken from the stored out: rounded to bfloat16, off by D[r] = u sum_f |G out| per head, and before that
        within the forward's own bound, off by E[r] = (2 EPS + 2 EPS max B) sum_e p A; beside the EPS of its float32 sum.  It enters
        ds = p (dp - delta) through p;
      ds: the factor p is off by rel, dp by EPS A, delta by D + E + EPS sum_f |G out|, so with C[r] = sum_f |G out| >= |delta|
        |ds - ref| <= Wd[e] := p ((2 rel + 3 EPS + 1e-6) (A[e] + C[r]) + D[r] + E[r])           (1e-6: the float32 products)
      dx_dst = sum_e ds att lrelu'(z):    u |ref| + sum_e Wd |att| lrelu' + EPS sum_e |t|        (the last: the float32 sum)
      dx_src = sum_e (p G + ds att lrelu'):  u |ref| + (rel + EPS) sum_e p |G| + sum_e Wd |att| lrelu' + EPS sum_e |t|
      datt   = sum_e ds lrelu(z):         sum_e Wd |lrelu(z)| + EPS sum_e |ds lrelu(z)|          (float32: no rounding to 16 bits)"""
    n, m, rowptr, col = small_graph(rng)
    check_gradients_16_bit(torch.bfloat16, n, m, rowptr, col, 64, 4)


def wrapper_gradients(g, Xd, Xs, att, G, h, heads):
    """(dx_dst, dx_src, datt) through the autograd wrapper"""
    dev = [t.to(DEV).requires_grad_() for t in (Xd, Xs, att)]
    out = gatv2_aggregate(g, *dev, heads=heads, negative_slope=SLOPE)
    out.backward(G.to(DEV))
    assert out.dtype == Xd.dtype and [t.grad.dtype for t in dev] == [Xd.dtype, Xd.dtype, torch.float32]
    return [t.grad for t in dev]


def check_gradients_16_bit(dtype, n, m, rowptr, col, h, heads, run=wrapper_gradients):
    """the bound of test_gradients_in_bfloat16 (u = 2^-8 / 2^-11) for any graph and head shape; run(g, Xd, Xs, att, G, h, heads) with host
    operands -> the three gradients on the device"""
    u, eps = U[dtype], 1e-5
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    hd = h // heads
    torch.manual_seed(22)
    Xd, Xs, G = (torch.randn(r, h).to(dtype) for r in (n, m, n))
    att = torch.randn(h) * hd ** -0.5
    grads = run(g, Xd, Xs, att, G, h, heads)
    cpu = [t.double().requires_grad_() for t in (Xd, Xs, att)]
    ref_out = ref_gatv2(rowptr, col, *cpu, heads, n, SLOPE)
    ref_out.backward(G.double())
    row = torch.repeat_interleave(torch.arange(n), torch.diff(torch.from_numpy(rowptr).long()))
    cc = torch.from_numpy(col).long()
    wide = lambda t: t.repeat_interleave(hd, dim=1)
    heads_sum = lambda t: t.view(-1, heads, hd).sum(-1)
    xd, xs, a, gg = Xd.double(), Xs.double(), att.double(), G.double()
    z = xd[row] + xs[cc]
    lz = torch.nn.functional.leaky_relu(z, SLOPE)
    dl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))
    s = heads_sum(lz * a)
    B = heads_sum((lz * a).abs())
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - mx[row])
    l = torch.zeros(n, heads, dtype=torch.float64).index_add_(0, row, e)
    P = e / l[row]
    lse = torch.where(l > 0, mx + torch.log(l.clamp_min(1e-300)), torch.zeros_like(l))
    rel = 2 * eps * B.max().item() + 2 * eps * (1 + lse.abs().max().item()) + eps
    A = heads_sum((gg[row] * xs[cc]).abs())
    C = heads_sum((gg * ref_out.detach()).abs())
    D = u * C
    ds = P * (heads_sum(gg[row] * xs[cc]) - heads_sum(gg * ref_out.detach())[row])
    E = (2 * eps + 2 * eps * B.max().item()) * torch.zeros(n, heads, dtype=torch.float64).index_add_(0, row, P * A)
    Wd = P * ((2 * rel + 3 * eps + 1e-6) * (A + C[row]) + D[row] + E[row])
    t_mag = wide(Wd) * a.abs() * dl
    t_abs = wide(ds.abs()) * a.abs() * dl
    bound_dst = torch.zeros(n, h, dtype=torch.float64).index_add_(0, row, t_mag + eps * t_abs)
    bound_src = torch.zeros(m, h, dtype=torch.float64).index_add_(0, cc, t_mag + eps * t_abs + (rel + eps) * wide(P) * gg[row].abs())
    bound_att = (wide(Wd) * lz.abs() + eps * wide(ds.abs()) * lz.abs()).sum(0)
    for name, d, c, bound, uu in (("x_dst", grads[0], cpu[0], bound_dst, u), ("x_src", grads[1], cpu[1], bound_src, u), ("att", grads[2], cpu[2], bound_att, 0.0)):
        assert not torch.isnan(d).any(), f"d{name}: not written"
        err = (d.cpu().double() - c.grad).abs()
        full = uu * c.grad.abs() + bound + 2.0 ** -24
        print(f"gatv2_aggregate {dtype} h={h} heads={heads} d{name}: max err / bound = {(err / full).max().item():.3f}")
        assert torch.all(err <= full), name


@pytest.mark.parametrize("mode", ["to", "autocast"])
@pytest.mark.parametrize("fused", [True, False])
def test_gatv2conv_in_bfloat16(rng, mode, fused):
    """after conv.to(torch.bfloat16) and under torch.autocast: forward and backward run, everything is finite and of the expected dtype"""
    n = 600
    rowptr, col = random_csr(rng, n, n, 9, empty_frac=0.1)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(0)
    conv = gnn.GATv2Conv(24, 8, heads=4, fused=fused).to(DEV)
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


def test_gatv2_sgd_steps_match_the_cpu_reference(rng):
    """a 2-layer GATv2, 4 SGD steps in float64: losses and parameter gradients as with the per-entry plain-torch layer on the CPU; then one
    float32 forward, fused against unfused"""
    n, f_in, hid, f_out, heads = 1500, 16, 32, 8, 4
    rowptr, col = random_csr(rng, n, n, 9)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.GATv2(f_in, hid, f_out, num_layers=2, dropout=0.0, heads=heads, fused=True).double()

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
        conv.forward = (lambda c: lambda x, adj_t: gatv2_reference(c, x, rowptr, col, n))(conv)
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
