"""Softmax aggregation per feature on the GPU: pygim_spmm_softmax and pygim_spmm_softmax_backward through the C ABI against the bounds of
include/pygim_hip.h, then pygim_amd.reduce.spmm_softmax (autograd) and gnn.GENConv / GEN.

  forward   |out - exact| <= (2 EPS + 2 Delta) sum_e p[e] |x[e]|  (+ u |exact| for a 16-bit out)      Delta = EPS max_e |t x[e]|
            |lse - exact| <= 2 EPS (1 + |exact|) + Delta                EPS = 1e-5 (float32 arithmetic) / 1e-12 (float64)
  backward  dX and dT.sum(0) against float64 autograd of the per-entry statement at GRAD_TOL of test_gatv2_gpu.py; 16-bit:
            u |ref| + |t| u sum_e |G| p |out| (the rounding of the stored out) + the float32 tolerance
The reference is float64 on the CPU, computed from the operands exactly as the kernels get them (16-bit X widened, t in the compute type)."""
import copy

import numpy as np
import pytest
import torch

import launch_shapes as ls
import run_edges
import test_reduce_gpu as t_red
from conftest import random_csr
from pygim_amd import _lib, gnn
from pygim_amd.attention import EdgeGraph, _gather_code
from pygim_amd.reduce import spmm_reduce, spmm_softmax
from pygim_amd.sparse_tensor import SparseTensorShim
from test_gatv2_gpu import GRAD_TOL
from test_launch_shapes_gpu import TORCH, Views
from test_multi_reduce_gpu import bits, nonfinite_graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = (torch.bfloat16, torch.float16)
EPS_T = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 1e-5, torch.float16: 1e-5}
ROUND = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NAN, INF = float("nan"), float("inf")


def compute_of(dtype):
    return torch.float32 if dtype in HALF else dtype


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call_fwd(dtype, n, rp, cc, X, t, h, want_lse=True, out=None):
    """X: [rows, ldx] device tensor whose first h columns are the operand; t: [h] device, compute type; out: a [n, h] view to write, or
    None for a fresh one.  out and lse are NaN-filled first, so that an element the kernels did not write shows"""
    code = _gather_code(dtype)
    nnz = cc.numel()
    ws = torch.empty(max(_lib.spmm_softmax_workspace(code, n, nnz, h), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, h), NAN, dtype=dtype, device=DEV)
    lse = torch.full((n, h), NAN, dtype=compute_of(dtype), device=DEV) if want_lse else None
    _lib.spmm_softmax(code, n, rp.data_ptr(), cc.data_ptr(), nnz, X.data_ptr(), X.stride(0), t.data_ptr(), h, out.data_ptr(), out.stride(0),
                      0 if lse is None else lse.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out, lse


def reference64(n, rowptr, col, X64, t64):
    """float64 on the CPU -> out, lse, sum_e p |x| and max_e |s| per (row, feature); rows without entries hold 0, -inf, 0, 0"""
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    h = X64.size(1)
    x = X64[coll]
    s = x * t64
    idx = row.unsqueeze(1).expand(-1, h)
    m = torch.full((n, h), -INF, dtype=torch.float64).scatter_reduce(0, idx, s, "amax", include_self=True)
    smax = torch.zeros(n, h, dtype=torch.float64).scatter_reduce(0, idx, s.abs(), "amax", include_self=True)
    shift = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - shift[row])
    zero = lambda: torch.zeros(n, h, dtype=torch.float64)
    den = zero().index_add_(0, row, e)
    safe = den.clamp(min=1e-300)
    out = zero().index_add_(0, row, e * x) / safe
    mag = zero().index_add_(0, row, e * x.abs()) / safe
    lse = torch.where(den > 0, shift + torch.log(safe), torch.full_like(m, -INF))
    return out, lse, mag, smax


def bounds(dtype, out, lse, mag, smax):
    eps = EPS_T[dtype]
    delta = eps * smax
    b_out = (2 * eps + 2 * delta) * mag + ROUND[dtype] * out.abs()
    b_lse = 2 * eps * (1 + lse.abs()) + delta
    return b_out, b_lse


def composition32(n, rowptr, col, X64, t64):
    """the same aggregation in float32 torch ops on the CPU: maximum, exp, two sums, one division"""
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    h = X64.size(1)
    x = X64.float()[coll]
    s = x * t64.float()
    idx = row.unsqueeze(1).expand(-1, h)
    m = torch.full((n, h), -INF).scatter_reduce(0, idx, s, "amax", include_self=True)
    shift = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - shift[row])
    den = torch.zeros(n, h).index_add_(0, row, e)
    out = torch.zeros(n, h).index_add_(0, row, e * x) / den.clamp(min=1e-30)
    return out, shift + torch.log(den)


def reference_stays_inside_its_own_bounds(n, rowptr, col, X64, t64):
    """on the CPU, before anything is launched: the float32 torch composition of the same inputs lies inside the float32 bounds -- the
    bounds are not so tight that a plain float32 evaluation would miss them"""
    out, lse, mag, smax = reference64(n, rowptr, col, X64, t64)
    b_out, b_lse = bounds(torch.float32, out, lse, mag, smax)
    o32, l32 = composition32(n, rowptr, col, X64, t64)
    full = torch.from_numpy(np.diff(rowptr) > 0)
    assert ((o32.double() - out).abs() <= b_out).all() and ((l32.double() - lse).abs()[full] <= b_lse[full]).all()


def same(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def check_fwd(name, dtype, n, rowptr, col, rp, cc, Xh, X, th, h, out_view=None):
    """Xh: the operand on the host [m, h] in dtype; X: the device tensor handed to the kernels (its first h columns equal Xh; any row
    stride); th: t on the host in the compute type.  out_view(t): the view of a guarded buffer the result goes to, or None."""
    t = th.to(DEV)
    fresh = lambda: None if out_view is None else out_view(torch.full((n, h), NAN, dtype=dtype, device=DEV))
    out, lse = call_fwd(dtype, n, rp, cc, X, t, h, True, fresh())
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), f"{name}: an element was not written"
    out2, lse2 = call_fwd(dtype, n, rp, cc, X, t, h, True, fresh())
    assert same(out2, out) and same(lse2, lse), f"{name}: two launches differ"
    out3, none = call_fwd(dtype, n, rp, cc, X, t, h, False, fresh())
    assert none is None and same(out3, out), f"{name}: out depends on whether lse is asked for"
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert (out[empty] == 0).all() and (lse[empty] == -INF).all(), f"{name}: an empty row"
    ref, ref_lse, mag, smax = reference64(n, rowptr, col, Xh.double(), th.double())
    b_out, b_lse = bounds(dtype, ref, ref_lse, mag, smax)
    e_out = (out.cpu().double() - ref).abs()
    full = ~empty.cpu()
    e_lse = (lse.cpu().double() - ref_lse).abs()[full]
    live = b_out > 0
    print(f"{name}: out err / bound {float((e_out[live] / b_out[live]).max()) if live.any() else 0.0:.3g}, "
          f"lse err / bound {float((e_lse / b_lse[full]).max()) if full.any() else 0.0:.3g}")
    assert (e_out <= b_out).all(), f"{name}: out"
    assert (e_lse <= b_lse[full]).all(), f"{name}: lse"
    return out, lse


def draw(rng, shape, dtype, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(lo, hi, size=shape)).to(dtype)


# ---- every launch shape of k_softmax_gather: the `mean` table (test_softmax_aggr_cpu proves kind 10 answers like SPMM_REDUCE) ----
@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c.dtype}-h{c.h}-{c.mis or 'aligned'}") for c in ls.TABLES["mean"]])
def test_every_launch_shape_on_the_edges_graph(rng, case):
    shape = _lib.gather_launch_shape(_lib.SHAPE_SPMM_SOFTMAX, ls.CODE[case.dtype], case.h, 1, case.mis is None)
    assert tuple(shape[k] for k in _lib.SHAPE_FIELDS) == case.shape, (case, shape)
    dtype, h = TORCH[case.dtype], case.h
    n, m, rowptr, col = run_edges.graph("edges")
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = draw(rng, (m, h), dtype)
    th = draw(rng, (h,), compute_of(dtype), -2.0, 4.0)
    reference_stays_inside_its_own_bounds(n, rowptr, col, Xh.double(), th.double())
    for which in (("X", "out") if case.mis else (None,)):
        views = Views(case, which)
        X = views("X", Xh.to(DEV))
        check_fwd(f"edges {case.dtype} h={h} {case.mis} {which}", dtype, n, rowptr, col, rp, cc, Xh, X, th, h, out_view=lambda t: views("out", t))
        views.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("h", [9, 256])
@pytest.mark.parametrize("graph", ["one-row", "whole-batches"])
def test_run_boundaries(rng, graph, h, dtype):
    n, m, rowptr, col = run_edges.graph(graph)
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = draw(rng, (m, h), dtype)
    th = draw(rng, (h,), compute_of(dtype), -2.0, 4.0)
    reference_stays_inside_its_own_bounds(n, rowptr, col, Xh.double(), th.double())
    check_fwd(f"{graph} {dtype} h={h}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), th, h)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_out_wider_than_h_keeps_its_padding(rng, dtype):
    n, m, rowptr, col = run_edges.graph("edges")
    rp, cc = t_red.dev_csr(rowptr, col)
    for h, pad in ((9, 5), (64, 8)):   # a scalar path and an aligned 16-byte path (the padding keeps the row stride a multiple of a piece)
        Xh = draw(rng, (m, h), dtype)
        t = draw(rng, (h,), compute_of(dtype), -2.0, 4.0).to(DEV)
        buf = torch.full((n, h + pad), 7.0, dtype=dtype, device=DEV)
        call_fwd(dtype, n, rp, cc, Xh.to(DEV), t, h, True, out=buf[:, :h])
        assert (buf[:, h:] == 7.0).all(), "the padding columns were written"
        want, _ = call_fwd(dtype, n, rp, cc, Xh.to(DEV), t, h, True)
        assert torch.equal(buf[:, :h].float(), want.float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("h", [9, 256])
def test_a_large_temperature_stays_finite_and_zero_is_the_mean(rng, h, dtype):
    n, m, rowptr, col = run_edges.graph("edges")
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = draw(rng, (m, h), dtype)
    big = torch.full((h,), 1e4, dtype=compute_of(dtype))
    out, lse = check_fwd(f"t=1e4 {dtype} h={h}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), big, h)
    assert torch.isfinite(out).all() and torch.isfinite(lse[torch.from_numpy(np.diff(rowptr) > 0).to(DEV)]).all()
    zero = torch.zeros(h, dtype=compute_of(dtype))
    out, lse = check_fwd(f"t=0 {dtype} h={h}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), zero, h)   # the reference at t = 0 is the mean
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    mean = spmm_reduce(g, Xh.to(DEV), "mean")
    assert torch.allclose(out.double(), mean.double(), rtol=4 * EPS_T[dtype] + 2 * ROUND[dtype], atol=4 * EPS_T[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_non_finite_inputs(rng, dtype):
    """X[0, 0] = NaN, X[1, 1] = +inf, X[2, 2] = -inf on the graph of test_multi_reduce_gpu (a hub over three runs that holds columns 0, 1, 2
    once each, and one-entry rows on each of them): every (row, feature) that gathers one of them is non-finite, every other keeps the
    bits of the call with 0 in those three places"""
    n, m, rowptr, col = nonfinite_graph()
    rp, cc = t_red.dev_csr(rowptr, col)
    h = 9
    clean = draw(rng, (m, h), dtype)
    clean[0, 0] = clean[1, 1] = clean[2, 2] = 0
    Xh = clean.clone()
    Xh[0, 0], Xh[1, 1], Xh[2, 2] = NAN, INF, -INF
    th = draw(rng, (h,), compute_of(dtype), -2.0, 4.0)
    th[1], th[2] = 1.5, 1.5   # +inf scores in feature 1, -inf scores in feature 2
    out, _ = call_fwd(dtype, n, rp, cc, Xh.to(DEV), th.to(DEV), h)
    base, _ = check_fwd(f"finite {dtype}", dtype, n, rowptr, col, rp, cc, clean, clean.to(DEV), th, h)
    hit = torch.zeros(n, h, dtype=torch.bool)
    for r, f in ((0, 0), (1, 0), (0, 1), (2, 1), (0, 2), (3, 2)):
        hit[r, f] = True
    out, base = out.cpu(), base.cpu()
    assert not torch.isfinite(out[hit]).any(), "a (row, feature) that gathers a non-finite score stored a finite number"
    assert torch.equal(bits(out)[~hit], bits(base)[~hit]), "another row or feature changed"
    assert out[0, 1] == INF and out[2, 1] == INF, "+inf with t > 0 wins its softmax"
    th[1], th[2] = -1.5, -1.5   # the signs of the scores swapped: still non-finite, and nothing else moves
    out, _ = call_fwd(dtype, n, rp, cc, Xh.to(DEV), th.to(DEV), h)
    base, _ = call_fwd(dtype, n, rp, cc, clean.to(DEV), th.to(DEV), h)
    assert not torch.isfinite(out.cpu()[hit]).any() and torch.equal(bits(out.cpu())[~hit], bits(base.cpu())[~hit])


def test_no_entries_and_no_rows(rng):
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        n, h = 7, 9
        rp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
        cc = torch.zeros(0, dtype=torch.int32, device=DEV)
        X = draw(rng, (5, h), dtype).to(DEV)
        t = torch.ones(h, dtype=compute_of(dtype), device=DEV)
        out, lse = call_fwd(dtype, n, rp, cc, X, t, h)
        assert (out == 0).all() and (lse == -INF).all()
        out, lse = call_fwd(dtype, 0, rp[:1], cc, X, t, h)
        assert out.shape == (0, h)
        dX, dT = call_bwd(dtype, 5, torch.zeros(6, dtype=torch.int32, device=DEV), cc, X, t, h, X[:0], X[:0], lse[:0])
        assert (dX == 0).all() and (dT == 0).all()
    g = EdgeGraph(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), (0, 5))
    assert spmm_softmax(g, torch.randn(5, 4, device=DEV)).shape == (0, 4)


def test_rejections(rng):
    n, m, rowptr, col = run_edges.graph("whole-batches")
    rp, cc = t_red.dev_csr(rowptr, col)
    nnz, h = len(col), 8
    X = draw(rng, (m, h), torch.float32).to(DEV)
    t = torch.ones(h, device=DEV)
    out = torch.zeros(n, h, device=DEV)
    need = _lib.spmm_softmax_workspace(_lib.FLT32, n, nnz, h)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)

    def call(dtype=_lib.FLT32, h=h, ldx=None, ldo=None, wsp=None, wsb=None, Xp=None):
        _lib.spmm_softmax(dtype, n, rp.data_ptr(), cc.data_ptr(), nnz, X.data_ptr() if Xp is None else Xp, X.stride(0) if ldx is None else ldx, t.data_ptr(), h,
                          out.data_ptr(), h if ldo is None else ldo, 0, ws.data_ptr() if wsp is None else wsp, need if wsb is None else wsb, stream())

    call()
    for bad in (dict(dtype=_lib.INT32), dict(dtype=_lib.INT8), dict(dtype=_lib.INT16), dict(dtype=_lib.INT64), dict(ldo=h - 1), dict(ldx=h - 1), dict(h=0),
                dict(h=_lib.GATHER_MAX_H + 1), dict(wsb=need - 1), dict(wsp=ws.data_ptr() + 4), dict(wsp=0), dict(Xp=X.cpu().data_ptr())):
        with pytest.raises(_lib.PygimError) as e:
            call(**bad)
        assert e.value.code == _lib.ERR_INVALID, bad
    # the backward: the same rejections
    G, lse, dX = torch.zeros(n, h, device=DEV), torch.zeros(n, h, device=DEV), torch.zeros(m, h, device=DEV)
    mt, nt, rpt, rows_t, _ = run_edges.transpose_csr(n, m, rowptr, col)
    rpt, rows_t = t_red.dev_csr(rpt, rows_t)
    need_b = _lib.spmm_softmax_backward_workspace(_lib.FLT32, m, nnz, h)

    def back(dtype=_lib.FLT32, h=h, ldg=h, ldd=h, wsp=None, wsb=None):
        _lib.spmm_softmax_backward(dtype, m, rpt.data_ptr(), rows_t.data_ptr(), nnz, X.data_ptr(), h, t.data_ptr(), h, G.data_ptr(), ldg, out.data_ptr(), h,
                                   lse.data_ptr(), dX.data_ptr(), ldd, 0, ws.data_ptr() if wsp is None else wsp, need_b if wsb is None else wsb, stream())

    back()
    for bad in (dict(dtype=_lib.INT32), dict(dtype=_lib.INT64), dict(ldg=h - 1), dict(ldd=h - 1), dict(h=_lib.GATHER_MAX_H + 1), dict(wsb=need_b - 1),
                dict(wsp=ws.data_ptr() + 4), dict(wsp=0)):
        with pytest.raises(_lib.PygimError) as e:
            back(**bad)
        assert e.value.code == _lib.ERR_INVALID, bad
    torch.cuda.synchronize()


# ---- the backward through the C ABI ----
def call_bwd(dtype, ncols, rpt, rows_t, X, t, h, G, out, lse, want_dt=True):
    """dX and dT are NaN-filled first, so that an element the kernels did not write shows"""
    code = _gather_code(dtype)
    nnz = rows_t.numel()
    ws = torch.empty(max(_lib.spmm_softmax_backward_workspace(code, ncols, nnz, h), 16), dtype=torch.uint8, device=DEV)
    dX = torch.full((ncols, h), NAN, dtype=dtype, device=DEV)
    dT = torch.full((ncols, h), NAN, dtype=compute_of(dtype), device=DEV) if want_dt else None
    _lib.spmm_softmax_backward(code, ncols, rpt.data_ptr(), rows_t.data_ptr(), nnz, X.data_ptr(), X.stride(0), t.data_ptr(), h, G.data_ptr(), h, out.data_ptr(),
                               h, lse.data_ptr(), dX.data_ptr(), h, 0 if dT is None else dT.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return dX, dT


def autograd64(n, rowptr, col, X64, t64, G64):
    """float64 autograd of the per-entry statement on the CSR of A -> out, lse, dX, dt"""
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    h = X64.size(1)
    X, t = X64.clone().requires_grad_(), t64.clone().requires_grad_()
    x = X[coll]
    s = x * t
    m = torch.full((n, h), -INF, dtype=torch.float64).scatter_reduce(0, row.unsqueeze(1).expand(-1, h), s.detach(), "amax", include_self=True)
    shift = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - shift[row])
    den = torch.zeros(n, h, dtype=torch.float64).index_add(0, row, e)
    out = torch.zeros(n, h, dtype=torch.float64).index_add(0, row, e * x) / den.clamp(min=1e-300)
    out.backward(G64)
    lse = shift + torch.log(den.detach().clamp(min=1e-300))
    return out.detach(), lse, X.grad, t.grad, (e.detach() / den.detach().clamp(min=1e-300)[row], row, coll)


def backward_problem(rng, graph, h, dtype):
    """the graph is the CSR of A^T: A is its transpose"""
    ncols, nrows, rpt, rows_t = run_edges.graph(graph)
    _, _, rowptr, col, _ = run_edges.transpose_csr(ncols, nrows, rpt, rows_t)   # the CSR of A: nrows rows, ncols columns
    Xh = draw(rng, (ncols, h), dtype)
    th = draw(rng, (h,), compute_of(dtype), -2.0, 4.0)
    Gh = draw(rng, (nrows, h), dtype)
    return ncols, nrows, rpt, rows_t, rowptr, col, Xh, th, Gh


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", [9, 64, 256])
@pytest.mark.parametrize("graph", ["edges-T", "one-row", "whole-batches"])
def test_backward_matches_float64_autograd(rng, graph, h, dtype):
    ncols, nrows, rpt, rows_t, rowptr, col, Xh, th, Gh = backward_problem(rng, graph, h, dtype)
    out64, lse64, dX64, dt64, _ = autograd64(nrows, rowptr, col, Xh.double(), th.double(), Gh.double())
    rp_d, rows_d = t_red.dev_csr(rpt, rows_t)
    args = (dtype, ncols, rp_d, rows_d, Xh.to(DEV), th.to(DEV), h, Gh.to(DEV), out64.to(dtype).to(DEV), lse64.to(dtype).to(DEV))
    dX, dT = call_bwd(*args)
    assert not torch.isnan(dX).any() and not torch.isnan(dT).any(), "an element was not written"
    none = torch.from_numpy(np.diff(rpt) == 0).to(DEV)
    assert (dX[none] == 0).all() and (dT[none] == 0).all(), "a column without entries"
    tol = GRAD_TOL[dtype]
    print(f"{graph} {dtype} h={h}: dX err {float((dX.cpu().double() - dX64).abs().max()):.3g}, dt err {float((dT.sum(0).cpu().double() - dt64).abs().max()):.3g}")
    assert torch.allclose(dX.cpu().double(), dX64, **tol), "dX"
    assert torch.allclose(dT.sum(0).cpu().double(), dt64, **tol), "dt"
    dX2, dT2 = call_bwd(*args)
    assert same(dX2, dX) and same(dT2, dT), "two launches differ"
    dX3, nothing = call_bwd(*args, want_dt=False)
    assert nothing is None and same(dX3, dX), "dX depends on whether dT is asked for"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h", [9, 256])
@pytest.mark.parametrize("graph", ["edges-T", "one-row"])
def test_backward_16_bit(rng, graph, h, dtype):
    """X, G, out and dX in 16 bits; the reference takes the same X and G widened and the exact out, so the kernel's error holds the rounding
    of the stored out (u |out| in every entry's x - out) and the one rounding of dX"""
    ncols, nrows, rpt, rows_t, rowptr, col, Xh, th, Gh = backward_problem(rng, graph, h, dtype)
    out64, lse64, dX64, dt64, (p, row, coll) = autograd64(nrows, rowptr, col, Xh.double(), th.double(), Gh.double())
    u = ROUND[dtype]
    mid = torch.zeros(ncols, h, dtype=torch.float64).index_add_(0, coll, (Gh.double()[row] * p * out64[row]).abs()) * u   # u sum_e |G| p |out|
    rp_d, rows_d = t_red.dev_csr(rpt, rows_t)
    dX, dT = call_bwd(dtype, ncols, rp_d, rows_d, Xh.to(DEV), th.to(DEV), h, Gh.to(DEV), out64.to(dtype).to(DEV), lse64.float().to(DEV))
    assert dX.dtype == dtype and dT.dtype == torch.float32 and not torch.isnan(dX).any() and not torch.isnan(dT).any()
    tol = GRAD_TOL[torch.float32]
    b_dx = u * dX64.abs() + th.double().abs() * mid + tol["atol"] + tol["rtol"] * dX64.abs()
    b_dt = (Xh.double().abs() * mid).sum(0) + tol["atol"] + tol["rtol"] * dt64.abs()
    e_dx, e_dt = (dX.cpu().double() - dX64).abs(), (dT.sum(0).cpu().double() - dt64).abs()
    print(f"{graph} {dtype} h={h}: dX err / bound {float((e_dx / b_dx).max()):.3g}, dt err / bound {float((e_dt / b_dt).max()):.3g}")
    assert (e_dx <= b_dx).all() and (e_dt <= b_dt).all()


# ---- the wrapper and the layer ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_spmm_softmax_and_its_gradients_match_the_cpu_reference(rng, dtype):
    n, m, rowptr, col = run_edges.graph("edges")
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    h = 24
    Xh, th, Gh = draw(rng, (m, h), dtype), draw(rng, (h,), dtype, -2.0, 4.0), draw(rng, (n, h), dtype)
    out64, _, dX64, dt64, _ = autograd64(n, rowptr, col, Xh.double(), th.double(), Gh.double())
    X, t = Xh.to(DEV).requires_grad_(), th.to(DEV).requires_grad_()
    out = spmm_softmax(g, X, t)
    out.backward(Gh.to(DEV))
    tol = GRAD_TOL[dtype]
    assert out.dtype == dtype and torch.allclose(out.detach().cpu().double(), out64, **tol)
    assert X.grad.dtype == dtype and torch.allclose(X.grad.cpu().double(), dX64, **tol)
    assert t.grad.shape == (h,) and t.grad.dtype == dtype and torch.allclose(t.grad.cpu().double(), dt64, **tol)
    s = torch.tensor(1.5, dtype=dtype, device=DEV, requires_grad=True)   # a 0-d temperature: its gradient is the sum over the features
    spmm_softmax(g, X.detach(), s).backward(Gh.to(DEV))
    _, _, _, ds64, _ = autograd64(n, rowptr, col, Xh.double(), torch.full((h,), 1.5, dtype=torch.float64), Gh.double())
    assert s.grad.shape == () and torch.allclose(s.grad.cpu().double(), ds64.sum(), rtol=tol["rtol"], atol=h * tol["atol"])
    comp = spmm_softmax(g, X.detach(), t.detach(), fused=False)
    assert torch.allclose(comp.cpu().double(), out64, **tol)


def gen_forward_cpu(conv, x, rowptr, col):
    """GENConv in torch ops on the CPU, a message per stored entry: relu(x_src[j]) + eps, scatter softmax per feature, + x_dst, the MLP"""
    n = x.size(0)
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    src = x if conv.lin_src is None else conv.lin_src(x)
    msg = torch.relu(src[coll]) + conv.eps
    F_ = msg.size(1)
    s = msg * conv.t
    m = torch.zeros(n, F_, dtype=x.dtype).scatter_reduce(0, row.unsqueeze(1).expand(-1, F_), s.detach(), "amax", include_self=False)
    e = torch.exp(s - m[row])
    den = torch.zeros(n, F_, dtype=x.dtype).index_add(0, row, e)
    agg = torch.zeros(n, F_, dtype=x.dtype).index_add(0, row, e * msg) / den.clamp(min=1e-300)
    dst = x if conv.lin_dst is None else conv.lin_dst(x)
    return conv.mlp(agg + dst)


def small_adj(rng, n):
    rowptr, col = random_csr(rng, n, n, 12, empty_frac=0.1, long_rows=((11, 64), (n // 2, 700)))
    return rowptr, col, SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_genconv_fused_matches_the_composition(rng, dtype):
    n = 300
    rowptr, col, adj = small_adj(rng, n)
    torch.manual_seed(4)
    fused = gnn.GENConv(24, 16, t=0.8, learn_t=True).to(dtype).to(DEV)
    plain = copy.deepcopy(fused)
    plain.fused = False
    x = torch.randn(n, 24, dtype=dtype, device=DEV)
    G = torch.randn(n, 16, dtype=dtype, device=DEV)
    res = []
    for conv in (fused, plain):
        xi = x.clone().requires_grad_()
        out = conv(xi, adj)
        out.backward(G)
        res.append([out.detach(), xi.grad] + [p.grad for p in conv.parameters()])
    tol = GRAD_TOL[dtype]
    for a, b in zip(*res):
        assert torch.allclose(a, b, rtol=tol["rtol"], atol=tol["atol"] * max(1.0, float(b.abs().max())))


def test_genconv_in_bfloat16_under_autocast(rng):
    n = 700
    rowptr, col, adj = small_adj(rng, n)
    torch.manual_seed(1)
    conv = gnn.GENConv(32, 16, learn_t=True).to(DEV)
    x = torch.randn(n, 32, device=DEV)
    want = conv(x, adj)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = conv(x.requires_grad_(), adj)
    assert out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    assert (out.float() - want).abs().max() <= 0.05 * want.abs().max(), "bfloat16 forward far from the float32 one"
    out.float().square().mean().backward()
    assert torch.isfinite(x.grad).all() and conv.t.grad is not None and torch.isfinite(conv.t.grad)


def test_gen_sgd_steps_match_the_cpu_reference(rng):
    """a 2-layer GEN with a learnable temperature, 4 SGD steps in float64: losses and parameter gradients as with the per-entry plain-torch
    layer on the CPU (the tolerances of test_gatv2_sgd_steps_match_the_cpu_reference)"""
    n, f_in, hid, f_out = 700, 16, 32, 8
    rowptr, col, adj = small_adj(rng, n)
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.GEN(f_in, hid, f_out, num_layers=2, dropout=0.0, learn_t=True).double()

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
        conv.forward = (lambda c: lambda x, adj_t: gen_forward_cpu(c, x, rowptr, col))(conv)
    l_gpu, g_gpu = run(copy.deepcopy(base), DEV)
    l_cpu, g_cpu = run(cpu_model, "cpu")
    assert np.allclose(l_gpu, l_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_gpu, g_cpu):
        for x, y in zip(a, b):
            assert torch.allclose(x, y, rtol=1e-9, atol=1e-11)
