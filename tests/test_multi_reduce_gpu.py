"""Several statistics in one gather on the GPU: pygim_spmm_multi_reduce through the C ABI against the identities and bounds of
include/pygim_hip.h, then pygim_amd.reduce.spmm_multi_reduce (autograd) and gnn.PNAConv / PNA.

  sum, mean                    the bits of pygim_spmm_values with unit weights / pygim_spmm_reduce MEAN without values
  max, min, arg_max, arg_min   the bits of pygim_spmm_reduce MAX / MIN without values (16-bit X: of that call on X widened to float32)
  var                          within 3 u mean(x^2) of the float64 two-pass value, u = 1e-5 (float32 arithmetic) / 1e-12 (float64)
  std                          within bound(var) / ref_std + 2 epsilon ref_std
  16-bit outputs               2^-8 |exact| (bfloat16) / 2^-11 |exact| (float16) more
Every call is made three ways -- all six statistics with both args (the MOMENTS + BEST kernel), the four moment statistics alone and
max / min alone (the two other instantiations) -- and the blocks of the smaller calls must have the bits of the six-statistic call."""
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
from pygim_amd.reduce import spmm_multi_reduce
from pygim_amd.sparse_tensor import SparseTensorShim
from test_launch_shapes_gpu import TORCH, Views

pytestmark = pytest.mark.gpu

DEV = "cuda"
SUM, MEAN, MIN, MAX, VAR, STD = range(6)
SIX = [SUM, MEAN, MIN, MAX, VAR, STD]
MOMENTS, BEST = [STD, SUM, VAR, MEAN], [MAX, MIN]
EPS = 1e-5
HALF = (torch.bfloat16, torch.float16)
U_T = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 1e-5, torch.float16: 1e-5}
EPS_T = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52, torch.bfloat16: 2.0 ** -23, torch.float16: 2.0 ** -23}   # of the arithmetic
ROUND = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call_multi(dtype, stats, eps, n, rp, cc, X, h, want_max, want_min, out=None):
    """X: [rows, ldx] device tensor whose first h columns are the operand; out: a [n, k * h] view to write, or None for a fresh
    NaN-filled one; returns (out, arg_max, arg_min), pre-filled so that an element the kernels did not write shows"""
    code = _gather_code(dtype)
    nnz = cc.numel()
    ws = torch.empty(max(_lib.spmm_multi_reduce_workspace(code, stats, n, nnz, h), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, len(stats) * h), NAN, dtype=dtype, device=DEV)
    amax = torch.full((n, h), -2, dtype=torch.int32, device=DEV) if want_max else None
    amin = torch.full((n, h), -2, dtype=torch.int32, device=DEV) if want_min else None
    _lib.spmm_multi_reduce(code, stats, eps, n, rp.data_ptr(), cc.data_ptr(), nnz, X.data_ptr(), X.stride(0), h, out.data_ptr(), out.stride(0),
                           0 if amax is None else amax.data_ptr(), 0 if amin is None else amin.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out, amax, amin


def call_single(dtype, op, n, rp, cc, X, h, want_arg, out_view=None):
    """pygim_spmm_reduce without values (any gather type for MEAN); out_view(t): where the result goes, as in check_six"""
    code = _gather_code(dtype)
    nnz = cc.numel()
    ws = torch.empty(max(_lib.spmm_reduce_workspace(code, op, n, nnz, h), 16), dtype=torch.uint8, device=DEV)
    out = torch.full((n, h), NAN, dtype=dtype, device=DEV)
    out = out if out_view is None else out_view(out)
    arg = torch.full((n, h), -2, dtype=torch.int32, device=DEV) if want_arg else None
    _lib.spmm_reduce(code, op, n, rp.data_ptr(), cc.data_ptr(), nnz, 0, X.data_ptr(), X.stride(0), h, out.data_ptr(), out.stride(0),
                     0 if arg is None else arg.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out, arg


def call_unit_sum(dtype, n, rp, cc, X, h, out_view=None):
    """pygim_spmm_values with unit weights and one head: the numerator of the mean"""
    code = _gather_code(dtype)
    nnz = cc.numel()
    ws = torch.empty(max(_lib.spmm_values_workspace(code, n, nnz, h, 1), 16), dtype=torch.uint8, device=DEV)
    out = torch.full((n, h), NAN, dtype=dtype, device=DEV)
    out = out if out_view is None else out_view(out)
    ones = torch.ones(max(nnz, 1), dtype=torch.float32 if dtype in HALF else dtype, device=DEV)
    _lib.spmm_values(code, n, rp.data_ptr(), cc.data_ptr(), nnz, ones.data_ptr(), 1, X.data_ptr(), X.stride(0), h, out.data_ptr(), out.stride(0),
                     ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out


def bits(t):
    """the elements as integers: equal means the same bits, NaN included"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def reference64(n, rowptr, col, X64):
    """float64 on the CPU, two passes: (count, mean, var, mean of squares) per (row, feature); rows without entries hold 0"""
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    cnt = torch.diff(rowl).clamp(min=1).unsqueeze(1).double()
    x = X64[coll]
    zero = lambda: torch.zeros(n, X64.size(1), dtype=torch.float64)
    mean = zero().index_add_(0, row, x) / cnt
    var = zero().index_add_(0, row, (x - mean[row]) ** 2) / cnt
    msq = zero().index_add_(0, row, x * x) / cnt
    return cnt, mean, var, msq


def bounds(dtype, mean, var, msq, eps):
    """(ref_std, bound of var, bound of std) as include/pygim_hip.h states them, the one rounding of a 16-bit output included"""
    u, e, r = U_T[dtype], EPS_T[dtype], ROUND[dtype]
    ref_std = torch.sqrt(var + eps)
    b_var = 3 * u * msq
    b_std = b_var / ref_std + 2 * e * ref_std
    return ref_std, b_var + r * var, b_std + r * ref_std


def reference_stays_inside_its_own_bounds(dtype, X64, n, rowptr, col, eps):
    """on the CPU, before anything is launched: the one-pass formula evaluated in float64 on these inputs lies inside the var / std bounds
    of the arithmetic under test -- the bounds are not so tight that the reference's own formula would miss them"""
    cnt, mean, var, msq = reference64(n, rowptr, col, X64)
    ref_std, b_var, b_std = bounds(dtype, mean, var, msq, eps)
    one_pass = torch.relu(msq - mean * mean)
    assert ((one_pass - var).abs() <= b_var).all() and ((torch.sqrt(one_pass + eps) - ref_std).abs() <= b_std).all()


def check_six(name, dtype, n, rowptr, col, rp, cc, Xh, X, h, eps=EPS, out_view=None, finite=True):
    """Xh: the operand on the host [m, h] in dtype; X: the device tensor handed to the kernels (its first h columns equal Xh; any row
    stride).  out_view(t): the view of a guarded buffer the six-statistic result goes to, or None."""
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    Xc = Xh.to(DEV)   # contiguous
    # every launch writes through out_view: the order of a sum depends on the lane layout, and the layout on the alignment of out too
    fresh = lambda k: None if out_view is None else out_view(torch.full((n, k * h), NAN, dtype=dtype, device=DEV))
    out, amax, amin = call_multi(dtype, SIX, eps, n, rp, cc, X, h, True, True, fresh(6))
    blk = lambda t, stats, s: t[:, stats.index(s) * h:(stats.index(s) + 1) * h]
    if finite:
        assert not torch.isnan(out).any(), f"{name}: an element was not written"
    # the same bits on a second launch, without the args, and from the two smaller instantiations
    out2, amax2, amin2 = call_multi(dtype, SIX, eps, n, rp, cc, X, h, True, True, fresh(6))
    same = lambda a, b: a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    assert same(out2, out) and torch.equal(amax, amax2) and torch.equal(amin, amin2), f"{name}: two launches differ"
    assert same(call_multi(dtype, SIX, eps, n, rp, cc, X, h, False, False, fresh(6))[0], out), f"{name}: the result depends on whether the args are asked for"
    mom, none_a, none_b = call_multi(dtype, MOMENTS, eps, n, rp, cc, X, h, False, False, fresh(4))
    assert none_a is None and none_b is None
    for s in MOMENTS:
        assert same(blk(mom, MOMENTS, s), blk(out, SIX, s)), f"{name}: statistic {s} of the moments-only kernel differs"
    best, bmax, bmin = call_multi(dtype, BEST, eps, n, rp, cc, X, h, True, True, fresh(2))
    for s in BEST:
        assert same(blk(best, BEST, s), blk(out, SIX, s)), f"{name}: statistic {s} of the best-only kernel differs"
    assert torch.equal(bmax, amax) and torch.equal(bmin, amin)
    # sum, mean: the bits of the single calls on the same operands (the same X, and an out misaligned in the same way: the order of a
    # sum depends on the lane layout, and the layout on the alignment)
    assert same(blk(out, SIX, MEAN), call_single(dtype, _lib.REDUCE_MEAN, n, rp, cc, X, h, False, out_view)[0]), f"{name}: mean"
    assert same(blk(out, SIX, SUM), call_unit_sum(dtype, n, rp, cc, X, h, out_view)), f"{name}: sum"
    # max, min and their args: the bits of the single calls (16-bit X: on X widened to float32; the winner is an element of X)
    wide = torch.float32 if dtype in HALF else dtype
    Xw = Xc.to(wide)
    for s, op, arg in ((MAX, _lib.REDUCE_MAX, amax), (MIN, _lib.REDUCE_MIN, amin)):
        want, want_arg = call_single(wide, op, n, rp, cc, Xw, h, True)
        assert same(blk(out, SIX, s).to(wide), want), f"{name}: {'max' if s == MAX else 'min'}"
        assert torch.equal(arg, want_arg), f"{name}: arg of {'max' if s == MAX else 'min'}"
    # empty rows
    for s in SIX:
        e = blk(out, SIX, s)[empty.to(DEV)]
        if s == STD:
            at = torch.sqrt(torch.tensor(eps, dtype=wide)).to(dtype)
            assert (e == at.to(DEV)).all(), f"{name}: std of an empty row is sqrt(eps)"
        else:
            assert (e == 0).all(), f"{name}: an empty row"
    assert (amax[empty.to(DEV)] == -1).all() and (amin[empty.to(DEV)] == -1).all()
    if not finite:
        return out, amax, amin
    # var, std: the bounds
    cnt, mean, var, msq = reference64(n, rowptr, col, Xh.double())
    ref_std, b_var, b_std = bounds(dtype, mean, var, msq, eps)
    ref_std[empty], b_std[empty] = eps ** 0.5, ROUND[dtype] * eps ** 0.5 + 2 * EPS_T[dtype] * eps ** 0.5
    e_var = (blk(out, SIX, VAR).cpu().double() - var).abs()
    e_std = (blk(out, SIX, STD).cpu().double() - ref_std).abs()
    live = b_var > 0
    print(f"{name}: var err / bound {float((e_var[live] / b_var[live]).max()) if live.any() else 0.0:.3g}, "
          f"std err / bound {float((e_std / b_std).max()):.3g}")
    assert (e_var <= b_var).all(), f"{name}: var"
    assert (e_std <= b_std).all(), f"{name}: std"
    assert (blk(out, SIX, VAR) >= 0).all(), "the clamp"
    return out, amax, amin


def draw(rng, shape, dtype, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(lo, hi, size=shape)).to(dtype)


# ---- every launch shape of k_multi_gather: the `mean` table (test_multi_reduce_cpu proves kind 9 answers like SPMM_REDUCE) ----
@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c.dtype}-h{c.h}-{c.mis or 'aligned'}") for c in ls.TABLES["mean"]])
def test_every_launch_shape_on_the_edges_graph(rng, case):
    shape = _lib.gather_launch_shape(_lib.SHAPE_SPMM_MULTI_REDUCE, ls.CODE[case.dtype], case.h, 1, case.mis is None)
    assert tuple(shape[k] for k in _lib.SHAPE_FIELDS) == case.shape, (case, shape)
    dtype, h = TORCH[case.dtype], case.h
    n, m, rowptr, col = run_edges.graph("edges")
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = draw(rng, (m, h), dtype)
    reference_stays_inside_its_own_bounds(dtype, Xh.double(), n, rowptr, col, EPS)
    for which in (("X", "out") if case.mis else (None,)):
        views = Views(case, which)
        X = views("X", Xh.to(DEV))
        check_six(f"edges {case.dtype} h={h} {case.mis} {which}", dtype, n, rowptr, col, rp, cc, Xh, X, h, out_view=lambda t: views("out", t))
        views.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("h", [9, 256])
@pytest.mark.parametrize("graph", ["one-row", "whole-batches"])
def test_run_boundaries(rng, graph, h, dtype):
    n, m, rowptr, col = run_edges.graph(graph)
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = draw(rng, (m, h), dtype)
    check_six(f"{graph} {dtype} h={h}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), h)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_out_wider_than_the_blocks_keeps_its_padding(rng, dtype):
    n, m, rowptr, col = run_edges.graph("edges")
    rp, cc = t_red.dev_csr(rowptr, col)
    for h, pad in ((9, 5), (64, 8)):   # a scalar path and an aligned 16-byte path (the padding keeps the row stride a multiple of a piece)
        Xh = draw(rng, (m, h), dtype)
        buf = torch.full((n, 3 * h + pad), 7.0, dtype=dtype, device=DEV)
        out, _, _ = call_multi(dtype, [STD, MAX, MEAN], EPS, n, rp, cc, Xh.to(DEV), h, False, False, out=buf[:, :3 * h])
        assert (buf[:, 3 * h:] == 7.0).all(), "the padding columns were written"
        want, _, _ = call_multi(dtype, [STD, MAX, MEAN], EPS, n, rp, cc, Xh.to(DEV), h, False, False)
        assert torch.equal(buf[:, :3 * h].float(), want.float())


def test_no_entries_and_no_rows(rng):
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        n, h = 7, 9
        rp = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
        cc = torch.zeros(0, dtype=torch.int32, device=DEV)
        X = draw(rng, (5, h), dtype).to(DEV)
        out, amax, amin = call_multi(dtype, SIX, EPS, n, rp, cc, X, h, True, True)
        want = torch.zeros(n, 6 * h, dtype=dtype)
        want[:, 5 * h:] = torch.sqrt(torch.tensor(EPS, dtype=torch.float32 if dtype in HALF else dtype)).to(dtype)
        assert torch.equal(out.cpu(), want) and (amax == -1).all() and (amin == -1).all()
        out, amax, amin = call_multi(dtype, SIX, EPS, 0, rp[:1], cc, X, h, True, True)
        assert out.shape == (0, 6 * h)
    g = EdgeGraph(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), (0, 5))
    assert spmm_multi_reduce(g, torch.randn(5, 4, device=DEV)).shape == (0, 16)


def test_rejections(rng):
    n, m, rowptr, col = run_edges.graph("whole-batches")
    rp, cc = t_red.dev_csr(rowptr, col)
    nnz, h = len(col), 8
    X = draw(rng, (m, h), torch.float32).to(DEV)
    out = torch.zeros(n, 6 * h, device=DEV)
    arg = torch.zeros(n, h, dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.spmm_multi_reduce_workspace(_lib.FLT32, SIX, n, nnz, h) + 16, dtype=torch.uint8, device=DEV)

    def call(dtype=_lib.FLT32, stats=(MEAN,), eps=EPS, h=h, ldo=None, amax=0, amin=0, wsp=None, wsb=None, Xp=None):
        _lib.spmm_multi_reduce(dtype, stats, eps, n, rp.data_ptr(), cc.data_ptr(), nnz, X.data_ptr() if Xp is None else Xp, X.stride(0), h, out.data_ptr(),
                               len(stats) * h if ldo is None else ldo, amax, amin, ws.data_ptr() if wsp is None else wsp,
                               ws.numel() - 16 if wsb is None else wsb, stream())

    call()
    call(stats=SIX, amax=arg.data_ptr(), amin=arg.data_ptr())
    need = _lib.spmm_multi_reduce_workspace(_lib.FLT32, SIX, n, nnz, h)
    for bad in (dict(dtype=_lib.INT32), dict(dtype=_lib.INT8, stats=(MAX,)), dict(stats=(6,)), dict(stats=(-1,)), dict(stats=(MEAN, MEAN)), dict(stats=()),
                dict(stats=SIX + [SUM]), dict(stats=(MEAN, MIN), amax=arg.data_ptr()), dict(stats=(MEAN, MAX), amin=arg.data_ptr()),
                dict(stats=(MEAN,), amax=arg.data_ptr()), dict(stats=(STD,), eps=0.0), dict(stats=(STD,), eps=-1.0), dict(stats=(STD,), eps=NAN),
                dict(stats=(STD,), eps=float("inf")), dict(stats=(MEAN, MAX), ldo=2 * h - 1), dict(h=_lib.GATHER_MAX_H + 1),
                dict(stats=SIX, wsb=need - 1), dict(stats=SIX, wsp=ws.data_ptr() + 4, wsb=need), dict(stats=SIX, wsp=0),
                dict(Xp=X.cpu().data_ptr())):
        with pytest.raises(_lib.PygimError) as e:
            call(**bad)
        assert e.value.code == _lib.ERR_INVALID, bad
    call(stats=(VAR,), eps=0.0)   # eps is STD's alone
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", [9, 256])
def test_ties_go_to_the_lowest_entry(rng, dtype, h):
    """X drawn from five integers: most max / min are decided by the tie rule, and every sum is exact"""
    n, m, rowptr, col = t_red.small_graph(rng)
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = torch.from_numpy(rng.integers(-2, 3, size=(m, h))).to(dtype)
    check_six(f"ties {dtype} h={h}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), h)


def nonfinite_graph():
    """row 0: a hub of 1 500 entries (three runs) that holds columns 0, 1 and 2 once each; rows 1, 2, 3: one entry each, columns 0, 1, 2;
    row 4: empty; rows 5 .. 39: eight entries each among the other columns"""
    r = np.random.default_rng(5)
    m = 60
    hub = r.integers(3, m, size=1500)
    hub[[7, 600, 1499]] = [0, 1, 2]
    rows = [hub, [0], [1], [2], []] + [r.integers(3, m, size=8) for _ in range(35)]
    rowptr = np.zeros(len(rows) + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(x) for x in rows])
    return len(rows), m, rowptr, np.concatenate([np.asarray(x, dtype=np.int32) for x in rows]).astype(np.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_non_finite_inputs(rng, dtype):
    """X[0, 0] = NaN, X[1, 1] = +inf, X[2, 2] = -inf.  S1 / S2 carry them as IEEE addition does: NaN gives NaN everywhere; an infinity
    gives sum and mean of its sign and var = inf - inf = NaN, so std NaN -- in that (row, feature) alone.  max / min follow FoldBest
    (check_six compares them and their args with pygim_spmm_reduce on the same X)."""
    n, m, rowptr, col = nonfinite_graph()
    rp, cc = t_red.dev_csr(rowptr, col)
    h = 9
    clean = draw(rng, (m, h), dtype)
    Xh = clean.clone()
    Xh[0, 0], Xh[1, 1], Xh[2, 2] = NAN, float("inf"), -float("inf")
    out, amax, amin = check_six(f"non-finite {dtype}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), h, finite=False)
    base, bmax, bmin = check_six(f"finite {dtype}", dtype, n, rowptr, col, rp, cc, clean, clean.to(DEV), h)
    out, base = out.cpu().float().view(n, 6, h), base.cpu().float().view(n, 6, h)
    hit = torch.zeros(n, 6, h, dtype=torch.bool)
    for r, f in ((0, 0), (1, 0), (0, 1), (2, 1), (0, 2), (3, 2)):
        hit[r, :, f] = True
    assert torch.equal(out[~hit], base[~hit]), "another row or feature changed"
    for r in (0, 1):      # NaN
        assert torch.isnan(out[r, [SUM, MEAN, VAR, STD], 0]).all()
    for r, f, sign in ((0, 1, 1.0), (2, 1, 1.0), (0, 2, -1.0), (3, 2, -1.0)):
        assert out[r, SUM, f] == sign * float("inf") and out[r, MEAN, f] == sign * float("inf") and torch.isnan(out[r, [VAR, STD], f]).all()
    assert torch.isnan(out[1, MAX, 0]) and torch.isnan(out[1, MIN, 0]) and amax[1, 0] == -1 and amin[1, 0] == -1, "a row of NaN alone: no entry won"
    assert torch.isfinite(out[0, [MAX, MIN], 0]).all(), "a NaN never wins against a number"
    assert out[0, MAX, 1] == float("inf") and amax[0, 1] == 600 and out[0, MIN, 2] == -float("inf") and amin[0, 2] == 1499
    assert out[2, MAX, 1] == float("inf") and out[2, MIN, 1] == float("inf") and amax[2, 1] == 1501


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h", [1, 9, 32, 100, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_continuous_inputs_with_a_mean(rng, graph, h, dtype):
    """values around 3 +- 1: mean(x^2) is about 30 times the variance, the cancellation of the one-pass formula is exercised"""
    n, m, rowptr, col = t_red.GRAPHS[graph](rng)
    rp, cc = t_red.dev_csr(rowptr, col)
    Xh = draw(rng, (m, h), dtype, 2.0, 4.0)
    reference_stays_inside_its_own_bounds(dtype, Xh.double(), n, rowptr, col, EPS)
    check_six(f"{graph} {dtype} h={h}", dtype, n, rowptr, col, rp, cc, Xh, Xh.to(DEV), h)


# ---- the gradient ----
def dense_terms(n, rowptr, col, X, G, reduces, eps, arg):
    """float64 on the CPU: dX of the statement (var = mean of squares minus squared mean, relu, sqrt(. + eps); max / min to the entry
    `arg` names) and the sum of the magnitudes of the products it is made of, per element of X"""
    h = X.size(1)
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    cnt, mean, var, msq = reference64(n, rowptr, col, X)
    Gb = lambda s: G[:, reduces.index(s) * h:(reduces.index(s) + 1) * h] if s in reduces else torch.zeros(n, h, dtype=torch.float64)
    std = torch.sqrt(var + eps)
    Uc = (2 / cnt) * (var > 0) * (Gb("var") + (Gb("std") / (2 * std) if "std" in reduces else 0))
    x = X[coll]
    entry = torch.arange(len(col)).unsqueeze(1)
    parts = [Gb("sum")[row], (Gb("mean") / cnt)[row], Uc[row] * x, -(Uc * mean)[row]]
    for s in ("max", "min"):
        if s in reduces:
            parts.append(torch.where(arg[s].long()[row] == entry, Gb(s)[row], torch.zeros((), dtype=torch.float64)))
    zero = lambda: torch.zeros(X.shape, dtype=torch.float64)
    dX = zero().index_add_(0, coll, sum(parts))
    mag = zero().index_add_(0, coll, sum(p.abs() for p in parts))
    return dX, mag


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("h", [9, 256])
@pytest.mark.parametrize("reduces", [("mean",), ("max", "min"), ("std",), ("sum", "mean", "min", "max", "var", "std")])
def test_backward_meets_the_bound(rng, reduces, h, dtype):
    """dX within u sum |terms| of the float64 statement (bfloat16: 2^-8 |exact| more for the one rounding of dX).  X lies on the grid
    k / 64 in (-1, 1) (exact in every type here).  The statement is discontinuous where var = 0 (relu's subgradient) and steep next to it
    (the gradient of sqrt(var + eps) multiplies the forward's own rounding of var, about 3 epsilon mean(x^2), by 1 / (2 (var + eps))):
    on the grid a row's variance is 0 exactly or at least 2.4e-4 / n, far above that rounding, so [var > 0] is the same in float32 and
    float64 and the amplified rounding stays below u (|x| + |mean|) |U| -- the test is of the kernels, not of the formula's conditioning
    at a point where two entries of a row differ by less than 1e-3 of their size."""
    n, m, rowptr, col = t_red.small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    X = (torch.from_numpy(rng.integers(-63, 64, size=(m, h))).double() / 64).to(dtype).to(DEV).requires_grad_()
    G = draw(rng, (n, len(reduces) * h), dtype)
    out, amax, amin = spmm_multi_reduce(g, X, reduces, eps=EPS, return_arg=True)
    out.backward(G.to(DEV))
    arg = {"max": None if amax is None else amax.cpu(), "min": None if amin is None else amin.cpu()}
    want, mag = dense_terms(n, rowptr, col, X.detach().cpu().double(), G.double(), reduces, EPS, arg)
    err = (X.grad.cpu().double() - want).abs()
    bound = U_T[dtype] * mag + ROUND[dtype] * want.abs()
    print(f"{reduces} {dtype} h={h}: dX err / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3g}")
    assert X.grad.dtype == dtype and (err <= bound).all()
    first, X.grad = X.grad.clone(), None
    out2 = spmm_multi_reduce(g, X, reduces, eps=EPS)
    out2.backward(G.to(DEV))
    assert torch.equal(out2, out) and torch.equal(X.grad, first), "a second forward and backward differ"


# ---- the layer ----
def pna_forward_cpu(conv, x, rowptr, col):
    """PNAConv in torch ops on the CPU, a message per stored entry: pre_nn(cat[x_i, x_j]), scatter reductions, scalers, post_nn, lin"""
    n = x.size(0)
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    msg = conv.pre_nn(torch.cat([x[row], x[coll]], -1))
    F_ = msg.size(1)
    d = torch.diff(rowl)
    cnt = d.clamp(min=1).unsqueeze(1).to(x.dtype)
    idx = row.unsqueeze(1).expand_as(msg)
    zero = lambda: torch.zeros(n, F_, dtype=x.dtype)
    mean = zero().index_add(0, row, msg) / cnt
    var = torch.relu(zero().index_add(0, row, msg * msg) / cnt - mean * mean)
    stat = {"sum": zero().index_add(0, row, msg), "mean": mean, "var": var, "std": torch.sqrt(var + conv.EPS),
            "max": zero().scatter_reduce(0, idx, msg, "amax", include_self=False), "min": zero().scatter_reduce(0, idx, msg, "amin", include_self=False)}
    out = torch.cat([stat[s] for s in conv.aggregators], 1)
    logd = torch.log(cnt + 1)
    avg = torch.log(d.to(x.dtype) + 1).mean()
    scaled = {"identity": out, "amplification": out * (logd / avg), "attenuation": out * (avg / logd)}
    return conv.lin(conv.post_nn(torch.cat([x, torch.cat([scaled[s] for s in conv.scalers], 1)], 1)))


def test_pna_matches_the_cpu_composition(rng):
    """PNA, two layers, float64: logits and one SGD step's gradients as with the same model whose layers run the per-entry statement on
    the CPU (the tolerances of test_reduce_gpu.test_sage_mean_matches_the_cpu_shim)"""
    n, f_in, hid, f_out = 700, 16, 32, 8
    rowptr, col = random_csr(rng, n, n, 12, empty_frac=0.1, long_rows=((11, 64), (300, 700)))
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.PNA(f_in, hid, f_out, num_layers=2, dropout=0.0, fused=True).double()

    def run(model, dev):
        model = model.to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        opt.zero_grad()
        logits = model(feats.to(dev), adj)
        loss = ((logits - target.to(dev)) ** 2).mean()
        loss.backward()
        return logits.detach().cpu(), loss.item(), [p.grad.cpu().clone() for p in model.parameters()]

    cpu_model = copy.deepcopy(base)
    for conv in cpu_model.convs:
        conv.forward = (lambda c: lambda x, adj_t: pna_forward_cpu(c, x, rowptr, col))(conv)
    y_gpu, l_gpu, g_gpu = run(copy.deepcopy(base), DEV)
    y_cpu, l_cpu, g_cpu = run(cpu_model, "cpu")
    assert torch.allclose(y_gpu, y_cpu, rtol=1e-10, atol=1e-12) and np.allclose(l_gpu, l_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_gpu, g_cpu):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
    composed = copy.deepcopy(base)   # the same parameters through one spmm_reduce per statistic
    for conv in composed.convs:
        conv.fused = False
    y_comp, _, g_comp = run(composed, DEV)
    assert torch.allclose(y_comp, y_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_comp, g_cpu):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)


def test_pnaconv_in_bfloat16_under_autocast(rng):
    n = 700
    rowptr, col = random_csr(rng, n, n, 12, empty_frac=0.1, long_rows=((11, 64), (300, 700)))
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(1)
    conv = gnn.PNAConv(32, 16).to(DEV)
    x = torch.randn(n, 32, device=DEV)
    want = conv(x, adj)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = conv(x, adj)
    assert out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    assert (out.float() - want).abs().max() <= 0.05 * want.abs().max(), "bfloat16 forward far from the float32 one"
