"""Messages with a feature-wide edge feature on the GPU: pygim_spmm_edge, pygim_spmm_edge_softmax and pygim_spmm_edge_backward through the C
ABI and pygim_amd.reduce.spmm_edge (autograd), then gnn.GINEConv / GENEConv.

  1. bit identity   E = -0.0, no activation, eps = 0: x + (-0.0) == x for every x, so the call returns the BITS (and arg, and lse) of
                    spmm_values with unit weights (sum), spmm_reduce (mean, max, min) and spmm_softmax -- at one width per launch class the
                    shape query reports.  This pins the fold order to the existing kernels'.
  2. forward        random X and E, half of X + E negative, relu and eps: sum / mean at TOL of test_reduce_gpu (TOL * sum |msg| (/ count)
                    + eps |ref|, + u |ref| for a 16-bit out); max / min equal to the type's own arithmetic, arg included (the result is
                    one message: add, max, add are exact IEEE operations on both sides); softmax at the bounds of test_softmax_aggr_gpu
                    with x := msg.
  3. backward       dE, dX and dt against the float64 statement at GRAD_TOL of test_gatv2_gpu (16-bit: + u |ref| and the rounding of the
                    stored out, as in test_softmax_aggr_gpu); dE of max / min is nonzero at arg alone; relu's gradient is exactly 0 where
                    x + e <= 0; two launches give equal bits.
  4. non-finite     a NaN and a +-inf in E reach only their own (row, feature); E = -inf under relu gives msg = eps and gradient 0.
  5. layers         GINEConv / GENEConv forward + backward match their fused=False selves.
The reference is float64 on the CPU, computed from the operands exactly as the kernels get them (16-bit operands widened)."""
import copy

import numpy as np
import pytest
import torch

import run_edges
import test_reduce_gpu as t_red
import test_softmax_aggr_gpu as t_soft
from pygim_amd import _lib, gnn
from pygim_amd.attention import EdgeGraph, _gather_code
from pygim_amd.reduce import spmm_edge
from pygim_amd.sparse_tensor import SparseTensorShim
from test_edge_message_cpu import edge_backward_statement, message
from test_gatv2_gpu import GRAD_TOL
from test_multi_reduce_gpu import bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = (torch.bfloat16, torch.float16)
ROUND = t_soft.ROUND
NAN, INF = float("nan"), float("inf")
SUM, MEAN, MAX, MIN, SOFTMAX = _lib.REDUCE_SUM, _lib.REDUCE_MEAN, _lib.REDUCE_MAX, _lib.REDUCE_MIN, _lib.REDUCE_SOFTMAX
OP = {"sum": SUM, "mean": MEAN, "max": MAX, "min": MIN, "softmax": SOFTMAX}
RUN = run_edges.RUN
# rows: empty first; a row that ends exactly at entry 512; an empty row on that boundary; one-entry rows; a row that ends at 1024 and one that
# begins there; a hub of 1200 entries that crosses the boundaries 1536 and 2048; empty rows in the middle and last
DEG = [0, 0, 200, 1, 311, 0, 1, 300, 210, 1, 100, 1200, 1, 0, 37, 64, 1, 0, 5, 9, 2, 0, 1, 17, 3, 0, 33, 1, 8, 2, 4, 0, 6, 1, 12, 7, 1, 3, 0, 0]
NCOLS = 61


def compute_of(dtype):
    return torch.float32 if dtype in HALF else dtype


def make_graph():
    rowptr, col = run_edges.csr_of(DEG, NCOLS, 77)
    rp = rowptr.astype(np.int64)
    n, nnz = len(DEG), len(col)
    assert n == 40 and 1800 <= nnz <= 2600
    assert rp[5] == RUN and rp[4] < RUN, "row 4 ends exactly at entry 512"
    assert rp[10] == 2 * RUN and rp[9] < 2 * RUN, "row 10 begins exactly at entry 1024"
    assert rp[11] < 3 * RUN < 4 * RUN < rp[12] and rp[12] - rp[11] == 1200, "the hub crosses two run boundaries"
    deg = np.diff(rp)
    assert deg[0] == 0 and deg[-1] == 0 and (deg[12:-1] == 0).any() and (deg == 1).sum() >= 5
    row = np.repeat(np.arange(n), deg)
    assert ((col[1:] == col[:-1]) & (row[1:] == row[:-1])).any(), "duplicate columns"
    return n, NCOLS, rowptr, col


N, M, ROWPTR, COL = make_graph()
NNZ = len(COL)
ROW = np.repeat(np.arange(N), np.diff(ROWPTR.astype(np.int64)))


def launch_classes(dtype_code, named):
    """one width per launch class that pygim_gather_launch_shape reports for SPMM_EDGE over h = 1 .. 520 (the smallest of each), and the
    widths the issue names: a class is (vec, pieces per lane, L, more than one chunk, flags)"""
    seen, widths = set(), set(named)
    key = lambda h: tuple(_lib.gather_launch_shape(_lib.SHAPE_SPMM_EDGE, dtype_code, h, 1, True)[k] for k in ("vec", "pieces", "L", "flags")) + (
        _lib.gather_launch_shape(_lib.SHAPE_SPMM_EDGE, dtype_code, h, 1, True)["chunks"] > 1,)
    for h in range(1, 521):
        if key(h) not in seen:
            seen.add(key(h))
            widths.add(h)
    assert {key(h) for h in widths} == seen
    return sorted(widths)


F32_WIDTHS = launch_classes(_lib.FLT32, (1, 3, 4, 36, 256, 260, 516))
CASES = [(torch.float32, h, None) for h in F32_WIDTHS] + [(torch.float32, 36, "odd-lde"), (torch.float32, 36, "offset-E")] + \
        [(torch.bfloat16, h, None) for h in (8, 256, 520)] + [(torch.float64, h, None) for h in (3, 130)]
CASE_IDS = [f"{str(d).split('.')[1]}-h{h}-{mis or 'aligned'}" for d, h, mis in CASES]


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


@pytest.fixture(autouse=True)
def keep_the_global_generators(backend):
    """tests elsewhere in the suite draw from torch's global generators without seeding them: leave them as they were found"""
    state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state_all()
    yield
    torch.set_rng_state(state)
    torch.cuda.set_rng_state_all(dev_state)


@pytest.fixture(scope="module")
def csr():
    return t_red.dev_csr(ROWPTR, COL)


def stream():
    return torch.cuda.current_stream().cuda_stream


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def misaligned(t, mis):
    """a device copy of t [rows, h] whose rows are what `mis` asks for: an odd row stride, or a base pointer 4 bytes past a 16-byte boundary"""
    rows, h = t.shape
    if mis == "odd-lde":
        buf = torch.zeros((rows, h + 1), dtype=t.dtype, device=DEV)
        view = buf[:, :h]
        assert view.stride(0) % 2 == 1
    elif mis == "offset-E":
        buf = torch.zeros(rows * h + 16, dtype=t.dtype, device=DEV)
        off = (16 - buf.data_ptr() % 16) % 16 // t.element_size() + 4 // t.element_size()
        view = buf[off:off + rows * h].view(rows, h)
        assert view.data_ptr() % 16 == 4
    else:
        return t.to(DEV).contiguous()
    view.copy_(t)
    return view


def call_edge(dtype, op, act, eps, rp, cc, X, E, h, t=None, want_arg=False, want_lse=False):
    """X [m, ldx], E [nnz, lde] device views whose first h columns are the operands -> (out, arg or None, lse or None), pre-filled so that an
    element the kernels did not write shows"""
    code = _gather_code(dtype)
    out = torch.full((N, h), NAN, dtype=dtype, device=DEV)
    arg = torch.full((N, h), -2, dtype=torch.int32, device=DEV) if want_arg else None
    lse = torch.full((N, h), NAN, dtype=compute_of(dtype), device=DEV) if want_lse else None
    if op == SOFTMAX:
        ws = torch.empty(max(_lib.spmm_edge_softmax_workspace(code, N, NNZ, h), 16), dtype=torch.uint8, device=DEV)
        _lib.spmm_edge_softmax(code, act, eps, N, rp.data_ptr(), cc.data_ptr(), NNZ, X.data_ptr(), X.stride(0), E.data_ptr(), E.stride(0), t.data_ptr(), h,
                               out.data_ptr(), h, 0 if lse is None else lse.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    else:
        ws = torch.empty(max(_lib.spmm_edge_workspace(code, op, N, NNZ, h), 16), dtype=torch.uint8, device=DEV)
        _lib.spmm_edge(code, op, act, eps, N, rp.data_ptr(), cc.data_ptr(), NNZ, X.data_ptr(), X.stride(0), E.data_ptr(), E.stride(0), h, out.data_ptr(), h,
                       0 if arg is None else arg.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return out, arg, lse


def call_backward(dtype, op, act, eps, rp, cc, X, E, G, h, arg=None, t=None, out=None, lse=None, want_dt=False):
    code = _gather_code(dtype)
    dE = torch.full((NNZ, h), NAN, dtype=dtype, device=DEV)
    runs = _lib.spmm_edge_backward_workspace(code, op, N, NNZ, h)
    assert runs == (NNZ + RUN - 1) // RUN
    part = torch.full((runs, h), NAN, dtype=compute_of(dtype), device=DEV) if want_dt else None
    ptr = lambda a: 0 if a is None else a.data_ptr()
    _lib.spmm_edge_backward(code, op, act, eps, N, rp.data_ptr(), cc.data_ptr(), NNZ, X.data_ptr(), X.stride(0), E.data_ptr(), E.stride(0), G.data_ptr(),
                            G.stride(0), ptr(arg), ptr(t), ptr(out), h, ptr(lse), h, dE.data_ptr(), h, ptr(part), stream())
    torch.cuda.synchronize()
    return dE, part


def draw(rng, shape, dtype, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(lo, hi, size=shape)).to(dtype)


# ---- 1. bit identity with the existing calls ----
@pytest.mark.parametrize("dtype,h,mis", CASES, ids=CASE_IDS)
def test_minus_zero_edge_features_give_the_bits_of_the_existing_calls(rng, csr, dtype, h, mis):
    rp, cc = csr
    code = _gather_code(dtype)
    ct = compute_of(dtype)
    Xh = draw(rng, (M, h), dtype)
    Xh[3, 0], Xh[5, h - 1] = -0.0, 0.0   # signed zeros among the features
    X = misaligned(Xh, mis)               # X misaligned like E: the existing call then takes the same one-element pieces
    E = misaligned(torch.full((NNZ, h), -0.0, dtype=dtype), mis)
    shape = _lib.gather_launch_shape(_lib.SHAPE_SPMM_EDGE, code, h, 1, mis is None)
    assert shape == _lib.gather_launch_shape(_lib.SHAPE_SPMM_REDUCE, code, h, 1, mis is None) == _lib.gather_launch_shape(_lib.SHAPE_SPMM_SOFTMAX, code, h, 1, mis is None)
    assert mis is None or shape["vec"] == 1
    # sum: spmm_values with unit weights
    ones = torch.ones((NNZ, 1), dtype=ct, device=DEV)
    want = torch.full((N, h), NAN, dtype=dtype, device=DEV)
    ws = torch.empty(max(_lib.spmm_values_workspace(code, N, NNZ, h, 1), 16), dtype=torch.uint8, device=DEV)
    _lib.spmm_values(code, N, rp.data_ptr(), cc.data_ptr(), NNZ, ones.data_ptr(), 1, X.data_ptr(), X.stride(0), h, want.data_ptr(), h, ws.data_ptr(), ws.numel(),
                     stream())
    torch.cuda.synchronize()
    got, _, _ = call_edge(dtype, SUM, _lib.ACT_NONE, 0.0, rp, cc, X, E, h)
    assert not torch.isnan(got).any() and same(got, want), "sum"
    # mean, max, min: spmm_reduce
    for name in ("mean",) + (() if dtype in HALF else ("max", "min")):
        want_arg = name != "mean"
        ws = torch.empty(max(_lib.spmm_reduce_workspace(code, OP[name], N, NNZ, h), 16), dtype=torch.uint8, device=DEV)
        want = torch.full((N, h), NAN, dtype=dtype, device=DEV)
        warg = torch.full((N, h), -2, dtype=torch.int32, device=DEV) if want_arg else None
        _lib.spmm_reduce(code, OP[name], N, rp.data_ptr(), cc.data_ptr(), NNZ, 0, X.data_ptr(), X.stride(0), h, want.data_ptr(), h,
                         0 if warg is None else warg.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        torch.cuda.synchronize()
        got, garg, _ = call_edge(dtype, OP[name], _lib.ACT_NONE, 0.0, rp, cc, X, E, h, want_arg=want_arg)
        assert same(got, want), name
        assert not want_arg or torch.equal(garg, warg), f"{name}: arg"
    # softmax: spmm_softmax, lse included
    t = draw(rng, (h,), ct, -2.0, 4.0).to(DEV)
    ws = torch.empty(max(_lib.spmm_softmax_workspace(code, N, NNZ, h), 16), dtype=torch.uint8, device=DEV)
    want = torch.full((N, h), NAN, dtype=dtype, device=DEV)
    wlse = torch.full((N, h), NAN, dtype=ct, device=DEV)
    _lib.spmm_softmax(code, N, rp.data_ptr(), cc.data_ptr(), NNZ, X.data_ptr(), X.stride(0), t.data_ptr(), h, want.data_ptr(), h, wlse.data_ptr(), ws.data_ptr(),
                      ws.numel(), stream())
    torch.cuda.synchronize()
    got, _, glse = call_edge(dtype, SOFTMAX, _lib.ACT_NONE, 0.0, rp, cc, X, E, h, t=t, want_lse=True)
    assert same(got, want) and same(glse, wlse), "softmax"
    nol, _, _ = call_edge(dtype, SOFTMAX, _lib.ACT_NONE, 0.0, rp, cc, X, E, h, t=t)
    assert same(nol, got), "out depends on whether lse is asked for"


# ---- 2. and 3. forward and backward against the float64 statement ----
def problem(rng, dtype, h, eps):
    """operands whose sums X[col] + E are negative for about half of the entries, and the float64 messages of the kernels' own operands"""
    Xh, Eh, Gh = draw(rng, (M, h), dtype), draw(rng, (NNZ, h), dtype), draw(rng, (N, h), dtype)
    th = draw(rng, (h,), compute_of(dtype), -2.0, 4.0)
    eps_c = float(torch.tensor(eps, dtype=compute_of(dtype)))   # eps as the kernels take it
    msg = message(Xh.double().numpy(), Eh.double().numpy(), COL.astype(np.int64), True, eps_c)
    pre = Xh.double().numpy()[COL] + Eh.double().numpy()
    assert 0.3 < (pre < 0).mean() < 0.7, "relu must cut about half"
    return Xh, Eh, Gh, th, eps_c, torch.from_numpy(msg), pre


@pytest.mark.parametrize("dtype,h,mis", CASES, ids=CASE_IDS)
def test_forward_and_backward_match_the_float64_statement(rng, csr, dtype, h, mis):
    rp, cc = csr
    ct = compute_of(dtype)
    eps = 0.125
    Xh, Eh, Gh, th, eps_c, msg, pre = problem(rng, dtype, h, eps)
    X, E, G, t = Xh.to(DEV), misaligned(Eh, mis), Gh.to(DEV), th.to(DEV)
    row = torch.from_numpy(ROW)
    count = torch.from_numpy(np.diff(ROWPTR)).clamp(min=1).unsqueeze(1).double()
    empty = torch.from_numpy(np.diff(ROWPTR) == 0)
    fin = torch.finfo(ct).eps
    tol, u = GRAD_TOL[ct], ROUND[dtype]
    close = lambda got, ref, extra=0.0: ((got.cpu().double() - ref).abs() <= tol["atol"] + tol["rtol"] * ref.abs() + u * ref.abs() + extra).all()
    live = torch.from_numpy(pre > 0)
    col_l = torch.from_numpy(COL.astype(np.int64))
    scatter = lambda dE: torch.zeros(M, h, dtype=torch.float64).index_add_(0, col_l, dE)
    stat = lambda name, **kw: edge_backward_statement(ROWPTR.astype(np.int64), COL.astype(np.int64), Xh.double().numpy(), Eh.double().numpy(),
                                                      Gh.double().numpy(), name, True, eps_c, **kw)

    # sum and mean: TOL of test_reduce_gpu on the magnitudes summed
    total = torch.zeros(N, h, dtype=torch.float64).index_add_(0, row, msg)
    mag = torch.zeros(N, h, dtype=torch.float64).index_add_(0, row, msg.abs())
    for name, ref, bound in (("sum", total, t_red.TOL[ct] * mag), ("mean", total / count, t_red.TOL[ct] * mag / count)):
        out, _, _ = call_edge(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, E, h)
        assert not torch.isnan(out).any() and (out.cpu()[empty] == 0).all(), f"{name}: a row was not written, or an empty row is not 0"
        err = (out.cpu().double() - ref).abs()
        print(f"{name} {dtype} h={h} {mis}: max err / bound = {float((err / (bound + (fin + u) * ref.abs()).clamp_min(1e-300)).max()):.3g}")
        assert (err <= bound + (fin + u) * ref.abs()).all(), name
        dE, _ = call_backward(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, E, G, h)
        ref_dE = torch.from_numpy(stat(name)[0])
        assert not torch.isnan(dE).any() and close(dE, ref_dE), f"{name}: dE"
        assert (dE.cpu()[~live] == 0).all(), f"{name}: relu's gradient where x + e <= 0"
        assert same(dE, call_backward(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, E, G, h)[0]), f"{name}: two launches differ"

    # max and min: one message, in the type's own arithmetic; the lowest entry wins a tie (relu makes many: every cut message is eps)
    if dtype not in HALF:
        own = torch.relu(Xh[col_l] + Eh) + torch.tensor(eps, dtype=dtype)
        for name in ("max", "min"):
            out, arg, _ = call_edge(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, E, h, want_arg=True)
            want, warg = torch.zeros(N, h, dtype=dtype), torch.full((N, h), -1, dtype=torch.int32)
            for r in range(N):
                a, b = int(ROWPTR[r]), int(ROWPTR[r + 1])
                if a < b:
                    m = own[a:b].numpy()
                    at = m.argmax(0) if name == "max" else m.argmin(0)   # numpy: the first of equal elements
                    want[r] = torch.from_numpy(np.take_along_axis(m, at[None, :], 0)[0])
                    warg[r] = torch.from_numpy((a + at).astype(np.int32))
            assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu(), warg), name
            dE, _ = call_backward(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, E, G, h, arg=arg)
            ref_dE = torch.from_numpy(stat(name, arg=warg.numpy())[0])
            assert close(dE, ref_dE), f"{name}: dE"
            at_arg = torch.zeros(NNZ, h, dtype=torch.bool)
            full = warg >= 0
            at_arg[warg[full].long(), torch.nonzero(full)[:, 1]] = True
            assert (dE.cpu()[~at_arg] == 0).all() and (dE.cpu()[~live] == 0).all(), f"{name}: dE is nonzero at arg and nowhere else"
            assert (dE.cpu()[at_arg & live] == Gh[row][at_arg & live]).all(), f"{name}: the winner takes G itself"
            assert same(dE, call_backward(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, E, G, h, arg=arg)[0]), f"{name}: two launches differ"

    # softmax: the bounds of spmm_softmax with x := msg (the messages as the features of a graph whose entry e gathers row e)
    ident = np.arange(NNZ, dtype=np.int32)
    ref, ref_lse, smag, smax = t_soft.reference64(N, ROWPTR, ident, msg, th.double())
    b_out, b_lse = t_soft.bounds(dtype, ref, ref_lse, smag, smax)
    out, _, lse = call_edge(dtype, SOFTMAX, _lib.ACT_RELU, eps, rp, cc, X, E, h, t=t, want_lse=True)
    assert not torch.isnan(out).any() and (out.cpu()[empty] == 0).all() and (lse.cpu()[empty] == -INF).all()
    e_out, e_lse = (out.cpu().double() - ref).abs(), (lse.cpu().double() - ref_lse).abs()[~empty]
    print(f"softmax {dtype} h={h} {mis}: out err / bound {float((e_out / b_out.clamp_min(1e-300))[~empty].max()):.3g}, "
          f"lse err / bound {float((e_lse / b_lse[~empty]).max()):.3g}")
    assert (e_out <= b_out).all() and (e_lse <= b_lse[~empty]).all(), "softmax"
    dE, part = call_backward(dtype, SOFTMAX, _lib.ACT_RELU, eps, rp, cc, X, E, G, h, t=t, out=out, lse=lse, want_dt=True)
    ref_dE, ref_dT = stat("softmax", t=th.double().numpy(), out=ref.numpy(), lse=ref_lse.numpy())
    ref_dE, ref_dT = torch.from_numpy(ref_dE), torch.from_numpy(ref_dT)
    p = torch.exp(th.double() * msg - ref_lse[row])
    mid = u * (Gh.double()[row] * p * ref[row]).abs()   # the rounding of the stored 16-bit out: u |G| p |out| per entry, times |t| in dE
    assert not torch.isnan(dE).any() and not torch.isnan(part).any()
    assert close(dE, ref_dE, th.double().abs() * mid), "softmax: dE"
    assert (dE.cpu()[~live] == 0).all(), "softmax: relu's gradient where x + e <= 0"
    assert close(part.sum(0), ref_dT, (msg.abs() * mid).sum(0)), "softmax: dt"
    again, part2 = call_backward(dtype, SOFTMAX, _lib.ACT_RELU, eps, rp, cc, X, E, G, h, t=t, out=out, lse=lse, want_dt=True)
    assert same(dE, again) and same(part, part2), "softmax: two launches differ"
    assert same(dE, call_backward(dtype, SOFTMAX, _lib.ACT_RELU, eps, rp, cc, X, E, G, h, t=t, out=out, lse=lse)[0]), "dE depends on whether dT_part is asked for"

    # dX: the autograd function sums the dE rows per column through spmm_values on the transposed structure
    if mis is None:
        g = EdgeGraph(torch.from_numpy(ROWPTR), torch.from_numpy(COL), (N, M))
        for name in ("sum", "softmax"):
            Xd, Ed, td = X.clone().requires_grad_(), Eh.to(DEV).requires_grad_(), t.clone().requires_grad_()
            o = spmm_edge(g, Xd, Ed, name, "relu", eps, td)
            o.backward(G)
            want_dE = torch.from_numpy(stat(name, **(dict(t=th.double().numpy(), out=ref.numpy(), lse=ref_lse.numpy()) if name == "softmax" else {}))[0])
            extra = th.double().abs() * mid if name == "softmax" else 0.0
            # every dE row is rounded to the storage type before it is summed: u |dE| per entry on top of the sum's own tolerance
            sum_mag = scatter(want_dE.abs())
            err = (Xd.grad.cpu().double() - scatter(want_dE)).abs()
            bound = tol["atol"] + tol["rtol"] * sum_mag + 2 * u * sum_mag + (scatter(extra) if name == "softmax" else 0.0)
            assert Xd.grad.dtype == dtype and (err <= bound).all(), f"{name}: dX"
            assert Ed.grad.dtype == dtype and close(Ed.grad, want_dE, extra), f"{name}: dE through autograd"
            if name == "softmax":
                assert td.grad.shape == (h,) and close(td.grad, ref_dT, (msg.abs() * mid).sum(0)), "dt through autograd"


# ---- 4. non-finite edge features ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nonfinite_edge_features_stay_in_their_own_row_and_feature(rng, csr, dtype):
    rp, cc = csr
    h = 36 if dtype == torch.float32 else 8
    eps = 0.25
    Xh, Eh, Gh, th, eps_c, _, _ = problem(rng, dtype, h, eps)
    X, G, t = Xh.to(DEV), Gh.to(DEV), th.to(DEV)
    hub = int(ROWPTR[11])
    plant = [(hub + 5, 0, NAN), (hub + 700, 1, INF), (int(ROWPTR[2]) + 3, 2, -INF), (int(ROWPTR[3]), 3, NAN), (hub + 1100, h - 1, -INF)]
    clean = {}
    for name in ("sum", "mean", "softmax") + (() if dtype in HALF else ("max", "min")):
        clean[name] = call_edge(dtype, OP[name], _lib.ACT_NONE, eps, rp, cc, X, Eh.to(DEV), h, t=t)[0].cpu()
    Ep = Eh.clone()
    hit = torch.zeros(N, h, dtype=torch.bool)
    for e, f, v in plant:
        Ep[e, f] = v
        hit[ROW[e], f] = True
    for name, base in clean.items():
        out = call_edge(dtype, OP[name], _lib.ACT_NONE, eps, rp, cc, X, Ep.to(DEV), h, t=t)[0].cpu()
        assert same(out[~hit], base[~hit]), f"{name}: a non-finite edge feature reached another (row, feature)"
        msg = torch.from_numpy(message(Xh.double().numpy(), Ep.double().numpy(), COL.astype(np.int64), False, eps_c))
        own = (Xh[torch.from_numpy(COL.astype(np.int64))] + Ep) + torch.tensor(eps, dtype=dtype)   # max / min: the type's own arithmetic
        for e, f, v in plant:   # against the statement: the fold applied to msg
            a, b = int(ROWPTR[ROW[e]]), int(ROWPTR[ROW[e] + 1])
            got = float(out[ROW[e], f])
            if name in ("sum", "mean"):   # NaN, or the infinity itself
                want = float(msg[a:b, f].sum())
                assert (got != got) if want != want else got == want, (name, e, f, v)
            elif name in ("max", "min"):   # a NaN never wins against a number; a row of one NaN stores NaN
                num = own[a:b, f][~torch.isnan(own[a:b, f])]
                want = NAN if num.numel() == 0 else float(num.max() if name == "max" else num.min())
                assert (got != got) if want != want else got == want, (name, e, f, v)
            else:   # a NaN or +-inf score: never a finite number (include/pygim_hip.h, pygim_spmm_softmax)
                assert not np.isfinite(got), (name, e, f, v)
    # E = -inf under relu: msg = eps, gradient 0
    Einf = Eh.clone()
    Einf[:, 0] = -INF
    out = call_edge(dtype, SUM, _lib.ACT_RELU, eps, rp, cc, X, Einf.to(DEV), h)[0].cpu()
    want = torch.from_numpy(np.diff(ROWPTR)).double() * eps_c
    assert torch.equal(out[:, 0].double(), want.to(dtype).double()), "E = -inf under relu gives msg = eps"
    for name in ("sum", "mean"):
        dE, _ = call_backward(dtype, OP[name], _lib.ACT_RELU, eps, rp, cc, X, Einf.to(DEV), G, h)
        assert (dE[:, 0] == 0).all() and not torch.isnan(dE).any()
    o, _, lse = call_edge(dtype, SOFTMAX, _lib.ACT_RELU, eps, rp, cc, X, Einf.to(DEV), h, t=t, want_lse=True)
    full = torch.from_numpy(np.diff(ROWPTR) > 0)
    assert torch.allclose(o.cpu()[full][:, 0].double(), torch.full((int(full.sum()),), eps_c, dtype=torch.float64), rtol=4 * t_soft.EPS_T[dtype] + 2 * ROUND[dtype])
    dE, _ = call_backward(dtype, SOFTMAX, _lib.ACT_RELU, eps, rp, cc, X, Einf.to(DEV), G, h, t=t, out=o, lse=lse)
    assert (dE[:, 0] == 0).all() and not torch.isnan(dE).any()


# ---- 5. the layers ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layer", ["gine", "gen-softmax", "gen-mean"])
def test_layers_match_their_composition(rng, layer, dtype):
    n, c, d = N, 16, 5
    adj = SparseTensorShim(rowptr=torch.from_numpy(ROWPTR).long(), col=torch.from_numpy(COL % n).long(), sparse_sizes=(n, n))
    torch.manual_seed(6)
    if layer == "gine":
        conv = gnn.GINEConv(torch.nn.Sequential(torch.nn.Linear(c, c), torch.nn.ReLU(), torch.nn.Linear(c, c)), train_eps=True, edge_dim=d)
    else:
        conv = gnn.GENEConv(c, c, d, aggr=layer.split("-")[1], learn_t=True, norm="layer")
    conv = conv.to(DEV).to(dtype)
    x = draw(rng, (n, c), dtype).to(DEV)
    e = draw(rng, (NNZ, d), dtype).to(DEV)
    G = draw(rng, (n, c), dtype).to(DEV)
    res = []
    for fused in (True, False):
        cv = copy.deepcopy(conv)
        cv.fused = fused
        xi, ei = x.clone().requires_grad_(), e.clone().requires_grad_()
        out = cv(xi, adj, ei)
        assert out.is_cuda and out.dtype == dtype
        out.backward(G)
        res.append([out.detach(), xi.grad, ei.grad] + [p.grad for p in cv.parameters()])
    tol = GRAD_TOL[torch.float32]
    u = ROUND[dtype]   # 16-bit: the composition rounds its result once more, and every gradient is a sum of once-rounded terms
    for a, b in zip(*res):
        assert a.shape == b.shape and torch.isfinite(a).all()
        scale = max(1.0, float(b.abs().max()))
        assert torch.allclose(a.double(), b.double(), rtol=tol["rtol"] + 4 * u, atol=(tol["atol"] + 4 * u) * scale)
