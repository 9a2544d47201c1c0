"""Mean / max / min aggregation on the GPU: pygim_spmm_reduce and pygim_spmm_reduce_backward through the C ABI against the CPU shim
(torch_sparse's semantics in plain torch ops) and float64 references, then pygim_amd.reduce (autograd) and gnn.SAGE(aggr="mean").

Max / min are compared bit for bit, the winning entry included: on X drawn from -2..2 and values from a set of three, ties are the
rule and every product is exact, so the tie rule (lowest entry index) decides most outputs.  Mean and the gradients use the project's
own bound (include/pygim_hip.h): 1e-5 (FLT32) / 1e-12 (DBL64) relative to the sum of the magnitudes a result is made of."""
import copy

import numpy as np
import pytest
import torch

from conftest import random_csr
from pygim_amd import _lib, gnn, pim_ops
from pygim_amd.attention import EdgeGraph
from pygim_amd.reduce import spmm_reduce
from pygim_amd.sparse_tensor import SparseTensorShim, _shim_matmul

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float64: 1e-12}
DEV = "cuda"
OP = {"mean": _lib.REDUCE_MEAN, "max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN}
ALL_TYPES = [torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float64]
FLOATS = [torch.float32, torch.float64]
SENTINEL = 77   # no product of -2..2 and 1..3 (rows the kernels never wrote must show)


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
    """one row of 21 000 entries (41 runs), one of 1 500, short rows and empty rows around them, and a hub column"""
    n, m = 400, 3000
    rowptr, col = random_csr(rng, n, m, 6, empty_frac=0.1, long_rows=((0, 3), (7, 21000), (150, 1500), (399, 0)))
    col[::3] = 3
    return n, m, rowptr, col


GRAPHS = {"small": small_graph, "hub": hub_graph}


def dev_csr(rowptr, col):
    return torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV)


def call_reduce(dtype, op, n, rp, cc, val, X, h, want_arg, out=None):
    """X: [rows, ldx] device tensor whose first h columns are the operand; returns (out, arg or None), pre-filled so that a row the
    kernels did not write shows"""
    code = pim_ops.DTYPE_CODE[dtype]
    nnz = cc.numel()
    ws = torch.empty(max(_lib.spmm_reduce_workspace(code, op, n, nnz, h), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((n, h), float("nan") if dtype.is_floating_point else SENTINEL, dtype=dtype, device=DEV)
    arg = torch.full((n, h), -2, dtype=torch.int32, device=DEV) if want_arg else None
    _lib.spmm_reduce(code, op, n, rp.data_ptr(), cc.data_ptr(), nnz, 0 if val is None else val.data_ptr(), X.data_ptr(), X.stride(0), h,
                     out.data_ptr(), out.stride(0), 0 if arg is None else arg.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, arg


def shim_reference(n, m, rowptr, col, val, X, reduce):
    """the CPU shim's matmul(reduce=...) and, for max / min, a first-best scan in entry order: the lowest entry of the row whose
    product equals the row's result"""
    rp, cc = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    adj = SparseTensorShim(rowptr=rp, col=cc, value=val, sparse_sizes=(n, m))
    out = _shim_matmul(adj, X, reduce)
    if reduce == "mean":
        return out, None
    row = adj.storage.row()
    msg = X[cc] if val is None else val.unsqueeze(1) * X[cc]
    entry = torch.arange(len(col)).unsqueeze(1).expand_as(msg)
    cand = torch.where(msg == out[row], entry, torch.full_like(entry, 2 ** 31 - 1))
    arg = torch.full(out.shape, -1, dtype=torch.int64).scatter_reduce(0, row.unsqueeze(1).expand_as(msg), cand, "amin", include_self=False)
    return out, arg.to(torch.int32)


def strides_of(graph, h, dtype):
    """a contiguous X, a wider row stride that keeps 16-byte alignment, and one that breaks it"""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    return (h, h + 2 * vec, h + 1) if graph == "small" else (h,)


@pytest.mark.parametrize("dtype", ALL_TYPES)
@pytest.mark.parametrize("h", [1, 9, 32, 100, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_max_min_with_ties_are_bit_equal_to_the_shim(rng, dtype, h, graph):
    check_max_min_with_ties(rng, dtype, h, graph)


def test_max_min_over_three_feature_chunks(rng):
    """h = 300: the misaligned stride gives 300 one-element pieces, three blockIdx.y chunks of 128, the last one partly empty"""
    check_max_min_with_ties(rng, torch.float32, 300, "small")


def check_max_min_with_ties(rng, dtype, h, graph):
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    nnz = len(col)
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    pool = [0.5, 1.0, 2.0] if dtype.is_floating_point else [1, 2, 3]
    for ldx in strides_of(graph, h, dtype):
        Xh = torch.from_numpy(rng.integers(-2, 3, size=(m, ldx))).to(dtype)
        X = Xh.to(DEV)
        for val in (None, torch.from_numpy(rng.choice(pool, size=nnz)).to(dtype)):
            vd = None if val is None else val.to(DEV)
            for reduce in ("max", "min"):
                want, want_arg = shim_reference(n, m, rowptr, col, val, Xh[:, :h].contiguous(), reduce)
                assert (want[empty] == 0).all() and (want_arg[empty] == -1).all() and (want_arg[~empty] >= 0).all()
                out, arg = call_reduce(dtype, OP[reduce], n, rp, cc, vd, X, h, True)
                assert torch.equal(out.cpu(), want), f"{reduce} {graph} {dtype} h={h} ldx={ldx} values={val is not None}"
                assert torch.equal(arg.cpu(), want_arg), f"arg of {reduce} {graph} {dtype} h={h} ldx={ldx} values={val is not None}"
                out2, arg2 = call_reduce(dtype, OP[reduce], n, rp, cc, vd, X, h, True)
                assert torch.equal(out, out2) and torch.equal(arg, arg2), "two launches differ"
                bare, none = call_reduce(dtype, OP[reduce], n, rp, cc, vd, X, h, False)
                assert none is None and torch.equal(bare, out), "the result depends on whether arg is asked for"


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("h", [1, 9, 32, 100, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_max_min_on_continuous_inputs_are_bit_equal_to_the_shim(rng, dtype, h, graph):
    """a max is one of the products, each a single IEEE multiply"""
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    Xh = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(dtype)
    val = torch.from_numpy(rng.uniform(-2, 2, size=len(col))).to(dtype)
    for reduce in ("max", "min"):
        want, want_arg = shim_reference(n, m, rowptr, col, val, Xh, reduce)
        out, arg = call_reduce(dtype, OP[reduce], n, rp, cc, val.to(DEV), Xh.to(DEV), h, True)
        assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu(), want_arg)
        assert torch.equal(out, call_reduce(dtype, OP[reduce], n, rp, cc, val.to(DEV), Xh.to(DEV), h, False)[0])


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("h", [1, 9, 32, 100, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_mean_parity(rng, dtype, h, graph):
    check_mean_parity(rng, dtype, h, graph)


def test_mean_parity_over_three_feature_chunks(rng):
    check_mean_parity(rng, torch.float32, 300, "small")


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("h", [9, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_mean_is_the_sum_of_spmm_values_divided_by_the_count(rng, dtype, h, graph):
    """the documented contract, bit for bit: the same walk and the same order as pygim_spmm_values with one head, then one IEEE
    division by the row's number of stored entries (done here on the CPU); empty rows are 0"""
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    nnz = len(col)
    code = pim_ops.DTYPE_CODE[dtype]
    X = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(DEV, dtype)
    val = torch.from_numpy(rng.uniform(-2, 2, size=nnz)).to(DEV, dtype)
    mean, _ = call_reduce(dtype, OP["mean"], n, rp, cc, val, X, h, False)
    ws = torch.empty(max(_lib.spmm_values_workspace(code, n, nnz, h, 1), 16), dtype=torch.uint8, device=DEV)
    total = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    _lib.spmm_values(code, n, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), 1, X.data_ptr(), h, h, total.data_ptr(), h, ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    count = torch.from_numpy(np.diff(rowptr)).clamp(min=1).to(dtype).unsqueeze(1)
    assert torch.equal(mean.cpu(), total.cpu() / count)


def check_mean_parity(rng, dtype, h, graph):
    n, m, rowptr, col = GRAPHS[graph](rng)
    rp, cc = dev_csr(rowptr, col)
    nnz = len(col)
    rowl, coll = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowl))
    count = torch.diff(rowl).clamp(min=1).unsqueeze(1).double()
    eps = torch.finfo(dtype).eps
    for ldx in strides_of(graph, h, dtype):
        Xh = torch.from_numpy(rng.uniform(-1, 1, size=(m, ldx))).to(dtype)
        X = Xh.to(DEV)
        for vh in (None, torch.from_numpy(rng.uniform(-2, 2, size=nnz)).to(dtype)):
            val = None if vh is None else vh.to(DEV)
            out, _ = call_reduce(dtype, OP["mean"], n, rp, cc, val, X, h, False)
            assert not torch.isnan(out).any(), "a row was not written"
            assert (out[torch.from_numpy(np.diff(rowptr) == 0).to(DEV)] == 0).all()
            msg = Xh[:, :h].double()[coll]   # the float64 reference on the CPU: a plain loop over the entries
            if vh is not None:
                msg = vh.double().unsqueeze(1) * msg
            ref = torch.zeros(n, h, dtype=torch.float64).index_add_(0, row, msg) / count
            mag = torch.zeros(n, h, dtype=torch.float64).index_add_(0, row, msg.abs())
            err = (out.cpu().double() - ref).abs()
            bound = TOL[dtype] * mag / count + eps * ref.abs()
            print(f"mean {graph} {dtype} h={h} ldx={ldx} values={vh is not None}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3e}")
            assert torch.all(err <= bound)
            assert torch.equal(out, call_reduce(dtype, OP["mean"], n, rp, cc, val, X, h, False)[0]), "two launches differ"


def test_strided_out_nnz0_and_bad_arguments(rng):
    n, m, rowptr, col = small_graph(rng)
    rp, cc = dev_csr(rowptr, col)
    h = 32
    Xh = torch.from_numpy(rng.integers(-2, 3, size=(m, h))).float()
    X = Xh.to(DEV)
    for reduce in ("mean", "max", "min"):
        wide = torch.full((n, h + 5), float("nan"), device=DEV)
        _, arg = call_reduce(torch.float32, OP[reduce], n, rp, cc, None, X, h, reduce != "mean", out=wide)
        want, want_arg = shim_reference(n, m, rowptr, col, None, Xh, reduce)
        assert torch.isnan(wide[:, h:]).all(), "stores outside out[:, :h]"
        if reduce == "mean":
            assert torch.allclose(wide[:, :h].cpu(), want, rtol=1e-5, atol=1e-6)
        else:
            assert torch.equal(wide[:, :h].cpu(), want) and torch.equal(arg.cpu(), want_arg)
    # nnz = 0: every row is empty
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    for reduce in ("mean", "max", "min"):
        out, arg = call_reduce(torch.float32, OP[reduce], n, rp0, cc[:0], None, X, h, reduce != "mean")
        assert (out == 0).all() and (arg is None or (arg == -1).all())
    out, arg = call_reduce(torch.int8, OP["max"], n, rp0, cc[:0], None, X.to(torch.int8), h, True)
    assert (out == 0).all() and (arg == -1).all()
    # integer products wrap like the type before they are compared: 3 * 100 is 44 in int8, 3 * -100 is -44
    x8 = torch.from_numpy(rng.choice([-100, -43, 0, 43, 100], size=(m, h))).to(torch.int8)
    v8 = torch.from_numpy(rng.choice([1, 3], size=len(col))).to(torch.int8)
    for reduce in ("max", "min"):
        want, want_arg = shim_reference(n, m, rowptr, col, v8, x8, reduce)
        out, arg = call_reduce(torch.int8, OP[reduce], n, rp, cc, v8.to(DEV), x8.to(DEV), h, True)
        assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu(), want_arg)
    dX = torch.full((m, h), float("nan"), device=DEV)
    _lib.spmm_reduce_backward(_lib.FLT32, m, torch.zeros(m + 1, dtype=torch.int32, device=DEV).data_ptr(), 0, 0, 0, 0, 0, h, 0, h, dX.data_ptr(), h)
    torch.cuda.synchronize()
    assert (dX == 0).all()
    # every PYGIM_ERR_INVALID case
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    o = torch.empty(n, h, device=DEV)
    a = torch.empty(n, h, dtype=torch.int32, device=DEV)
    head = (n, rp.data_ptr(), cc.data_ptr(), len(col), 0, X.data_ptr(), h, h, o.data_ptr(), h)
    with pytest.raises(_lib.PygimError):   # a workspace smaller than pygim_spmm_reduce_workspace says
        _lib.spmm_reduce(_lib.FLT32, OP["max"], *head, 0, ws.data_ptr(), 16)
    with pytest.raises(_lib.PygimError):
        _lib.spmm_reduce(_lib.FLT32, OP["mean"], *head, 0, ws.data_ptr(), 16)
    for op in (0, 4):                      # an unknown op ("sum" is not served here)
        with pytest.raises(_lib.PygimError):
            _lib.spmm_reduce(_lib.FLT32, op, *head, 0, ws.data_ptr(), ws.numel())
        with pytest.raises(_lib.PygimError):
            _lib.spmm_reduce_workspace(_lib.FLT32, op, n, len(col), h)
    with pytest.raises(_lib.PygimError):   # an integer mean
        _lib.spmm_reduce(_lib.INT32, OP["mean"], *head, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):
        _lib.spmm_reduce_workspace(_lib.INT32, OP["mean"], n, len(col), h)
    with pytest.raises(_lib.PygimError):   # arg with mean
        _lib.spmm_reduce(_lib.FLT32, OP["mean"], *head, a.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):   # an integer type with the backward
        _lib.spmm_reduce_backward(_lib.INT32, m, rp.data_ptr(), cc.data_ptr(), cc.data_ptr(), len(col), 0, o.data_ptr(), h, a.data_ptr(), h, o.data_ptr(), h)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("h", [9, 256])
@pytest.mark.parametrize("graph", ["small", "hub"])
def test_backward_parity(rng, dtype, h, graph):
    check_backward_parity(rng, dtype, h, graph)


def check_backward_parity(rng, dtype, h, graph, view=lambda name, t: t):
    """view(name, tensor): the buffer G / dX is handed over in (another row stride or start; NaN around it)"""
    n, m, rowptr, col = GRAPHS[graph](rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    gt, perm = g.transposed()
    perm32 = perm.to(torch.int32)
    nnz = len(col)
    code = pim_ops.DTYPE_CODE[dtype]
    X = torch.from_numpy(rng.integers(-2, 3, size=(m, h))).to(DEV, dtype)   # tie-heavy: most of the gradient hangs on the tie rule
    G = torch.from_numpy(rng.normal(0, 1, size=(n, h))).to(DEV, dtype)
    entry = torch.arange(nnz, device=DEV).unsqueeze(1)
    for val in (None, torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=nnz)).to(DEV, dtype)):
        _, arg = call_reduce(dtype, OP["max"], n, g.rowptr, g.col, val, X, h, True)

        def run():
            dX = view("dX", torch.full((m, h), float("nan"), dtype=dtype, device=DEV))
            Gv = view("G", G)
            _lib.spmm_reduce_backward(code, m, gt.rowptr.data_ptr(), gt.col.data_ptr(), perm32.data_ptr(), nnz, 0 if val is None else val.data_ptr(),
                                      Gv.data_ptr(), Gv.stride(0), arg.data_ptr(), h, dX.data_ptr(), dX.stride(0), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return dX

        dX = run()
        assert not torch.isnan(dX).any(), "a row was not written"
        row = g.row.long()
        contrib = torch.where(arg[row].long() == entry, G[row].double() * (1.0 if val is None else val.double().unsqueeze(1)), 0.0)
        ref = torch.zeros(m, h, dtype=torch.float64, device=DEV).index_add_(0, g.col.long(), contrib)
        mag = torch.zeros(m, h, dtype=torch.float64, device=DEV).index_add_(0, g.col.long(), contrib.abs())
        err = (dX.double() - ref).abs()
        print(f"reduce backward {graph} {dtype} h={h} values={val is not None}: max err / mag = {(err / mag.clamp_min(1e-300)).max().item():.3e}")
        assert torch.all(err <= TOL[dtype] * mag)
        assert torch.equal(dX, run()), "two launches differ"


@pytest.mark.parametrize("dtype", FLOATS)
def test_autograd_on_device_matches_the_cpu_shim(rng, dtype):
    """forward and gradients of spmm_reduce against the shim's differentiable torch ops in float64.  Bounds: the kernels' own (TOL of
    the magnitudes summed) plus, for mean, one rounding each of w / count and G / count (2 eps of the same magnitudes)."""
    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert g.rowptr.is_cuda
    nnz, h = len(col), 32
    rp, cc = torch.from_numpy(rowptr).long(), torch.from_numpy(col).long()
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rp))
    count = torch.diff(rp).clamp(min=1).double()
    eps = torch.finfo(dtype).eps
    v = torch.from_numpy(rng.uniform(0.5, 2, size=nnz)).to(dtype)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(dtype)
    G = torch.from_numpy(rng.normal(0, 1, size=(n, h))).to(dtype)
    for reduce in ("mean", "max"):
        vd, Xd = v.to(DEV).requires_grad_(reduce == "mean"), X.to(DEV).requires_grad_()
        out = spmm_reduce(g, Xd, reduce, value=vd)
        assert out.is_cuda
        out.backward(G.to(DEV))
        msg = (v.double().unsqueeze(1) * X.double()[cc]).abs()
        if reduce == "mean":
            vc, Xc = v.double().clone().requires_grad_(), X.double().clone().requires_grad_()
            ref = _shim_matmul(SparseTensorShim(rowptr=rp, col=cc, value=vc, sparse_sizes=(n, m)), Xc, reduce)
            ref.backward(G.double())
            want_dx = Xc.grad
            mag = torch.zeros(n, h, dtype=torch.float64).index_add_(0, row, msg) / count.unsqueeze(1)
            assert torch.all((out.detach().cpu().double() - ref.detach()).abs() <= TOL[dtype] * mag + eps * ref.detach().abs())
            wg = (v.double() / count[row]).unsqueeze(1) * G.double()[row]
            mag_x = torch.zeros(m, h, dtype=torch.float64).index_add_(0, cc, wg.abs())
            mag_v = ((G.double() / count.unsqueeze(1))[row] * X.double()[cc]).abs().sum(1)
            assert torch.all((vd.grad.cpu().double() - vc.grad).abs() <= (TOL[dtype] + 2 * eps) * mag_v)
        else:
            # the result is one product, exactly; the shim's own autograd splits a tie between its entries, so the gradient's reference
            # is the float64 sum over the entries that won by the shim's first-best scan
            ref, ref_arg = shim_reference(n, m, rowptr, col, v, X, reduce)
            _, arg = spmm_reduce(g, Xd.detach(), reduce, value=vd, return_arg=True)
            assert torch.equal(out.detach().cpu(), ref) and torch.equal(arg.cpu(), ref_arg)
            won = ref_arg.long()[row] == torch.arange(nnz).unsqueeze(1)
            wg = torch.where(won, v.double().unsqueeze(1) * G.double()[row], 0.0)
            want_dx = torch.zeros(m, h, dtype=torch.float64).index_add_(0, cc, wg)
            mag_x = torch.zeros(m, h, dtype=torch.float64).index_add_(0, cc, wg.abs())
            with pytest.raises(NotImplementedError):
                spmm_reduce(g, Xd, reduce, value=v.to(DEV).requires_grad_())
        err = (Xd.grad.cpu().double() - want_dx).abs()
        print(f"autograd {reduce} {dtype}: max dX err / mag = {(err / mag_x.clamp_min(1e-300)).max().item():.3e}")
        assert torch.all(err <= (TOL[dtype] + 2 * eps) * mag_x)
        # CPU tensors are staged to the device and come home
        out_host = spmm_reduce(g, X, reduce, value=v)
        assert not out_host.is_cuda and torch.equal(out_host, out.detach().cpu())


def test_sage_mean_matches_the_cpu_shim(rng):
    """SAGE(aggr="mean"), two layers, float64: logits and one SGD step's gradients as with the same model whose layers aggregate with the
    shim on the CPU (the tolerances of test_attention_gpu.test_gat_sgd_steps_match_the_cpu_reference)"""
    n, f_in, hid, f_out = 700, 16, 32, 8
    rowptr, col = random_csr(rng, n, n, 12, empty_frac=0.1, long_rows=((11, 64), (300, 700)))
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    base = gnn.SAGE(f_in, hid, f_out, num_layers=2, dropout=0.0, aggr="mean").double()

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
        conv.forward = (lambda c: lambda x, adj_t: c.lin_l(_shim_matmul(adj_t, x, "mean")) + c.lin_r(x))(conv)
    y_gpu, l_gpu, g_gpu = run(copy.deepcopy(base), DEV)
    y_cpu, l_cpu, g_cpu = run(cpu_model, "cpu")
    assert torch.allclose(y_gpu, y_cpu, rtol=1e-10, atol=1e-12) and np.allclose(l_gpu, l_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_gpu, g_cpu):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)
