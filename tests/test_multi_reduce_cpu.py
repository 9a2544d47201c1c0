"""Several statistics in one gather on CPU: pygim_amd.reduce.spmm_multi_reduce, SparseGroupBase.mul_multi_reduce and gnn.PNAConv / PNA
driven with the C-ABI test double of test_half_cpu.py (it knows the 16-bit codes), extended here with numpy statements of
pygim_spmm_multi_reduce_workspace and pygim_spmm_multi_reduce; the autograd formula against torch.autograd through a dense per-entry
statement; PNAConv against PyG's per-edge arithmetic written out; and, without a device, the new launch-shape kind and the workspace
function of the real library."""
import types

import numpy as np
import pytest
import torch

import launch_shapes as ls
import pygim_amd
from fake_abi import NP_OF, PygimError, _view
from pygim_amd import _lib, gnn, pim_ops
from pygim_amd.attention import EdgeGraph
from pygim_amd.backend_pim import spmm as spmm_mod
from pygim_amd.reduce import STAT_CODE, spmm_multi_reduce, spmm_reduce
from test_attention_cpu import _rows
from test_half_cpu import BF16, FLT16, FakeLibH, load16, store16
from test_reduce_cpu import first_best, multigraph, shim_of

SUM, MEAN, MIN, MAX, VAR, STD = range(6)
ALL = ("sum", "mean", "min", "max", "var", "std")
EPS = 1e-5


def multi_statement(rowptr, col, X, stats, eps):
    """the statistics row by row in float64: two-pass variance (the mean first, then the mean of the squared distances), clamped by
    construction; first-best max / min in entry order.  -> (out [n, k * h], arg_max, arg_min)"""
    n, h = len(rowptr) - 1, X.shape[1]
    out = np.zeros((n, len(stats) * h))
    amax, amin = np.full((n, h), -1, np.int32), np.full((n, h), -1, np.int32)
    for r in range(n):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        x = X[col[a:b]]
        for j, s in enumerate(stats):
            blk = out[r, j * h:(j + 1) * h]
            if a == b:
                blk[:] = np.sqrt(eps) if s == STD else 0.0
                continue
            mean = x.sum(0) / (b - a)
            var = ((x - mean) ** 2).sum(0) / (b - a)
            if s in (MAX, MIN):
                for f in range(h):
                    blk[f], at = first_best(x[:, f], 2 if s == MAX else 3)
                    (amax if s == MAX else amin)[r, f] = a + at
            else:
                blk[:] = {SUM: x.sum(0), MEAN: mean, VAR: var, STD: np.sqrt(var + eps)}[s]
    return out, amax, amin


class FakeLibM(FakeLibH):
    """... with the two entry points of spmm_multi_reduce, stated row by row"""

    def spmm_multi_reduce_workspace(self, dtype, stats, nrows, nnz, h):
        stats = list(stats)
        if dtype < self.FLT32 or not 1 <= len(stats) <= 6 or len(set(stats)) != len(stats) or any(s not in range(6) for s in stats):
            raise PygimError(1, "bad spmm_multi_reduce_workspace arguments")
        return 80

    def spmm_multi_reduce(self, dtype, stats, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, h, out_ptr, ldo, amax_ptr, amin_ptr, ws_ptr, ws_bytes,
                          stream=0):
        self.calls.append("spmm_multi_reduce")
        self.seen.append(("spmm_multi_reduce", dtype))
        stats = list(stats)
        k = len(stats)
        assert ws_bytes >= 80 and ldo >= k * h and len(set(stats)) == k
        assert not (amax_ptr and MAX not in stats) and not (amin_ptr and MIN not in stats) and not (STD in stats and not eps > 0)
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        ncols = int(col.max()) + 1 if nnz else 0
        X = load16(x_ptr, ncols, ldx, h, dtype) if dtype in (FLT16, BF16) else _rows(x_ptr, ncols, ldx, h, NP_OF[dtype]).astype(np.float64)
        out, amax, amin = multi_statement(rowptr, col, X, stats, eps)
        if dtype in (FLT16, BF16):
            store16(out_ptr, nrows, ldo, k * h, dtype, out)
        else:
            _rows(out_ptr, nrows, ldo, k * h, NP_OF[dtype])[:] = out.astype(NP_OF[dtype])
        if amax_ptr:
            _view(amax_ptr, nrows * h, np.int32).reshape(nrows, h)[:] = amax
        if amin_ptr:
            _view(amin_ptr, nrows * h, np.int32).reshape(nrows, h)[:] = amin


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibM()
    monkeypatch.setattr(pim_ops, "_lib", f)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pim_ops._variant = None
    yield f
    if pim_ops._library is not None:
        assert pim_ops._library != "native"
        pim_ops._library._destroy()
        pim_ops._library = None
    pim_ops._variant = None
    pim_ops._groups.clear()


def graph_of(rng, n=24, m=19):
    rowptr, col = multigraph(rng, n, m)
    return rowptr, col, EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))


def test_public_names():
    assert pygim_amd.spmm_multi_reduce is spmm_multi_reduce
    assert hasattr(spmm_mod.SparseTensorCOO, "mul_multi_reduce")
    assert STAT_CODE == {"sum": _lib.STAT_SUM, "mean": _lib.STAT_MEAN, "min": _lib.STAT_MIN, "max": _lib.STAT_MAX, "var": _lib.STAT_VAR,
                         "std": _lib.STAT_STD}
    for name in ("pygim_spmm_multi_reduce", "pygim_spmm_multi_reduce_workspace"):
        assert name in _lib.EXPORTS
    assert _lib.SHAPE_SPMM_MULTI_REDUCE == 9


def test_argument_validation(rng, fake):
    rowptr, col, g = graph_of(rng)
    X = torch.randn(19, 6, dtype=torch.float64)
    for bad in (("median",), ("mean", "add"), (), ("mean", "mean"), ("std", "max", "std")):
        with pytest.raises(ValueError):
            spmm_multi_reduce(g, X, bad)
    with pytest.raises(TypeError):
        spmm_multi_reduce(g, X.int())
    with pytest.raises(TypeError):
        spmm_multi_reduce(g, X.long(), ("max",))
    with pytest.raises(ValueError):
        spmm_multi_reduce(g, X[:-1])
    with pytest.raises(ValueError):
        spmm_multi_reduce(g, X[:, 0])
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            spmm_multi_reduce(g, X, ("std",), eps=eps)
    assert fake.calls == []
    spmm_multi_reduce(g, X, ("var", "max"), eps=0.0)   # eps matters to std alone
    assert fake.calls == ["spmm_multi_reduce"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("reduces", [("mean", "min", "max", "std"), ("std", "sum"), ("max",), ("min", "var", "mean"), ALL, ALL[::-1]])
def test_blocks_follow_reduces_and_match_the_single_calls(rng, fake, dtype, reduces):
    rowptr, col, g = graph_of(rng)
    h = 5
    X = torch.from_numpy(rng.uniform(2, 4, size=(19, h))).to(dtype)
    out = spmm_multi_reduce(g, X, reduces)
    assert out.dtype == dtype and out.shape == (24, len(reduces) * h) and fake.calls == ["spmm_multi_reduce"]
    want, wmax, wmin = multi_statement(rowptr, col, X.double().numpy(), [STAT_CODE[s] for s in reduces], EPS)
    tol = {torch.float64: 1e-12, torch.float32: 1e-6, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    assert np.allclose(out.double().numpy(), want, rtol=tol, atol=tol)
    empty = np.diff(rowptr) == 0
    assert empty.any()
    for j, s in enumerate(reduces):   # the empty-row values, per block
        blk = out[torch.from_numpy(empty), j * h:(j + 1) * h].double()
        assert torch.allclose(blk, torch.full_like(blk, EPS ** 0.5 if s == "std" else 0.0), rtol=tol, atol=0)
    out2, amax, amin = spmm_multi_reduce(g, X, reduces, return_arg=True)
    assert torch.equal(out2, out)
    assert (amax is None) == ("max" not in reduces) and (amin is None) == ("min" not in reduces)
    if amax is not None:
        assert amax.dtype == torch.int32 and np.array_equal(amax.numpy(), wmax) and (amax[torch.from_numpy(empty)] == -1).all()
    if amin is not None:
        assert np.array_equal(amin.numpy(), wmin)
    # the composition of spmm_reduce calls gives the same statistics (and the same arg tensors)
    fake.calls.clear()
    comp, cmax, cmin = spmm_multi_reduce(g, X, reduces, return_arg=True, fused=False)
    assert "spmm_multi_reduce" not in fake.calls and set(fake.calls) == {"spmm_reduce"}
    ctol = tol if dtype != torch.float32 else 2e-5   # mean(x^2) - mean(x)^2 in float32 on values around 3: 2 u 9 / var ~ 1e-5
    assert comp.dtype == dtype and np.allclose(comp.double().numpy(), want, rtol=ctol, atol=ctol)
    for a, b in ((amax, cmax), (amin, cmin)):
        assert (a is None and b is None) or torch.equal(a, b)
    for j, s in enumerate(reduces):   # a statistic does not depend on its neighbours in the list
        if s in ("mean", "max", "min") and dtype in (torch.float64, torch.float32):
            assert np.allclose(out[:, j * h:(j + 1) * h].numpy(), spmm_reduce(g, X, s).numpy(), rtol=tol, atol=tol)


def test_mul_multi_reduce_uses_the_structure_and_no_group(rng, fake):
    pim_ops.load("spmm")
    n, m, h = 30, 21, 4
    rowptr, col = multigraph(rng, n, m)
    x = torch.randn(m, h, dtype=torch.float64)
    for value in (None, torch.rand(len(col)) + 0.5):   # stored values are not used: unit weights
        A = spmm_mod.SparseTensorCOO(shim_of(rowptr, col, n, m, value), dtype=torch.float64, format="CSR")
        fake.calls.clear()
        got = A.mul_multi_reduce(x, ("mean", "std", "max"), 1e-3)
        assert fake.calls == ["spmm_multi_reduce"] and not fake.groups and A.sp_info_ptr is None
        want, _, _ = multi_statement(rowptr, col, x.numpy(), [MEAN, STD, MAX], 1e-3)
        assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        A.mul_multi_reduce(x, ("median",))


# ---- the autograd formula against torch.autograd through a dense per-entry statement ----
def grad_graph():
    """row 0: four entries; row 1: one entry; row 2: empty; row 3: three entries of ONE column (a constant row: var = 0, the gradient is 0
    through the clamp); row 4: two entries"""
    rowptr = torch.tensor([0, 4, 5, 5, 8, 10])
    col = torch.tensor([2, 0, 3, 1, 4, 5, 5, 5, 1, 3])
    return rowptr, col, EdgeGraph(rowptr, col, (5, 6))


def dense_statement(rowptr, col, X, reduces, eps):
    """torch ops per row, differentiable by torch.autograd: PyG's formulas (mean of squares minus squared mean, relu, sqrt(. + eps))"""
    rows = []
    for r in range(len(rowptr) - 1):
        x = X[col[rowptr[r]:rowptr[r + 1]]]
        if x.size(0) == 0:
            rows.append(torch.cat([torch.full((X.size(1),), eps ** 0.5 if s == "std" else 0.0, dtype=X.dtype) for s in reduces]))
            continue
        mean = x.mean(0)
        var = torch.relu((x * x).mean(0) - mean * mean)
        stat = {"sum": x.sum(0), "mean": mean, "min": x.min(0).values, "max": x.max(0).values, "var": var, "std": torch.sqrt(var + eps)}
        rows.append(torch.cat([stat[s] for s in reduces]))
    return torch.stack(rows)


def distinct(rng, m, h):
    return torch.from_numpy(rng.permutation(m * h).reshape(m, h) / (m * h) + 0.5).double()


@pytest.mark.parametrize("reduces", [("mean",), ("max", "min"), ("std",), ("var",), ("sum", "std"), ("mean", "min", "max", "std"), ALL])
def test_the_backward_matches_torch_autograd(rng, fake, reduces):
    rowptr, col, g = grad_graph()
    h = 3
    X = distinct(rng, 6, h).requires_grad_()
    G = torch.from_numpy(rng.uniform(-1, 1, size=(5, len(reduces) * h)))
    out = spmm_multi_reduce(g, X, reduces, eps=1e-3)
    out.backward(G)
    got, X.grad = X.grad.clone(), None
    want_out = dense_statement(rowptr, col, X, reduces, 1e-3)
    want_out.backward(G)
    assert torch.allclose(out, want_out, rtol=1e-12, atol=1e-12)
    assert (got - X.grad).abs().max() <= 1e-9 * X.grad.abs().max(), "dX differs from torch.autograd's"
    if {"var", "std"} & set(reduces):
        assert (out[3, reduces.index("var" if "var" in reduces else "std") * h] - (0.0 if "var" in reduces else 1e-3 ** 0.5)).abs() < 1e-12
    # the two A^T products are one call on [P | U]; max / min go through the kernel that exists
    assert fake.calls.count("spmm_values") == (1 if set(reduces) - {"max", "min"} else 0)
    assert fake.calls.count("spmm_reduce_backward") == len({"max", "min"} & set(reduces))
    assert torch.autograd.gradcheck(lambda b: spmm_multi_reduce(g, b, reduces, eps=1e-3), (distinct(rng, 6, h).requires_grad_(),), eps=1e-7, atol=1e-6)
    with pytest.raises(RuntimeError):   # no double backward
        Y = distinct(rng, 6, h).requires_grad_()
        gx, = torch.autograd.grad(spmm_multi_reduce(g, Y, reduces, eps=1e-3).sum(), Y, create_graph=True)
        gx.sum().backward()


def test_the_backward_in_bfloat16_takes_float32_statistics(rng, fake):
    rowptr, col, g = grad_graph()
    X = (distinct(rng, 6, 8) * 4).bfloat16().requires_grad_()
    out = spmm_multi_reduce(g, X, ("mean", "min", "max", "std"))
    assert out.dtype == torch.bfloat16
    G = torch.from_numpy(rng.uniform(-1, 1, size=(5, 32))).bfloat16()
    out.backward(G)
    Xd = X.detach().double().requires_grad_()
    dense_statement(rowptr, col, Xd, ("mean", "min", "max", "std"), EPS).backward(G.double())
    assert X.grad.dtype == torch.bfloat16
    assert (X.grad.double() - Xd.grad).abs().max() <= 2.0 ** -8 * Xd.grad.abs().max() + 1e-6
    assert ("spmm_multi_reduce", fake.FLT32) in fake.seen and ("spmm_values", fake.FLT32) in fake.seen, "mean and var again, and P | U, in float32"


# ---- PNAConv against PyG's per-edge arithmetic ----
def pyg_pna(conv, x, rowptr, col, avg_log):
    """PNAConv.forward of PyG (towers = 1, one pre-layer, no edge features) written out: a message per stored entry from
    cat([x_i, x_j]) through pre_nn, per-row aggregation loops, DegreeScalerAggregation's scalers, post_nn and lin"""
    n, F_ = x.size(0), conv.in_channels
    row = torch.repeat_interleave(torch.arange(n), torch.diff(rowptr))
    msg = conv.pre_nn(torch.cat([x[row], x[col]], -1))   # [E, F]
    aggs = []
    for r in range(n):
        e = msg[rowptr[r]:rowptr[r + 1]]
        if e.size(0) == 0:
            aggs.append(torch.cat([torch.full((F_,), conv.EPS ** 0.5 if s == "std" else 0.0, dtype=x.dtype) for s in conv.aggregators]))
            continue
        mean = e.mean(0)
        var = (e * e).mean(0) - mean * mean
        stat = {"sum": e.sum(0), "mean": mean, "min": e.min(0).values, "max": e.max(0).values, "var": torch.relu(var),
                "std": torch.sqrt(torch.relu(var) + conv.EPS)}
        aggs.append(torch.cat([stat[s] for s in conv.aggregators]))
    out = torch.stack(aggs)
    deg = torch.diff(rowptr).clamp(min=1).to(x.dtype).unsqueeze(1)
    scaled = {"identity": out, "amplification": out * (torch.log(deg + 1) / avg_log), "attenuation": out * (avg_log / torch.log(deg + 1))}
    out = torch.cat([scaled[s] for s in conv.scalers], -1)
    return conv.lin(conv.post_nn(torch.cat([x, out], -1)))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("aggregators,scalers,post_layers,with_deg",
                         [(("mean", "min", "max", "std"), ("identity", "amplification", "attenuation"), 1, True),
                          (("sum", "var", "max"), ("attenuation", "identity"), 2, False)])
def test_pnaconv_matches_pyg_per_edge_arithmetic(rng, fake, fused, aggregators, scalers, post_layers, with_deg):
    n = 40
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    d = np.diff(rowptr)
    hist = torch.from_numpy(np.bincount(d)) if with_deg else None   # PyG's degree histogram
    avg_log = float((np.log(np.arange(len(np.bincount(d))) + 1.0) * np.bincount(d)).sum() / n)   # PyG's formula; without deg: the first adjacency's
    torch.manual_seed(3)
    conv = gnn.PNAConv(7, 5, aggregators=aggregators, scalers=scalers, deg=hist, post_layers=post_layers, fused=fused).double()
    x = torch.from_numpy(rng.permutation(n * 7).reshape(n, 7) / (n * 7.0) - 0.5).requires_grad_()
    G = torch.randn(n, 5, dtype=torch.float64)
    out = conv(x, adj)
    out.backward(G)
    got = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    assert abs(float(conv.avg_log) - avg_log) <= 1e-12 * avg_log
    want = pyg_pna(conv, x, torch.from_numpy(rowptr).long(), torch.from_numpy(col).long(), avg_log)
    want.backward(G)
    assert out.shape == (n, 5) and (out - want).abs().max() <= 1e-9 * want.abs().max()
    for a, b in zip(got, [x.grad] + [p.grad for p in conv.parameters()]):
        assert (a - b).abs().max() <= 1e-9 * max(b.abs().max(), 1e-3)
    if fused:   # (without "mean" in the list the backward of var takes the mean again: one spmm_reduce)
        assert fake.calls.count("spmm_multi_reduce") == 1, "one gather per layer"
        assert ("spmm_reduce" in fake.calls) == ("mean" not in aggregators)
    else:
        assert "spmm_multi_reduce" not in fake.calls and "spmm_reduce" in fake.calls
    with pytest.raises(NotImplementedError):
        conv(x, types.SimpleNamespace(row_sharded=True))


def test_pnaconv_rejects_what_it_does_not_implement():
    for kw in (dict(towers=2), dict(pre_layers=2), dict(edge_dim=3)):
        with pytest.raises(NotImplementedError):
            gnn.PNAConv(8, 8, **kw)
    with pytest.raises(ValueError):
        gnn.PNAConv(8, 8, aggregators=("median",))
    with pytest.raises(ValueError):
        gnn.PNAConv(8, 8, scalers=("linear",))
    assert gnn.PNAConv(8, 8).fused == gnn.PNA_FUSED_DEFAULT and gnn.PNA(5, 8, 3).convs[0].fused == gnn.PNA_FUSED_DEFAULT


@pytest.mark.parametrize("mode", ["to", "autocast"])
def test_pnaconv_in_bfloat16(rng, fake, mode):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(2)
    conv = gnn.PNAConv(8, 8)
    x = torch.randn(n, 8)
    if mode == "to":
        conv, x = conv.to(torch.bfloat16), x.to(torch.bfloat16)
        out = conv(x.requires_grad_(), adj)
        assert out.dtype == torch.bfloat16
    else:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = conv(x.requires_grad_(), adj)
    out.float().square().mean().backward()
    assert out.shape == (n, 8) and torch.isfinite(out).all() and x.grad.dtype == x.dtype and torch.isfinite(x.grad).all()
    assert ("spmm_multi_reduce", BF16) in fake.seen


def test_pna_stack_trains(rng, fake):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(0)
    model = gnn.PNA(5, 8, 3, num_layers=2, dropout=0.0).double()
    x, y = torch.randn(n, 5, dtype=torch.float64), torch.randn(n, 3, dtype=torch.float64)
    opt = torch.optim.SGD(model.parameters(), lr=0.02)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((model(x, adj) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert losses[-1] < losses[0]


# ---- the real library without a device: the launch-shape kind and the workspace function ----
def test_kind_9_answers_like_the_mean_fold_over_its_whole_domain():
    """so the `mean` table of launch_shapes.py covers every launch shape of k_multi_gather"""
    for dtype in ls.FAMILIES["mean"]["dtypes"]:
        for h, _ in ls.domain("mean", dtype):
            for aligned in (True, False):
                want = _lib.gather_launch_shape(_lib.SHAPE_SPMM_REDUCE, ls.CODE[dtype], h, 1, aligned)
                assert _lib.gather_launch_shape(_lib.SHAPE_SPMM_MULTI_REDUCE, ls.CODE[dtype], h, 1, aligned) == want
    for heads in (0, 2, 4):   # the entry point has no heads: the query takes 1 and nothing else
        with pytest.raises(_lib.PygimError):
            _lib.gather_launch_shape(9, _lib.FLT32, 32, heads)
    for code in (_lib.INT8, _lib.INT16, _lib.INT32, _lib.INT64):
        with pytest.raises(_lib.PygimError):
            _lib.gather_launch_shape(9, code, 32, 1)
    assert _lib.gather_launch_shape(9, _lib.BF16, _lib.GATHER_MAX_H, 1)["chunks"] > 1
    with pytest.raises(_lib.PygimError):
        _lib.gather_launch_shape(9, _lib.FLT32, _lib.GATHER_MAX_H + 1, 1)


def test_the_workspace_function_rejects_bad_arguments_and_counts_the_components():
    ws = _lib.spmm_multi_reduce_workspace
    six = list(range(6))
    for call in (lambda: ws(_lib.INT32, [MEAN], 4, 10, 8), lambda: ws(_lib.FLT32, [], 4, 10, 8), lambda: ws(_lib.FLT32, six + [0], 4, 10, 8),
                 lambda: ws(_lib.FLT32, [MEAN, MEAN], 4, 10, 8), lambda: ws(_lib.FLT32, [6], 4, 10, 8), lambda: ws(_lib.FLT32, [-1], 4, 10, 8),
                 lambda: ws(_lib.FLT32, [MEAN], -1, 10, 8), lambda: ws(_lib.FLT32, [MEAN], 4, -1, 8), lambda: ws(_lib.FLT32, [MEAN], 4, 2 ** 31, 8),
                 lambda: ws(_lib.FLT32, [MEAN], 4, 10, 0), lambda: ws(_lib.FLT32, [MEAN], 4, 10, _lib.GATHER_MAX_H + 1)):
        with pytest.raises(_lib.PygimError):
            call()
    # per run two slots of h elements of every component, each sub-array rounded up to 16 bytes: nnz = 1000 is two runs, h = 9
    sub4, sub8 = (2 * 2 * 9 * 4 + 15) // 16 * 16, (2 * 2 * 9 * 8 + 15) // 16 * 16
    assert ws(_lib.FLT32, [MEAN], 4, 1000, 9) == ws(_lib.FLT32, [SUM, STD, VAR], 4, 1000, 9) == 2 * sub4
    assert ws(_lib.FLT32, [MAX], 4, 1000, 9) == ws(_lib.FLT32, [MIN, MAX], 4, 1000, 9) == 4 * sub4
    assert ws(_lib.FLT32, six, 4, 1000, 9) == ws(_lib.BF16, six, 4, 1000, 9) == ws(_lib.FLT16, [STD, MIN], 4, 1000, 9) == 6 * sub4
    assert ws(_lib.DBL64, six, 4, 1000, 9) == 4 * sub8 + 2 * sub4
    assert ws(_lib.FLT32, six, 4, 0, 9) == 0
