"""Mean / max / min aggregation on CPU: the shim's matmul(reduce=...) against a per-row loop, and pygim_amd.reduce (spmm_reduce),
SparseGroupBase.mul_reduce and gnn.SAGEConv(aggr=...) driven with the C-ABI test double of test_attention_cpu.py, extended here with
numpy statements of pygim_spmm_reduce_workspace, pygim_spmm_reduce and pygim_spmm_reduce_backward."""
import types

import numpy as np
import pytest
import torch

import pygim_amd
from conftest import random_csr
from fake_abi import NP_OF, PygimError, _view
from pygim_amd import gnn, pim_ops, quantize
from pygim_amd.attention import EdgeGraph
from pygim_amd.backend_pim import spmm as spmm_mod
from pygim_amd.reduce import spmm_reduce
from pygim_amd.sparse_tensor import SparseTensorShim, _shim_matmul
from test_attention_cpu import FakeLibA, _rows

MEAN, MAX, MIN = 1, 2, 3


def first_best(prod, op):
    """(value, position) of the first best element of a 1-d array: the tie rule of the kernels"""
    best, at = prod[0], 0
    for k in range(1, len(prod)):
        if (prod[k] > best) if op == MAX else (prod[k] < best):
            best, at = prod[k], k
    return best, at


class FakeLibR(FakeLibA):
    """... with the entry points of pygim_amd.reduce, stated entry by entry"""

    def spmm_reduce_workspace(self, dtype, op, nrows, nnz, h):
        if op not in (MEAN, MAX, MIN) or (op == MEAN and dtype < self.FLT32):
            raise PygimError(1, "bad spmm_reduce_workspace arguments")
        return 48

    def spmm_reduce(self, dtype, op, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, x_ptr, ldx, h, out_ptr, ldo, arg_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("spmm_reduce")
        assert op in (MEAN, MAX, MIN) and ws_bytes >= 48 and not (op == MEAN and (arg_ptr or dtype < self.FLT32))
        npdt = NP_OF[dtype]
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        out = _rows(out_ptr, nrows, ldo, h, npdt)
        arg = _view(arg_ptr, nrows * h, np.int32).reshape(nrows, h) if arg_ptr else None
        out[:] = 0
        if arg is not None:
            arg[:] = -1
        if nnz == 0:
            return
        X = _rows(x_ptr, int(col.max()) + 1, ldx, h, npdt)
        val = _view(val_ptr, nnz, npdt) if val_ptr else np.ones(nnz, dtype=npdt)
        with np.errstate(over="ignore"):
            msg = val[:, None] * X[col]   # the type's own arithmetic
        for r in range(nrows):
            a, b = rowptr[r], rowptr[r + 1]
            if a == b:
                continue
            if op == MEAN:
                out[r] = (msg[a:b].astype(np.float64).sum(0) / (b - a)).astype(npdt)
                continue
            for f in range(h):
                out[r, f], at = first_best(msg[a:b, f], op)
                if arg is not None:
                    arg[r, f] = a + at

    def spmm_reduce_backward(self, dtype, ncols, rowptr_t_ptr, rows_t_ptr, perm_ptr, nnz, val_ptr, g_ptr, ldg, arg_ptr, h, dx_ptr, ldd, stream=0):
        self.calls.append("spmm_reduce_backward")
        assert dtype >= self.FLT32
        npdt = NP_OF[dtype]
        rowptr_t = _view(rowptr_t_ptr, ncols + 1, np.int32).astype(np.int64)
        rows_t = _view(rows_t_ptr, nnz, np.int32).astype(np.int64)
        perm = _view(perm_ptr, nnz, np.int32).astype(np.int64)
        dX = _rows(dx_ptr, ncols, ldd, h, npdt)
        dX[:] = 0
        if nnz == 0:
            return
        nrows = int(rows_t.max()) + 1
        G = _rows(g_ptr, nrows, ldg, h, npdt).astype(np.float64)
        arg = _view(arg_ptr, nrows * h, np.int32).reshape(nrows, h)
        val = _view(val_ptr, nnz, npdt).astype(np.float64) if val_ptr else np.ones(nnz)
        for c in range(ncols):
            acc = np.zeros(h)
            for k in range(rowptr_t[c], rowptr_t[c + 1]):
                e, r = perm[k], rows_t[k]
                acc += np.where(arg[r] == e, val[e] * G[r], 0.0)
            dX[c] = acc.astype(npdt)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibR()
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


def multigraph(rng, n, m, deg=4):
    """duplicates, empty rows and a long row"""
    rowptr, col = random_csr(rng, n, m, deg, empty_frac=0.2, long_rows=((5, 4 * deg),))
    col[rowptr[5] + 1] = col[rowptr[5]]   # a certain duplicate
    assert (np.diff(rowptr) == 0).any()
    return rowptr, col


def shim_of(rowptr, col, n, m, value=None):
    return SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), value=value, sparse_sizes=(n, m))


def loop_reference(rowptr, col, value, X, reduce):
    """torch_sparse.matmul(reduce=...) row by row: (out, arg)"""
    n, h = len(rowptr) - 1, X.size(1)
    out = torch.zeros(n, h, dtype=X.dtype)
    arg = torch.full((n, h), -1, dtype=torch.int32)
    for r in range(n):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        if a == b:
            continue
        msg = X[torch.from_numpy(col[a:b]).long()]
        if value is not None:
            msg = value[a:b].unsqueeze(1) * msg
        if reduce == "mean":
            s = msg.sum(0, dtype=X.dtype)
            out[r] = s / (b - a) if X.is_floating_point() else torch.div(s, b - a, rounding_mode="floor")
            continue
        for f in range(h):
            v, at = first_best(msg[:, f].tolist(), MAX if reduce == "max" else MIN)
            out[r, f], arg[r, f] = v, a + at
    return out, arg


def draw(rng, shape, dtype, lo=-3, hi=4):
    if dtype.is_floating_point:
        return torch.from_numpy(rng.uniform(-1, 1, size=shape)).to(dtype)
    return torch.from_numpy(rng.integers(lo, hi, size=shape)).to(dtype)


@pytest.mark.parametrize("with_value", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32])
@pytest.mark.parametrize("reduce", ["mean", "max", "min"])
def test_shim_matmul_matches_a_per_row_loop(rng, reduce, dtype, with_value):
    n, m, h = 60, 40, 5
    rowptr, col = multigraph(rng, n, m)
    value = draw(rng, (len(col),), dtype, 1, 4) if with_value else None
    X = draw(rng, (m, h), dtype)
    got = _shim_matmul(shim_of(rowptr, col, n, m, value), X, reduce)
    want, _ = loop_reference(rowptr, col, value, X, reduce)
    assert got.dtype == dtype and got.shape == (n, h)
    assert (got[np.diff(rowptr) == 0] == 0).all()
    if dtype.is_floating_point and reduce == "mean":
        assert torch.allclose(got, want, rtol=1e-5 if dtype == torch.float32 else 1e-12, atol=1e-6 if dtype == torch.float32 else 1e-14)
    else:
        assert torch.equal(got, want)


def test_shim_matmul_sum_is_unchanged(rng):
    n, m = 60, 40
    rowptr, col = multigraph(rng, n, m)
    for dtype in (torch.float32, torch.int32):
        value = draw(rng, (len(col),), dtype, 1, 4)
        X = draw(rng, (m, 6), dtype)
        adj = shim_of(rowptr, col, n, m, value)
        want = torch.zeros(n, 6, dtype=dtype).index_add_(0, adj.storage.row(), value.unsqueeze(1) * X[adj.storage.col()])
        for name in ("sum", "add"):
            got = _shim_matmul(adj, X, name)
            assert got.dtype == dtype and torch.allclose(got, want)
        assert torch.equal(_shim_matmul(adj, X), _shim_matmul(adj, X, "sum"))
    with pytest.raises(AssertionError):
        _shim_matmul(adj, X, "mul")


def test_public_names():
    assert pygim_amd.spmm_reduce is spmm_reduce
    assert hasattr(spmm_mod.SparseTensorCOO, "mul_reduce")


@pytest.mark.parametrize("reduce,dtype", [(r, d) for r in ("mean", "max", "min") for d in (torch.float64, torch.float32, torch.int16)
                                          if not (r == "mean" and d == torch.int16)])   # integer mean is refused: test_argument_validation
def test_spmm_reduce_through_the_fake(rng, fake, reduce, dtype):
    n, m, h = 24, 19, 6
    rowptr, col = multigraph(rng, n, m)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    X = draw(rng, (m, h), dtype)
    for value in (None, draw(rng, (len(col),), dtype, 1, 4)):
        fake.calls.clear()
        want, want_arg = loop_reference(rowptr, col, value, X, reduce)
        got = spmm_reduce(g, X, reduce, value=value)
        assert fake.calls == ["spmm_reduce"]
        if reduce == "mean":
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
            continue
        assert torch.equal(got, want)
        out2, arg = spmm_reduce(g, X, reduce, value=value, return_arg=True)
        assert torch.equal(out2, want) and arg.dtype == torch.int32 and torch.equal(arg, want_arg)
        assert torch.equal(got, _shim_matmul(shim_of(rowptr, col, n, m, value), X, reduce))


def test_argument_validation(rng, fake):
    n, m = 24, 19
    rowptr, col = multigraph(rng, n, m)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    nnz = len(col)
    v, X = torch.rand(nnz, dtype=torch.float64), torch.randn(m, 6, dtype=torch.float64)
    for bad in ("sum", "add", "mul", None):
        with pytest.raises(ValueError, match="spmm_values"):
            spmm_reduce(g, X, bad)
    with pytest.raises(TypeError):
        spmm_reduce(g, X, "max", value=v.float())          # dtype mismatch
    with pytest.raises(TypeError):
        spmm_reduce(g, X.int(), "mean")                     # integer mean
    with pytest.raises(TypeError):
        spmm_reduce(g, X.half(), "max")                     # not one of the six types
    with pytest.raises(ValueError):
        spmm_reduce(g, X[:-1], "max")                       # X does not cover the columns
    with pytest.raises(ValueError):
        spmm_reduce(g, X[:, 0], "max")
    with pytest.raises(ValueError):
        spmm_reduce(g, X, "min", value=v[:-1])
    with pytest.raises(ValueError):
        spmm_reduce(g, X, "min", value=v.unsqueeze(1))      # no multi-head values
    with pytest.raises(ValueError):
        spmm_reduce(g, X, "mean", return_arg=True)
    with pytest.raises(NotImplementedError, match="value"):
        spmm_reduce(g, X, "max", value=v.clone().requires_grad_())
    assert fake.calls == []


def tie_free(rng, m, h):
    """X whose entries are all distinct and far apart compared with gradcheck's step"""
    return torch.from_numpy(rng.permutation(m * h).reshape(m, h) / (m * h) - 0.5).double()


def test_gradcheck_mean(rng, fake):
    n, m, h = 12, 9, 4
    rowptr, col = multigraph(rng, n, m, deg=3)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    v = torch.rand(len(col), dtype=torch.float64).add_(0.5).requires_grad_()
    X = torch.randn(m, h, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: spmm_reduce(g, b, "mean", value=a), (v, X))
    assert torch.autograd.gradcheck(lambda b: spmm_reduce(g, b, "mean"), (X,))
    assert {"spmm_reduce", "spmm_values", "sddmm"} <= set(fake.calls) and "spmm_reduce_backward" not in fake.calls


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_gradcheck_max_min(rng, fake, reduce):
    n, m, h = 12, 9, 4
    rowptr, col = random_csr(rng, n, m, 3, empty_frac=0.2)
    keep = np.concatenate([np.unique(col[rowptr[r]:rowptr[r + 1]]) for r in range(n)])   # no duplicates: no row has a tie
    rowptr = np.concatenate([[0], np.cumsum([len(np.unique(col[rowptr[r]:rowptr[r + 1]])) for r in range(n)])]).astype(np.int32)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(keep), (n, m))
    v = torch.rand(len(keep), dtype=torch.float64).add_(0.5)
    X = tie_free(rng, m, h).requires_grad_()
    assert torch.autograd.gradcheck(lambda b: spmm_reduce(g, b, reduce), (X,), eps=1e-7)
    assert torch.autograd.gradcheck(lambda b: spmm_reduce(g, b, reduce, value=v), (X,), eps=1e-7)
    assert "spmm_reduce_backward" in fake.calls
    out = spmm_reduce(g, X, reduce)
    with pytest.raises(RuntimeError):   # no double backward
        gx, = torch.autograd.grad(out.sum(), X, create_graph=True)
        gx.sum().backward()


def test_planted_ties_send_the_gradient_to_the_lowest_entry(fake):
    # row 0: columns 2, 0, 2, 1 -- X[2] == X[0] in feature 0, so entries 0, 1 and 2 tie for the maximum there
    rowptr = torch.tensor([0, 4, 4, 6])
    col = torch.tensor([2, 0, 2, 1, 1, 0])
    g = EdgeGraph(rowptr, col, (3, 3))
    X = torch.tensor([[5.0, 1.0], [3.0, 7.0], [5.0, 2.0]], dtype=torch.float64, requires_grad=True)
    out, arg = spmm_reduce(g, X, "max", return_arg=True)
    assert out.tolist() == [[5.0, 7.0], [0.0, 0.0], [5.0, 7.0]]
    assert arg.tolist() == [[0, 3], [-1, -1], [5, 4]]
    G = torch.tensor([[1.0, 10.0], [100.0, 100.0], [1000.0, 10000.0]], dtype=torch.float64)
    out.backward(G)
    # feature 0 of row 0 goes to entry 0 (column 2) alone, although entries 1 (column 0) and 2 (column 2 again) hold the same value
    assert X.grad.tolist() == [[1000.0, 0.0], [0.0, 10010.0], [1.0, 0.0]]


def test_mul_reduce_uses_the_stored_values_and_no_group(rng, fake):
    pim_ops.load("spmm")
    n, m, h = 30, 21, 4
    rowptr, col = multigraph(rng, n, m)
    x = torch.randn(m, h, dtype=torch.float64)
    v0 = torch.rand(len(col)) + 0.5   # float32 values, float64 operand: cast to B's dtype
    for value in (None, v0):
        adj = shim_of(rowptr, col, n, m, value)
        A = spmm_mod.SparseTensorCOO(adj, dtype=torch.float64, format="CSR")
        for reduce in ("mean", "max", "min"):
            fake.calls.clear()
            got = A.mul_reduce(x, reduce)
            assert fake.calls == ["spmm_reduce"] and not fake.groups and A.sp_info_ptr is None
            want = _shim_matmul(adj, x, reduce) if value is None else _shim_matmul(shim_of(rowptr, col, n, m, v0.double()), x, reduce)
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        A.mul_reduce(x, "sum")


def test_sageconv_sum_issues_todays_calls(rng, fake, monkeypatch):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    seen = []
    real = quantize.message_and_aggregate
    monkeypatch.setattr(gnn, "message_and_aggregate", lambda a, x: (seen.append((a, x.shape)), real(a, x))[1])
    torch.manual_seed(1)
    x = torch.randn(n, 7)
    default = gnn.SAGEConv(7, 4)
    explicit = gnn.SAGEConv(7, 4, aggr="sum")
    explicit.load_state_dict(default.state_dict())
    want = default.lin_l(real(adj, x)) + default.lin_r(x)
    assert torch.equal(default(x, adj), want) and torch.equal(explicit(x, adj), want)
    assert seen == [(adj, x.shape)] * 2 and fake.calls == [], "aggr='sum' is message_and_aggregate and nothing else"
    assert gnn.SAGE(5, 8, 3).convs[0].aggr == "sum"
    with pytest.raises(ValueError):
        gnn.SAGEConv(7, 4, aggr="median")


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sageconv_mean_and_max_match_the_shim(rng, fake, aggr):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(2)
    conv = gnn.SAGEConv(7, 4, aggr=aggr).double()
    x = tie_free(rng, n, 7).requires_grad_()
    G = torch.randn(n, 4, dtype=torch.float64)
    out = conv(x, adj)
    out.backward(G)
    got = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    want_out = conv.lin_l(_shim_matmul(adj, x, aggr)) + conv.lin_r(x)
    want_out.backward(G)
    assert torch.allclose(out, want_out, rtol=1e-12, atol=1e-12)
    for a, b in zip(got, [x.grad] + [p.grad for p in conv.parameters()]):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    assert "spmm_reduce" in fake.calls
    sharded = types.SimpleNamespace(row_sharded=True)
    with pytest.raises(NotImplementedError):
        conv(x, sharded)


def test_sage_stack_with_mean_trains(rng, fake):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(0)
    model = gnn.SAGE(5, 8, 3, num_layers=2, dropout=0.0, aggr="mean").double()
    x, y = torch.randn(n, 5, dtype=torch.float64), torch.randn(n, 3, dtype=torch.float64)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((model(x, adj) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert losses[-1] < losses[0]
