"""Softmax aggregation per feature on CPU: pygim_amd.reduce.spmm_softmax, matmul_softmax / SparseGroupBase.mul_softmax and gnn.GENConv / GEN
driven with the C-ABI test double of test_half_cpu.py (it knows the 16-bit codes), extended here with numpy float64 statements of
pygim_spmm_softmax, pygim_spmm_softmax_backward and their workspace functions; the autograd function against torch.autograd through a
dense per-entry statement; GENConv against PyG's per-edge arithmetic written out; and, without a device, the two new launch-shape kinds
and the workspace functions of the real library."""
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
from pygim_amd.reduce import matmul_softmax, spmm_reduce, spmm_softmax
from test_attention_cpu import _rows
from test_half_cpu import BF16, FLT16, FakeLibH, load16, store16
from test_reduce_cpu import multigraph, shim_of

HALF_CODES = (FLT16, BF16)


def softmax_statement(rowptr, col, X, t):
    """row by row in float64: (out [n, h], lse [n, h]); rows without entries hold 0 and -inf"""
    n, h = len(rowptr) - 1, X.shape[1]
    out, lse = np.zeros((n, h)), np.full((n, h), -np.inf)
    for r in range(n):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        if a == b:
            continue
        x = X[col[a:b]]
        s = x * t
        m = s.max(0)
        e = np.exp(s - m)
        out[r] = (e * x).sum(0) / e.sum(0)
        lse[r] = m + np.log(e.sum(0))
    return out, lse


def softmax_backward_statement(rowptr_t, rows_t, X, t, G, out, lse):
    """column by column of A, in float64, as include/pygim_hip.h states the backward: (dX [ncols, h], dT [ncols, h])"""
    ncols, h = len(rowptr_t) - 1, X.shape[1]
    dX, dT = np.zeros((ncols, h)), np.zeros((ncols, h))
    for c in range(ncols):
        rows = rows_t[int(rowptr_t[c]):int(rowptr_t[c + 1])]
        if len(rows) == 0:
            continue
        p = np.exp(t * X[c] - lse[rows])
        a = (G[rows] * p).sum(0)
        b = (G[rows] * p * (X[c] - out[rows])).sum(0)
        dX[c] = a + t * b
        dT[c] = X[c] * b
    return dX, dT


class FakeLibS(FakeLibH):
    """... with the four entry points of spmm_softmax, stated row by row"""

    def _compute(self, dtype):
        return np.float32 if dtype in HALF_CODES else NP_OF[dtype]

    def _load(self, ptr, rows, ld, h, dtype):
        return load16(ptr, rows, ld, h, dtype) if dtype in HALF_CODES else _rows(ptr, rows, ld, h, NP_OF[dtype]).astype(np.float64)

    def _store(self, ptr, rows, ld, h, dtype, values):
        if dtype in HALF_CODES:
            store16(ptr, rows, ld, h, dtype, values)
        else:
            _rows(ptr, rows, ld, h, NP_OF[dtype])[:] = values.astype(NP_OF[dtype])

    def spmm_softmax_workspace(self, dtype, nrows, nnz, h):
        if dtype < self.FLT32 or nrows < 0 or nnz < 0 or h < 1:
            raise PygimError(1, "bad spmm_softmax_workspace arguments")
        return 96

    def spmm_softmax(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, t_ptr, h, out_ptr, ldo, lse_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("spmm_softmax")
        self.seen.append(("spmm_softmax", dtype))
        assert ws_bytes >= 96 and ldo >= h and ldx >= h
        rowptr, col, _ = self._csr(nrows, rowptr_ptr, col_ptr, nnz)
        ct = self._compute(dtype)
        t = _view(t_ptr, h, ct).astype(np.float64)   # the compute type, whatever X is
        X = self._load(x_ptr, int(col.max()) + 1 if nnz else 0, ldx, h, dtype)
        out, lse = softmax_statement(rowptr, col, X, t)
        self._store(out_ptr, nrows, ldo, h, dtype, out)
        if lse_ptr:
            _view(lse_ptr, nrows * h, ct).reshape(nrows, h)[:] = lse.astype(ct)

    def spmm_softmax_backward_workspace(self, dtype, ncols, nnz, h):
        if dtype < self.FLT32 or ncols < 0 or nnz < 0 or h < 1:
            raise PygimError(1, "bad spmm_softmax_backward_workspace arguments")
        return 64

    def spmm_softmax_backward(self, dtype, ncols, rowptr_t_ptr, rows_t_ptr, nnz, x_ptr, ldx, t_ptr, h, g_ptr, ldg, out_ptr, ldo, lse_ptr, dx_ptr, ldd, dt_ptr,
                              ws_ptr, ws_bytes, stream=0):
        self.calls.append("spmm_softmax_backward")
        self.seen.append(("spmm_softmax_backward", dtype))
        assert ws_bytes >= 64 and min(ldx, ldg, ldo, ldd) >= h
        rowptr_t, rows_t, _ = self._csr(ncols, rowptr_t_ptr, rows_t_ptr, nnz)
        ct = self._compute(dtype)
        nrows = int(rows_t.max()) + 1 if nnz else 0
        t = _view(t_ptr, h, ct).astype(np.float64)
        X = self._load(x_ptr, ncols, ldx, h, dtype)
        G, out = self._load(g_ptr, nrows, ldg, h, dtype), self._load(out_ptr, nrows, ldo, h, dtype)
        lse = _view(lse_ptr, nrows * h, ct).reshape(nrows, h).astype(np.float64) if nrows else np.zeros((0, h))
        dX, dT = softmax_backward_statement(rowptr_t, rows_t, X, t, G, out, lse)
        self._store(dx_ptr, ncols, ldd, h, dtype, dX)
        if dt_ptr:
            _view(dt_ptr, ncols * h, ct).reshape(ncols, h)[:] = dT.astype(ct)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibS()
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
    assert pygim_amd.spmm_softmax is spmm_softmax and pygim_amd.matmul_softmax is matmul_softmax
    assert hasattr(spmm_mod.SparseTensorCOO, "mul_softmax")
    for name in ("pygim_spmm_softmax", "pygim_spmm_softmax_workspace", "pygim_spmm_softmax_backward", "pygim_spmm_softmax_backward_workspace"):
        assert name in _lib.EXPORTS
    assert _lib.SHAPE_SPMM_SOFTMAX == 10 and _lib.SHAPE_SPMM_SOFTMAX_BACKWARD == 11
    assert hasattr(gnn, "GENConv") and hasattr(gnn, "GEN")


def test_argument_validation(rng, fake):
    rowptr, col, g = graph_of(rng)
    X = torch.randn(19, 6, dtype=torch.float64)
    for bad in (X.int(), X.long()):
        with pytest.raises(TypeError):
            spmm_softmax(g, bad)
    with pytest.raises(TypeError):
        spmm_softmax(g, X, t=torch.ones(6, dtype=torch.int64))
    for bad in (X[:-1], X[:, 0]):
        with pytest.raises(ValueError):
            spmm_softmax(g, bad)
    for t in (torch.ones(5, dtype=torch.float64), torch.ones(2, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            spmm_softmax(g, X, t)
    with pytest.raises(NotImplementedError):
        matmul_softmax(types.SimpleNamespace(row_sharded=True), X)
    assert fake.calls == []
    spmm_softmax(g, X, 0.5)
    assert fake.calls == ["spmm_softmax"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("t_kind", ["float", "0-d", "vector"])
def test_forward_matches_the_statement_and_the_composition(rng, fake, dtype, t_kind):
    rowptr, col, g = graph_of(rng)
    h = 5
    X = torch.from_numpy(rng.uniform(-1, 1, size=(19, h))).to(dtype)
    tv = rng.uniform(-2, 4, size=h)
    t = {"float": 1.5, "0-d": torch.tensor(1.5), "vector": torch.from_numpy(tv).float()}[t_kind]
    t64 = tv.astype(np.float32).astype(np.float64) if t_kind == "vector" else np.full(h, 1.5)
    out = spmm_softmax(g, X, t)
    assert out.dtype == dtype and out.shape == (24, h) and fake.calls == ["spmm_softmax"]
    want, _ = softmax_statement(rowptr, col, X.double().numpy(), t64)
    tol = {torch.float64: 1e-12, torch.float32: 1e-6, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    assert np.allclose(out.double().numpy(), want, rtol=tol, atol=tol)
    empty = np.diff(rowptr) == 0
    assert empty.any() and (out[torch.from_numpy(empty)] == 0).all()
    fake.calls.clear()
    comp = spmm_softmax(g, X, t, fused=False)   # X[col], edge_softmax with heads = h, spmm_values with heads = h
    assert fake.calls == ["edge_softmax", "spmm_values"]
    assert comp.dtype == dtype and np.allclose(comp.double().numpy(), want, rtol=2 * tol, atol=2 * tol)


def test_mul_softmax_uses_the_structure_and_no_group(rng, fake):
    pim_ops.load("spmm")
    n, m, h = 30, 21, 4
    rowptr, col = multigraph(rng, n, m)
    x = torch.randn(m, h, dtype=torch.float64)
    for value in (None, torch.rand(len(col)) + 0.5):   # stored values are not used: unit weights
        A = spmm_mod.SparseTensorCOO(shim_of(rowptr, col, n, m, value), dtype=torch.float64, format="CSR")
        fake.calls.clear()
        got = A.mul_softmax(x, 2.0)
        assert fake.calls == ["spmm_softmax"] and not fake.groups and A.sp_info_ptr is None
        want, _ = softmax_statement(rowptr, col, x.numpy(), np.full(h, 2.0))
        assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
        assert torch.equal(matmul_softmax(A, x, 2.0), got)


# ---- the autograd function against torch.autograd through a dense per-entry statement ----
def grad_graph():
    """row 0: four entries; row 1: one entry; row 2: empty; row 3: three entries of ONE column; row 4: two entries; column 0 is used once,
    columns 6 and 7 never"""
    rowptr = torch.tensor([0, 4, 5, 5, 8, 10])
    col = torch.tensor([2, 0, 3, 1, 4, 5, 5, 5, 1, 3])
    return rowptr, col, EdgeGraph(rowptr, col, (5, 8))


def dense_statement(rowptr, col, X, t):
    """torch ops per row, differentiable by torch.autograd: softmax of t * x over the row's entries, per feature"""
    rows = []
    for r in range(len(rowptr) - 1):
        x = X[col[rowptr[r]:rowptr[r + 1]]]
        rows.append(torch.zeros(X.size(1), dtype=X.dtype) if x.size(0) == 0 else (torch.softmax(x * t, 0) * x).sum(0))
    return torch.stack(rows)


@pytest.mark.parametrize("t_kind", ["float", "0-d", "vector"])
def test_the_backward_matches_torch_autograd(rng, fake, t_kind):
    rowptr, col, g = grad_graph()
    h = 3
    X = torch.from_numpy(rng.uniform(-1, 1, size=(8, h))).requires_grad_()
    t = {"float": 1.7, "0-d": torch.tensor(1.7, dtype=torch.float64), "vector": torch.from_numpy(rng.uniform(-2, 4, size=h))}[t_kind]
    if torch.is_tensor(t):
        t.requires_grad_()
    G = torch.from_numpy(rng.uniform(-1, 1, size=(5, h)))
    out = spmm_softmax(g, X, t)
    out.backward(G)
    assert fake.calls == ["spmm_softmax", "spmm_softmax_backward"], "one forward and one backward call"
    got_x, X.grad = X.grad.clone(), None
    got_t = None
    if torch.is_tensor(t):
        got_t, t.grad = t.grad.clone(), None
        assert got_t.shape == t.shape and got_t.dtype == t.dtype
    want = dense_statement(rowptr, col, X, t)
    want.backward(G)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert (got_x - X.grad).abs().max() <= 1e-10 * X.grad.abs().max(), "dX differs from torch.autograd's"
    assert (got_x[6:] == 0).all(), "columns without entries"
    if got_t is not None:
        assert (got_t - t.grad).abs().max() <= 1e-10 * t.grad.abs().max(), "dt differs from torch.autograd's"
    # dT is asked for only when t needs a gradient; X alone, t alone
    Y = X.detach().clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda b: spmm_softmax(g, b, 1.7), (Y,), eps=1e-7, atol=1e-6)
    if torch.is_tensor(t):
        assert torch.autograd.gradcheck(lambda tt: spmm_softmax(g, X.detach(), tt), (t.detach().clone().requires_grad_(),), eps=1e-7, atol=1e-6)
    with pytest.raises(RuntimeError):   # no double backward
        gx, = torch.autograd.grad(spmm_softmax(g, Y, 1.7).sum(), Y, create_graph=True)
        gx.sum().backward()


def test_dt_is_requested_only_when_t_needs_it(rng, fake, monkeypatch):
    rowptr, col, g = grad_graph()
    asked = []
    inner = fake.spmm_softmax_backward
    monkeypatch.setattr(fake, "spmm_softmax_backward", lambda *a, **k: (asked.append(bool(a[16])), inner(*a, **k))[1])
    X = torch.randn(8, 3, dtype=torch.float64, requires_grad=True)
    spmm_softmax(g, X, torch.tensor(2.0, dtype=torch.float64)).sum().backward()
    spmm_softmax(g, X, torch.tensor(2.0, dtype=torch.float64, requires_grad=True)).sum().backward()
    assert asked == [False, True]
    fake.calls.clear()
    spmm_softmax(g, X.detach(), 2.0)
    assert fake.calls == ["spmm_softmax"]


def test_the_backward_in_bfloat16(rng, fake):
    rowptr, col, g = grad_graph()
    h = 8
    X = torch.from_numpy(rng.uniform(-1, 1, size=(8, h))).bfloat16().requires_grad_()
    t = torch.tensor(1.25, dtype=torch.bfloat16, requires_grad=True)
    tv = torch.from_numpy(rng.uniform(0.5, 2, size=h)).float().requires_grad_()
    G = torch.from_numpy(rng.uniform(-1, 1, size=(5, h))).bfloat16()
    for tt in (t, tv):
        out = spmm_softmax(g, X, tt)
        assert out.dtype == torch.bfloat16
        out.backward(G)
        assert X.grad.dtype == torch.bfloat16 and X.grad.shape == X.shape and tt.grad.dtype == tt.dtype and tt.grad.shape == tt.shape
        Xd, td = X.detach().double().requires_grad_(), tt.detach().double().requires_grad_()
        dense_statement(rowptr, col, Xd, td).backward(G.double())
        # the stored out is rounded to bfloat16 before the backward reads it: |t| u sum |G| p |out| <= 2 u |t| per entry here
        assert (X.grad.double() - Xd.grad).abs().max() <= 2.0 ** -8 * Xd.grad.abs().max() + 4 * 2.0 ** -8 * float(td.detach().abs().max())
        X.grad = None
    assert ("spmm_softmax", BF16) in fake.seen and ("spmm_softmax_backward", BF16) in fake.seen


def test_the_limits_of_t(rng, fake):
    rowptr, col, g = graph_of(rng)
    X = torch.from_numpy(rng.uniform(-1, 1, size=(19, 7)))
    assert torch.allclose(spmm_softmax(g, X, 0.0), spmm_reduce(g, X, "mean"), rtol=1e-13, atol=1e-13)
    # t -> inf approaches max: the weight of an entry d below the maximum is exp(-t d); distinct values differ by more than 1e-4 here
    big = spmm_softmax(g, X, 1e6)
    assert torch.isfinite(big).all() and torch.allclose(big, spmm_reduce(g, X, "max"), rtol=0, atol=1e-12)
    low = spmm_softmax(g, X, -1e6)
    assert torch.allclose(low, spmm_reduce(g, X, "min"), rtol=0, atol=1e-12)


# ---- GENConv against PyG's per-edge arithmetic ----
def pyg_gen(conv, x, rowptr, col):
    """GENConv.forward of PyG (no edge features) written out: a message per stored entry relu(x_j) + eps, the aggregation per row in
    loops, + x_dst, the MLP"""
    n = x.size(0)
    src = x if conv.lin_src is None else conv.lin_src(x)
    msg = torch.relu(src[col]) + conv.eps   # [E, F]
    aggs = []
    for r in range(n):
        e = msg[rowptr[r]:rowptr[r + 1]]
        if e.size(0) == 0:
            aggs.append(torch.zeros(msg.size(1), dtype=x.dtype))
        elif conv.aggr == "softmax":
            aggs.append((torch.softmax(e * conv.t, 0) * e).sum(0))
        else:
            aggs.append({"mean": lambda: e.mean(0), "max": lambda: e.max(0).values, "sum": lambda: e.sum(0)}[conv.aggr]())
    dst = x if conv.lin_dst is None else conv.lin_dst(x)
    return conv.mlp(torch.stack(aggs) + dst)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("aggr,cin,learn_t", [("softmax", 7, True), ("softmax", 5, False), ("mean", 7, False), ("max", 5, False), ("sum", 7, False)])
def test_genconv_matches_pyg_per_edge_arithmetic(rng, fake, fused, aggr, cin, learn_t):
    n = 40
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(3)
    conv = gnn.GENConv(cin, 5, aggr=aggr, t=0.7, learn_t=learn_t, fused=fused).double()
    assert (conv.lin_src is None) == (cin == 5) and (conv.lin_dst is None) == (cin == 5)
    assert isinstance(conv.t, torch.nn.Parameter) == learn_t
    x = torch.from_numpy(rng.permutation(n * cin).reshape(n, cin) / (n * float(cin)) - 0.5).requires_grad_()
    G = torch.randn(n, 5, dtype=torch.float64)
    out = conv(x, adj)
    out.backward(G)
    got = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad()
    want = pyg_gen(conv, x, torch.from_numpy(rowptr).long(), torch.from_numpy(col).long())
    want.backward(G)
    assert out.shape == (n, 5) and (out - want).abs().max() <= 1e-9 * want.abs().max()
    for a, b in zip(got, [x.grad] + [p.grad for p in conv.parameters()]):
        assert (a - b).abs().max() <= 1e-9 * max(b.abs().max(), 1e-3)
    if aggr == "softmax":
        assert ("spmm_softmax" in fake.calls) == fused and ("spmm_softmax_backward" in fake.calls) == fused
        assert ("edge_softmax" in fake.calls) == (not fused)
    else:
        assert "spmm_softmax" not in fake.calls
    with pytest.raises(NotImplementedError):
        conv(x, types.SimpleNamespace(row_sharded=True))
    with pytest.raises(NotImplementedError):
        conv(x, adj, edge_attr=torch.zeros(len(col), 3))


def test_genconv_structure_and_rejections():
    for kw in (dict(aggr="powermean"), dict(edge_dim=3)):
        with pytest.raises(NotImplementedError) as e:
            gnn.GENConv(8, 8, **kw)
        assert "GENConv" in str(e.value)
    with pytest.raises(ValueError):
        gnn.GENConv(8, 8, aggr="median")
    conv = gnn.GENConv(8, 6, expansion=3)
    kinds = [type(m).__name__ for m in conv.mlp]
    assert kinds == ["Linear", "BatchNorm1d", "ReLU", "Linear"] and conv.mlp[0].out_features == 18 and conv.mlp[3].out_features == 6
    assert gnn.GENConv(8, 8).fused and gnn.GEN(5, 8, 3).convs[0].fused and gnn.GEN(5, 8, 3).convs[0].aggr == "softmax"


@pytest.mark.parametrize("mode", ["to", "autocast"])
def test_genconv_in_bfloat16(rng, fake, mode):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(2)
    conv = gnn.GENConv(8, 8, learn_t=True)
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
    assert conv.t.grad is not None and conv.t.grad.dtype == conv.t.dtype and conv.t.grad.shape == conv.t.shape
    want = ("spmm_softmax", BF16) if mode == "to" else None
    assert want is None or want in fake.seen
    assert "spmm_softmax" in fake.calls and "spmm_softmax_backward" in fake.calls


def test_gen_stack_trains(rng, fake):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(0)
    model = gnn.GEN(5, 8, 3, num_layers=2, dropout=0.0, learn_t=True).double()
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


# ---- the real library without a device: the launch-shape kinds and the workspace functions ----
@pytest.mark.parametrize("kind", [10, 11])
def test_kinds_10_and_11_answer_like_the_mean_fold_over_its_whole_domain(kind):
    """so the `mean` table of launch_shapes.py covers every launch shape of k_softmax_gather and k_softmax_grad (h = 1 .. 1100, the four
    gather types, aligned and not)"""
    assert (_lib.SHAPE_SPMM_SOFTMAX, _lib.SHAPE_SPMM_SOFTMAX_BACKWARD) == (10, 11)
    assert set(ls.FAMILIES["mean"]["dtypes"]) == {"f32", "f64", "bf16", "f16"}
    for dtype in ls.FAMILIES["mean"]["dtypes"]:
        dom = ls.domain("mean", dtype)
        assert [h for h, _ in dom] == list(range(1, 1101))
        for h, _ in dom:
            for aligned in (True, False):
                want = _lib.gather_launch_shape(_lib.SHAPE_SPMM_REDUCE, ls.CODE[dtype], h, 1, aligned)
                assert _lib.gather_launch_shape(kind, ls.CODE[dtype], h, 1, aligned) == want
    for heads in (0, 2, 4):   # the entry points have no heads: the query takes 1 and nothing else
        with pytest.raises(_lib.PygimError):
            _lib.gather_launch_shape(kind, _lib.FLT32, 32, heads)
    for code in (_lib.INT8, _lib.INT16, _lib.INT32, _lib.INT64):
        with pytest.raises(_lib.PygimError):
            _lib.gather_launch_shape(kind, code, 32, 1)
    assert _lib.gather_launch_shape(kind, _lib.BF16, _lib.GATHER_MAX_H, 1)["chunks"] > 1
    with pytest.raises(_lib.PygimError):
        _lib.gather_launch_shape(kind, _lib.FLT32, _lib.GATHER_MAX_H + 1, 1)


def test_the_workspace_functions_reject_bad_arguments_and_count_the_components():
    fwd, bwd = _lib.spmm_softmax_workspace, _lib.spmm_softmax_backward_workspace
    for ws in (fwd, bwd):
        for call in (lambda: ws(_lib.INT32, 4, 10, 8), lambda: ws(_lib.INT8, 4, 10, 8), lambda: ws(_lib.INT64, 4, 10, 8), lambda: ws(_lib.FLT32, -1, 10, 8),
                     lambda: ws(_lib.FLT32, 4, -1, 8), lambda: ws(_lib.FLT32, 4, 2 ** 31, 8), lambda: ws(_lib.FLT32, 4, 10, 0),
                     lambda: ws(_lib.FLT32, 4, 10, _lib.GATHER_MAX_H + 1)):
            with pytest.raises(_lib.PygimError):
                call()
    # per run two slots of h elements of every component, each sub-array rounded up to 16 bytes: nnz = 1000 is two runs, h = 9
    sub4, sub8 = (2 * 2 * 9 * 4 + 15) // 16 * 16, (2 * 2 * 9 * 8 + 15) // 16 * 16
    assert fwd(_lib.FLT32, 4, 1000, 9) == fwd(_lib.BF16, 4, 1000, 9) == fwd(_lib.FLT16, 4, 1000, 9) == 3 * sub4   # m, den, num
    assert bwd(_lib.FLT32, 4, 1000, 9) == bwd(_lib.BF16, 4, 1000, 9) == bwd(_lib.FLT16, 4, 1000, 9) == 2 * sub4   # a, b
    assert fwd(_lib.DBL64, 4, 1000, 9) == 3 * sub8 and bwd(_lib.DBL64, 4, 1000, 9) == 2 * sub8
    assert fwd(_lib.FLT32, 4, 0, 9) == bwd(_lib.FLT32, 4, 0, 9) == 0
    assert fwd(_lib.FLT32, 4, 1000, 9) == _lib.spmm_multi_reduce_workspace(_lib.FLT32, [_lib.STAT_MEAN], 4, 1000, 9) // 2 * 3
