"""Messages with a feature-wide edge feature on CPU: pygim_amd.reduce.spmm_edge, matmul_edge / SparseGroupBase.mul_edge and gnn.GINEConv /
GINE / GENEConv driven with the C-ABI test double of test_softmax_aggr_cpu.py, extended here with numpy float64 statements of
pygim_spmm_edge, pygim_spmm_edge_softmax, pygim_spmm_edge_backward and their workspace functions; the autograd function against
torch.autograd through a dense per-entry statement; the layers against PyG's per-edge arithmetic written out; and, without a device, the two
new launch-shape kinds, the workspace functions and the argument checks of the real library."""
import ctypes

import numpy as np
import pytest
import torch

import launch_shapes as ls
import pygim_amd
from fake_abi import PygimError, _view
from pygim_amd import _lib, gnn, pim_ops
from pygim_amd.attention import EdgeGraph
from pygim_amd.backend_pim import spmm as spmm_mod
from pygim_amd.reduce import matmul_edge, spmm_edge
from test_reduce_cpu import first_best, multigraph, shim_of
from test_softmax_aggr_cpu import FakeLibS

SUM, MEAN, MAX, MIN, SOFTMAX = 4, 1, 2, 3, 5   # PYGIM_REDUCE_*
OP_OF = {"sum": SUM, "mean": MEAN, "max": MAX, "min": MIN, "softmax": SOFTMAX}
FOLDS = ("sum", "mean", "max", "min", "softmax")
ACTS = (None, "relu")


def message(X, E, col, relu, eps):
    """msg [nnz, h] in float64: act(X[col] + E) + eps; relu keeps NaN; eps = 0 is not added"""
    m = X[col] + E
    if relu:
        m = np.where(m < 0, 0.0, m)
    return m + eps if eps != 0 else m


def edge_statement(rowptr, col, X, E, reduce, relu, eps, t=None):
    """row by row in float64: (out [n, h], arg [n, h] (max / min, else None), lse [n, h] (softmax, else None)); rows without entries hold 0,
    -1 and -inf"""
    n, h = len(rowptr) - 1, X.shape[1]
    msg = message(X, E, col, relu, eps)
    out = np.zeros((n, h))
    arg = np.full((n, h), -1, dtype=np.int32) if reduce in ("max", "min") else None
    lse = np.full((n, h), -np.inf) if reduce == "softmax" else None
    for r in range(n):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        if a == b:
            continue
        m = msg[a:b]
        if reduce == "sum":
            out[r] = m.sum(0)
        elif reduce == "mean":
            out[r] = m.sum(0) / (b - a)
        elif reduce == "softmax":
            s = m * t
            top = s.max(0)
            e = np.exp(s - top)
            out[r] = (e * m).sum(0) / e.sum(0)
            lse[r] = top + np.log(e.sum(0))
        else:
            for f in range(h):
                out[r, f], at = first_best(m[:, f], OP_OF[reduce])
                arg[r, f] = a + at
    return out, arg, lse


def edge_backward_statement(rowptr, col, X, E, G, reduce, relu, eps, arg=None, t=None, out=None, lse=None):
    """entry by entry in float64, as include/pygim_hip.h states the backward: (dE [nnz, h], dT [h] (softmax, else None))"""
    n, h = len(rowptr) - 1, X.shape[1]
    row = np.repeat(np.arange(n), np.diff(rowptr))
    msg = message(X, E, col, relu, eps)
    live = (X[col] + E > 0) if relu else np.ones_like(msg, dtype=bool)
    dT = None
    if reduce == "sum":
        c = G[row]
    elif reduce == "mean":
        c = G[row] / np.diff(rowptr)[row][:, None]
    elif reduce == "softmax":
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.exp(t * msg - lse[row])
            c = G[row] * p * (1 + t * (msg - out[row]))
            dT = (G[row] * p * msg * (msg - out[row])).sum(0)
    else:
        c = np.where(arg[row] == np.arange(len(col))[:, None], G[row], 0.0)
    return np.where(live, c, 0.0), dT


class FakeLibE(FakeLibS):
    """... with the six entry points of spmm_edge, stated in float64"""

    def _args(self, dtype, op, act, eps):
        half = dtype in (6, 7)
        if op not in (SUM, MEAN, MAX, MIN, SOFTMAX) or act not in (0, 1) or eps != eps or dtype < self.FLT32 or (half and op in (MAX, MIN)):
            raise PygimError(1, "bad spmm_edge arguments")

    def spmm_edge_workspace(self, dtype, op, nrows, nnz, h):
        self._args(dtype, op, 0, 0.0)
        if op == SOFTMAX or nrows < 0 or nnz < 0 or h < 1:
            raise PygimError(1, "bad spmm_edge_workspace arguments")
        return 80

    def spmm_edge_softmax_workspace(self, dtype, nrows, nnz, h):
        self._args(dtype, SOFTMAX, 0, 0.0)
        return 96

    def spmm_edge_backward_workspace(self, dtype, op, nrows, nnz, h):
        self._args(dtype, op, 0, 0.0)
        return (nnz + 511) // 512

    def _operands(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, h):
        rowptr, col, _ = self._csr(nrows, rowptr_ptr, col_ptr, nnz)
        assert min(ldx, lde) >= h and (e_ptr or nnz == 0)
        X = self._load(x_ptr, int(col.max()) + 1 if nnz else 0, ldx, h, dtype)
        E = self._load(e_ptr, nnz, lde, h, dtype) if nnz else np.zeros((0, h))
        return rowptr, col, X, E

    def spmm_edge(self, dtype, op, act, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, h, out_ptr, ldo, arg_ptr, ws_ptr, ws_bytes, stream=0):
        self.calls.append("spmm_edge")
        self.seen.append(("spmm_edge", dtype))
        self._args(dtype, op, act, eps)
        assert op != SOFTMAX and ws_bytes >= 80 and ldo >= h and not (arg_ptr and op in (SUM, MEAN))
        rowptr, col, X, E = self._operands(dtype, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, h)
        name = {v: k for k, v in OP_OF.items()}[op]
        out, arg, _ = edge_statement(rowptr, col, X, E, name, act == 1, eps)
        self._store(out_ptr, nrows, ldo, h, dtype, out)
        if arg_ptr:
            _view(arg_ptr, nrows * h, np.int32).reshape(nrows, h)[:] = arg

    def spmm_edge_softmax(self, dtype, act, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, t_ptr, h, out_ptr, ldo, lse_ptr, ws_ptr, ws_bytes,
                          stream=0):
        self.calls.append("spmm_edge_softmax")
        self.seen.append(("spmm_edge_softmax", dtype))
        self._args(dtype, SOFTMAX, act, eps)
        assert ws_bytes >= 96 and ldo >= h
        rowptr, col, X, E = self._operands(dtype, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, h)
        ct = self._compute(dtype)
        t = _view(t_ptr, h, ct).astype(np.float64)
        out, _, lse = edge_statement(rowptr, col, X, E, "softmax", act == 1, eps, t)
        self._store(out_ptr, nrows, ldo, h, dtype, out)
        if lse_ptr:
            _view(lse_ptr, nrows * h, ct).reshape(nrows, h)[:] = lse.astype(ct)

    def spmm_edge_backward(self, dtype, op, act, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, g_ptr, ldg, arg_ptr, t_ptr, out_ptr, ldo, lse_ptr,
                           h, de_ptr, ldde, dt_part_ptr, stream=0):
        self.calls.append("spmm_edge_backward")
        self.seen.append(("spmm_edge_backward", dtype))
        self._args(dtype, op, act, eps)
        assert min(ldg, ldde) >= h and not (dt_part_ptr and op != SOFTMAX)
        if nnz == 0:
            return
        rowptr, col, X, E = self._operands(dtype, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, h)
        ct = self._compute(dtype)
        G = self._load(g_ptr, nrows, ldg, h, dtype)
        kw = {}
        if op in (MAX, MIN):
            kw["arg"] = _view(arg_ptr, nrows * h, np.int32).reshape(nrows, h)
        if op == SOFTMAX:
            kw = dict(t=_view(t_ptr, h, ct).astype(np.float64), out=self._load(out_ptr, nrows, ldo, h, dtype),
                      lse=_view(lse_ptr, nrows * h, ct).reshape(nrows, h).astype(np.float64))
        name = {v: k for k, v in OP_OF.items()}[op]
        dE, dT = edge_backward_statement(rowptr, col, X, E, G, name, act == 1, eps, **kw)
        self._store(de_ptr, nnz, ldde, h, dtype, dE)
        if dt_part_ptr:   # one row per run; the double leaves the whole sum in run 0
            runs = (nnz + 511) // 512
            part = _view(dt_part_ptr, runs * h, ct).reshape(runs, h)
            part[:] = 0
            part[0] = dT.astype(ct)


@pytest.fixture(autouse=True)
def keep_the_global_generator():
    """tests elsewhere in the suite draw from torch's global generator without seeding it: leave it as it was found"""
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibE()
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
    assert pygim_amd.spmm_edge is spmm_edge and pygim_amd.matmul_edge is matmul_edge
    assert hasattr(spmm_mod.SparseTensorCOO, "mul_edge")
    for name in ("pygim_spmm_edge", "pygim_spmm_edge_workspace", "pygim_spmm_edge_softmax", "pygim_spmm_edge_softmax_workspace",
                 "pygim_spmm_edge_backward", "pygim_spmm_edge_backward_workspace"):
        assert name in _lib.EXPORTS
    assert _lib.SHAPE_SPMM_EDGE == 12 and _lib.SHAPE_SPMM_EDGE_BACKWARD == 13
    assert _lib.REDUCE_SUM not in (_lib.REDUCE_MEAN, _lib.REDUCE_MAX, _lib.REDUCE_MIN) and (_lib.REDUCE_SUM, _lib.REDUCE_SOFTMAX) == (SUM, SOFTMAX)
    assert hasattr(gnn, "GINEConv") and hasattr(gnn, "GINE") and issubclass(gnn.GENEConv, gnn.GENConv)


def test_argument_validation(rng, fake):
    rowptr, col, g = graph_of(rng)
    X = torch.randn(19, 6, dtype=torch.float64)
    E = torch.randn(g.nnz, 6, dtype=torch.float64)
    for bad in (X.int(), X.long()):
        with pytest.raises(TypeError):
            spmm_edge(g, bad, E)
    with pytest.raises(TypeError):
        spmm_edge(g, X, E.float())
    for reduce in ("max", "min"):   # 16-bit max / min stays the TypeError it is in spmm_reduce
        with pytest.raises(TypeError):
            spmm_edge(g, X.bfloat16(), E.bfloat16(), reduce)
    with pytest.raises(TypeError):
        spmm_edge(g, X, E, "softmax", t=torch.ones(6, dtype=torch.int64))
    for bx, be in ((X[:-1], E), (X[:, 0], E), (X, E[:-1]), (X, E[:, :5])):
        with pytest.raises(ValueError):
            spmm_edge(g, bx, be)
    for kw in (dict(reduce="median"), dict(act="tanh"), dict(eps=float("nan")), dict(reduce="sum", return_arg=True),
               dict(reduce="softmax", t=torch.ones(5, dtype=torch.float64))):
        with pytest.raises(ValueError):
            spmm_edge(g, X, E, **kw)
    assert fake.calls == []
    spmm_edge(g, X, E, "mean", "relu", 0.5)
    assert fake.calls == ["spmm_edge"]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("reduce", FOLDS)
def test_forward_matches_the_statement_and_the_composition(rng, fake, reduce, act):
    rowptr, col, g = graph_of(rng)
    h = 5
    X = torch.from_numpy(rng.uniform(-1, 1, size=(19, h)))
    E = torch.from_numpy(rng.uniform(-1, 1, size=(g.nnz, h)))
    tv = rng.uniform(-2, 4, size=h)
    want, want_arg, _ = edge_statement(rowptr, col, X.numpy(), E.numpy(), reduce, act == "relu", 0.25, tv)
    got = spmm_edge(g, X, E, reduce, act, 0.25, torch.from_numpy(tv))
    assert fake.calls == ["spmm_edge_softmax" if reduce == "softmax" else "spmm_edge"]
    assert got.shape == (24, h) and np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    assert empty.any() and (got[empty] == 0).all()
    fake.calls.clear()
    comp = spmm_edge(g, X, E, reduce, act, 0.25, torch.from_numpy(tv), fused=False)   # X[col] + E, then the functions that exist
    assert "spmm_edge" not in fake.calls and "spmm_edge_softmax" not in fake.calls and fake.calls
    assert np.allclose(comp.numpy(), want, rtol=1e-12, atol=1e-12), "fused=False differs from fused=True"
    if reduce in ("max", "min"):
        for fused in (True, False):
            out, arg = spmm_edge(g, X, E, reduce, act, 0.25, fused=fused, return_arg=True)
            assert arg.dtype == torch.int32 and np.array_equal(arg.numpy(), want_arg) and np.allclose(out.numpy(), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_the_narrower_types_round_once(rng, fake, dtype):
    rowptr, col, g = graph_of(rng)
    h = 8
    X = torch.from_numpy(rng.uniform(-1, 1, size=(19, h))).to(dtype)
    E = torch.from_numpy(rng.uniform(-1, 1, size=(g.nnz, h))).to(dtype)
    u = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    tiny = 2.0 ** -25 if dtype == torch.float16 else 1e-30   # half the spacing of float16's subnormals: a message of eps alone lies among them
    for reduce in ("sum", "mean", "softmax"):
        want, _, _ = edge_statement(rowptr, col, X.double().numpy(), E.double().numpy(), reduce, True, 1e-7, np.full(h, 1.5))
        got = spmm_edge(g, X, E, reduce, "relu", 1e-7, 1.5)
        assert got.dtype == dtype and (np.abs(got.double().numpy() - want) <= u * np.abs(want) + tiny).all()
    code = {torch.float32: _lib.FLT32, torch.bfloat16: _lib.BF16, torch.float16: _lib.FLT16}[dtype]
    assert ("spmm_edge", code) in fake.seen and ("spmm_edge_softmax", code) in fake.seen


def test_mul_edge_uses_the_structure_and_no_group(rng, fake):
    pim_ops.load("spmm")
    n, m, h = 30, 21, 4
    rowptr, col = multigraph(rng, n, m)
    x = torch.randn(m, h, dtype=torch.float64)
    e = torch.randn(len(col), h, dtype=torch.float64)
    for value in (None, torch.rand(len(col)) + 0.5):   # stored values are not used: unit weights
        A = spmm_mod.SparseTensorCOO(shim_of(rowptr, col, n, m, value), dtype=torch.float64, format="CSR")
        fake.calls.clear()
        got = A.mul_edge(x, e, "sum", "relu")
        assert fake.calls == ["spmm_edge"] and not fake.groups and A.sp_info_ptr is None
        want, _, _ = edge_statement(rowptr, col, x.numpy(), e.numpy(), "sum", True, 0.0)
        assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
        assert torch.equal(matmul_edge(A, x, e, "sum", "relu"), got)


# ---- the autograd function against torch.autograd through a dense per-entry statement ----
def grad_graph():
    """row 0: four entries; row 1: one entry; row 2: empty; row 3: three entries of ONE column; row 4: two entries; column 0 is used once,
    columns 6 and 7 never"""
    rowptr = torch.tensor([0, 4, 5, 5, 8, 10])
    col = torch.tensor([2, 0, 3, 1, 4, 5, 5, 5, 1, 3])
    return rowptr, col, EdgeGraph(rowptr, col, (5, 8))


def dense_statement(rowptr, col, X, E, reduce, act, eps, t=None):
    """torch ops per entry and per row, differentiable by torch.autograd"""
    msg = X[col] + E
    if act == "relu":
        msg = torch.relu(msg)
    msg = msg + eps
    rows = []
    for r in range(len(rowptr) - 1):
        m = msg[rowptr[r]:rowptr[r + 1]]
        if m.size(0) == 0:
            rows.append(torch.zeros(X.size(1), dtype=X.dtype))
        else:
            rows.append({"sum": lambda: m.sum(0), "mean": lambda: m.mean(0), "max": lambda: m.max(0).values, "min": lambda: m.min(0).values,
                         "softmax": lambda: (torch.softmax(m * t, 0) * m).sum(0)}[reduce]())
    return torch.stack(rows)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("reduce,t_kind", [("sum", None), ("mean", None), ("max", None), ("min", None), ("softmax", "float"), ("softmax", "vector")])
def test_the_backward_matches_torch_autograd(rng, fake, reduce, act, t_kind):
    rowptr, col, g = grad_graph()
    h = 3
    X = torch.from_numpy(rng.uniform(-1, 1, size=(8, h))).requires_grad_()
    E = torch.from_numpy(rng.uniform(-1, 1, size=(10, h))).requires_grad_()
    assert not (act == "relu") or ((X.detach()[col] + E.detach()) < 0).any(), "relu must cut something"
    t = {None: 1.0, "float": 1.7, "vector": torch.from_numpy(rng.uniform(-2, 4, size=h)).requires_grad_()}[t_kind]
    G = torch.from_numpy(rng.uniform(-1, 1, size=(5, h)))
    out = spmm_edge(g, X, E, reduce, act, 0.125, t)
    out.backward(G)
    fwd = "spmm_edge_softmax" if reduce == "softmax" else "spmm_edge"
    assert fake.calls == [fwd, "spmm_edge_backward", "spmm_values"], "one forward call, one for dE, and the sum kernel on the transposed structure for dX"
    got_x, got_e, X.grad, E.grad = X.grad.clone(), E.grad.clone(), None, None
    got_t = None
    if torch.is_tensor(t):
        got_t, t.grad = t.grad.clone(), None
        assert got_t.shape == t.shape and got_t.dtype == t.dtype
    want = dense_statement(rowptr, col, X, E, reduce, act, 0.125, t)
    want.backward(G)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert (got_e - E.grad).abs().max() <= 1e-10 * E.grad.abs().max(), "dE differs from torch.autograd's"
    assert (got_x - X.grad).abs().max() <= 1e-10 * X.grad.abs().max(), "dX differs from torch.autograd's"
    assert (got_x[6:] == 0).all(), "columns without entries"
    if act == "relu":
        assert (got_e[(X.detach()[col] + E.detach()) <= 0] == 0).all(), "relu's gradient is exactly 0 where x + e <= 0"
    if reduce in ("max", "min"):
        assert ((got_e != 0).sum(0) <= 4).all(), "at most one entry per (row, feature) takes a gradient"
    if got_t is not None:
        assert (got_t - t.grad).abs().max() <= 1e-10 * t.grad.abs().max(), "dt differs from torch.autograd's"
    Y, F_ = X.detach().clone().requires_grad_(), E.detach().clone().requires_grad_()
    tf = t.detach() if torch.is_tensor(t) else t
    assert torch.autograd.gradcheck(lambda a, b: spmm_edge(g, a, b, reduce, act, 0.125, tf), (Y, F_), eps=1e-7, atol=1e-6)
    if torch.is_tensor(t):
        assert torch.autograd.gradcheck(lambda tt: spmm_edge(g, X.detach(), E.detach(), reduce, act, 0.125, tt), (t.detach().clone().requires_grad_(),),
                                        eps=1e-7, atol=1e-6)
    with pytest.raises(RuntimeError):   # no double backward
        gx, = torch.autograd.grad(spmm_edge(g, Y, F_, reduce, act, 0.125, tf).sum(), Y, create_graph=True)
        gx.sum().backward()


def test_only_what_needs_a_gradient_is_computed(rng, fake, monkeypatch):
    rowptr, col, g = grad_graph()
    asked = []
    inner = fake.spmm_edge_backward
    monkeypatch.setattr(fake, "spmm_edge_backward", lambda *a, **k: (asked.append(bool(a[22])), inner(*a, **k))[1])
    X = torch.randn(8, 3, dtype=torch.float64)
    E = torch.randn(10, 3, dtype=torch.float64, requires_grad=True)
    spmm_edge(g, X, E, "softmax", "relu", 0.0, torch.tensor(2.0, dtype=torch.float64)).sum().backward()
    assert fake.calls == ["spmm_edge_softmax", "spmm_edge_backward"], "E alone: no sum over the transposed structure"
    spmm_edge(g, X, E, "softmax", "relu", 0.0, torch.tensor(2.0, dtype=torch.float64, requires_grad=True)).sum().backward()
    assert asked == [False, True], "dT_part is asked for only when t needs a gradient"
    fake.calls.clear()
    spmm_edge(g, X, E.detach(), "softmax")
    assert fake.calls == ["spmm_edge_softmax"]


def test_the_backward_in_bfloat16(rng, fake):
    rowptr, col, g = grad_graph()
    h = 8
    X = torch.from_numpy(rng.uniform(-1, 1, size=(8, h))).bfloat16().requires_grad_()
    E = torch.from_numpy(rng.uniform(-1, 1, size=(10, h))).bfloat16().requires_grad_()
    t = torch.tensor(1.25, dtype=torch.bfloat16, requires_grad=True)
    G = torch.from_numpy(rng.uniform(-1, 1, size=(5, h))).bfloat16()
    out = spmm_edge(g, X, E, "softmax", "relu", 1e-7, t)
    assert out.dtype == torch.bfloat16
    out.backward(G)
    assert X.grad.dtype == torch.bfloat16 and E.grad.dtype == torch.bfloat16 and E.grad.shape == E.shape and t.grad.dtype == t.dtype and t.grad.shape == t.shape
    Xd, Ed, td = X.detach().double().requires_grad_(), E.detach().double().requires_grad_(), t.detach().double().requires_grad_()
    dense_statement(rowptr, col, Xd, Ed, "softmax", "relu", 1e-7, td).backward(G.double())
    # the stored out is rounded to bfloat16 before the backward reads it: |t| u sum |G| p |out| <= 2 u |t| per entry here (as in test_softmax_aggr_cpu)
    assert (E.grad.double() - Ed.grad).abs().max() <= 2.0 ** -8 * Ed.grad.abs().max() + 4 * 2.0 ** -8 * float(td.detach().abs())


# ---- the layers against PyG's per-edge arithmetic ----
def pyg_gine(conv, x, edge_attr, rowptr, col):
    """GINEConv.forward of PyG written out: a message per stored entry relu(x_j + lin(e_ij)), summed per row in a loop"""
    e = edge_attr if conv.lin is None else conv.lin(edge_attr)
    msg = torch.relu(x[col] + e)
    agg = torch.stack([msg[rowptr[r]:rowptr[r + 1]].sum(0) for r in range(x.size(0))])
    return conv.nn(agg + (1 + conv.eps) * x)


def pyg_gen_edge(conv, x, edge_attr, rowptr, col):
    """GENConv.forward of PyG with edge_dim (GENEConv here) written out: a message per stored entry relu(x_j + lin_edge(e_ij)) + eps, the aggregation per
    row in loops, + x_dst, the MLP"""
    src = x if conv.lin_src is None else conv.lin_src(x)
    e = edge_attr if conv.lin_edge is None else conv.lin_edge(edge_attr)
    msg = torch.relu(src[col] + e) + conv.eps
    aggs = []
    for r in range(x.size(0)):
        m = msg[rowptr[r]:rowptr[r + 1]]
        if m.size(0) == 0:
            aggs.append(torch.zeros(msg.size(1), dtype=x.dtype))
        elif conv.aggr == "softmax":
            aggs.append((torch.softmax(m * conv.t, 0) * m).sum(0))
        else:
            aggs.append({"mean": lambda: m.mean(0), "max": lambda: m.max(0).values, "sum": lambda: m.sum(0)}[conv.aggr]())
    dst = x if conv.lin_dst is None else conv.lin_dst(x)
    return conv.mlp(torch.stack(aggs) + dst)


def check_layer(conv, reference, x, edge_attr, rowptr, col, adj):
    G = torch.randn(x.size(0), reference(conv, x, edge_attr, rowptr, col).size(1), dtype=torch.float64)
    leaves = [x, edge_attr] + list(conv.parameters())
    out = conv(x, adj, edge_attr)
    out.backward(G)
    got = [p.grad.clone() for p in leaves]
    for p in leaves:
        p.grad = None
    want = reference(conv, x, edge_attr, rowptr, col)
    want.backward(G)
    assert (out - want).abs().max() <= 1e-9 * want.abs().max()
    for a, p in zip(got, leaves):
        assert (a - p.grad).abs().max() <= 1e-9 * max(p.grad.abs().max(), 1e-3)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("edge_dim,train_eps", [(3, True), (None, False)])
def test_gineconv_matches_pyg_per_edge_arithmetic(rng, fake, fused, edge_dim, train_eps):
    n, c = 40, 6
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(4)
    mlp = torch.nn.Sequential(torch.nn.Linear(c, 7), torch.nn.ReLU(), torch.nn.Linear(7, 5))
    conv = gnn.GINEConv(mlp, eps=0.3, train_eps=train_eps, edge_dim=edge_dim, fused=fused).double()
    assert isinstance(conv.eps, torch.nn.Parameter) == train_eps and (conv.lin is None) == (edge_dim is None)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(n, c))).requires_grad_()
    edge_attr = torch.from_numpy(rng.uniform(-1, 1, size=(len(col), edge_dim or c))).requires_grad_()
    check_layer(conv, pyg_gine, x, edge_attr, torch.from_numpy(rowptr).long(), torch.from_numpy(col).long(), adj)
    assert ("spmm_edge" in fake.calls) == fused and ("spmm_edge_backward" in fake.calls) == fused
    with pytest.raises(ValueError):
        conv(x, adj, torch.zeros(len(col), (edge_dim or c) + 1, dtype=torch.float64))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("aggr,cin,edge_dim,learn_t", [("softmax", 7, 3, True), ("softmax", 5, 5, False), ("mean", 7, 5, False), ("max", 5, 2, False),
                                                       ("sum", 7, 4, False)])
def test_geneconv_matches_pyg_per_edge_arithmetic(rng, fake, fused, aggr, cin, edge_dim, learn_t):
    n = 40
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(3)
    conv = gnn.GENEConv(cin, 5, edge_dim, aggr=aggr, t=0.7, learn_t=learn_t, fused=fused).double()
    assert (conv.lin_edge is None) == (edge_dim == 5), "lin_edge exactly when edge_dim differs from out_channels, as in PyG"
    x = torch.from_numpy(rng.permutation(n * cin).reshape(n, cin) / (n * float(cin)) - 0.5).requires_grad_()
    edge_attr = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(len(col), edge_dim))).requires_grad_()
    check_layer(conv, pyg_gen_edge, x, edge_attr, torch.from_numpy(rowptr).long(), torch.from_numpy(col).long(), adj)
    fwd = "spmm_edge_softmax" if aggr == "softmax" else "spmm_edge"
    assert (fwd in fake.calls) == fused and ("spmm_edge_backward" in fake.calls) == fused
    fake.calls.clear()
    conv(x, adj)   # edge_attr=None: the layer without edge features
    assert "spmm_edge" not in fake.calls and "spmm_edge_softmax" not in fake.calls
    with pytest.raises(ValueError):
        conv(x, adj, torch.zeros(len(col), edge_dim + 1, dtype=torch.float64))


def test_geneconv_draws_genconvs_parameters_and_genconv_still_refuses_edge_features(rng, fake):
    torch.manual_seed(5)
    plain = gnn.GENConv(7, 5, learn_t=True)
    torch.manual_seed(5)
    edged = gnn.GENEConv(7, 5, 3, learn_t=True)
    assert plain.lin_edge is None and plain.edge_dim is None and edged.lin_edge.in_features == 3
    have = dict(edged.named_parameters())
    for name, p in plain.named_parameters():
        assert torch.equal(p, have[name])
    for bad in (0, None):
        with pytest.raises(ValueError):
            gnn.GENEConv(7, 5, bad)
    with pytest.raises(NotImplementedError) as e:   # the class without edge features says where they are
        gnn.GENConv(7, 5, edge_dim=3)
    assert "GENEConv" in str(e.value)
    n = 12
    rowptr, col = multigraph(rng, n, n)
    with pytest.raises(NotImplementedError) as e:
        plain(torch.randn(n, 7), shim_of(rowptr, col, n, n), torch.zeros(len(col), 3))
    assert "GENEConv" in str(e.value)


@pytest.mark.parametrize("mode", ["to", "autocast"])
@pytest.mark.parametrize("layer", ["gen", "gine"])
def test_layers_in_bfloat16(rng, fake, layer, mode):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(2)
    if layer == "gen":
        conv = gnn.GENEConv(8, 8, 3, learn_t=True)
    else:
        conv = gnn.GINEConv(torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8)), edge_dim=3)
    x, e = torch.randn(n, 8), torch.randn(len(col), 3)
    if mode == "to":
        conv, x, e = conv.to(torch.bfloat16), x.to(torch.bfloat16), e.to(torch.bfloat16)
        out = conv(x.requires_grad_(), adj, e.requires_grad_())
        assert out.dtype == torch.bfloat16
    else:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = conv(x.requires_grad_(), adj, e.requires_grad_())
    out.float().square().mean().backward()
    assert out.shape == (n, 8) and torch.isfinite(out).all()
    assert x.grad.dtype == x.dtype and torch.isfinite(x.grad).all() and e.grad.shape == e.shape and torch.isfinite(e.grad).all()
    if layer == "gen":
        assert conv.t.grad is not None and conv.t.grad.shape == conv.t.shape
    fwd = "spmm_edge_softmax" if layer == "gen" else "spmm_edge"
    assert fwd in fake.calls and "spmm_edge_backward" in fake.calls
    if mode == "to":
        assert (fwd, _lib.BF16) in fake.seen


@pytest.mark.parametrize("kind", ["gine", "gen"])
def test_the_stacks_train_with_edge_features(rng, fake, kind):
    n = 22
    rowptr, col = multigraph(rng, n, n)
    adj = shim_of(rowptr, col, n, n)
    torch.manual_seed(0)
    if kind == "gine":
        model = gnn.GINE(5, 8, 3, edge_dim=4, num_layers=2, dropout=0.0, train_eps=True).double()
    else:
        model = gnn.GEN(5, 8, 3, num_layers=2, dropout=0.0, learn_t=True, edge_dim=4).double()
    x, y = torch.randn(n, 5, dtype=torch.float64), torch.randn(n, 3, dtype=torch.float64)
    e = torch.randn(len(col), 4, dtype=torch.float64)
    opt = torch.optim.SGD(model.parameters(), lr=0.02)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((model(x, adj, e) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert losses[-1] < losses[0]


# ---- the real library without a device: the launch-shape kinds, the workspace functions and the argument checks ----
@pytest.mark.parametrize("kind", [12, 13])
def test_kinds_12_and_13_answer_like_the_folds_without_edge_features(kind):
    """so the `mean` table of launch_shapes.py covers every launch shape of k_edge_gather, k_edge_softmax_gather and k_edge_message_grad
    (h = 1 .. 1100, the four gather types, aligned and not)"""
    assert (_lib.SHAPE_SPMM_EDGE, _lib.SHAPE_SPMM_EDGE_BACKWARD) == (12, 13)
    for dtype in ls.FAMILIES["mean"]["dtypes"]:
        for h, _ in ls.domain("mean", dtype):
            for aligned in (True, False):
                want = _lib.gather_launch_shape(_lib.SHAPE_SPMM_REDUCE, ls.CODE[dtype], h, 1, aligned)
                assert _lib.gather_launch_shape(_lib.SHAPE_SPMM_SOFTMAX, ls.CODE[dtype], h, 1, aligned) == want
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
    with pytest.raises(_lib.PygimError):
        _lib.gather_launch_shape(14, _lib.FLT32, 32, 1)


def test_the_workspace_functions_of_the_real_library():
    fold, soft, back = _lib.spmm_edge_workspace, _lib.spmm_edge_softmax_workspace, _lib.spmm_edge_backward_workspace
    for op in (_lib.REDUCE_SUM, _lib.REDUCE_MEAN, _lib.REDUCE_MAX, _lib.REDUCE_MIN):
        for ws in (fold, back):
            for call in (lambda: ws(_lib.INT32, op, 4, 10, 8), lambda: ws(_lib.FLT32, op, -1, 10, 8), lambda: ws(_lib.FLT32, op, 4, -1, 8),
                         lambda: ws(_lib.FLT32, op, 4, 2 ** 31, 8), lambda: ws(_lib.FLT32, op, 4, 10, 0),
                         lambda: ws(_lib.FLT32, op, 4, 10, _lib.GATHER_MAX_H + 1)):
                with pytest.raises(_lib.PygimError):
                    call()
    for ws in (fold, back):
        for op in (0, 6, -1):
            with pytest.raises(_lib.PygimError):
                ws(_lib.FLT32, op, 4, 10, 8)
        for op in (_lib.REDUCE_MAX, _lib.REDUCE_MIN):   # 16-bit max / min
            for code in (_lib.BF16, _lib.FLT16):
                with pytest.raises(_lib.PygimError):
                    ws(code, op, 4, 10, 8)
    with pytest.raises(_lib.PygimError):
        fold(_lib.FLT32, _lib.REDUCE_SOFTMAX, 4, 10, 8)   # the softmax fold has its own entry point
    for call in (lambda: soft(_lib.INT32, 4, 10, 8), lambda: soft(_lib.FLT32, 4, 10, 0), lambda: soft(_lib.FLT32, 4, 10, _lib.GATHER_MAX_H + 1)):
        with pytest.raises(_lib.PygimError):
            call()
    # the folds need what they need without E: the sum what spmm_values needs, mean / max / min what spmm_reduce needs, the softmax what spmm_softmax needs
    for code in (_lib.FLT32, _lib.DBL64, _lib.BF16, _lib.FLT16):
        assert fold(code, _lib.REDUCE_SUM, 4, 1000, 9) == fold(code, _lib.REDUCE_MEAN, 4, 1000, 9) == _lib.spmm_reduce_workspace(code, _lib.REDUCE_MEAN, 4, 1000, 9)
        assert fold(code, _lib.REDUCE_SUM, 4, 1000, 9) >= _lib.spmm_values_workspace(code, 4, 1000, 9, 1)
        assert soft(code, 4, 1000, 9) == _lib.spmm_softmax_workspace(code, 4, 1000, 9)
    for code in (_lib.FLT32, _lib.DBL64):
        for op in (_lib.REDUCE_MAX, _lib.REDUCE_MIN):
            assert fold(code, op, 4, 1000, 9) == _lib.spmm_reduce_workspace(code, op, 4, 1000, 9)
    # the backward has no scratch: its query counts the runs of 512 entries, the rows of dT_part
    for nnz, runs in ((0, 0), (1, 1), (512, 1), (513, 2), (1800, 4)):
        assert back(_lib.FLT32, _lib.REDUCE_SOFTMAX, 4, nnz, 9) == back(_lib.BF16, _lib.REDUCE_SUM, 4, nnz, 9) == runs


def test_the_real_library_rejects_bad_arguments_before_any_launch():
    """every PYGIM_ERR_INVALID case of the three entry points, with null or host pointers and no device: the argument checks come before
    the library asks for a device"""
    nan = float("nan")
    host = np.zeros(64, dtype=np.int32)
    p = host.ctypes.data

    def invalid(call):
        with pytest.raises(_lib.PygimError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID, str(e.value)

    def fold(dtype=_lib.FLT32, op=_lib.REDUCE_SUM, act=_lib.ACT_RELU, eps=0.0, nnz=4, h=8, e_ptr=0, others=0, arg=0, lde=8):
        return lambda: _lib.spmm_edge(dtype, op, act, eps, 2, others, others, nnz, others, 8, e_ptr, lde, h, others, 8, arg, others, 1 << 20)

    def soft(dtype=_lib.FLT32, act=_lib.ACT_RELU, eps=0.0, nnz=4, h=8, e_ptr=0, others=0, lde=8):
        return lambda: _lib.spmm_edge_softmax(dtype, act, eps, 2, others, others, nnz, others, 8, e_ptr, lde, others, h, others, 8, 0, others, 1 << 20)

    def back(dtype=_lib.FLT32, op=_lib.REDUCE_SOFTMAX, act=_lib.ACT_RELU, eps=0.0, nnz=4, h=8, e_ptr=0, others=0, part=0, lde=8):
        return lambda: _lib.spmm_edge_backward(dtype, op, act, eps, 2, others, others, nnz, others, 8, e_ptr, lde, others, 8, others, others, others, 8, others,
                                               h, others, 8, part)

    for make in (fold, soft, back):
        invalid(make(act=2))                       # an unknown act
        invalid(make(act=-1))
        invalid(make(eps=nan))                     # NaN eps
        invalid(make(dtype=_lib.INT32))            # a type the fold does not take
        invalid(make(dtype=_lib.INT8))
        invalid(make(h=_lib.GATHER_MAX_H + 1, lde=_lib.GATHER_MAX_H + 1))   # h > RG_MAX_H
        invalid(make(h=0))
        invalid(make(lde=7))                       # a row stride of E below h
        invalid(make())                            # every pointer NULL with nnz > 0
        invalid(make(others=p))                    # E alone NULL with nnz > 0 (and the others not device memory)
        invalid(make(others=p, e_ptr=p))           # host pointers
    for make in (fold, back):
        for op in (0, 6, -1):                      # an unknown op
            invalid(make(op=op))
        for op in (_lib.REDUCE_MAX, _lib.REDUCE_MIN):
            for code in (_lib.BF16, _lib.FLT16):   # 16-bit max / min
                invalid(make(dtype=code, op=op))
    invalid(fold(op=_lib.REDUCE_SOFTMAX))          # the softmax fold has its own entry point
    invalid(fold(op=_lib.REDUCE_SUM, arg=p))       # sum and mean have no arg
    invalid(fold(op=_lib.REDUCE_MEAN, arg=p))
    invalid(back(op=_lib.REDUCE_SUM, part=p))      # dT_part belongs to the softmax
    # E = NULL is what is named when everything else is there: the message lists E among the pointers
    with pytest.raises(_lib.PygimError) as e:
        fold(others=p)()
    assert "E" in str(e.value) and ctypes.sizeof(ctypes.c_void_p) == 8
