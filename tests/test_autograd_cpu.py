"""Gradients of ``SparseTensorCOO.mul`` on CPU: the three wrappers driven through pygim_amd.autograd with the C-ABI test
double of tests/fake_abi.py, extended here with numpy statements of pygim_group_create_transposed and pygim_sddmm."""
import types

import numpy as np
import pytest
import torch

from conftest import random_csr
from fake_abi import CSR, NP_OF, FakeLib, PygimError, _view
from pygim_amd import autograd, pim_ops
from pygim_amd.backend_pim import grande as grande_mod
from pygim_amd.backend_pim import spmm as spmm_mod
from pygim_amd.backend_pim import spmv as spmv_mod
from pygim_amd.sparse_tensor import SparseTensorShim, _shim_matmul


def np_transpose(fmt, parts):
    """A^T of the column blocks side by side, as CSR: entries of each global column in their order in A (a stable sort)"""
    rows, cols, vals, col0 = [], [], [], 0
    for p in parts:
        if fmt == CSR:
            r = np.repeat(np.arange(p["nrows"]), np.diff(p["idx0"].astype(np.int64)))
        else:
            r = p["idx0"].astype(np.int64)
        rows.append(r)
        cols.append(p["col"].astype(np.int64) + col0)
        vals.append(p["val"])
        col0 += p["ncols"]
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(col, kind="stable")
    rowptr = np.zeros(col0 + 1, dtype=np.int32)
    np.cumsum(np.bincount(col, minlength=col0), out=rowptr[1:])
    val = None if all(v is None for v in vals) else np.concatenate(vals)[order]
    return rowptr, row[order].astype(np.int32), val, col0


class FakeLibT(FakeLib):
    """the fake ABI with the two entry points of the backward"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def group_serial(self, handle):
        if int(handle) not in self.groups:
            raise PygimError(1, "unknown group handle")
        return int(handle)

    def group_create_transposed(self, fmt, dtype, idx0, cols, vals, nrows, ncols, nnz, n_dense, dense_cols, h):
        self.calls.append("transposed")
        npdt = NP_OF[dtype]
        parts = []
        for i in range(len(cols)):
            n0 = nrows[i] + 1 if fmt == CSR else nnz[i]
            parts.append(dict(idx0=_view(idx0[i], n0, np.int32).copy(), col=_view(cols[i], nnz[i], np.int32).copy(),
                              val=None if vals is None else _view(vals[i], nnz[i], npdt).copy(), nrows=int(nrows[i]),
                              ncols=int(ncols[i])))
        rowptr, colT, valT, ncolsT = np_transpose(fmt, parts)
        self.next += 1
        self.groups[self.next] = dict(fmt=CSR, dt=npdt, parts=[dict(idx0=rowptr, col=colT, val=valT, nrows=ncolsT, ncols=int(nrows[0]))],
                                      n_dense=[1], dense_cols=[int(h)], h=int(h))
        return self.next

    def spmm_run_group(self, handle, b_ptrs, out_ptr, stream=0, x_unchanged=False):
        self.calls.append("run")
        super().spmm_run_group(handle, b_ptrs, out_ptr, stream, x_unchanged)

    def sddmm(self, dtype, nrows, rowptr_ptr, col_ptr, nnz, g_ptr, ldg, x_ptr, ldx, h, out_ptr, stream=0):
        self.calls.append("sddmm")
        npdt = NP_OF[dtype]
        rowptr = _view(rowptr_ptr, nrows + 1, np.int32).astype(np.int64)
        col = _view(col_ptr, nnz, np.int32).astype(np.int64)
        G = _view(g_ptr, nrows * ldg, npdt).reshape(nrows, ldg)[:, :h]
        X = _view(x_ptr, (int(col.max()) + 1) * ldx, npdt).reshape(-1, ldx)[:, :h]
        row = np.repeat(np.arange(nrows), np.diff(rowptr))
        _view(out_ptr, nnz, npdt)[:] = np.einsum("ef,ef->e", G[row].astype(np.float64), X[col].astype(np.float64)).astype(npdt)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLibT()
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


def make_adj(rng, n=40, m=None, deg=4, value=None):
    m = m or n
    rowptr, col = random_csr(rng, n, m, deg, long_rows=((3, 3 * deg),))
    val = None if value is None else torch.from_numpy(rng.uniform(0.5, 2.0, size=len(col))).to(value)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), value=val, sparse_sizes=(n, m))
    return adj


def spmm_A(adj, dtype, fmt="CSR", sp_parts=1, ds_parts=1, h=6):
    torch.ops.pim_ops.dpu_init_ranks(sp_parts * ds_parts)
    return spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=dtype, sp_format=fmt, sp_parts=sp_parts, ds_parts=ds_parts,
                                                                hidden_size=h))


def test_routing_without_grad_is_todays_single_call(rng, fake):
    pim_ops.load("spmm")
    adj = make_adj(rng)
    for dtype in (torch.float32, torch.int32):
        A = spmm_A(adj, dtype)
        x = torch.ones(40, 6, dtype=dtype, requires_grad=dtype.is_floating_point)
        fake.calls.clear()
        with torch.no_grad():
            out = A.mul(x)
        assert fake.calls == ["run"] and out.grad_fn is None
    # integer groups never take the Function, and plain float inputs without requires_grad neither
    A = spmm_A(adj, torch.float64)
    fake.calls.clear()
    out = A.mul(torch.ones(40, 6, dtype=torch.float64))
    assert fake.calls == ["run"] and out.grad_fn is None and A._handle_t is None


def test_forward_under_grad_is_the_same_product(rng, fake):
    pim_ops.load("spmm")
    adj = make_adj(rng)
    A = spmm_A(adj, torch.float64, h=5)
    x = torch.randn(40, 5, dtype=torch.float64)
    plain = A.mul(x)
    fake.calls.clear()
    xg = x.clone().requires_grad_()
    out = A.mul(xg)
    assert fake.calls == ["run"] and A._handle_t is None, "the forward built a transposed group or launched extra work"
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    out.backward(torch.ones_like(out))
    assert fake.calls == ["run", "transposed", "run"] and A._handle_t is not None


@pytest.mark.parametrize("fmt,sp_parts,ds_parts", [("CSR", 1, 1), ("CSR", 3, 2), ("COO", 1, 2), ("COO", 3, 1)])
def test_gradcheck_spmm(rng, fake, fmt, sp_parts, ds_parts):
    pim_ops.load("spmm")
    adj = make_adj(rng, n=30, m=23, value=torch.float64)
    A = spmm_A(adj, torch.float64, fmt, sp_parts, ds_parts, h=4)
    x = torch.randn(23, 4, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(A.mul, (x,))


def test_gradcheck_spmm_values(rng, fake):
    pim_ops.load("spmm")
    base = make_adj(rng, n=20, m=17, value=torch.float64)
    rowptr, col, v0 = base.csr()
    x = torch.randn(17, 3, dtype=torch.float64, requires_grad=True)

    def f(v, x):
        adj = SparseTensorShim(rowptr=rowptr, col=col, value=v, sparse_sizes=(20, 17))
        return spmm_A(adj, torch.float64, "CSR", 2, 1, h=3).mul(x)

    assert torch.autograd.gradcheck(f, (v0.clone().requires_grad_(), x))


def test_gradcheck_grande(rng, fake):
    pim_ops.load("grande")
    adj = make_adj(rng, n=26)
    dpus = torch.ops.pim_ops.dpu_init_ranks(2)
    A = grande_mod.prepare_pim_spmm_grande(adj, types.SimpleNamespace(data_type=torch.float64, sp_format="CSR", sp_parts=2, hidden_size=11), dpus)
    x = torch.randn(26, 11, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(A.mul, (x,))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gradcheck_spmv(rng, fake, dtype):
    pim_ops.load("spmv")
    adj = make_adj(rng, n=29)  # float32: padded to 30 rows and columns
    torch.ops.pim_ops.dpu_init_ranks(2)
    A = spmv_mod.prepare_pim_spmv(adj, types.SimpleNamespace(data_type=dtype, sp_format="COO", sp_parts=1, ds_parts=2, hidden_size=4))
    x = torch.randn(29, 4, dtype=dtype, requires_grad=True)
    if dtype == torch.float64:
        assert torch.autograd.gradcheck(A.mul, (x,))
    g = torch.randn(29, 4, dtype=dtype)
    A.mul(x).backward(g)
    want = adj.to_dense(torch.float64).t() @ g.double()
    assert x.grad.shape == (29, 4) and torch.allclose(x.grad.double(), want, atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gradients_match_cpu_path(rng, fake, dtype):
    pim_ops.load("spmm")
    adj = make_adj(rng, n=35, m=28, value=dtype)
    adj.storage.value().requires_grad_()
    A = spmm_A(adj, dtype, "CSR", 2, 1, h=5)
    x = torch.randn(28, 5, dtype=dtype, requires_grad=True)
    g = torch.randn(35, 5, dtype=dtype)
    A.mul(x).backward(g)
    gx, gv = x.grad.clone(), adj.storage.value().grad.clone()
    x.grad = None
    # dX: the --version cpu path (_shim_matmul, the values held fixed); dvalue: the same product written densely with autograd
    # (torch's sparse CSR backward does not take a value gradient of a matrix with duplicate entries)
    fixed = SparseTensorShim(rowptr=adj.storage.rowptr(), col=adj.storage.col(), value=adj.storage.value().detach(), sparse_sizes=(35, 28))
    _shim_matmul(fixed, x).backward(g)
    v = adj.storage.value().detach().clone().requires_grad_()
    dense = torch.zeros(35, 28, dtype=dtype).index_put((adj.storage.row(), adj.storage.col()), v, accumulate=True)
    (dense @ x.detach()).backward(g)
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-12, atol=1e-12)
    assert torch.allclose(gx, x.grad, **tol) and torch.allclose(gv, v.grad, **tol)


def test_mul_t_and_lifetimes(rng, fake):
    pim_ops.load("spmm")
    adj = make_adj(rng, n=30, m=21)
    A = spmm_A(adj, torch.int32, "COO", 3, 1, h=4)
    g = torch.randint(-3, 4, (30, 4), dtype=torch.int32)
    got = A.mul_t(g)
    assert torch.equal(got, (adj.to_dense(torch.float64).t() @ g.double()).to(torch.int32))
    A.prepare_backward()
    held = A._handle_t
    assert held is not None and held[0] in fake.groups
    A.to_pim_group(4, 1)   # a new forward group: the transposed one goes
    assert held[0] not in fake.groups and A._handle_t is None
    A.mul_t(g)
    held = A._handle_t
    A.free_group()
    assert held[0] not in fake.groups and A._handle_t is None


def test_sddmm_public_function(rng, fake):
    rowptr, col = random_csr(rng, 12, 9, 3)
    G = torch.randn(12, 5, dtype=torch.float64)
    X = torch.randn(9, 5, dtype=torch.float64)
    import pygim_amd

    got = pygim_amd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(col), G, X)
    row = np.repeat(np.arange(12), np.diff(rowptr))
    want = (G.numpy()[row] * X.numpy()[col]).sum(1)
    assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    with pytest.raises(TypeError):
        autograd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(col), G.int(), X.int())
    bad = col.copy()
    if len(bad):
        bad[0] = 9
        with pytest.raises(ValueError):
            autograd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(bad), G, X)
