"""Gradients of the aggregation on the GPU: the group of A^T built on the device (pygim_group_create_transposed), the SDDMM of the
edge values (pygim_sddmm) and the autograd Function the three wrappers route ``mul`` through (pygim_amd/autograd.py)."""
import types

import numpy as np
import pytest
import torch

import oracle
from conftest import NP_DTYPES, coalesce, driver_features, random_csr
from pygim_amd import _lib, autograd, pim_ops, synth
from pygim_amd.backend_pim import grande as grande_mod
from pygim_amd.backend_pim import spmm as spmm_mod
from pygim_amd.backend_pim import spmv as spmv_mod
from pygim_amd.sparse_tensor import SparseTensorShim, _shim_matmul

pytestmark = pytest.mark.gpu

CODE = {"INT8": _lib.INT8, "INT16": _lib.INT16, "INT32": _lib.INT32, "INT64": _lib.INT64, "FLT32": _lib.FLT32, "DBL64": _lib.DBL64}


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def _ptr(a):
    return a.ctypes.data if a is not None else 0


def np_transpose(parts_csr, nrows):
    """A^T of row-major CSR column blocks side by side: np.argsort(global column, kind="stable") of the entries"""
    rows, cols, vals, col0 = [], [], [], 0
    for rowptr, col, val, ncols in parts_csr:
        rows.append(np.repeat(np.arange(nrows), np.diff(rowptr.astype(np.int64))))
        cols.append(col.astype(np.int64) + col0)
        vals.append(val)
        col0 += ncols
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(col, kind="stable")
    rp = np.zeros(col0 + 1, dtype=np.int32)
    np.cumsum(np.bincount(col, minlength=col0), out=rp[1:])
    val = None if vals[0] is None else np.concatenate(vals)[order]
    return rp, row[order].astype(np.int32), val


def make_matrix(rng, nrows, ncols, deg, hub=False):
    """duplicates (a multigraph), empty rows, the last fifth of the columns empty, optionally a hub column of >= 5000 entries"""
    rowptr, col = random_csr(rng, nrows, max(1, ncols * 4 // 5), deg, empty_frac=0.1)
    if hub:  # every row also hits column 3 (twice in every 7th row): a long row of A^T
        rows = np.repeat(np.arange(nrows), np.diff(rowptr.astype(np.int64)))
        extra = np.concatenate([np.arange(nrows), np.arange(0, nrows, 7)])
        rows = np.concatenate([rows, extra])
        col = np.concatenate([col, np.full(len(extra), 3, dtype=np.int32)])
        order = np.lexsort((col, rows))
        rows, col = rows[order], col[order].astype(np.int32)
        rowptr = np.zeros(nrows + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows, minlength=nrows), out=rowptr[1:])
    return rowptr.astype(np.int32), col


def split_cols(rowptr, col, val, nrows, ncols, sp_parts):
    """column blocks with local column ids (CSR per block)"""
    step = -(-ncols // sp_parts)
    rows = np.repeat(np.arange(nrows), np.diff(rowptr.astype(np.int64)))
    out = []
    for i in range(sp_parts):
        a, b = i * step, min(ncols, (i + 1) * step)
        keep = (col >= a) & (col < b)
        rp = np.zeros(nrows + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows[keep], minlength=nrows), out=rp[1:])
        out.append((rp, (col[keep] - a).astype(np.int32), None if val is None else val[keep], b - a))
    return out


def values_for(rng, dt, n):
    if dt in ("FLT32", "DBL64"):
        return rng.uniform(-2, 2, size=n).astype(NP_DTYPES[dt])
    v = np.ones(n, dtype=NP_DTYPES[dt])  # mostly unit weights: the pattern + correction split of the creation path
    v[rng.random(n) < 0.02] = 3
    return v


def transposed_product(fmt, parts, nrows, dt, h, G, device_inputs=False):
    npdt = NP_DTYPES[dt]
    idx0s, cols, vals, ncols = [], [], [], []
    for rp, c, v, nc in parts:
        if fmt == "CSR":
            idx0s.append(rp)
            cols.append(c)
            vals.append(v)
        else:
            r, cc, vv = np.repeat(np.arange(nrows), np.diff(rp.astype(np.int64))).astype(np.int32), c, v
            idx0s.append(r)
            cols.append(cc)
            vals.append(vv)
        ncols.append(nc)
    keep = []
    if device_inputs:
        to = lambda a: keep.append(torch.from_numpy(np.ascontiguousarray(a)).cuda()) or keep[-1].data_ptr()  # noqa: E731
    else:
        to = lambda a: keep.append(np.ascontiguousarray(a)) or _ptr(keep[-1])  # noqa: E731
    hd = _lib.group_create_transposed(_lib.COO if fmt == "COO" else _lib.CSR, CODE[dt], [to(a) for a in idx0s], [to(a) for a in cols],
                                      None if vals[0] is None else [to(v.astype(npdt)) for v in vals], [nrows] * len(parts), ncols,
                                      [len(c) for c in cols], [1] * len(parts), [h] * len(parts), h)
    try:
        info = _lib.group_info(hd)
        assert info["total_rows"] == sum(ncols) and info["total_cols"] == nrows and info["n_parts"] == 1 and info["h"] == h
        out = np.full((sum(ncols), h), 77, dtype=npdt)
        _lib.spmm_run_group(hd, [_ptr(G)], _ptr(out))
    finally:
        _lib.group_free(hd)
    return out


@pytest.mark.parametrize("dt", list(CODE))
@pytest.mark.parametrize("fmt", ["CSR", "COO"])
@pytest.mark.parametrize("sp_parts", [1, 3])
def test_transposed_group_parity(rng, dt, fmt, sp_parts):
    npdt = NP_DTYPES[dt]
    h = 20
    for nrows, ncols, deg, hub in ((6000, 6000, 6, True), (300, 250, 9, False), (220, 700, 5, True)):
        rowptr, col = make_matrix(rng, nrows, ncols, deg, hub)
        if fmt == "COO":  # COO input is coalesced (torch's coalesce()): no duplicates
            r, col, _ = coalesce(rowptr, col, npdt)
            rowptr = np.zeros(nrows + 1, dtype=np.int32)
            np.cumsum(np.bincount(r, minlength=nrows), out=rowptr[1:])
        val = values_for(rng, dt, len(col))
        parts = split_cols(rowptr, col, val, nrows, ncols, sp_parts)
        rpT, colT, valT = np_transpose([(p[0], p[1], p[2], p[3]) for p in parts], nrows)
        if hub:
            assert np.diff(rpT.astype(np.int64)).max() >= 5000 or nrows < 5000
        G = driver_features(rng, nrows, h, npdt)
        ref = oracle.spmm_csr(rpT, colT, valT, G)
        got = transposed_product(fmt, parts, nrows, dt, h, G, device_inputs=(sp_parts == 3))
        # small-integer features (and, for the floats, weights summed exactly): every type bit for bit
        if dt not in ("FLT32", "DBL64"):
            assert np.array_equal(got, ref), (dt, fmt, sp_parts, nrows, ncols)
        if dt in ("FLT32", "DBL64"):
            Gf = rng.uniform(-1, 1, size=(nrows, h)).astype(npdt)
            ref = oracle.spmm_csr(rpT, colT, valT, Gf)
            scale = oracle.spmm_csr(rpT, colT, None if valT is None else np.abs(valT).astype(np.float64), np.abs(Gf).astype(np.float64))
            got = transposed_product(fmt, parts, nrows, dt, h, Gf)
            tol = 1e-5 if dt == "FLT32" else 1e-12
            assert np.all(np.abs(got.astype(np.float64) - ref) <= tol * scale + 1e-30)
            if dt == "FLT32" and not hub:
                old = _lib.set_tunable("lds_col_split_f32", 0)
                try:
                    got = transposed_product(fmt, parts, nrows, dt, h, Gf)
                finally:
                    _lib.set_tunable("lds_col_split_f32", old)
                assert got.tobytes() == ref.tobytes()


def test_transposed_group_rejects_what_create_rejects(rng):
    rowptr, col = random_csr(rng, 50, 40, 4)
    bad = col.copy()
    bad[0] = 40
    with pytest.raises(_lib.PygimError) as e:
        _lib.group_create_transposed(_lib.CSR, _lib.INT32, [_ptr(rowptr)], [_ptr(bad)], None, [50], [40], [len(col)], [1], [8], 8)
    assert e.value.code == _lib.ERR_INVALID
    r = np.repeat(np.arange(50), np.diff(rowptr)).astype(np.int32)[::-1].copy()
    with pytest.raises(_lib.PygimError) as e:
        _lib.group_create_transposed(_lib.COO, _lib.INT32, [_ptr(r)], [_ptr(col)], None, [50], [40], [len(col)], [1], [8], 8)
    assert e.value.code == _lib.ERR_UNSORTED


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------
def adj_of(rng, n, m, deg, value=None):
    rowptr, col = random_csr(rng, n, m, deg, long_rows=((2, 3000),) if n > 2 else ())
    val = None if value is None else torch.from_numpy(rng.uniform(0.5, 2.0, size=len(col))).to(value)
    return SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), value=val, sparse_sizes=(n, m))


def exact_t(adj, g):
    """A^T . G in float64 on the CPU (small integers: exact)"""
    rowptr, col, val = adj.csr()
    row = torch.repeat_interleave(torch.arange(adj.size(0)), torch.diff(rowptr))
    w = torch.ones(col.numel(), dtype=torch.float64) if val is None else val.double()
    return torch.zeros(adj.size(1), g.size(1), dtype=torch.float64).index_add_(0, col, g.double().cpu()[row] * w[:, None])


def wrappers(rng, dtype):
    """(name, A, x shape) for the three wrappers on one graph"""
    n, h = 3100, 24
    adj = adj_of(rng, n, n, 7)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(2)
    yield "spmm", adj, spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=dtype, sp_format="CSR", sp_parts=2, ds_parts=2, hidden_size=h)), h
    yield "spmm-coo", adj, spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=dtype, sp_format="COO", sp_parts=1, ds_parts=1, hidden_size=h)), h
    pim_ops.load("grande")
    dpus = torch.ops.pim_ops.dpu_init_ranks(2)
    yield "grande", adj, grande_mod.prepare_pim_spmm_grande(adj, types.SimpleNamespace(data_type=dtype, sp_format="CSR", sp_parts=2, hidden_size=h), dpus), h
    pim_ops.load("spmv")
    torch.ops.pim_ops.dpu_init_ranks(1)
    yield "spmv", adj, spmv_mod.prepare_pim_spmv(adj, types.SimpleNamespace(data_type=dtype, sp_format="COO", sp_parts=1, ds_parts=4, hidden_size=4)), h
    pim_ops.load("spmm")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_x_grad_is_the_transposed_product(rng, dtype):
    for name, adj, A, h in wrappers(rng, dtype):
        for dev in ("cpu", "cuda"):
            x = synth.features(adj.size(1), h, dtype, seed=1).to(dev).requires_grad_()
            g = synth.features(adj.size(0), h, dtype, seed=2).to(dev)
            A.mul(x).backward(g)
            assert x.grad is not None, (name, dev)
            assert x.grad.shape == x.shape and x.grad.device == x.device and x.grad.dtype == dtype
            assert torch.equal(x.grad.cpu().double(), exact_t(adj, g)), (name, dev)


def test_value_grad_and_gradcheck(rng):
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    for dtype, tol in ((torch.float32, 1e-5), (torch.float64, 1e-12)):
        adj = adj_of(rng, 900, 700, 12, value=dtype)
        v = adj.storage.value().requires_grad_()
        A = spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=dtype, sp_format="CSR", sp_parts=1, ds_parts=1, hidden_size=33))
        x = torch.randn(700, 33, dtype=dtype, device="cuda")
        g = torch.randn(900, 33, dtype=dtype, device="cuda")
        A.mul(x).backward(g)
        rowptr, col, _ = adj.csr()
        row = np.repeat(np.arange(900), np.diff(rowptr.numpy()))
        gh, xh = g.double().cpu().numpy(), x.double().cpu().numpy()
        ref = np.array([float(np.dot(gh[r], xh[c])) for r, c in zip(row, col.numpy())])
        scale = np.abs(gh[row] * xh[col.numpy()]).sum(1)
        assert np.all(np.abs(v.grad.double().numpy() - ref) <= tol * scale + 1e-300)
    # small DBL64 graphs end to end (both operands, CPU and device)
    rowptr, col = random_csr(rng, 15, 11, 3)
    for dev in ("cpu", "cuda"):
        def f(v, x):
            adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), value=v, sparse_sizes=(15, 11))
            A = spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=torch.float64, sp_format="CSR", sp_parts=2, ds_parts=1, hidden_size=3))
            return A.mul(x)

        v0 = torch.rand(len(col), dtype=torch.float64, requires_grad=True)
        x0 = torch.randn(11, 3, dtype=torch.float64, device=dev, requires_grad=True)
        assert torch.autograd.gradcheck(f, (v0, x0))


@pytest.mark.parametrize("h", [1, 3, 7, 16, 64, 100, 256, 300, 1100])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sddmm_widths_and_hubs(rng, h, dtype):
    rowptr, col = random_csr(rng, 400, 500, 9, empty_frac=0.2, long_rows=[(5, 6000), (399, 70)])
    G = torch.randn(400, h, dtype=dtype, device="cuda")
    X = torch.randn(500, h, dtype=dtype, device="cuda")
    a = autograd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(col), G, X)
    b = autograd.sddmm(torch.from_numpy(rowptr), torch.from_numpy(col), G, X)
    assert torch.equal(a, b)  # deterministic
    row = torch.from_numpy(np.repeat(np.arange(400), np.diff(rowptr))).cuda()
    c = torch.from_numpy(col).long().cuda()
    ref = (G.double()[row] * X.double()[c]).sum(1)
    scale = (G.double()[row] * X.double()[c]).abs().sum(1)
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    assert torch.all((a.double() - ref).abs() <= tol * scale)
    # strided rows (ldg / ldx > h) and an unaligned start take the element-per-lane form
    Gw = torch.randn(400, h + 3, dtype=dtype, device="cuda")
    Xw = torch.randn(501, h + 1, dtype=dtype, device="cuda")
    out = torch.empty(len(col), dtype=dtype, device="cuda")
    rp, cc = torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()
    _lib.sddmm(pim_ops.DTYPE_CODE[dtype], 400, rp.data_ptr(), cc.data_ptr(), len(col), Gw.data_ptr(), h + 3, Xw[1:].data_ptr(), h + 1, h,
               out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ref = (Gw.double()[row, :h] * Xw[1:].double()[c, :h]).sum(1)
    scale = (Gw.double()[row, :h] * Xw[1:].double()[c, :h]).abs().sum(1)
    assert torch.all((out.double() - ref).abs() <= tol * scale)
    with pytest.raises(_lib.PygimError):
        _lib.sddmm(_lib.INT32, 400, rp.data_ptr(), cc.data_ptr(), len(col), Gw.data_ptr(), h, Xw.data_ptr(), h, h, out.data_ptr())


def test_forward_unchanged_and_lazy_transposed_group(rng):
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    adj = adj_of(rng, 2000, 2000, 30, value=torch.float32)
    A = spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=torch.float32, sp_format="CSR", sp_parts=1, ds_parts=1, hidden_size=64))
    x = torch.randn(2000, 64, device="cuda")
    plain = A.mul(x)
    serial_before = _lib.group_serial(A.sp_info_ptr)
    xg = x.clone().requires_grad_()
    adj.storage.value().requires_grad_()
    out = A.mul(xg)
    assert out.grad_fn is not None and A._handle_t is None
    assert out.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    out.sum().backward()
    assert A._handle_t is not None and A._handle_t[1] > serial_before


def test_lifetimes_of_the_transposed_group(rng):
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    adj = adj_of(rng, 500, 400, 6)
    args = types.SimpleNamespace(data_type=torch.float32, sp_format="CSR", sp_parts=2, ds_parts=1, hidden_size=8)
    g = torch.randn(500, 8, device="cuda")

    def alive(held):
        try:
            return _lib.group_serial(held[0]) == held[1]
        except _lib.PygimError:
            return False

    A = spmm_mod.prepare_pim_spmm(adj, args)
    A.prepare_backward()
    held = A._handle_t
    assert alive(held)
    A.to_pim_group(8, 1)          # a new forward group: the old A^T group goes
    assert not alive(held) and A._handle_t is None
    A.mul_t(g)
    held = A._handle_t
    A.free_group()
    assert not alive(held) and A._handle_t is None
    A.to_pim_group(8, 1)
    A.mul_t(g)
    held, fwd = A._handle_t, A._handle
    torch.ops.pim_ops.dpu_release()  # every group freed by the library
    torch.ops.pim_ops.dpu_init_ranks(1)
    B = spmm_mod.prepare_pim_spmm(adj, args)  # may reuse the addresses: A must not free B's groups
    B.prepare_backward()
    A.free_group()
    assert alive((B.sp_info_ptr, _lib.group_serial(B.sp_info_ptr))) and alive(B._handle_t)
    held = B._handle_t
    del B                          # object death frees both
    import gc

    gc.collect()
    assert not alive(held)
    del A


def test_full_size_reddit_f32_h256():
    dev = torch.device("cuda", 0)
    n, nnz, d_max = synth.SHAPES["reddit"]
    h = 256
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    adj = SparseTensorShim(rowptr=rowptr.long(), col=col.long(), sparse_sizes=(n, n))
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    A = spmm_mod.SparseTensorCOO(adj, dtype=torch.float32, format="CSR")
    A.to_pim_group(h, 1)
    x = synth.features(n, h, torch.float32, seed=0, device=dev).requires_grad_()
    g = synth.features(n, h, torch.float32, seed=1, device=dev)
    A.mul(x).backward(g)
    # the exact A^T . G (small integers: every sum exact in float64 and in float32), all 59.6 M outputs, in blocks of entries
    row = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), torch.diff(rowptr.long()))
    ref = torch.zeros(n, h, dtype=torch.float64, device=dev)
    step = 1 << 21
    for s in range(0, nnz, step):
        ref.index_add_(0, col[s:s + step].long(), g[row[s:s + step].long()].double())
    assert torch.equal(x.grad.double(), ref)
    del ref
    # sddmm on the same graph, real-valued operands, a seeded sample of 1 M entries against float64
    G = synth.features(n, h, torch.float32, seed=2, device=dev, kind="uniform")
    X = synth.features(n, h, torch.float32, seed=3, device=dev, kind="uniform")
    out = autograd.sddmm(rowptr, col, G, X)
    pick = torch.from_numpy(np.random.default_rng(7).integers(0, nnz, size=1 << 20)).to(dev)
    prod = G.double()[row[pick].long()] * X.double()[col[pick].long()]
    assert torch.all((out[pick].double() - prod.sum(1)).abs() <= 1e-5 * prod.abs().sum(1))
    A.free_group()


def test_sgd_steps_match_the_cpu_path(rng):
    """a 2-layer stack on adj.mul (not quantised), a few SGD steps: losses and parameter gradients as on the --version cpu path"""
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    n, f_in, f_hid, f_out = 1500, 16, 32, 8
    adj = adj_of(rng, n, n, 9, value=torch.float64)
    A = spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=torch.float64, sp_format="CSR", sp_parts=1, ds_parts=1, hidden_size=f_hid))
    A2 = spmm_mod.prepare_pim_spmm(adj, types.SimpleNamespace(data_type=torch.float64, sp_format="CSR", sp_parts=1, ds_parts=1, hidden_size=f_out))
    feats = torch.randn(n, f_in, dtype=torch.float64)
    target = torch.randn(n, f_out, dtype=torch.float64)
    torch.manual_seed(0)
    w0 = [torch.randn(f_in, f_hid, dtype=torch.float64) * 0.2, torch.randn(f_hid, f_out, dtype=torch.float64) * 0.2]

    def run(agg1, agg2, dev):
        ws = [w.clone().to(dev).requires_grad_() for w in w0]
        opt = torch.optim.SGD(ws, lr=0.05)
        losses, grads = [], []
        for _ in range(4):
            opt.zero_grad()
            hdn = torch.relu(agg1(feats.to(dev) @ ws[0]))
            out = agg2(hdn @ ws[1])
            loss = ((out - target.to(dev)) ** 2).mean()
            loss.backward()
            losses.append(loss.item())
            grads.append([w.grad.cpu().clone() for w in ws])
            opt.step()
        return losses, grads

    fixed = SparseTensorShim(rowptr=adj.storage.rowptr(), col=adj.storage.col(), value=adj.storage.value(), sparse_sizes=(n, n))
    l_gpu, g_gpu = run(A.mul, A2.mul, "cuda")
    l_cpu, g_cpu = run(lambda t: _shim_matmul(fixed, t), lambda t: _shim_matmul(fixed, t), "cpu")
    assert np.allclose(l_gpu, l_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_gpu, g_cpu):
        for x, y in zip(a, b):
            assert torch.allclose(x, y, rtol=1e-9, atol=1e-11)
