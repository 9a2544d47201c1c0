"""16-bit features (bfloat16, float16) of the gather family on the GPU: pygim_spmm_values, pygim_spmm_reduce (mean), pygim_gat_aggregate and
pygim_sddmm with PYGIM_BF16 / PYGIM_FLT16 through the C ABI, and the wrappers, their gradients and the layers on top of them.

Storage is 16 bits, arithmetic is float32, a finished row is rounded once.  Two kinds of checks follow from that:
  * sums that are exact in float32 in any order (integer features, values in {0.5, 1, 2}) must come out bit for bit as the float64 sum
    rounded to the type -- a partial result held in 16 bits anywhere (a slot, a lane-group exchange) breaks it;
  * random data meets  |got - want| <= u |want| + TOL32 * sum |w . x| + 2^-24  with u = 2^-8 (bfloat16) / 2^-11 (float16), the half-ulp of
    the one final rounding, TOL32 the FLT32 contract of the call (1e-5; 2e-5 for gat_aggregate) and 2^-24 for results that fall below
    the type's normal range.
The graph is small but reaches every branch of the walker: a row over six 512-entry runs, one that starts in the middle of a run,
short rows that share a run, empty rows (the last one among them), duplicates."""
import numpy as np
import pytest
import torch

from pygim_amd import _lib, autograd, gnn
from pygim_amd.attention import EdgeGraph, gat_aggregate, spmm_values
from pygim_amd.reduce import spmm_reduce
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_cpu import ref_spmm
from test_attention_gpu import dev_csr, spmm_reference
from test_gat_fused_cpu import ref_gat_aggregate
from test_gat_fused_gpu import gat_reference_dev

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = [torch.bfloat16, torch.float16]
CODE = {torch.bfloat16: _lib.BF16, torch.float16: _lib.FLT16}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = 2.0 ** -24
# (h, heads): one piece; several; L = 32 (two entries per wave instruction), also with 4 heads; 64 pieces, the whole wave; 65 pieces, two per
# lane with a partly filled last piece; gridDim.y = 2; the scalar path (100, 7, and 8 heads of 4 features)
WIDTHS = [(8, 1), (64, 1), (256, 1), (256, 4), (512, 1), (520, 1), (1040, 1), (100, 1), (7, 1), (32, 8)]
N, M = 300, 257


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def csr_of(deg, seed):
    r = np.random.default_rng(seed)
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = r.integers(0, M, size=int(rowptr[-1]))
    for i in range(len(deg)):
        col[rowptr[i]:rowptr[i + 1]].sort()
    return rowptr.astype(np.int32), col.astype(np.int32)


def main_graph():
    r = np.random.default_rng(7)
    deg = r.integers(1, 13, size=N)
    deg[r.random(N) < 0.1] = 0
    deg[0], deg[5], deg[20], deg[150], deg[N - 1] = 3, 3000, 4, 1100, 0
    rowptr, col = csr_of(deg, 8)
    col[rowptr[20] + 1] = col[rowptr[20]]   # a certain duplicate (the long rows have many)
    assert rowptr[5] // 512 == 0 and (rowptr[6] - 1) // 512 == 5, "the long row spans six runs"
    assert rowptr[150] % 512 != 0 and rowptr[150] // 512 != (rowptr[151] - 1) // 512, "the second long row starts inside a run and leaves it"
    return rowptr, col


def empty_graph():
    return np.zeros(N + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)


def single_run_graph():
    r = np.random.default_rng(9)
    deg = r.integers(0, 4, size=N)
    deg[N - 1] = 0
    rowptr, col = csr_of(deg, 10)
    assert 0 < len(col) < 512
    return rowptr, col


def boundary_graph():
    """a row ends exactly on entry 511, another on 1023 = nnz - 1: no row is cut, nnz is a multiple of 512"""
    deg = np.zeros(N, dtype=np.int64)
    deg[:100] = 5
    deg[100] = 12          # 512 entries in rows 0 .. 100
    deg[101:201] = 5
    deg[250] = 12          # 1024 in all
    rowptr, col = csr_of(deg, 11)
    assert len(col) == 1024 and 512 in rowptr
    return rowptr, col


GRAPHS = {"main": main_graph, "nnz0": empty_graph, "one-run": single_run_graph, "boundary": boundary_graph}
_cache = {}


def graph(name):
    """(rowptr, col) on the host, (rowptr, col) on the device; built once"""
    if name not in _cache:
        rowptr, col = GRAPHS[name]()
        _cache[name] = (rowptr, col) + tuple(dev_csr(rowptr, col))
    return _cache[name]


def strides(h):
    """contiguous, a wider stride that keeps 16-byte rows, and one that breaks them"""
    return (h, h + 8, h + 1)


def features(rng, ld, dtype, kind):
    if kind == "int":
        return torch.from_numpy(rng.integers(-8, 9, size=(M, ld)).astype(np.float32)).to(DEV, dtype)
    if kind == "away":   # magnitudes in [0.5, 2), random signs: a result near zero is a cancellation of large terms
        x = rng.uniform(0.5, 2.0, size=(M, ld)) * rng.choice([-1.0, 1.0], size=(M, ld))
        return torch.from_numpy(x.astype(np.float32)).to(DEV, dtype)
    x = torch.from_numpy(rng.standard_normal((M, ld)).astype(np.float32)).to(DEV, dtype)
    return x.abs() if kind == "abs" else x


def call_values(dtype, rp, cc, val, heads, X, h, op=None, out=None):
    """pygim_spmm_values (op None) or pygim_spmm_reduce MEAN on 16-bit X [M, ldx]; val float32 (None: unit weights, mean only); out:
    [N, ldo], NaN-filled before the call"""
    nnz = cc.numel()
    if out is None:
        out = torch.full((N, h), float("nan"), dtype=dtype, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    if op is None:
        ws = torch.empty(max(_lib.spmm_values_workspace(CODE[dtype], N, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
        _lib.spmm_values(CODE[dtype], N, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), heads, X.data_ptr(), X.stride(0), h, out.data_ptr(), out.stride(0),
                         ws.data_ptr(), ws.numel(), stream)
    else:
        ws = torch.empty(max(_lib.spmm_reduce_workspace(CODE[dtype], op, N, nnz, h), 16), dtype=torch.uint8, device=DEV)
        _lib.spmm_reduce(CODE[dtype], op, N, rp.data_ptr(), cc.data_ptr(), nnz, 0 if val is None else val.data_ptr(), X.data_ptr(), X.stride(0), h,
                         out.data_ptr(), out.stride(0), 0, ws.data_ptr(), ws.numel(), stream)
    torch.cuda.synchronize()
    return out


def test_workspace_sizes_are_the_float32_ones():
    for code in CODE.values():
        assert _lib.spmm_values_workspace(code, N, 5000, 256, 4) == _lib.spmm_values_workspace(_lib.FLT32, N, 5000, 256, 4)
        assert _lib.gat_aggregate_workspace(code, N, 5000, 256, 4) == _lib.gat_aggregate_workspace(_lib.FLT32, N, 5000, 256, 4)
        assert _lib.spmm_reduce_workspace(code, _lib.REDUCE_MEAN, N, 5000, 256) == _lib.spmm_reduce_workspace(_lib.FLT32, _lib.REDUCE_MEAN, N, 5000, 256)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("h,heads", WIDTHS)
def test_exact_sums_bit_for_bit(rng, dtype, h, heads):
    """integer features in [-8, 8], values in {0.5, 1, 2}: |partial sum| <= 48 000 < 2^24 and a multiple of 0.5, so float32 accumulation is
    exact in any order and the result is the float64 sum rounded once"""
    for name in GRAPHS:
        rowptr, col, rp, cc = graph(name)
        val = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=(len(col), heads)).astype(np.float32)).to(DEV)
        for ld in strides(h) if name == "main" else (h,):
            X = features(rng, ld, dtype, "int")
            out = call_values(dtype, rp, cc, val, heads, X, h)
            ref, _ = spmm_reference(N, rowptr, col, val, heads, X, h)
            assert torch.equal(out, ref.to(dtype)), f"{name} h={h} heads={heads} ldx={ld}"
            assert (out[torch.from_numpy(np.diff(rowptr) == 0).to(DEV)] == 0).all()
    # the wrapper, with the values in X's dtype (0.5, 1 and 2 are exact there): the same bits, in X's dtype, and twice
    rowptr, col, rp, cc = graph("main")
    g = EdgeGraph(rp, cc, (N, M))
    X = features(rng, h, dtype, "int")
    val = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=(len(col), heads)).astype(np.float32)).to(DEV)
    got = spmm_values(g, val.to(dtype), X, heads=heads)
    assert got.dtype == dtype and torch.equal(got, call_values(dtype, rp, cc, val, heads, X, h)) and torch.equal(got, spmm_values(g, val, X, heads=heads))


def within(got, want, mag, u, tol32, tag):
    err = (got.double() - want).abs()
    bound = u * want.abs() + tol32 * mag + TINY
    print(f"{tag}: max err / bound = {(err / bound).max().item():.3f}")
    return bool(torch.all(err <= bound))


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("h,heads", WIDTHS)
def test_random_sums_and_means_meet_the_bound(rng, dtype, h, heads):
    """X ~ N(0, 1) rounded to the type (and |X|: same-sign products in the long rows), values in (0.5, 1); the mean with and without values"""
    rp, cc, val = check_random_sums_and_means(rng, dtype, h, heads)
    if heads == 1:   # the wrapper: the bits of the C ABI
        X = features(rng, h, dtype, "normal")
        g = EdgeGraph(rp, cc, (N, M))
        assert torch.equal(spmm_reduce(g, X, "mean", value=val[:, 0]), call_values(dtype, rp, cc, val, 1, X, h, op=_lib.REDUCE_MEAN))


def check_random_sums_and_means(rng, dtype, h, heads):
    rowptr, col, rp, cc = graph("main")
    cnt = torch.from_numpy(np.maximum(np.diff(rowptr), 1)).to(DEV).double().unsqueeze(1)
    val = torch.from_numpy(rng.uniform(0.5, 1.0, size=(len(col), heads)).astype(np.float32)).to(DEV)
    for kind in ("normal", "abs"):
        for ld in strides(h) if kind == "normal" else (h,):
            X = features(rng, ld, dtype, kind)
            out = call_values(dtype, rp, cc, val, heads, X, h)
            ref, mag = spmm_reference(N, rowptr, col, val, heads, X, h)
            assert within(out, ref, mag, U[dtype], 1e-5, f"spmm_values {dtype} {kind} h={h} heads={heads} ldx={ld}")
            assert torch.equal(out, call_values(dtype, rp, cc, val, heads, X, h)), "two launches differ"
            if heads == 1:
                for v in (val, None):
                    mean = call_values(dtype, rp, cc, v, 1, X, h, op=_lib.REDUCE_MEAN)
                    r1, m1 = (ref, mag) if v is not None else spmm_reference(N, rowptr, col, torch.ones_like(val), 1, X, h)
                    assert within(mean, r1 / cnt, m1 / cnt, U[dtype], 1e-5, f"mean {dtype} {kind} h={h} ldx={ld} values={v is not None}")
    return rp, cc, val


def call_gat(dtype, rp, cc, a_dst, a_src, heads, slope, X, h, want_lse=True, out=None):
    nnz = cc.numel()
    ws = torch.empty(max(_lib.gat_aggregate_workspace(CODE[dtype], N, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((N, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((N, heads), float("nan"), dtype=torch.float32, device=DEV) if want_lse else None
    _lib.gat_aggregate(CODE[dtype], N, rp.data_ptr(), cc.data_ptr(), nnz, a_dst.data_ptr(), a_src.data_ptr(), heads, slope, X.data_ptr(), X.stride(0), h,
                       out.data_ptr(), out.stride(0), lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("h,heads", WIDTHS)
def test_gat_aggregate_meets_the_bound(rng, dtype, h, heads):
    """float32 node terms in (-4, 4), and multiples of 1/8 in [-40, 40] with slope 0.25 (scores of magnitude 80, exact in float32: the online
    rescale at work, only exp and the sums round); out within u |want| + 2e-5 sum p |x|, lse (float32) within 2e-5 (1 + |lse|).
    The bound has no absolute term, and float16 has no relative precision u below 2^-14.  With the large scores a row's softmax is
    close to one-hot, so a result can be as small as a single x: there |x| lies in [0.5, 2) with random signs -- a result below 2^-14 is
    then a cancellation of terms whose 2e-5 sum p |x| >= 1e-5 covers the 2^-25 of a subnormal's rounding.  With scores in (-8, 8) and
    x ~ N(0, 1) a row of two or more entries mixes several x of ordinary size and the same term covers it; a row of one entry copies
    its x."""
    for name in GRAPHS:
        rowptr, col, rp, cc = graph(name)
        empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
        for scale, slope in ((4.0, 0.2), (40.0, 0.25)) if name == "main" else ((4.0, 0.2),):
            if scale == 4.0:
                a_dst = torch.from_numpy(rng.uniform(-4, 4, size=(N, heads)).astype(np.float32)).to(DEV)
                a_src = torch.from_numpy(rng.uniform(-4, 4, size=(M, heads)).astype(np.float32)).to(DEV)
            else:
                a_dst = torch.from_numpy((rng.integers(-320, 321, size=(N, heads)) / 8).astype(np.float32)).to(DEV)
                a_src = torch.from_numpy((rng.integers(-320, 321, size=(M, heads)) / 8).astype(np.float32)).to(DEV)
            for ld in strides(h) if (name == "main" and scale == 4.0) else (h,):
                X = features(rng, ld, dtype, "normal" if scale == 4.0 else "away")
                out, lse = call_gat(dtype, rp, cc, a_dst, a_src, heads, slope, X, h)
                assert not torch.isnan(out).any() and not torch.isnan(lse).any(), "a row was not written"
                assert (out[empty] == 0).all() and (lse[empty] == 0).all()
                ref, mag, lse_ref, _, _ = gat_reference_dev(N, rowptr, col, a_dst, a_src, heads, slope, X, h)
                err = (out.double() - ref).abs()
                bound = U[dtype] * ref.abs() + 2e-5 * mag
                lerr = (lse.double() - lse_ref).abs()
                print(f"gat {name} {dtype} h={h} heads={heads} ldx={ld} |z|<={2 * scale:.0f}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}, "
                      f"lse = {(lerr / (2e-5 * (1 + lse_ref.abs()))).max().item():.3f}")
                assert torch.all(err <= bound) and torch.all(lerr <= 2e-5 * (1 + lse_ref.abs()))
                out2, lse2 = call_gat(dtype, rp, cc, a_dst, a_src, heads, slope, X, h)
                out3, none = call_gat(dtype, rp, cc, a_dst, a_src, heads, slope, X, h, want_lse=False)
                assert torch.equal(out, out2) and torch.equal(lse, lse2) and none is None and torch.equal(out, out3)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("h,heads", WIDTHS)
def test_sddmm_float32_out(rng, dtype, h, heads):
    """16-bit G and X, float32 out, nothing rounded: within 1e-5 sum_f |G . X|.  The main graph has batches of 64 entries inside the long
    rows (G kept in registers) and batches that cross rows"""
    del heads
    for name in ("main", "one-run", "boundary"):
        rowptr, col, rp, cc = graph(name)
        row = torch.repeat_interleave(torch.arange(N, device=DEV), torch.diff(torch.from_numpy(rowptr).long().to(DEV)))
        for ld in strides(h) if name == "main" else (h,):
            G = torch.from_numpy(rng.standard_normal((N, ld)).astype(np.float32)).to(DEV, dtype)
            X = features(rng, ld, dtype, "normal")
            out = torch.full((len(col),), float("nan"), dtype=torch.float32, device=DEV)
            _lib.sddmm(CODE[dtype], N, rp.data_ptr(), cc.data_ptr(), len(col), G.data_ptr(), ld, X.data_ptr(), ld, h, out.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            prod = G[:, :h].double()[row] * X[:, :h].double()[cc.long()]
            err = (out.double() - prod.sum(1)).abs()
            print(f"sddmm {name} {dtype} h={h} ld={ld}: max err / bound = {(err / (1e-5 * prod.abs().sum(1)).clamp_min(1e-300)).max().item():.3f}")
            assert torch.all(err <= 1e-5 * prod.abs().sum(1))
    rowptr, col, rp, cc = graph("main")
    G, X = torch.zeros(N, h, device=DEV, dtype=dtype), torch.ones(M, h, device=DEV, dtype=dtype)
    got = autograd.sddmm(rp, cc, G, X)
    assert got.dtype == torch.float32 and got.shape == (len(col),)


def t_mag(rowptr, col, w, G, heads):
    """sum over the entries of a column of |w . G[row]|: what a gradient dX is made of, float64 on the host"""
    row = torch.repeat_interleave(torch.arange(N), torch.diff(torch.from_numpy(rowptr).long()))
    msg = w.double().reshape(len(col), heads).repeat_interleave(G.size(1) // heads, dim=1) * G.double()[row]
    return torch.zeros(M, G.size(1), dtype=torch.float64).index_add_(0, torch.from_numpy(col).long(), msg.abs())


F32_TOL = dict(rtol=1e-4, atol=1e-4)   # the float32 autograd tolerance of test_attention_gpu / test_gat_fused_gpu


@pytest.mark.parametrize("dtype", HALF)
def test_gradients_of_spmm_values_and_mean(rng, dtype):
    torch.manual_seed(11)
    rowptr, col, rp, cc = graph("main")
    g = EdgeGraph(rp, cc, (N, M))
    h, heads = 64, 4
    val = torch.from_numpy(rng.uniform(0.5, 1.0, size=(len(col), heads)).astype(np.float32))
    X = torch.randn(M, h).to(dtype)
    G = torch.randn(N, h).to(dtype)
    vd, Xd = val.to(DEV).requires_grad_(), X.to(DEV).requires_grad_()
    out = spmm_values(g, vd, Xd, heads=heads)
    out.backward(G.to(DEV))
    assert out.dtype == dtype and vd.grad.dtype == torch.float32 and Xd.grad.dtype == dtype
    vc, Xc = val.double().requires_grad_(), X.double().requires_grad_()
    ref_spmm(rowptr, col, vc, Xc, heads, N).backward(G.double())
    assert torch.allclose(vd.grad.cpu().double(), vc.grad, **F32_TOL)
    assert within(Xd.grad.cpu(), Xc.grad, t_mag(rowptr, col, val, G, heads), U[dtype], 1e-5, f"spmm_values dX {dtype}")
    # values in X's dtype: they are taken as float32, their gradient comes back in theirs
    v16 = val.to(DEV, dtype).requires_grad_()
    spmm_values(g, v16, Xd.detach(), heads=heads).backward(G.to(DEV))
    assert v16.grad.dtype == dtype
    # the mean, with float32 values
    cnt = torch.from_numpy(np.maximum(np.diff(rowptr), 1)).double().unsqueeze(1)
    vd, Xd = val[:, 0].to(DEV).requires_grad_(), X.to(DEV).requires_grad_()
    out = spmm_reduce(g, Xd, "mean", value=vd)
    out.backward(G.to(DEV))
    assert out.dtype == dtype and vd.grad.dtype == torch.float32 and Xd.grad.dtype == dtype
    vc, Xc = val[:, 0].double().requires_grad_(), X.double().requires_grad_()
    (ref_spmm(rowptr, col, vc, Xc, 1, N) / cnt).backward(G.double())
    assert torch.allclose(vd.grad.cpu().double(), vc.grad, **F32_TOL)
    row = torch.repeat_interleave(torch.arange(N), torch.diff(torch.from_numpy(rowptr).long()))
    assert within(Xd.grad.cpu(), Xc.grad, t_mag(rowptr, col, val[:, 0].double() / cnt[row, 0], G, 1), U[dtype], 1e-5, f"mean dX {dtype}")


@pytest.mark.parametrize("dtype", HALF)
def test_gradients_of_gat_aggregate(rng, dtype):
    torch.manual_seed(12)
    rowptr, col, rp, cc = graph("main")
    g = EdgeGraph(rp, cc, (N, M))
    h, heads = 64, 4
    a_dst, a_src = torch.randn(N, heads), torch.randn(M, heads)
    X, G = torch.randn(M, h).to(dtype), torch.randn(N, h).to(dtype)
    dev = [t.to(DEV).requires_grad_() for t in (a_dst, a_src, X)]
    out = gat_aggregate(g, *dev, 0.2)
    out.backward(G.to(DEV))
    assert out.dtype == dtype and [t.grad.dtype for t in dev] == [torch.float32, torch.float32, dtype]
    cpu = [t.double().requires_grad_() for t in (a_dst, a_src, X)]
    ref = ref_gat_aggregate(rowptr, col, *cpu, 0.2, N)
    ref.backward(G.double())
    for name, d, c in zip(("a_dst", "a_src"), dev, cpu):
        print(f"gat_aggregate {dtype} d{name}: max abs err = {(d.grad.cpu().double() - c.grad).abs().max().item():.3e}")
        assert torch.allclose(d.grad.cpu().double(), c.grad, **F32_TOL), name
    row = torch.repeat_interleave(torch.arange(N), torch.diff(torch.from_numpy(rowptr).long()))
    z = torch.nn.functional.leaky_relu(a_dst.double()[row] + a_src.double()[torch.from_numpy(col).long()], 0.2)
    m = torch.full((N, heads), -float("inf"), dtype=torch.float64).index_reduce_(0, row, z, "amax", include_self=True)
    e = torch.exp(z - m[row])
    p = e / torch.zeros(N, heads, dtype=torch.float64).index_add_(0, row, e)[row]
    assert within(dev[2].grad.cpu(), cpu[2].grad, t_mag(rowptr, col, p, G, heads), U[dtype], 1e-5, f"gat_aggregate dX {dtype}")
    # node terms in X's dtype: taken as float32, gradients in theirs
    dev = [t.to(DEV, dtype).requires_grad_() for t in (a_dst, a_src, X)]
    gat_aggregate(g, *dev, 0.2).backward(G.to(DEV))
    assert [t.grad.dtype for t in dev] == [dtype] * 3


@pytest.mark.parametrize("code", [_lib.BF16, _lib.FLT16])
def test_rejections_before_any_launch(code):
    rowptr, col, rp, cc = graph("main")
    nnz, h, heads = len(col), 64, 4
    X = torch.zeros(M, h, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(N, h, dtype=torch.bfloat16, device=DEV)
    val = torch.zeros(nnz, heads, device=DEV)
    a = torch.zeros(max(N, M), heads, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    arg = torch.zeros(N, h, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.PygimError):   # max / min have no 16-bit form
        _lib.spmm_reduce(code, _lib.REDUCE_MAX, N, rp.data_ptr(), cc.data_ptr(), nnz, 0, X.data_ptr(), h, h, o.data_ptr(), h, 0, ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):
        _lib.spmm_reduce_workspace(code, _lib.REDUCE_MIN, N, nnz, h)
    with pytest.raises(_lib.PygimError):
        _lib.edge_softmax(code, N, rp.data_ptr(), nnz, val.data_ptr(), heads, val.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(_lib.PygimError):
        _lib.edge_softmax_workspace(code, N, nnz, heads)
    with pytest.raises(_lib.PygimError):
        _lib.spmm_reduce_backward(code, M, rp.data_ptr(), cc.data_ptr(), cc.data_ptr(), 0, 0, o.data_ptr(), h, arg.data_ptr(), h, X.data_ptr(), h)
    with pytest.raises(_lib.PygimError):   # no 16-bit device groups
        _lib.group_create(_lib.CSR, code, [rp.data_ptr()], [cc.data_ptr()], None, [N], [M], [nnz], [1], [h], h)
    # a workspace one byte short
    need = _lib.spmm_values_workspace(code, N, nnz, h, heads)
    with pytest.raises(_lib.PygimError):
        _lib.spmm_values(code, N, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), heads, X.data_ptr(), h, h, o.data_ptr(), h, ws.data_ptr(), need - 1)
    need = _lib.gat_aggregate_workspace(code, N, nnz, h, heads)
    with pytest.raises(_lib.PygimError):
        _lib.gat_aggregate(code, N, rp.data_ptr(), cc.data_ptr(), nnz, a.data_ptr(), a.data_ptr(), heads, 0.2, X.data_ptr(), h, h, o.data_ptr(), h, 0,
                           ws.data_ptr(), need - 1)
    need = _lib.spmm_reduce_workspace(code, _lib.REDUCE_MEAN, N, nnz, h)
    with pytest.raises(_lib.PygimError):
        _lib.spmm_reduce(code, _lib.REDUCE_MEAN, N, rp.data_ptr(), cc.data_ptr(), nnz, 0, X.data_ptr(), h, h, o.data_ptr(), h, 0, ws.data_ptr(), need - 1)
    torch.cuda.synchronize()
    assert (o == 0).all(), "a rejected call wrote its output"


def square_adj():
    rowptr, col, _, _ = graph("main")
    rp = np.concatenate([rowptr[:M + 1].astype(np.int64)])
    return SparseTensorShim(rowptr=torch.from_numpy(rp), col=torch.from_numpy(col[:rp[-1]].astype(np.int64)), sparse_sizes=(M, M))


@pytest.mark.parametrize("mode", ["to", "autocast"])
@pytest.mark.parametrize("layer", ["gat-fused", "gat", "sage-mean"])
def test_layers_in_bfloat16(layer, mode):
    """after model.to(torch.bfloat16) and under torch.autocast: forward and backward run, everything is finite and of the expected dtype"""
    adj = square_adj()
    torch.manual_seed(0)
    if layer == "sage-mean":
        conv = gnn.SAGEConv(24, 32, aggr="mean").to(DEV)
    else:
        conv = gnn.GATConv(24, 8, heads=4, fused=layer == "gat-fused").to(DEV)
    x = torch.randn(M, 24, device=DEV)
    if mode == "to":
        conv, x = conv.to(torch.bfloat16), x.to(torch.bfloat16)
        out = conv(x.requires_grad_(), adj)
        assert out.dtype == torch.bfloat16
    else:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = conv(x.requires_grad_(), adj)
        assert out.dtype in (torch.bfloat16, torch.float32)
    out.float().square().mean().backward()
    assert out.shape == (M, 32) and torch.isfinite(out).all()
    assert x.grad.dtype == x.dtype and torch.isfinite(x.grad).all()
    for p in conv.parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and torch.isfinite(p.grad).all()


def test_fused_layer_is_its_hand_composition():
    adj = square_adj()
    torch.manual_seed(1)
    conv = gnn.GATConv(24, 8, heads=4, fused=True).to(DEV, torch.bfloat16)
    x = torch.randn(M, 24, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        xp = conv.lin(x).view(-1, 4, 8)
        a_src, a_dst = (xp * conv.att_src).sum(-1), (xp * conv.att_dst).sum(-1)
        want = gat_aggregate(EdgeGraph.of(adj), a_dst, a_src, xp.reshape(-1, 32), conv.negative_slope) + conv.bias
        assert torch.equal(conv(x, adj), want)
