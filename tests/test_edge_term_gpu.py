"""Edge terms on the GPU: pygim_gat_aggregate_edge and pygim_sparse_attention_bias through the C ABI against the float64 reference of
edge_term_ref.py on the device (its docstring states the bounds: those of the base calls' own tests), and gat_aggregate(a_edge=) /
sparse_attention(bias=) / gnn.GATConv(edge_dim=) (autograd, training) against the per-entry CPU reference of test_edge_term_cpu.py, which
also shows on the reference alone that the parity cases here fail for a term that is ignored or misplaced."""
import copy

import numpy as np
import pytest
import torch

import edge_term_ref as er
import test_sparse_attention_gpu as base_sa
from pygim_amd import _lib, gnn
from pygim_amd.attention import EdgeGraph, gat_aggregate, sparse_attention
from pygim_amd.sparse_tensor import SparseTensorShim
from test_attention_gpu import dev_csr
from test_edge_term_cpu import gatconv_edge_reference, ref_gat_edge, ref_sa_bias
from test_sparse_attention_gpu import CODE, lse_type, strided

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = (0x9E3779B9 << 32) | 0x1234ABCD
assert er.SA_SHAPES == base_sa.SHAPES


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def call(kind, dtype, n, rp, cc, A, B, V, term, h, heads, scalar, p=0.0, seed=0, entry="edge", want_lse=True, ws_bytes=None):
    """one C call -> (out, lse or None), NaN-filled before it.  A, B, V: device tensors whose first columns are the operands (gat: A, B the
    node terms).  entry: "edge" (the entry point with a term), "dropout" or "base" (term is then not passed).  ws_bytes: a workspace of that
    size instead of what the workspace function says (for shapes it rejects)"""
    nnz = cc.numel()
    code = CODE[dtype]
    wsf = _lib.gat_aggregate_workspace if kind == "gat" else _lib.sparse_attention_workspace
    ws = torch.empty(max(wsf(code, n, nnz, h, heads), 16) if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((n, heads), float("nan"), dtype=lse_type(dtype), device=DEV) if want_lse else None
    tail = (out.data_ptr(), out.stride(0), lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    if kind == "gat":
        args = (code, n, rp.data_ptr(), cc.data_ptr(), nnz, A.data_ptr(), B.data_ptr(), heads, scalar, V.data_ptr(), V.stride(0), h) + tail
        fn = {"edge": _lib.gat_aggregate_edge, "dropout": _lib.gat_aggregate_dropout, "base": _lib.gat_aggregate}[entry]
    else:
        args = (code, n, rp.data_ptr(), cc.data_ptr(), nnz, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), V.data_ptr(), V.stride(0), h, heads,
                scalar) + tail
        fn = {"edge": _lib.sparse_attention_bias, "dropout": _lib.sparse_attention_dropout, "base": _lib.sparse_attention}[entry]
    if entry == "edge":
        fn(*args, term.data_ptr() if term is not None else 0, p, seed)
    elif entry == "dropout":
        fn(*args, p, seed)
    else:
        fn(*args)
    torch.cuda.synchronize()
    return out, lse


def setup(kind, gname, h, heads, dtype):
    n, m, rowptr, col = er.graph(gname)
    rp, cc = dev_csr(rowptr, col)
    ops = er.operands(kind, n, m, len(col), h, heads, dtype)
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ops.items()}
    return n, m, rowptr, col, rp, cc, ops, dev


def check(tag, kind, dtype, n, rowptr, rp, cc, A, B, V, term, h, heads, scalar, r, p=0.0, seed=0, skip=None):
    """one call under the bounds of the reference r, every row written, empty rows zero, a second launch bit-equal.  skip: bool [n, heads],
    the (row, head) pairs that are not compared"""
    out, lse = call(kind, dtype, n, rp, cc, A, B, V, term, h, heads, scalar, p, seed)
    hd = h // heads
    use = torch.ones(n, heads, dtype=torch.bool, device=DEV) if skip is None else ~skip
    usef = use.repeat_interleave(hd, dim=1)
    assert not torch.isnan(out[usef]).any() and not torch.isnan(lse[use]).any(), "a row was not written"
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert (out[empty] == 0).all() and (lse[empty] == 0).all()
    err, bound = (out.double() - r["ref"]).abs(), er.out_bound(kind, dtype, r, h, heads)
    lerr, lbound = (lse.double() - r["lse"]).abs(), er.lse_bound(kind, dtype, r)
    print(f"{kind} edge term {tag}: max err / bound = {(err / bound.clamp_min(1e-300))[usef].max().item():.3e}, "
          f"lse max err / bound = {(lerr / lbound)[use].max().item():.3e}")
    assert torch.all(err[usef] <= bound[usef])
    assert torch.all(lerr[use] <= lbound[use])
    out2, lse2 = call(kind, dtype, n, rp, cc, A, B, V, term, h, heads, scalar, p, seed)
    assert torch.equal(out.view(torch.uint8), out2.view(torch.uint8)) and torch.equal(lse.view(torch.uint8), lse2.view(torch.uint8)), "two launches differ"
    return out, lse


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", er.GAT_WIDTHS)
@pytest.mark.parametrize("gname", er.GRAPH_NAMES)
def test_gat_aggregate_edge_parity(dtype, h, gname):
    """the widths and head counts of test_gat_aggregate_parity: every lane layout; on the small graph X also with a padded aligned row
    stride and with a misaligned one"""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    for heads in [k for k in er.GAT_HEADS if h % k == 0]:
        n, m, rowptr, col, rp, cc, ops, dev = setup("gat", gname, h, heads, dtype)
        r = er.reference("gat", dtype, n, rowptr, col, er.as_float64(ops, DEV), h, heads, DEV)
        for ldx in ((h, h + 2 * vec, h + 1) if gname == "small" else (h,)):
            check(f"{gname} {dtype} h={h} heads={heads} ldx={ldx}", "gat", dtype, n, rowptr, rp, cc, dev["A"], dev["B"], strided(dev["V"], ldx), dev["term"],
                  h, heads, er.SLOPE, r)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", er.SA_SHAPES)
@pytest.mark.parametrize("gname", er.GRAPH_NAMES)
def test_sparse_attention_bias_parity(dtype, h, heads, gname):
    """the shapes of test_sparse_attention_parity; on the small graph every operand also with a padded aligned row stride and with a
    misaligned one"""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    n, m, rowptr, col, rp, cc, ops, dev = setup("sa", gname, h, heads, dtype)
    r = er.reference("sa", dtype, n, rowptr, col, er.as_float64(ops, DEV), h, heads, DEV)
    lds = [(h, h, h)]
    if gname == "small":
        for ld in (h + 2 * vec, h + 1):
            lds += [(ld, h, h), (h, ld, h), (h, h, ld)]
    for ldq, ldk, ldv in lds:
        check(f"{gname} {dtype} h={h} heads={heads} ld={ldq},{ldk},{ldv}", "sa", dtype, n, rowptr, rp, cc, strided(dev["A"], ldq), strided(dev["B"], ldk),
              strided(dev["V"], ldv), dev["term"], h, heads, ops["scalar"], r)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["gat", "sa"])
def test_a_zero_term_stores_the_bits_of_the_base_call(kind, dtype, p):
    """z + 0 and scale * s + 0 are exact: out and lse of the base entry point (p = 0) / of the _dropout entry point (p = 0.5, one seed)"""
    for h, heads in [(9, 3), (32, 4), (100, 4), (256, 8), (512, 2)]:
        n, m, rowptr, col, rp, cc, ops, dev = setup(kind, "edges", h, heads, dtype)
        zero = torch.zeros_like(dev["term"])
        got = call(kind, dtype, n, rp, cc, dev["A"], dev["B"], dev["V"], zero, h, heads, ops["scalar"], p, SEED)
        want = call(kind, dtype, n, rp, cc, dev["A"], dev["B"], dev["V"], None, h, heads, ops["scalar"], p, SEED, entry="dropout" if p > 0 else "base")
        for a, b, name in zip(got, want, ("out", "lse")):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (kind, dtype, h, heads, name)
        other = call(kind, dtype, n, rp, cc, dev["A"], dev["B"], dev["V"], dev["term"], h, heads, ops["scalar"], p, SEED)
        assert not torch.equal(other[0].view(torch.uint8), want[0].view(torch.uint8)), "the term is read"


@pytest.mark.parametrize("gname", er.GRAPH_NAMES)
@pytest.mark.parametrize("kind", ["gat", "sa"])
def test_dropout_with_a_term(kind, gname):
    """the mask of pygim_attention_dropout_host on the probabilities of the scores WITH the term; lse has the bits of the p = 0 call with
    the same term"""
    dtype = torch.float32
    for h, heads in [(9, 3), (32, 4), (256, 8), (512, 2)]:
        n, m, rowptr, col, rp, cc, ops, dev = setup(kind, gname, h, heads, dtype)
        for p in (0.3, 0.5):
            keep = _lib.attention_dropout_host(len(col), heads, 0, p, SEED)
            w = np.where(keep != 0, 1.0 / (1.0 - p), 0.0)
            assert 0 < keep.mean() < 1
            r = er.reference(kind, dtype, n, rowptr, col, er.as_float64(ops, DEV), h, heads, DEV, w=w)
            _, lse = check(f"{gname} dropout p={p} h={h} heads={heads}", kind, dtype, n, rowptr, rp, cc, dev["A"], dev["B"], dev["V"], dev["term"], h, heads,
                           ops["scalar"], r, p, SEED)
            _, lse0 = call(kind, dtype, n, rp, cc, dev["A"], dev["B"], dev["V"], dev["term"], h, heads, ops["scalar"])
            assert torch.equal(lse.view(torch.uint8), lse0.view(torch.uint8)), "lse runs over all entries, dropped ones included"


@pytest.mark.parametrize("dtype", er.HALF)
@pytest.mark.parametrize("kind", ["gat", "sa"])
def test_16_bit_features_with_a_float32_term(kind, dtype):
    """the bound of test_half_gpu.py: u * |exact| on top of the float32 bound, exact = float64 on the 16-bit inputs"""
    for gname in er.GRAPH_NAMES:
        for h, heads in [(32, 4), (256, 8), (100, 4)]:
            n, m, rowptr, col, rp, cc, ops, dev = setup(kind, gname, h, heads, dtype)
            assert dev["term"].dtype == torch.float32 and dev["V"].dtype == dtype
            r = er.reference(kind, dtype, n, rowptr, col, er.as_float64(ops, DEV), h, heads, DEV)
            check(f"{gname} {dtype} h={h} heads={heads}", kind, dtype, n, rowptr, rp, cc, dev["A"], dev["B"], dev["V"], dev["term"], h, heads, ops["scalar"], r)


@pytest.mark.parametrize("h,heads", [(32, 4), (256, 8)])
@pytest.mark.parametrize("kind", ["gat", "sa"])
def test_minus_infinity_terms_mask_entries(kind, h, heads):
    """the edges graph: row 5 is a hub of 1024 entries cut across runs, row 11 reaches from inside run 6 to inside run 9, row 7 has one entry
    on each side of a run boundary.  Half the entries of rows 5 and 11 are masked for every head: the result is that of the graph without
    them.  Row 7 is masked entirely for head 0: NaN and lse = -inf for that head, as for a -inf node term, the other heads and the rows
    around it as before."""
    dtype = torch.float32
    n, m, rowptr, col, rp, cc, ops, dev = setup(kind, "edges", h, heads, dtype)
    rp64 = rowptr.astype(np.int64)
    assert rp64[6] - rp64[5] == 1024 and rp64[8] - rp64[7] == 2
    rng = np.random.default_rng(3)
    gone = np.zeros(len(col), dtype=bool)
    for row in (5, 11):
        gone[rp64[row]:rp64[row + 1]] = rng.random(rp64[row + 1] - rp64[row]) < 0.5
        gone[rp64[row]] = False
    term = ops["term"].clone()
    term[torch.from_numpy(gone)] = -float("inf")
    term[rp64[7]:rp64[8], 0] = -float("inf")
    # the reference: the graph without the masked entries of rows 5 and 11 (row 7 keeps its entries; its head 0 is not compared)
    rp2, col2 = er.remove_entries(n, rowptr, col, gone)
    ops2 = dict(ops, term=ops["term"][torch.from_numpy(~gone)])
    r = er.reference(kind, dtype, n, rp2, col2, er.as_float64(ops2, DEV), h, heads, DEV)
    skip = torch.zeros(n, heads, dtype=torch.bool, device=DEV)
    skip[7, 0] = True
    out, lse = check(f"-inf h={h} heads={heads}", kind, dtype, n, rowptr, rp, cc, dev["A"], dev["B"], dev["V"], term.to(DEV), h, heads, ops["scalar"], r, skip=skip)
    hd = h // heads
    assert torch.isnan(out[7, :hd]).all() and lse[7, 0] == -float("inf"), "a (row, head) with nothing but -inf terms"
    assert not torch.isnan(out[7, hd:]).any() and not torch.isnan(out[6]).any() and not torch.isnan(out[8]).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_autograd_on_device_matches_the_cpu_reference(rng, dtype):
    from test_attention_gpu import small_graph

    n, m, rowptr, col = small_graph(rng)
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    assert g.rowptr.is_cuda
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-11)
    heads, h = 4, 32
    torch.manual_seed(23)
    a_dst, a_src = torch.randn(n, heads, dtype=dtype), torch.randn(m, heads, dtype=dtype)
    Q, X, V = torch.randn(n, h, dtype=dtype), torch.randn(m, h, dtype=dtype), torch.randn(m, h, dtype=dtype)
    term = torch.randn(len(col), heads, dtype=dtype)
    G = torch.randn(n, h, dtype=dtype)

    def compare(name, host, run_dev, run_ref):
        cpu = [t.clone().double().requires_grad_() for t in host]
        ref = run_ref(*cpu)
        ref.backward(G.double())
        dev = [t.to(DEV).requires_grad_() for t in host]
        out = run_dev(*dev)
        assert out.is_cuda
        out.backward(G.to(DEV))
        assert torch.allclose(out.detach().cpu().double(), ref.detach(), **tol)
        for i, (d, c) in enumerate(zip(dev, cpu)):
            print(f"{name} autograd {dtype} operand {i}: max abs err = {(d.grad.cpu().double() - c.grad).abs().max().item():.3e}")
            assert d.grad.dtype == dtype and d.grad.shape == d.shape and torch.allclose(d.grad.cpu().double(), c.grad, **tol), (name, i)
        out_host = run_dev(*host)   # CPU tensors are staged to the device and come home
        assert not out_host.is_cuda and torch.equal(out_host, out.detach().cpu())

    compare("gat_aggregate(a_edge=)", (a_dst, a_src, X, term), lambda a, b, x, e: gat_aggregate(g, a, b, x, 0.2, a_edge=e),
            lambda a, b, x, e: ref_gat_edge(rowptr, col, a, b, e, x, 0.2, n))
    for fused in (True, False):
        compare(f"sparse_attention(bias=, fused={fused})", (Q, X, V, term), lambda q, k, v, b: sparse_attention(g, q, k, v, heads=heads, fused=fused, bias=b),
                lambda q, k, v, b: ref_sa_bias(rowptr, col, q, k, v, b, heads, n))


def test_fused_gatconv_with_edge_features_sgd_steps_match_the_cpu_reference(rng):
    """GATConv(edge_dim=4, heads=2, fused=True): three SGD steps in float64, losses and every parameter gradient as with the per-entry
    plain-torch statement of PyG's formula on the CPU; then one float32 forward, fused against unfused"""
    from conftest import random_csr

    n, f_in, f_out, heads, d = 1500, 16, 8, 2, 4
    rowptr, col = random_csr(rng, n, n, 9)
    adj = SparseTensorShim(rowptr=torch.from_numpy(rowptr).long(), col=torch.from_numpy(col).long(), sparse_sizes=(n, n))
    torch.manual_seed(0)
    feats = torch.randn(n, f_in, dtype=torch.float64)
    edge_attr = torch.randn(len(col), d, dtype=torch.float64)
    target = torch.randn(n, f_out * heads, dtype=torch.float64)
    base = gnn.GATConv(f_in, f_out, heads=heads, fused=True, edge_dim=d).double()

    def run(conv, dev, forward):
        conv = conv.to(dev)
        opt = torch.optim.SGD(conv.parameters(), lr=0.05)
        losses, grads = [], []
        for _ in range(3):
            opt.zero_grad()
            loss = ((forward(conv, feats.to(dev), edge_attr.to(dev)) - target.to(dev)) ** 2).mean()
            loss.backward()
            losses.append(loss.item())
            grads.append([p.grad.cpu().clone() for p in conv.parameters()])
            opt.step()
        return losses, grads

    l_gpu, g_gpu = run(copy.deepcopy(base), DEV, lambda c, x, e: c(x, adj, e))
    l_cpu, g_cpu = run(copy.deepcopy(base), "cpu", lambda c, x, e: gatconv_edge_reference(c, x, e, rowptr, col, n))
    assert np.allclose(l_gpu, l_cpu, rtol=1e-10, atol=1e-12)
    for a, b in zip(g_gpu, g_cpu):
        assert len(a) == 6
        for x, y in zip(a, b):
            assert torch.allclose(x, y, rtol=1e-9, atol=1e-11)
    fused = copy.deepcopy(base).float().to(DEV).eval()
    plain = copy.deepcopy(fused)
    plain.fused = False
    with torch.no_grad():
        a, b = (c(feats.float().to(DEV), adj, edge_attr.float().to(DEV)) for c in (fused, plain))
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)


def test_rejected_arguments_answer_before_any_launch():
    h, heads = 32, 4
    for kind in ("gat", "sa"):
        n, m, rowptr, col, rp, cc, ops, dev = setup(kind, "small", h, heads, torch.float32)
        A, B, V, term, s = dev["A"], dev["B"], dev["V"], dev["term"], ops["scalar"]

        def rejected(**kw):
            a = dict(term=term, heads=heads, p=0.0)
            a.update(kw)
            with pytest.raises(_lib.PygimError) as e:
                call(kind, torch.float32, n, rp, cc, A, B, V, a["term"], h, a["heads"], s, a["p"], SEED, ws_bytes=1 << 22)
            assert e.value.code == _lib.ERR_INVALID

        rejected(term=None)                                     # a NULL term with nnz > 0
        for p in (-0.1, 1.0, 1.5, float("nan")):
            rejected(p=p)
        rejected(heads=5)                                       # heads must divide h
        if kind == "sa":
            wide = torch.zeros(max(n, m), 257, device=DEV)      # a head of 257 features
            with pytest.raises(_lib.PygimError) as e:
                call("sa", torch.float32, n, rp, cc, wide, wide, wide, term[:, :1].contiguous(), 257, 1, 1.0, ws_bytes=1 << 22)
            assert e.value.code == _lib.ERR_INVALID
        # nothing was launched: a rejected call leaves out and lse as they were
        out = torch.full((n, h), float("nan"), device=DEV)
        lse = torch.full((n, heads), float("nan"), device=DEV)
        ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
        tail = (out.data_ptr(), h, lse.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        with pytest.raises(_lib.PygimError):
            if kind == "gat":
                _lib.gat_aggregate_edge(_lib.FLT32, n, rp.data_ptr(), cc.data_ptr(), len(col), A.data_ptr(), B.data_ptr(), heads, s, V.data_ptr(), h, h, *tail,
                                        0, 0.0, SEED)
            else:
                _lib.sparse_attention_bias(_lib.FLT32, n, rp.data_ptr(), cc.data_ptr(), len(col), A.data_ptr(), h, B.data_ptr(), h, V.data_ptr(), h, h, heads,
                                           s, *tail, 0, 0.0, SEED)
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(lse).all()
        # nnz = 0 takes a NULL term: every row is empty
        rp0 = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
        out0, lse0 = call(kind, torch.float32, n, rp0, cc[:0], A, B, V, None, h, heads, s)
        assert (out0 == 0).all() and (lse0 == 0).all()
