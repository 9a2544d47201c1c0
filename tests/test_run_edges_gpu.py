"""The run boundaries of the entry-run walker, on purpose instead of by luck of a seed: every entry point of the gather family on the
hand-built graphs of run_edges.py (a row that is exactly a run, a cut row that starts on a run boundary and ends on a run's last entry,
a run of two cut rows, nnz % 512 == 1, leading and trailing empty rows, one row, whole batches) and on the transpose of `edges`.

Nothing is restated here: the graphs are registered with the existing GPU files under their names, and the checks are those files' own
(check_* helpers, or the body of a parametrised test called with a graph name it is not parametrised over), with their references and
their bounds: NaN-pre-filled outputs fully written, empty rows exactly zero with arg == -1 and lse == 0, a second launch bit-equal."""
import numpy as np
import pytest
import torch

import run_edges
import test_attention_gpu as t_att
import test_gat_fused_gpu as t_gat
import test_gatv2_gpu as t_v2
import test_half_gpu as t_half
import test_reduce_gpu as t_red
import test_sparse_attention_gpu as t_sa
from pygim_amd import _lib, pim_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = list(run_edges.GRAPHS)
ROW_WIDTHS = [8, 32, 256, 520]               # eight lane groups (FLT32), 16-byte pieces, the whole wave, two pieces per lane + a second chunk
HEAD_SHAPES = [(32, 4), (256, 1), (100, 4)]

for _mod in (t_att, t_red, t_sa, t_v2):      # t_gat shares t_att's dict
    for _name in NAMES:
        _mod.GRAPHS.setdefault(_name, (lambda k: lambda rng: run_edges.graph(k))(_name))


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def test_the_graphs_are_what_they_are_for():
    for name in NAMES:
        n, m, rowptr, col = run_edges.graph(name)
        assert rowptr[0] == 0 and rowptr[-1] == len(col) and len(rowptr) == n + 1 and col.max() < m
    n, m, rowptr, col = run_edges.graph("edges-T")
    assert (n, m) == (97, 25) and np.array_equal(np.bincount(col, minlength=25), run_edges.EDGES_DEG)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", ROW_WIDTHS)
@pytest.mark.parametrize("graph", NAMES)
def test_spmm_values(rng, dtype, h, graph):
    """heads 1, 4 and 8"""
    t_att.check_spmm_values_parity(rng, dtype, h, graph)


@pytest.mark.parametrize("h", ROW_WIDTHS)
@pytest.mark.parametrize("graph", NAMES)
def test_spmm_values_bf16(rng, h, graph):
    """BF16 X and out, float32 values and accumulation: test_half_gpu's bound (u |ref| + 1e-5 sum |v x| + 2^-24), heads 1 and 4"""
    dtype = torch.bfloat16
    n, m, rowptr, col = run_edges.graph(graph)
    rp, cc = t_att.dev_csr(rowptr, col)
    nnz = len(col)
    X = torch.from_numpy(rng.standard_normal((m, h)).astype(np.float32)).to(DEV, dtype)
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    for heads in (1, 4):
        val = torch.from_numpy(rng.uniform(0.5, 1.0, size=(nnz, heads)).astype(np.float32)).to(DEV)

        def run():
            ws = torch.empty(max(_lib.spmm_values_workspace(_lib.BF16, n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
            out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
            _lib.spmm_values(_lib.BF16, n, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), heads, X.data_ptr(), h, h, out.data_ptr(), h, ws.data_ptr(),
                             ws.numel(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out

        out = run()
        assert not torch.isnan(out).any(), "a row was not written"
        assert (out[empty] == 0).all()
        ref, mag = t_att.spmm_reference(n, rowptr, col, val, heads, X, h)
        assert t_half.within(out, ref, mag, t_half.U[dtype], 1e-5, f"spmm_values {graph} bf16 h={h} heads={heads}")
        assert torch.equal(out, run()), "two launches differ"


@pytest.mark.parametrize("h", ROW_WIDTHS)
@pytest.mark.parametrize("graph", NAMES)
def test_mean(rng, h, graph):
    t_red.check_mean_parity(rng, torch.float32, h, graph)


@pytest.mark.parametrize("dtype", t_red.ALL_TYPES)
@pytest.mark.parametrize("h", ROW_WIDTHS)
@pytest.mark.parametrize("graph", NAMES)
def test_max_min_with_arg(rng, dtype, h, graph):
    """features in -2 .. 2, values in three powers of two: most rows are decided by the tie rule; out and arg bit-equal to the shim"""
    t_red.check_max_min_with_ties(rng, dtype, h, graph)


@pytest.mark.parametrize("dtype", t_red.FLOATS)
@pytest.mark.parametrize("h", [8, 256, 520])
@pytest.mark.parametrize("graph", NAMES)
def test_max_backward(rng, dtype, h, graph):
    """walks the transpose: `edges` gives it 97 short rows that point into the cut rows, `edges-T` the cut rows themselves"""
    t_red.test_backward_parity(rng, dtype, h, graph)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("heads", [1, 3, 4])
@pytest.mark.parametrize("graph", NAMES)
def test_edge_softmax_forward_and_backward(rng, dtype, heads, graph):
    """nnz % 64 == 1 and nnz % 1024 == 1 on `edges`: a last batch and a last wave of one entry"""
    t_att.test_edge_softmax_parity(rng, dtype, heads, graph)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", ROW_WIDTHS + [100])
@pytest.mark.parametrize("graph", NAMES)
def test_gat_aggregate(rng, dtype, h, graph):
    """heads 1, 4 and 8 where they divide h; (100, 4): one-element pieces"""
    t_gat.test_gat_aggregate_parity(rng, dtype, h, graph)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", HEAD_SHAPES)
@pytest.mark.parametrize("graph", NAMES)
def test_sparse_attention(rng, dtype, h, heads, graph):
    t_sa.test_sparse_attention_parity(rng, dtype, h, heads, graph)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", HEAD_SHAPES)
@pytest.mark.parametrize("graph", NAMES)
def test_gatv2_forward(rng, dtype, h, heads, graph):
    t_v2.test_gatv2_forward_parity(rng, dtype, h, heads, graph)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", HEAD_SHAPES)
@pytest.mark.parametrize("graph", NAMES)
def test_gatv2_backward(rng, dtype, h, heads, graph):
    """both directions per graph: with `edges` as A the plain direction walks the edge structure, with `edges-T` as A the transposed one"""
    t_v2.test_gatv2_backward_parity(rng, dtype, h, heads, graph)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", [8, 32, 256, 520])
@pytest.mark.parametrize("graph", NAMES)
def test_sddmm(rng, dtype, h, graph):
    """nnz % 256 == 1 on `edges`: a last 256-entry wave of one entry.  The bound of test_autograd_gpu.test_sddmm_widths_and_hubs:
    TOL * sum_f |G[r, f] X[c, f]| per entry"""
    n, m, rowptr, col = run_edges.graph(graph)
    rp, cc = t_att.dev_csr(rowptr, col)
    G = torch.from_numpy(rng.standard_normal((n, h))).to(DEV, dtype)
    X = torch.from_numpy(rng.standard_normal((m, h))).to(DEV, dtype)
    check_sddmm(f"{graph} {dtype} h={h}", dtype, n, rp, cc, G, X, h)


def check_sddmm(tag, dtype, n, rp, cc, G, X, h):
    """G, X: [rows, ld] device tensors whose first h columns are the operands (16-bit types: a float32 result, test_half_gpu's 1e-5)"""
    half = dtype in t_half.HALF
    code = t_half.CODE[dtype] if half else pim_ops.DTYPE_CODE[dtype]
    nnz = cc.numel()

    def run():
        out = torch.full((nnz,), float("nan"), dtype=torch.float32 if half else dtype, device=DEV)
        _lib.sddmm(code, n, rp.data_ptr(), cc.data_ptr(), nnz, G.data_ptr(), G.stride(0), X.data_ptr(), X.stride(0), h, out.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out

    out = run()
    assert not torch.isnan(out).any(), "an entry was not written"
    row = torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(rp.long()))
    prod = G[:, :h].double()[row] * X[:, :h].double()[cc.long()]
    err = (out.double() - prod.sum(1)).abs()
    bound = (1e-5 if half else t_att.TOL[dtype]) * prod.abs().sum(1)
    print(f"sddmm {tag}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert torch.all(err <= bound)
    assert torch.equal(out, run()), "two launches differ"
