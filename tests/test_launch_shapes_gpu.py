"""Every launch shape of the gather kernels, on purpose instead of by luck of a list: the cases of tests/launch_shapes.py (proven
complete by test_launch_shapes_cpu.py) run through the existing GPU files' own checks, on their `small` graph (700 rows, about 9 000
entries, rows of 64, 128 and 700 entries) and on run_edges' `edges` (cut rows: the workspace slot stores depend on the lane layout too).

Nothing is restated here.  A case goes through the check helper of the file that owns the entry point (or through the body of its
parametrised test, called with the case's numbers), with that file's float64 reference and bounds: NaN-pre-filled outputs fully
written, empty rows exactly zero, a second launch bit-equal.  Misalignment is put under those helpers: the file's call_* function is
replaced, for the test, by a wrapper that hands one operand over in another buffer -- a row stride that is no multiple of a 16-byte
piece, or a start one element into an aligned buffer while the stride stays a multiple of a piece -- NaN all around it, and checks
after every call that the NaN around an output is still there.  Every operand that the launcher's alignment test names takes its turn,
out included.  The 16-bit types go through the 16-bit tests of the owning files: test_half_gpu's on its own graphs (`main` has cut rows),
and the GATv2 backward under the bound of test_gatv2_gpu.test_gradients_in_bfloat16 on `small`.

Also here: the GATv2 datt reduction at one, two and three levels, the head-wise kernels' second launch, and the rejection of rows that
one launch cannot hold."""
import inspect

import pytest
import torch

import launch_shapes as ls
import run_edges
import test_attention_gpu as t_att
import test_gat_fused_gpu as t_gat
import test_gatv2_gpu as t_v2
import test_half_gpu as t_half
import test_reduce_gpu as t_red
import test_run_edges_gpu as t_edges
import test_sparse_attention_gpu as t_sa
from pygim_amd import _lib
from pygim_amd.attention import EdgeGraph

pytestmark = pytest.mark.gpu

DEV = "cuda"
TORCH = {"i8": torch.int8, "i16": torch.int16, "i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "f64": torch.float64,
         "f16": torch.float16, "bf16": torch.bfloat16}
GRAPH_NAMES = ("small", "edges")
NAN = float("nan")

for _mod in (t_att, t_red, t_sa, t_v2):      # t_gat shares t_att's dict
    _mod.GRAPHS.setdefault("edges", lambda rng: run_edges.graph("edges"))


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def cases(family, keep=lambda c: True):
    return [pytest.param(c, id=f"{c.dtype}-h{c.h}-k{c.heads}-{c.mis or 'aligned'}") for c in ls.TABLES[family] if c.heads < 65537 and keep(c)]


def is_half(c):
    return c.dtype in ("f16", "bf16")


class Views:
    """view(name, t): t itself, or -- for the operand `which` of a misaligned case -- the same values in a buffer with a row stride of
    w + 1 elements ("stride"), or starting one element into a 16-byte aligned buffer with a stride that is a multiple of the piece
    ("base"; contiguous=True: the stride stays w, for the [nnz, heads] arrays of edge_softmax).  The buffer is NaN (77 for integers)
    outside the view: nothing may read it, and check() says whether something wrote it."""

    def __init__(self, case, which, contiguous=False):
        self.mis, self.which, self.contiguous = case.mis, which, contiguous
        self.vec = 16 // torch.empty(0, dtype=TORCH[case.dtype]).element_size()
        self.guards = []

    def __call__(self, name, t):
        if self.mis is None or name != self.which or t is None:
            return t
        rows, w = t.shape
        fill = NAN if t.dtype.is_floating_point else t_red.SENTINEL
        if self.mis == "stride":
            ld, off = w + 1, 0
        else:
            ld, off = (w if self.contiguous else (w + self.vec - 1) // self.vec * self.vec + self.vec), 1
        buf = torch.full((rows * ld + self.vec,), fill, dtype=t.dtype, device=t.device)
        v = buf.as_strided((rows, w), (ld, 1), off)
        v.copy_(t)
        if self.mis == "base":
            assert v.data_ptr() % 16 != 0 and (self.contiguous or (ld * t.element_size()) % 16 == 0)
        outside = torch.ones(buf.numel(), dtype=torch.bool, device=t.device)
        outside.as_strided((rows, w), (ld, 1), off).fill_(False)
        self.guards.append((buf, outside, fill))
        return v

    def check(self):
        for buf, outside, fill in self.guards:
            pad = buf[outside]
            assert bool(torch.isnan(pad).all() if buf.dtype.is_floating_point else (pad == fill).all()), "a store outside the operand"
        self.guards.clear()


def through(call, views, operands, out=None, out_shape=None):
    """`call` (a call_* helper of an existing file) with the named operands handed over through `views`; `out`: the name of its output
    argument (made here, NaN-filled, when the helper leaves it to the callee), out_shape(arguments) -> (rows, width, dtype)"""
    sig = inspect.signature(call)

    def wrapped(*args, **kwargs):
        ba = sig.bind(*args, **kwargs)
        ba.apply_defaults()
        for name in operands:
            ba.arguments[name] = views(name, ba.arguments[name])
        if out is not None and views.which == out and views.mis is not None:
            if ba.arguments[out] is None:
                rows, w, dtype = out_shape(ba.arguments)
                ba.arguments[out] = torch.full((rows, w), NAN if dtype.is_floating_point else t_red.SENTINEL, dtype=dtype, device=DEV)
            ba.arguments[out] = views(out, ba.arguments[out])
        res = call(*ba.args, **ba.kwargs)
        views.check()
        return res

    return wrapped


def HALF_OUT(a):
    """the output of test_half_gpu's call helpers: [N, h] on its own graphs"""
    return t_half.N, a["h"], a["dtype"]


def turns(case, operands):
    """the operands a case misaligns, one per run (an aligned case: one run, nothing misaligned)"""
    return operands if case.mis else (None,)


def says(kind, case):
    """the query still says what the table states (the CPU file proves it for the whole table; this ties the GPU run to it)"""
    shape = _lib.gather_launch_shape(kind, ls.CODE[case.dtype], case.h, case.heads, case.mis is None)
    assert tuple(shape[k] for k in _lib.SHAPE_FIELDS) == case.shape, (case, shape)
    print(f"{case.h} x {case.heads} {case.dtype} {case.mis}: {case.why}")


# ---- the row walkers ----
@pytest.mark.parametrize("case", cases("walker"))
def test_spmm_values(rng, monkeypatch, case):
    says(_lib.SHAPE_SPMM_VALUES, case)
    dtype = TORCH[case.dtype]
    for which in turns(case, ("X", "out")):
        if is_half(case):   # test_half_gpu: sums (and, with one head, means) on its own graphs
            views = Views(case, which)
            monkeypatch.setattr(t_half, "strides", lambda h: (h,))
            monkeypatch.setattr(t_half, "call_values", through(t_half.call_values, views, ("X",), "out", HALF_OUT))
            t_half.check_random_sums_and_means(rng, dtype, case.h, case.heads)
        else:
            views = Views(case, which)
            monkeypatch.setattr(t_att, "call_spmm_values", through(t_att.call_spmm_values, views, ("X",), "out", lambda a: (a["n"], a["h"], a["dtype"])))
            for graph in GRAPH_NAMES:
                t_att.check_spmm_values_parity(rng, dtype, case.h, graph, head_counts=(case.heads,), ldxs=(case.h,))
        monkeypatch.undo()


@pytest.mark.parametrize("case", cases("walker"))
def test_gat_aggregate(rng, monkeypatch, case):
    says(_lib.SHAPE_GAT_AGGREGATE, case)
    dtype, h, heads = TORCH[case.dtype], case.h, case.heads
    for which in turns(case, ("X", "out")):
        views = Views(case, which)
        if is_half(case):
            monkeypatch.setattr(t_half, "strides", lambda h: (h,))
            monkeypatch.setattr(t_half, "call_gat", through(t_half.call_gat, views, ("X",), "out", HALF_OUT))
            t_half.test_gat_aggregate_meets_the_bound(rng, dtype, h, heads)
        else:
            monkeypatch.setattr(t_gat, "call_gat", through(t_gat.call_gat, views, ("X",), "out", lambda a: (a["n"], a["h"], a["dtype"])))
            for graph in GRAPH_NAMES:
                n, m, rowptr, col = t_att.GRAPHS[graph](rng)
                rp, cc = t_att.dev_csr(rowptr, col)
                a_dst = torch.from_numpy(rng.uniform(-4, 4, size=(n, heads))).to(DEV, dtype)
                a_src = torch.from_numpy(rng.uniform(-4, 4, size=(m, heads))).to(DEV, dtype)
                X = torch.from_numpy(rng.uniform(-1, 1, size=(m, h))).to(DEV, dtype)
                t_gat.check_against_reference(f"{graph} {dtype} h={h} heads={heads} {case.mis} {which}", dtype, n, rowptr, col, rp, cc, a_dst, a_src,
                                              heads, 0.2, X, h)
        monkeypatch.undo()


@pytest.mark.parametrize("case", cases("mean"))
def test_mean(rng, monkeypatch, case):
    says(_lib.SHAPE_SPMM_REDUCE, case)
    dtype = TORCH[case.dtype]
    for which in turns(case, ("X", "out")):
        views = Views(case, which)
        if is_half(case):
            monkeypatch.setattr(t_half, "strides", lambda h: (h,))
            monkeypatch.setattr(t_half, "call_values", through(t_half.call_values, views, ("X",), "out", HALF_OUT))
            t_half.check_random_sums_and_means(rng, dtype, case.h, 1)
        else:
            monkeypatch.setattr(t_red, "strides_of", lambda graph, h, dtype: (h,))
            monkeypatch.setattr(t_red, "call_reduce", through(t_red.call_reduce, views, ("X",), "out", lambda a: (a["n"], a["h"], a["dtype"])))
            for graph in GRAPH_NAMES:
                t_red.check_mean_parity(rng, dtype, case.h, graph)
        monkeypatch.undo()


@pytest.mark.parametrize("case", cases("maxmin"))
def test_max_min_with_arg(rng, monkeypatch, case):
    """every class in FLT32, in DBL64 and in an integer type: out and arg bit-equal to the shim, most rows decided by the tie rule"""
    says(_lib.SHAPE_SPMM_REDUCE, case)
    for which in turns(case, ("X", "out")):
        views = Views(case, which)
        monkeypatch.setattr(t_red, "strides_of", lambda graph, h, dtype: (h,))
        monkeypatch.setattr(t_red, "call_reduce", through(t_red.call_reduce, views, ("X",), "out", lambda a: (a["n"], a["h"], a["dtype"])))
        for graph in GRAPH_NAMES:
            t_red.check_max_min_with_ties(rng, TORCH[case.dtype], case.h, graph)
        monkeypatch.undo()


@pytest.mark.parametrize("case", cases("reduce_bwd"))
def test_max_backward(rng, case):
    says(_lib.SHAPE_SPMM_REDUCE_BACKWARD, case)
    for which in turns(case, ("G", "dX")):
        views = Views(case, which)
        for graph in GRAPH_NAMES:
            t_red.check_backward_parity(rng, TORCH[case.dtype], case.h, graph, view=views)
            views.check()


# ---- the head-wise kernels ----
def head_operands(rng, dtype, rows, h):
    """the distributions of the owning files' parity tests (16-bit: magnitudes in [0.5, 2) with random signs for the summed operand)"""
    a = torch.from_numpy(rng.uniform(-2, 2, size=(rows[0], h))).to(DEV, dtype)
    b = torch.from_numpy(rng.uniform(-2, 2, size=(rows[1], h))).to(DEV, dtype)
    if dtype in t_half.HALF:
        c = torch.from_numpy(rng.uniform(0.5, 2, size=(rows[1], h)) * rng.choice([-1.0, 1.0], size=(rows[1], h))).to(DEV, dtype)
    else:
        c = torch.from_numpy(rng.uniform(-1, 1, size=(rows[1], h))).to(DEV, dtype)
    return a, b, c


@pytest.mark.parametrize("case", cases("head"))
def test_sparse_attention(rng, monkeypatch, case):
    says(_lib.SHAPE_SPARSE_ATTENTION, case)
    dtype, h, heads = TORCH[case.dtype], case.h, case.heads
    scale = (h // heads) ** -0.5
    for graph in GRAPH_NAMES:
        n, m, rowptr, col = t_sa.GRAPHS[graph](rng)
        rp, cc = t_att.dev_csr(rowptr, col)
        Q, K, V = head_operands(rng, dtype, (n, m), h)
        reference = t_sa.sa_reference_dev(dtype, n, rowptr, col, Q, K, V, h, heads, scale)
        for which in turns(case, ("Q", "K", "V", "out")):
            views = Views(case, which)
            monkeypatch.setattr(t_sa, "call_sa", through(t_sa.call_sa, views, ("Q", "K", "V"), "out", lambda a: (a["n"], a["h"], a["dtype"])))
            t_sa.check(f"{graph} {dtype} h={h} heads={heads} {case.mis} {which}", dtype, n, rowptr, rp, cc, Q, K, V, h, heads, scale, reference)
            monkeypatch.undo()


@pytest.mark.parametrize("case", cases("head"))
def test_gatv2_forward(rng, monkeypatch, case):
    says(_lib.SHAPE_GATV2_AGGREGATE, case)
    dtype, h, heads = TORCH[case.dtype], case.h, case.heads
    for graph in GRAPH_NAMES:
        n, m, rowptr, col = t_v2.GRAPHS[graph](rng)
        rp, cc = t_att.dev_csr(rowptr, col)
        Xd, _, Xs = head_operands(rng, dtype, (n, m), h)
        if dtype not in t_half.HALF:
            Xs = Xs * 2   # uniform in (-2, 2), as test_gatv2_forward_parity draws it
        att = t_v2.make_att(rng, h, heads, dtype)
        reference = t_v2.reference_dev(dtype, n, rowptr, col, Xd, Xs, att, h, heads)
        for which in turns(case, ("Xd", "Xs", "out")):
            views = Views(case, which)
            monkeypatch.setattr(t_v2, "call_fwd", through(t_v2.call_fwd, views, ("Xd", "Xs"), "out", lambda a: (a["n"], a["h"], a["dtype"])))
            t_v2.check_fwd(f"{graph} {dtype} h={h} heads={heads} {case.mis} {which}", dtype, n, rowptr, rp, cc, Xd, Xs, att, h, heads, reference)
            monkeypatch.undo()


def gatv2_backward_operands(dtype, n, m, h, heads):
    """test_gatv2_backward_parity's: randn, att randn / sqrt(hd)"""
    torch.manual_seed(21)
    Xd, Xs, G = (torch.randn(r, h, dtype=dtype, device=DEV) for r in (n, m, n))
    return Xd, Xs, G, torch.randn(h, dtype=dtype, device=DEV) * (h // heads) ** -0.5


@pytest.mark.parametrize("case", cases("head", lambda c: not is_half(c)))
def test_gatv2_backward(rng, monkeypatch, case):
    """both directions against float64 autograd, datt included"""
    says(_lib.SHAPE_GATV2_BACKWARD, case)
    dtype, h, heads = TORCH[case.dtype], case.h, case.heads
    for graph in GRAPH_NAMES:
        n, m, rowptr, col = t_v2.GRAPHS[graph](rng)
        g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
        gt, _ = g.transposed()
        Xd, Xs, G, att = gatv2_backward_operands(dtype, n, m, h, heads)
        want, lse, delta = t_v2.backward_case(dtype, n, m, rowptr, col, Xd, Xs, att, G, h, heads)
        for which in turns(case, ("own", "oth", "G", "d_own")):
            views = Views(case, which)
            monkeypatch.setattr(t_v2, "call_bwd", through(t_v2.call_bwd, views, ("own", "oth", "G"), "d_own", lambda a: (a["nrows"], a["h"], a["dtype"])))
            t_v2.check_bwd(f"{graph} {dtype} h={h} heads={heads} {case.mis} {which}", dtype, g, gt, Xd, Xs, att, G, lse, delta, h, heads, want)
            monkeypatch.undo()


@pytest.mark.parametrize("case", cases("head", is_half))
def test_gatv2_backward_16_bit(rng, monkeypatch, case):
    """BF16 / FLT16 x_dst, x_src, G and gradients, float32 att, lse, delta and datt: the forward and both directions of the backward
    through the C ABI as the autograd wrapper composes them (delta from the stored, once-rounded out), under the bound that
    test_gatv2_gpu.test_gradients_in_bfloat16 derives, against float64 on the CPU; on the `small` graph"""
    says(_lib.SHAPE_GATV2_BACKWARD, case)
    dtype, h, heads = TORCH[case.dtype], case.h, case.heads
    n, m, rowptr, col = t_v2.GRAPHS["small"](rng)

    def run(g, Xd, Xs, att, G, h, heads):
        gt, _ = g.transposed()
        Xd, Xs, att, G = (t.to(DEV) for t in (Xd, Xs, att, G))
        rp, cc = t_att.dev_csr(rowptr, col)
        out, lse = t_v2.call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads)
        delta = (G.float() * out.float()).view(n, heads, h // heads).sum(-1).contiguous()
        dxd, datt = t_v2.call_bwd(dtype, False, n, rp, cc, Xd, Xs, att, h, heads, G, lse, delta)
        dxs, none = t_v2.call_bwd(dtype, True, m, gt.rowptr.to(DEV, torch.int32), gt.col.to(DEV, torch.int32), Xs, Xd, att, h, heads, G, lse, delta)
        again, datt2 = t_v2.call_bwd(dtype, False, n, rp, cc, Xd, Xs, att, h, heads, G, lse, delta)
        assert none is None and torch.equal(dxd, again) and torch.equal(datt, datt2), "two launches differ"
        return dxd, dxs, datt

    for which in turns(case, ("own", "oth", "G", "d_own")):
        views = Views(case, which)
        monkeypatch.setattr(t_v2, "call_bwd", through(t_v2.call_bwd, views, ("own", "oth", "G"), "d_own", lambda a: (a["nrows"], a["h"], a["dtype"])))
        t_v2.check_gradients_16_bit(dtype, n, m, rowptr, col, h, heads, run=run)
        monkeypatch.undo()


# ---- sddmm and edge_softmax ----
@pytest.mark.parametrize("case", cases("sddmm"))
def test_sddmm(rng, case):
    says(_lib.SHAPE_SDDMM, case)
    dtype, h = TORCH[case.dtype], case.h
    for graph in GRAPH_NAMES:
        n, m, rowptr, col = t_att.GRAPHS[graph](rng)
        rp, cc = t_att.dev_csr(rowptr, col)
        G = torch.from_numpy(rng.standard_normal((n, h))).to(DEV, dtype)
        X = torch.from_numpy(rng.standard_normal((m, h))).to(DEV, dtype)
        for which in turns(case, ("G", "X")):
            views = Views(case, which)
            t_edges.check_sddmm(f"{graph} {dtype} h={h} {case.mis} {which}", dtype, n, rp, cc, views("G", G), views("X", X), h)


@pytest.mark.parametrize("case", cases("edge_softmax"))
def test_edge_softmax_forward_and_backward(rng, monkeypatch, case):
    """a, b and out one element into their buffers while heads % V == 0: the pointer half of the vec condition, forward and backward"""
    says(_lib.SHAPE_EDGE_SOFTMAX, case)
    for which in turns(case, ("a", "b", "out")):
        views = Views(case, which, contiguous=True)
        monkeypatch.setattr(t_att, "call_softmax", through(t_att.call_softmax, views, ("a", "b"), "out", lambda a: (a["nnz"], a["heads"], a["dtype"])))
        for graph in GRAPH_NAMES:
            t_att.test_edge_softmax_parity(rng, TORCH[case.dtype], case.heads, graph)
        monkeypatch.undo()


# ---- the second launch of the head-wise kernels: 65 537 chunks of one head ----
def two_launch_case():
    (case,) = [c for c in ls.TABLES["head"] if c.heads == 65537]
    assert (case.h, case.heads) == ls.TWO_LAUNCHES and dict(zip(_lib.SHAPE_FIELDS, case.shape))["launches"] == 2
    return case


def test_two_launches_sparse_attention_and_gatv2_forward():
    """hd = 33 scalar, heads = 65 537: one head per block, blockIdx.y chunks 0 .. 65534 in the first launch and head0 = 65535 in the
    second; compared with the float64 reference like every other case (test_launch_shapes_cpu.py: a reference with the second launch's
    heads zeroed violates the bound)"""
    case = two_launch_case()
    dtype, h, heads = torch.float32, case.h, case.heads
    for kind in (_lib.SHAPE_SPARSE_ATTENTION, _lib.SHAPE_GATV2_AGGREGATE):
        says(kind, case)
    n, m, rowptr, col = ls.two_launch_graph()
    rp, cc = t_att.dev_csr(rowptr, col)
    Q, K, V, att = (torch.from_numpy(t).to(DEV) for t in ls.two_launch_operands())
    scale = 33 ** -0.5
    t_sa.check("two launches", dtype, n, rowptr, rp, cc, Q, K, V, h, heads, scale, t_sa.sa_reference_dev(dtype, n, rowptr, col, Q, K, V, h, heads, scale))
    t_v2.check_fwd("two launches", dtype, n, rowptr, rp, cc, Q, K, att, h, heads, t_v2.reference_dev(dtype, n, rowptr, col, Q, K, att, h, heads))


def test_two_launches_gatv2_backward():
    """both directions, against float64 autograd with test_gatv2_backward_parity's tolerance"""
    case = two_launch_case()
    says(_lib.SHAPE_GATV2_BACKWARD, case)
    dtype, h, heads = torch.float32, case.h, case.heads
    n, m, rowptr, col = ls.two_launch_graph()
    g = EdgeGraph(torch.from_numpy(rowptr), torch.from_numpy(col), (n, m))
    gt, _ = g.transposed()
    Xd, Xs, G, att = gatv2_backward_operands(dtype, n, m, h, heads)
    want, lse, delta = t_v2.backward_case(dtype, n, m, rowptr, col, Xd, Xs, att, G, h, heads)
    t_v2.check_bwd("two launches", dtype, g, gt, Xd, Xs, att, G, lse, delta, h, heads, want)


# ---- the reduction depth of the GATv2 datt ----
@pytest.mark.parametrize("runs,h,heads,dtype", [c + (d,) for c in ls.DATT_CASES for d in (torch.float32, torch.float64) if (c[0], d) != (65537, torch.float32)])
def test_gatv2_datt_reduction_depth(runs, h, heads, dtype):
    """256 runs: one level, the boundary n > GV2_RED; 257: two levels, the second block holds one partial; 513: two levels with a ragged
    last block; 65 537: three levels (the depth of the Reddit-shaped graph), h = heads = 1.  pygim_gatv2_backward, not transposed, datt
    requested, against the float64 closed form of launch_shapes.datt_reference under test_gatv2_backward_parity's bound for datt
    (GRAD_TOL: |got - ref| <= atol + rtol |ref|).  Operands of one sign keep every run's part of datt away from a cancellation:
    test_launch_shapes_cpu.py shows on the reference alone that a result without any one run violates the bound, by a factor of 15
    (FLT32, 513 runs) to 1 400 (DBL64, the single entry of run 65 536) at the least.

    Three levels run in DBL64 only (the kernels are one template).  The FLT32 bound, rtol = atol = 1e-4, does not follow from the depth
    of the summation there, and a bound that does cannot fail: a partial is up to 512 sequential float32 adds and each of the three
    levels up to 256 more, so the sum is off by up to (512 + 3 * 256) * 2^-24 = 7.6e-5 of sum |terms|; the terms have both signs (ds
    sums to zero over a row), sum |terms| = 30.0 against datt = 4.886, so that is 2.3e-3 absolute against the 5.9e-4 the existing
    bound allows -- and against the 7.5e-5 a whole run contributes.  The existing bound is not widened from what the kernel returns,
    and no test is kept that could not tell a lost run."""
    assert ls.datt_levels(runs) == {256: 1, 257: 2, 513: 2, 65537: 3}[runs]
    n, m, rowptr, col = ls.datt_graph(runs, DEV)
    Xd, Xs, G, att = (t.to(DEV) for t in ls.datt_operands(runs, h, heads, dtype))
    ref, lse, delta, _ = ls.datt_reference(rowptr, col, Xd, Xs, att, G, h, heads, slope=t_v2.SLOPE)
    ct = t_v2.compute_type(dtype)
    args = (dtype, False, n, rowptr, col, Xd, Xs, att, h, heads, G, lse.to(ct).contiguous(), delta.to(ct).contiguous())
    d1, datt = t_v2.call_bwd(*args)
    d2, datt2 = t_v2.call_bwd(*args)
    assert not torch.isnan(datt).any() and not torch.isnan(d1).any() and torch.equal(datt, datt2) and torch.equal(d1, d2), "two launches differ"
    if runs < 65537:   # the closed form against the reference of test_gatv2_backward_parity (float64 autograd), so the two cannot drift
        want, lse_p, delta_p = t_v2.backward_case(dtype, n, m, rowptr.cpu().numpy(), col.cpu().numpy(), Xd, Xs, att, G, h, heads)
        assert torch.allclose(ref, want[2], rtol=1e-11, atol=0) and torch.allclose(lse, lse_p.double(), rtol=1e-6) and \
            torch.allclose(delta, delta_p.double(), rtol=1e-5, atol=1e-7)
    tol = t_v2.GRAD_TOL[dtype]
    err = (datt.double() - ref).abs()
    print(f"datt runs={runs} levels={ls.datt_levels(runs)} {dtype}: max err / (atol + rtol |ref|) = "
          f"{(err / (tol['atol'] + tol['rtol'] * ref.abs())).max().item():.3e}, |ref| = {ref.abs().min().item():.3e} .. {ref.abs().max().item():.3e}")
    assert torch.allclose(datt.double(), ref, **tol)


# ---- rows that one launch cannot hold ----
def test_too_wide_rows_are_rejected_before_any_launch():
    """h > 65535 * 128: PYGIM_ERR_INVALID from the size check, before any pointer is looked at (so the pointers here are a few bytes)"""
    h = _lib.GATHER_MAX_H + 1
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    p, big = t.data_ptr(), 1 << 40
    st = torch.cuda.current_stream().cuda_stream
    calls = {
        "spmm_values": lambda: _lib.spmm_values(_lib.FLT32, 1, p, p, 1, p, 1, p, h, h, p, h, p, big, st),
        "gat_aggregate": lambda: _lib.gat_aggregate(_lib.FLT32, 1, p, p, 1, p, p, 1, 0.2, p, h, h, p, h, 0, p, big, st),
        "spmm_reduce": lambda: _lib.spmm_reduce(_lib.FLT32, _lib.REDUCE_MAX, 1, p, p, 1, 0, p, h, h, p, h, 0, p, big, st),
        "spmm_reduce_backward": lambda: _lib.spmm_reduce_backward(_lib.FLT32, 1, p, p, p, 1, 0, p, h, p, h, p, h, st),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.PygimError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID and "sizes" in str(e.value), name
    torch.cuda.synchronize()
    assert (t == 0).all()
