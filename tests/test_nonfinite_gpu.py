"""NaN, +-inf and -0.0 through the gather family on the GPU.  The reference is float64 torch on the device, from the operands as stored.
The rule of every test: the set of non-finite outputs, and for infinities their sign, equals the reference's exactly; every other output
meets the bound of the file that tests the same entry point on finite inputs (imported from there, not restated).

Masked scores.  A score of -inf is how an attention mask is written: its probability is exactly 0 and the softmax runs over the rest, so
the reference of a partially masked row is the reference on the graph WITHOUT the masked entries (run_edges.pruned_csr), with that
graph's magnitudes and bounds.  A (row, head) whose scores are all -inf is 0 / 0: NaN across the head's features, lse = -inf, as
torch.softmax and torch.logsumexp give."""
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
from pygim_amd import _lib
from pygim_amd.attention import EdgeGraph, edge_softmax, gat_aggregate, spmm_values
from test_gat_fused_cpu import ref_gat_aggregate

pytestmark = pytest.mark.gpu

DEV = "cuda"
CODE = t_sa.CODE
HALF = (torch.bfloat16, torch.float16)
TINY32 = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    yield
    _lib.release()


def compute_type(dtype):
    return torch.float32 if dtype in HALF else dtype


def get_graph(name, rng):
    if name == "small":
        return t_att.small_graph(rng)
    return run_edges.graph(name)


def row_of(n, rowptr):
    return torch.repeat_interleave(torch.arange(n, device=DEV), torch.diff(torch.from_numpy(np.asarray(rowptr)).long().to(DEV)))


def same_nonfinite(got, want, tag):
    """the NaNs and the infinities of each sign stand where the reference (rounded to the type of `got`) has them -> where both are finite"""
    w = want.to(got.dtype)
    for name, f in (("NaN", torch.isnan), ("+inf", torch.isposinf), ("-inf", torch.isneginf)):
        a, b = f(got), f(w)
        assert torch.equal(a, b), f"{tag}: {name} at {int((a & ~b).sum())} places the reference has none, missing at {int((~a & b).sum())}"
    return torch.isfinite(w)


# ---- 1. containment in the sums -------------------------------------------------------------------------------------------------

def call_sum(dtype, mean, n, rp, cc, val, heads, X, h):
    nnz = cc.numel()
    out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if mean:
        ws = torch.empty(max(_lib.spmm_reduce_workspace(CODE[dtype], _lib.REDUCE_MEAN, n, nnz, h), 16), dtype=torch.uint8, device=DEV)
        _lib.spmm_reduce(CODE[dtype], _lib.REDUCE_MEAN, n, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), X.data_ptr(), X.stride(0), h, out.data_ptr(), h, 0,
                         ws.data_ptr(), ws.numel(), st)
    else:
        ws = torch.empty(max(_lib.spmm_values_workspace(CODE[dtype], n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
        _lib.spmm_values(CODE[dtype], n, rp.data_ptr(), cc.data_ptr(), nnz, val.data_ptr(), heads, X.data_ptr(), X.stride(0), h, out.data_ptr(), h,
                         ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h", [8, 32, 256, 520])
@pytest.mark.parametrize("graph", ["edges", "small"])
def test_sums_contain_their_non_finite_inputs(rng, dtype, h, graph):
    """spmm_values (heads 1 and 4) and the mean.  A NaN at X[c0, f0], +inf at X[c1, f1], -inf at X[c2, f1] and a NaN value on one entry: out is
    non-finite exactly where the float64 reference is (inf - inf = NaN where both meet), and EVERY other element has the bits of the call
    without the four specials -- a lane that multiplied something it should have skipped by zero would show here.  The column c3 holds
    60 000 at feature f2 and its entries the value 2 (in both calls): those sums are finite in float32 and lie beyond 65504, so FLT16
    stores +-inf where the rounded reference has it, and BF16 / FLT32 / DBL64 store the number."""
    n, m, rowptr, col = get_graph(graph, rng)
    rp, cc = t_att.dev_csr(rowptr, col)
    nnz = len(col)
    ct = compute_type(dtype)
    cnt = torch.from_numpy(np.maximum(np.diff(rowptr), 1)).to(DEV).double().unsqueeze(1)
    c0, c1, c2, c3 = (int(c) for c in rng.choice(m, size=4, replace=False))
    f0, f1, f2 = 1, h - 1, h // 2
    e_nan = int(rowptr[np.flatnonzero(np.diff(rowptr) >= 3)[2]]) + 1            # the second entry of some row
    X0 = torch.from_numpy(rng.uniform(-1, 1, size=(m, h)).astype(np.float32)).to(DEV, dtype)
    X0[c3, f2] = 60000.0
    X1 = X0.clone()
    X1[c0, f0], X1[c1, f1], X1[c2, f1] = float("nan"), float("inf"), -float("inf")
    for heads in (1, 4):
        v0 = torch.from_numpy(rng.uniform(0.5, 2, size=(nnz, heads)) * rng.choice([-1.0, 1.0], size=(nnz, heads))).to(DEV, ct)
        v0[cc.long() == c3] = 2.0
        v1 = v0.clone()
        v1[e_nan, heads - 1] = float("nan")
        for mean in ((False, True) if heads == 1 else (False,)):
            tag = f"{'mean' if mean else 'spmm_values'} {graph} {dtype} h={h} heads={heads}"
            clean = call_sum(dtype, mean, n, rp, cc, v0, heads, X0, h)
            out = call_sum(dtype, mean, n, rp, cc, v1, heads, X1, h)
            ref, _ = t_att.spmm_reference(n, rowptr, col, v1, heads, X1, h)
            ref0, mag0 = t_att.spmm_reference(n, rowptr, col, v0, heads, X0, h)
            if mean:
                ref, ref0, mag0 = ref / cnt, ref0 / cnt, mag0 / cnt
            assert torch.isnan(ref).any() and torch.isinf(ref).any(), "the specials reach no row of this graph"
            fin = same_nonfinite(out, ref, tag)
            assert torch.equal(out[fin], clean[fin]), f"{tag}: a special input changed an output it has no part in"
            fin0 = same_nonfinite(clean, ref0, tag + " (no specials)")
            if dtype == torch.float16 and not mean:
                assert torch.isinf(clean).any() and not torch.isinf(ref0).any(), "no FLT16 sum went beyond 65504"
            # the bounds of test_attention_gpu (sum), test_reduce_gpu (mean) and test_half_gpu (16-bit), on the call without the specials
            u = t_half.U.get(dtype, torch.finfo(dtype).eps if mean else 0.0)
            err = (clean.double() - ref0).abs()[fin0]
            bound = (u * ref0.abs() + t_att.TOL[ct] * mag0 + (t_half.TINY if dtype in HALF else 0.0))[fin0]
            print(f"{tag}: {int((~fin).sum())} non-finite outputs, max err / bound of the rest = {(err / bound.clamp_min(1e-300)).max().item():.3e}")
            assert torch.all(err <= bound)
            assert torch.equal(out[fin], call_sum(dtype, mean, n, rp, cc, v1, heads, X1, h)[fin]), "two launches differ"


# ---- 2. the rules of max / min ---------------------------------------------------------------------------------------------------

def best_reference(n, rowptr, col, val, X, h, reduce):
    """the documented rule, on the products as the type forms them (one IEEE multiply): among the products that are numbers the best
    one, among equal ones (-0.0 == +0.0) the lowest entry; no number in the row: NaN and -1; no entry: 0 and -1"""
    row = row_of(n, rowptr)
    msg = X[:, :h][torch.from_numpy(np.asarray(col)).long().to(DEV)]
    if val is not None:
        msg = val.unsqueeze(1) * msg
    nnz = msg.size(0)
    number = ~torch.isnan(msg)
    worst = -float("inf") if reduce == "max" else float("inf")
    key = torch.where(number, msg.double(), torch.full_like(msg, worst, dtype=torch.float64))
    best = torch.full((n, h), worst, dtype=torch.float64, device=DEV).index_reduce_(0, row, key, "amax" if reduce == "max" else "amin")
    none = float(2 ** 31 - 1)                                   # entry indices as float64: exact, and index_reduce_ takes them on every device
    entry = torch.arange(nnz, device=DEV, dtype=torch.float64).unsqueeze(1).expand(nnz, h)
    cand = torch.where(number & (key == best[row]), entry, torch.full_like(entry, none))
    arg = torch.full((n, h), none, dtype=torch.float64, device=DEV).index_reduce_(0, row, cand, "amin").long()
    won = arg < 2 ** 31 - 1
    out = torch.gather(msg, 0, arg.clamp_max(nnz - 1))
    empty = torch.from_numpy(np.diff(np.asarray(rowptr)) == 0).to(DEV).unsqueeze(1)
    out = torch.where(won, out, torch.full_like(out, float("nan")))
    out = torch.where(empty, torch.zeros_like(out), out)
    return out, torch.where(won, arg, torch.full_like(arg, -1)).to(torch.int32)


def assert_bits(got, want, tag):
    """equal as floats, NaN where NaN, and the same sign bit on every number (so -0.0 is not +0.0)"""
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{tag}: NaN pattern"
    ok = ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok]) and torch.equal(torch.signbit(got[ok]), torch.signbit(want[ok])), tag


def special_values(rng, dtype):
    """per-entry values on `edges` that make NaN products wherever a row can hide them from a fold; X has no zero, so a value's NaN,
    infinity or signed zero is the product's"""
    n, m, rowptr, col = run_edges.graph("edges")
    rp = rowptr.astype(np.int64)
    nan, inf = float("nan"), float("inf")
    v = rng.choice([0.5, 1.0, 2.0], size=len(col))
    e = np.arange(len(col))
    v[(e < rp[4]) & (e % 8 == 3)] = nan                       # row 3 = run 0: one lane group in eight (h = 32 in FLT32) sees only NaN
    v[run_edges.RUN:2 * run_edges.RUN] = nan                  # row 5: its whole first run; the number comes from the next run's slot
    v[rp[6]] = nan                                            # row 6: first in the row
    v[rp[9] - 1] = nan                                        # row 8: last in the row
    v[rp[9] + 251:rp[9] + 351] = nan                          # row 9: in the middle
    v[7 * run_edges.RUN - 1:8 * run_edges.RUN + 1] = nan      # row 11: a whole run and the entries on the far side of both its boundaries
    v[rp[13]:rp[14]] = nan                                    # row 13 (one entry) and row 14 (63): every product NaN
    v[rp[14]:rp[15]] = nan
    v[rp[15] + 5], v[rp[15] + 40] = inf, -inf                 # rows 15, 16: infinities win or lose as numbers
    v[rp[16] + 64], v[rp[16] + 1] = inf, inf
    v[rp[19]:rp[20]] = [-0.0, 0.0, 0.0, -0.0, 0.0, -0.0, 0.0]  # rows 19, 21: nothing but zeros of both signs
    v[rp[21]:rp[22]] = rng.choice([0.0, -0.0], size=int(rp[22] - rp[21]))
    sel = (e >= rp[20]) & (e < rp[21]) & (e % 8 != 5)
    v[sel] = nan                                              # row 20: the numbers stand in ONE lane group
    all_nan = (13, 14)
    return n, m, rowptr, col, torch.from_numpy(v).to(DEV, dtype), all_nan


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h", [8, 32, 256])
def test_max_min_rules_for_nan_inf_and_signed_zero(rng, dtype, h):
    n, m, rowptr, col, val, all_nan = special_values(rng, dtype)
    rp, cc = t_att.dev_csr(rowptr, col)
    nnz = len(col)
    X = torch.from_numpy(rng.choice([-2.0, -1.0, 1.0, 2.0], size=(m, h))).to(DEV, dtype)
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    g = EdgeGraph(torch.from_numpy(np.array(rowptr)), torch.from_numpy(np.array(col)), (n, m))
    gt, perm = g.transposed()
    perm32 = perm.to(torch.int32)
    for reduce in ("max", "min"):
        tag = f"{reduce} {dtype} h={h}"
        want, want_arg = best_reference(n, rowptr, col, val, X, h, reduce)
        out, arg = t_red.call_reduce(dtype, t_red.OP[reduce], n, rp, cc, val, X, h, True)
        assert_bits(out, want, tag)
        assert torch.equal(arg, want_arg), f"arg of {tag}"
        # what the reference must show for the test to mean something
        for r in all_nan:
            assert torch.isnan(out[r]).all() and (arg[r] == -1).all(), f"{tag}: a row of NaN products stores NaN and arg -1"
        rest = torch.ones(n, dtype=torch.bool, device=DEV)
        rest[list(all_nan)] = False
        assert not torch.isnan(out[rest]).any() and (arg[rest & ~empty] >= 0).all() and (arg[empty] == -1).all(), f"{tag}: a number replaces a NaN"
        assert (out[empty] == 0).all()
        for r in (19, 21):
            first = int(rowptr[r])
            assert (arg[r] == first).all() and (out[r] == 0).all(), f"{tag}: among -0.0 and +0.0 the lower entry wins"
            assert torch.equal(torch.signbit(out[r]), torch.signbit(val[first] * X[int(col[first])])), f"{tag}: out carries the winner's sign bit"
        far = torch.isposinf(out[15:17]) if reduce == "max" else torch.isneginf(out[15:17])
        assert far.any(), f"{tag}: an infinity of the right sign wins as a number"
        out2, arg2 = t_red.call_reduce(dtype, t_red.OP[reduce], n, rp, cc, val, X, h, True)
        assert_bits(out2, out, tag + " second launch")
        assert torch.equal(arg, arg2)
        bare, _ = t_red.call_reduce(dtype, t_red.OP[reduce], n, rp, cc, val, X, h, False)
        assert_bits(bare, out, tag + " without arg")
        # the backward on these args: an entry that did not win passes nothing on, whatever its value is; rows with arg -1 give nothing
        G = torch.from_numpy(rng.normal(0, 1, size=(n, h))).to(DEV, dtype)
        dX = torch.full((m, h), float("nan"), dtype=dtype, device=DEV)
        _lib.spmm_reduce_backward(CODE[dtype], m, gt.rowptr.data_ptr(), gt.col.data_ptr(), perm32.data_ptr(), nnz, val.data_ptr(), G.data_ptr(), h,
                                  arg.data_ptr(), h, dX.data_ptr(), h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        row = g.row.long()
        entry = torch.arange(nnz, device=DEV).unsqueeze(1)
        contrib = torch.where(arg[row].long() == entry, G[row].double() * val.double().unsqueeze(1), 0.0)
        ref = torch.zeros(m, h, dtype=torch.float64, device=DEV).index_add_(0, g.col.long(), contrib)
        mag = torch.zeros(m, h, dtype=torch.float64, device=DEV).index_add_(0, g.col.long(), contrib.abs())
        fin = same_nonfinite(dX, ref, tag + " backward")    # +-inf where an infinite value won; a NaN value never won, so it reaches nothing
        assert fin.sum() > fin.numel() // 2
        assert torch.all((dX.double() - ref).abs()[fin] <= t_red.TOL[dtype] * mag[fin])


@pytest.mark.parametrize("dtype", [torch.int8, torch.int16, torch.int32, torch.int64])
def test_integer_rows_of_the_far_end_return_their_first_entry(dtype):
    """every product is the type's minimum (max) or maximum (min), the value a row starts from: the first entry still wins, arg is not -1"""
    n, m, rowptr, col = run_edges.graph("edges")
    rp, cc = t_att.dev_csr(rowptr, col)
    first = torch.from_numpy(np.where(np.diff(rowptr) > 0, rowptr[:-1], -1).astype(np.int32)).to(DEV).unsqueeze(1)
    empty = first < 0
    info = torch.iinfo(dtype)
    for h in (8, 32):
        for reduce, far in (("max", info.min), ("min", info.max)):
            X = torch.full((m, h), far, dtype=dtype, device=DEV)
            out, arg = t_red.call_reduce(dtype, t_red.OP[reduce], n, rp, cc, None, X, h, True)
            assert torch.equal(out, torch.where(empty, 0, far).to(dtype).expand(n, h)), f"{reduce} {dtype} h={h}"
            assert torch.equal(arg, first.expand(n, h)), f"arg of {reduce} {dtype} h={h}"


# ---- 3. masked scores --------------------------------------------------------------------------------------------------------------

def edges_masked():
    n, m, rowptr, col = run_edges.graph("edges")
    mask = run_edges.masked_entries(rowptr)
    col_m = run_edges.masked_columns(col, mask)
    rowptr_p, col_p = run_edges.pruned_csr(rowptr, col_m, mask)
    return n, m, rowptr, col_m, mask, rowptr_p, col_p


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_edge_softmax_with_masked_scores(rng, dtype, heads):
    """-inf on the masked entries, in every head and in head 0 alone (heads are independent), forward and backward; then small with a
    random third of its entries masked"""
    for graph in ("edges", "small"):
        n, m, rowptr, col = get_graph(graph, rng)
        rp, _ = t_att.dev_csr(rowptr, col)
        nnz = len(col)
        row = row_of(n, rowptr)
        mask = torch.from_numpy(run_edges.masked_entries(rowptr) if graph == "edges" else rng.random(nnz) < 0.33).to(DEV)
        base = torch.from_numpy(rng.normal(0, 3, size=(nnz, heads))).to(DEV, dtype)
        for which in ("all heads", "head 0"):
            tag = f"edge_softmax {graph} {dtype} heads={heads}, {which} masked"
            s = base.clone()
            if which == "all heads":
                s[mask] = -float("inf")
            else:
                s[mask, 0] = -float("inf")
            P = t_att.call_softmax(dtype, n, rp, nnz, s, heads)
            ref = t_att.softmax_reference(n, row, s)
            left = torch.zeros(n, heads, device=DEV).index_add_(0, row, torch.isfinite(s).float())
            dead = (left == 0)[row]                                   # the entries of fully masked (row, head)s
            assert torch.equal(torch.isnan(ref), dead), "the reference: NaN exactly on the fully masked (row, head)s"
            if graph == "edges":
                rows = torch.unique(row[dead.any(1)]).tolist()
                assert tuple(rows) == run_edges.FULLY_MASKED_ROWS
            fin = same_nonfinite(P, ref, tag)
            assert (P[torch.isinf(s) & ~dead] == 0).all(), f"{tag}: a masked entry has probability exactly 0"
            err = (P.double() - ref).abs()[fin]
            print(f"{tag}: max rel err = {(err / ref[fin].clamp_min(TINY32)).max().item():.3e}")
            assert torch.all(err <= t_att.TOL[dtype] * ref[fin] + TINY32)
            if which == "head 0" and heads > 1:
                clean = t_att.call_softmax(dtype, n, rp, nnz, base, heads)
                assert torch.equal(P[:, 1:], clean[:, 1:]), f"{tag}: the other heads changed"
            P2 = t_att.call_softmax(dtype, n, rp, nnz, s, heads)
            assert torch.equal(P[fin], P2[fin]) and torch.equal(torch.isnan(P), torch.isnan(P2)), "two launches differ"
            # backward on the exact probabilities rounded to the type: 0 on the masked entries, NaN on the fully masked (row, head)s
            Pin = ref.to(dtype)
            dP = torch.from_numpy(rng.normal(0, 1, size=(nnz, heads))).to(DEV, dtype)
            got = t_att.call_softmax(dtype, n, rp, nnz, Pin, heads, dP)
            t = Pin.double() * dP.double()
            tsum = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, t)
            tabs = torch.zeros(n, heads, dtype=torch.float64, device=DEV).index_add_(0, row, t.abs())
            want = Pin.double() * (dP.double() - tsum[row])
            bfin = same_nonfinite(got, want, tag + " backward")
            assert torch.equal(~bfin, dead)
            assert (got[torch.isinf(s) & ~dead] == 0).all(), f"{tag}: a masked entry gets gradient exactly 0"
            assert torch.all((got.double() - want).abs()[bfin] <= (t_att.TOL[dtype] * (tabs[row] + t.abs()))[bfin])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_edge_softmax_with_one_inf_and_one_nan_score(rng, dtype):
    """+inf in (row 8, head 0) and NaN in (row 11, head 1), in a middle run of that row: those two (row, head)s are NaN throughout, as in
    the reference (inf - inf), and nothing else changes by a bit"""
    n, m, rowptr, col = run_edges.graph("edges")
    rp, _ = t_att.dev_csr(rowptr, col)
    nnz, heads = len(col), 4
    row = row_of(n, rowptr)
    base = torch.from_numpy(rng.normal(0, 3, size=(nnz, heads))).to(DEV, dtype)
    s = base.clone()
    s[int(rowptr[8]) + 17, 0] = float("inf")
    s[7 * run_edges.RUN + 100, 1] = float("nan")
    P = t_att.call_softmax(dtype, n, rp, nnz, s, heads)
    ref = t_att.softmax_reference(n, row, s)
    want_nan = torch.zeros(nnz, heads, dtype=torch.bool, device=DEV)
    want_nan[row == 8, 0] = True
    want_nan[row == 11, 1] = True
    assert torch.equal(torch.isnan(ref), want_nan)
    fin = same_nonfinite(P, ref, f"edge_softmax {dtype} +inf and NaN")
    assert torch.equal(P[fin], t_att.call_softmax(dtype, n, rp, nnz, base, heads)[fin])


def call_gat(dtype, n, rp, cc, a_dst, a_src, heads, slope, X, h):
    nnz = cc.numel()
    ws = torch.empty(max(_lib.gat_aggregate_workspace(CODE[dtype], n, nnz, h, heads), 16), dtype=torch.uint8, device=DEV)
    out = torch.full((n, h), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((n, heads), float("nan"), dtype=compute_type(dtype), device=DEV)
    _lib.gat_aggregate(CODE[dtype], n, rp.data_ptr(), cc.data_ptr(), nnz, a_dst.data_ptr(), a_src.data_ptr(), heads, slope, X.data_ptr(), X.stride(0), h,
                       out.data_ptr(), h, lse.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, lse


def compose(full, pruned, masked_heads, hd):
    """per head: the reference on the pruned graph where the head is masked, on the whole graph where it is not"""
    pick = torch.tensor(masked_heads, device=DEV)
    return tuple(torch.where(pick.repeat_interleave(hd if a.size(1) != len(masked_heads) else 1), b, a) for a, b in zip(full, pruned))


def check_masked(tag, out, lse, ref, bound, lse_ref, lbound, dead_rows, masked_heads, hd, rowptr):
    """dead_rows: the fully masked rows; they are NaN / -inf in the masked heads and ordinary in the others"""
    heads = len(masked_heads)
    dead = torch.zeros(lse.shape, dtype=torch.bool, device=DEV)
    for r in dead_rows:
        dead[r] = torch.tensor(masked_heads, device=DEV)
    dead_f = dead.repeat_interleave(hd, dim=1)
    assert torch.equal(torch.isnan(out), dead_f), f"{tag}: out is NaN exactly on the fully masked (row, head)s: {int(torch.isnan(out).sum())} NaN, " \
                                                  f"in rows {torch.unique(torch.nonzero(torch.isnan(out))[:, 0]).tolist()[:12]}"
    assert torch.equal(torch.isneginf(lse), dead) and torch.isfinite(lse[~dead]).all(), f"{tag}: lse is -inf exactly there"
    assert torch.isfinite(out[~dead_f]).all()
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert (out[empty] == 0).all() and (lse[empty] == 0).all()
    err = (out.double() - ref).abs()[~dead_f]
    lerr = (lse.double() - lse_ref).abs()[~dead]
    print(f"{tag}: max err / bound = {(err / bound[~dead_f].clamp_min(1e-300)).max().item():.3e}, lse = {(lerr / lbound[~dead]).max().item():.3e}")
    assert torch.all(err <= bound[~dead_f]) and torch.all(lerr <= lbound[~dead])
    assert heads == lse.size(1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("h", [8, 32, 256])
def test_gat_aggregate_with_masked_source_nodes(rng, dtype, h):
    """a_src[c] = -inf drops source node c from every neighbourhood.  The masked entries of `edges` point at the masked nodes (stored order
    is the contract: the columns of those rows are no longer sorted).  heads = 1; heads = 4 with every head masked and with head 0 alone."""
    n, m, rowptr, col_m, mask, rowptr_p, col_p = edges_masked()
    rp, cc = t_att.dev_csr(rowptr, col_m)
    ct = compute_type(dtype)
    tol = t_gat.TOL[ct]
    X = torch.from_numpy(rng.uniform(0.5, 2, size=(m, h)) * rng.choice([-1.0, 1.0], size=(m, h))).to(DEV, dtype)
    for heads, masked_heads in ((1, [True]), (4, [True] * 4), (4, [True, False, False, False])):
        hd = h // heads
        tag = f"gat_aggregate {dtype} h={h} heads={heads} masked heads={sum(masked_heads)}"
        a_dst = torch.from_numpy(rng.uniform(-4, 4, size=(n, heads))).to(DEV, ct)
        a_fin = torch.from_numpy(rng.uniform(-4, 4, size=(m, heads))).to(DEV, ct)
        a_src = a_fin.clone()
        a_src[torch.from_numpy(run_edges.MASKED_COLS).to(DEV).unsqueeze(1), torch.tensor(masked_heads, device=DEV).nonzero().squeeze(1)] = -float("inf")
        out, lse = call_gat(dtype, n, rp, cc, a_dst, a_src, heads, 0.2, X, h)
        full = t_gat.gat_reference_dev(n, rowptr, col_m, a_dst, a_fin, heads, 0.2, X, h)[:3]
        pruned = t_gat.gat_reference_dev(n, rowptr_p, col_p, a_dst, a_fin, heads, 0.2, X, h)[:3]
        ref, mag, lse_ref = compose(full, pruned, masked_heads, hd)
        bound = t_half.U.get(dtype, 0.0) * ref.abs() + tol * mag
        check_masked(tag, out, lse, ref, bound, lse_ref, tol * (1 + lse_ref.abs()), run_edges.FULLY_MASKED_ROWS, masked_heads, hd, rowptr)
        out2, lse2 = call_gat(dtype, n, rp, cc, a_dst, a_src, heads, 0.2, X, h)
        ok = ~torch.isnan(out)
        assert torch.equal(out[ok], out2[ok]) and torch.equal(torch.isnan(out), torch.isnan(out2)) and torch.equal(lse, lse2), "two launches differ"
        if not all(masked_heads):   # the unmasked heads: the bits of the call without a mask
            clean, lse_c = call_gat(dtype, n, rp, cc, a_dst, a_fin, heads, 0.2, X, h)
            assert torch.equal(out[:, hd:], clean[:, hd:]) and torch.equal(lse[:, 1:], lse_c[:, 1:]), f"{tag}: the other heads changed"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("h,heads", [(32, 4), (256, 1), (100, 4)])
def test_sparse_attention_with_masked_keys(rng, dtype, h, heads):
    """Q in (0.5, 2) and K[masked node] = -inf: every product is -inf, so the score is exactly -inf; V is finite.  Every head masked,
    and (heads > 1) head 0 alone."""
    n, m, rowptr, col_m, mask, rowptr_p, col_p = edges_masked()
    rp, cc = t_att.dev_csr(rowptr, col_m)
    hd = h // heads
    scale = hd ** -0.5
    Q = torch.from_numpy(rng.uniform(0.5, 2, size=(n, h))).to(DEV, dtype)
    K_fin = torch.from_numpy(rng.uniform(-2, 2, size=(m, h))).to(DEV, dtype)
    V = torch.from_numpy(rng.uniform(0.5, 2, size=(m, h)) * rng.choice([-1.0, 1.0], size=(m, h))).to(DEV, dtype)
    cases = [[True] * heads] + ([[True] + [False] * (heads - 1)] if heads > 1 else [])
    for masked_heads in cases:
        tag = f"sparse_attention {dtype} h={h} heads={heads} masked heads={sum(masked_heads)}"
        K = K_fin.clone()
        K[torch.from_numpy(run_edges.MASKED_COLS).to(DEV), :(h if all(masked_heads) else hd)] = -float("inf")
        out, lse = t_sa.call_sa(dtype, n, rp, cc, Q, K, V, h, heads, scale)
        full = t_sa.sa_reference_dev(dtype, n, rowptr, col_m, Q, K_fin, V, h, heads, scale)[:4]
        pruned = t_sa.sa_reference_dev(dtype, n, rowptr_p, col_p, Q, K_fin, V, h, heads, scale)[:4]
        ref, mag, lse_ref, delta = compose(full, pruned, masked_heads, hd)
        bound = t_sa.out_bound(dtype, ref, mag, delta, h, heads)
        lbound = 2 * t_sa.EPS[dtype] * (1 + lse_ref.abs()) + delta
        check_masked(tag, out, lse, ref, bound, lse_ref, lbound, run_edges.FULLY_MASKED_ROWS, masked_heads, hd, rowptr)
        out2, lse2 = t_sa.call_sa(dtype, n, rp, cc, Q, K, V, h, heads, scale)
        ok = ~torch.isnan(out)
        assert torch.equal(out[ok], out2[ok]) and torch.equal(torch.isnan(out), torch.isnan(out2)) and torch.equal(lse, lse2), "two launches differ"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,heads", [(32, 4), (256, 1), (100, 4)])
def test_gatv2_contains_a_nan_feature(rng, dtype, h, heads):
    """GATv2 has no masking interface (the gathered row is score and value at once); what holds is containment: a NaN at x_src[c0, f0]
    makes NaN the (row, head)s that have c0 among their entries and head(f0) as their head, as in the reference, and nothing else"""
    n, m, rowptr, col = get_graph("small", rng)
    rp, cc = t_att.dev_csr(rowptr, col)
    hd = h // heads
    Xd = torch.from_numpy(rng.uniform(-2, 2, size=(n, h))).to(DEV, dtype)
    Xs = torch.from_numpy(rng.uniform(-2, 2, size=(m, h))).to(DEV, dtype)
    att = t_v2.make_att(rng, h, heads, dtype)
    c0, f0 = int(col[len(col) // 2]), h - 1
    clean, lse_c = t_v2.call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads)
    Xs[c0, f0] = float("nan")
    out, lse = t_v2.call_fwd(dtype, n, rp, cc, Xd, Xs, att, h, heads)
    ref = t_v2.reference_dev(dtype, n, rowptr, col, Xd, Xs, att, h, heads)[0]
    hit = torch.zeros(n, dtype=torch.bool, device=DEV)
    hit[row_of(n, rowptr)[cc.long() == c0]] = True
    want = torch.zeros(n, h, dtype=torch.bool, device=DEV)
    want[:, (heads - 1) * hd:] = hit.unsqueeze(1)
    assert hit.any() and torch.equal(torch.isnan(ref), want), "the reference: NaN on the rows that gather c0, in the last head"
    fin = same_nonfinite(out, ref, f"gatv2 {dtype} h={h} heads={heads}")
    assert torch.equal(out[fin], clean[fin]), "a NaN feature changed an output it has no part in"
    assert torch.equal(torch.isnan(lse), want[:, ::hd]) and torch.equal(lse[~want[:, ::hd]], lse_c[~want[:, ::hd]])


# ---- the wrappers: forward and gradients with partially masked rows ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_wrappers_with_masked_source_nodes(rng, dtype):
    """gat_aggregate (what GATConv(fused=True) calls) against leaky_relu -> edge_softmax -> spmm_values (what fused=False calls), with
    a_src = -inf on the masked nodes and no fully masked row: the forwards agree, every gradient is finite, is zero on the masked nodes
    and entries, and matches float64 autograd of the per-entry reference on the CPU (the tolerances of the autograd tests of
    test_gat_fused_gpu.py)"""
    n, m, rowptr, col = run_edges.graph("edges")
    mask = run_edges.masked_entries(rowptr)
    for r in run_edges.FULLY_MASKED_ROWS:
        mask[rowptr[r]:rowptr[r + 1]] = False
    col_m = run_edges.masked_columns(col, mask)
    g = EdgeGraph(torch.from_numpy(np.array(rowptr)), torch.from_numpy(col_m), (n, m))
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-11)
    heads, h = 4, 32
    masked_nodes = torch.from_numpy(run_edges.MASKED_COLS)
    a_dst, a_src = torch.randn(n, heads, dtype=dtype), torch.randn(m, heads, dtype=dtype)
    a_src[masked_nodes] = -float("inf")
    X, G = torch.randn(m, h, dtype=dtype), torch.randn(n, h, dtype=dtype)

    def fused(ad, asrc, x):
        return gat_aggregate(g, ad, asrc, x, 0.2)

    def unfused(ad, asrc, x):
        score = torch.nn.functional.leaky_relu(ad.index_select(0, g.row.long()) + asrc.index_select(0, g.col.long()), 0.2)
        return spmm_values(g, edge_softmax(g, score), x, heads=heads)

    cpu = [t.clone().double().requires_grad_() for t in (a_dst, a_src, X)]
    ref = ref_gat_aggregate(rowptr, col_m, *cpu, 0.2, n)
    ref.backward(G.double())
    assert torch.isfinite(ref).all() and all(torch.isfinite(c.grad).all() for c in cpu), "the reference itself"
    outs = []
    for name, fn in (("fused", fused), ("unfused", unfused)):
        dev = [t.to(DEV).requires_grad_() for t in (a_dst, a_src, X)]
        out = fn(*dev)
        out.backward(G.to(DEV))
        outs.append(out.detach())
        assert torch.isfinite(out).all(), f"{name}: a masked neighbour made a row non-finite"
        assert torch.allclose(out.detach().cpu().double(), ref.detach(), **tol), name
        for gname, d, c in zip(("a_dst", "a_src", "X"), dev, cpu):
            assert torch.isfinite(d.grad).all(), f"{name}: d{gname} is not finite"
            print(f"{name} {dtype} d{gname}: max abs err = {(d.grad.cpu().double() - c.grad).abs().max().item():.3e}")
            assert torch.allclose(d.grad.cpu().double(), c.grad, **tol), f"{name}: d{gname}"
        assert (dev[1].grad[masked_nodes.to(DEV)] == 0).all() and (dev[2].grad[masked_nodes.to(DEV)] == 0).all(), f"{name}: a masked node got gradient"
    assert torch.allclose(outs[0], outs[1], **tol)
    # the probabilities themselves: exactly 0 on the masked entries, and so is their gradient
    sd = torch.randn(len(col_m), heads, dtype=dtype)
    sd[torch.from_numpy(mask)] = -float("inf")
    sd = sd.to(DEV).requires_grad_()
    P = edge_softmax(g, sd)
    P.backward(torch.randn(len(col_m), heads, dtype=dtype, device=DEV))
    mk = torch.from_numpy(mask).to(DEV)
    assert torch.isfinite(P).all() and (P[mk] == 0).all() and torch.isfinite(sd.grad).all() and (sd.grad[mk] == 0).all()
