"""A refactor of the entry-run gather kernels (row_gather_dev.hpp and its siblings: the shared fix-up preamble rg_cut_row and launch
dispatch rg_dispatch, and any later attempt to share the walk itself) must change no bit and cost no time: this build against the
parent commit's libpygim_hip.so, both loaded in one process (OtherBuild of exp_attention.py) and run on the same tensors.  JSON lines.
  --section bits: every gather that contains the walk, on the three hand-built graphs of tests/run_edges.py (edges, one-row,
    whole-batches: a row that is exactly one run, a row cut over four runs, one entry either side of a run boundary, empty rows on a
    boundary, a last run of one entry, batches that end on row ends), at one width per lane layout -- h = 3 (scalar, L < 64), 32 (16-byte
    pieces, several lane groups), 256 (whole wave), 520 (two pieces per lane and a second blockIdx.y chunk) -- float32 and bfloat16,
    float64 and int8 as well for max / min.  One line per call with "equal": torch.equal on the bytes of every output of the two
    builds.  The calls: spmm_values heads 1 and 4; spmm_reduce mean, max, min with arg; spmm_multi_reduce with all six statistics and
    both args; gat_aggregate, sparse_attention and gatv2_aggregate with lse, and once more with dropout 0.5 (seed 9);
    gatv2_backward in both directions, without and with dropout.  What cannot be called is a line with "skipped": heads = 4 does not
    divide h = 3 (heads = 3 takes its place); a head of 520 features is wider than the 256 the head-wise kernels take (h = 520 runs
    with heads = 4 only); max / min have no 16-bit form.  The last line counts the calls and the unequal ones; exit status 1 if any.
  --section time: the forward calls above and gatv2 forward + backward on the Reddit-shaped graph, h = 256, heads 1 and 8, float32
    and bfloat16, parent and this build alternating over two rounds after one discarded pass each (the method of --section dropout of
    exp_attention.py).  s = the largest relative difference between the parent's own two rounds over all calls; a call passes when
    new_ms <= parent_ms * (1 + s) in both rounds.  The last line holds s and the calls that do not pass.
    python scripts/exp_walker_refactor.py --parent-lib PATH [--section bits|time|all] [--iters 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import torch  # noqa: E402

from exp_attention import OtherBuild, timed  # noqa: E402
from pygim_amd import _lib, attention, pim_ops, reduce, synth  # noqa: E402

SLOPE, SEED = 0.2, 9
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64, "i8": torch.int8}


class ParentBuild(OtherBuild):
    """every entry point this build declares argument types for, not only those of the dropout section"""
    NAMES = tuple(n for n in _lib.EXPORTS if getattr(getattr(_lib.lib(), n), "argtypes", None) is not None or n in OtherBuild.NAMES)


def features(rows, h, dtype, seed, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    if dtype == torch.int8:
        return torch.randint(-128, 128, (rows, h), dtype=torch.int8, device=dev, generator=gen)
    return (torch.rand(rows, h, dtype=torch.float64 if dtype == torch.float64 else torch.float32, device=dev, generator=gen) * 2 - 1).to(dtype)


def forward_calls(g, h, heads, dtype, dev, with_heads=True, plain=True):
    """name -> function that returns the call's outputs; the operands are made once and shared by both builds"""
    n, m = g.nrows, g.ncols
    ct = attention._compute_dtype(dtype)
    gen = torch.Generator(device=dev).manual_seed(4)
    calls = {}
    if dtype in (torch.float32, torch.bfloat16, torch.float64) and with_heads:
        X, Xd = features(m, h, dtype, 5, dev), features(n, h, dtype, 6, dev)
        val = torch.rand(g.nnz, heads, dtype=ct, device=dev, generator=gen)
        a_dst = torch.randn(n, heads, dtype=ct, device=dev, generator=gen) * 2
        a_src = torch.randn(m, heads, dtype=ct, device=dev, generator=gen) * 2
        att = torch.randn(h, dtype=ct, device=dev, generator=gen) * (h // heads) ** -0.5
        calls[f"spmm_values heads={heads}"] = lambda: (attention._run_spmm_values(g, val, X, heads),)
        for p in (0.0, 0.5):
            tag = f" heads={heads}" + (" dropout=0.5" if p else "")
            calls["gat_aggregate" + tag] = lambda p=p: attention._run_gat_aggregate(g, a_dst, a_src, X, heads, SLOPE, True, p, SEED)
            if h // heads <= 256:
                calls["sparse_attention" + tag] = lambda p=p: attention._run_sparse_attention(g, Xd, X, X, heads, (h // heads) ** -0.5, True, p, SEED)
                calls["gatv2_aggregate" + tag] = lambda p=p: attention._run_gatv2_aggregate(g, Xd, X, att, heads, SLOPE, True, p, SEED)
    if plain:
        X = features(m, h, dtype, 7, dev)
        ops = ("mean", "max", "min") if dtype in (torch.float32, torch.float64) else ("mean",) if dtype == torch.bfloat16 else ("max", "min")
        for op in ops:
            calls[f"spmm_reduce {op}"] = lambda op=op: reduce._run_spmm_reduce(g, None, X, reduce.REDUCE_CODE[op], op != "mean")
        if dtype in (torch.float32, torch.bfloat16):
            calls["spmm_multi_reduce sum,mean,min,max,var,std"] = lambda: reduce._run_multi_reduce(g, X, list(range(6)), 1e-5, True, True)
    return calls


def backward_calls(g, h, heads, dtype, dev):
    """gatv2_backward on the graph of A and on that of A^T, without and with dropout; lse and delta come from this build's forward"""
    n, m = g.nrows, g.ncols
    ct = attention._compute_dtype(dtype)
    gen = torch.Generator(device=dev).manual_seed(4)
    Xd, Xs, G = features(n, h, dtype, 6, dev), features(m, h, dtype, 5, dev), features(n, h, dtype, 8, dev)
    att = torch.randn(h, dtype=ct, device=dev, generator=gen) * (h // heads) ** -0.5
    gt, _ = g.transposed()
    calls = {}
    for p in (0.0, 0.5):
        out, lse = attention._run_gatv2_aggregate(g, Xd, Xs, att, heads, SLOPE, True, p, SEED)
        delta = (G.to(ct) * out.to(ct)).view(n, heads, h // heads).sum(-1).contiguous()
        tag = f" heads={heads}" + (" dropout=0.5" if p else "")
        calls["gatv2_backward rows" + tag] = lambda p=p, lse=lse, delta=delta: attention._run_gatv2_backward(
            g, False, Xd, Xs, att, heads, SLOPE, G, lse, delta, True, p, SEED)
        calls["gatv2_backward transposed" + tag] = lambda p=p, lse=lse, delta=delta: attention._run_gatv2_backward(
            gt, True, Xs, Xd, att, heads, SLOPE, G, lse, delta, False, p, SEED, g.entry_ids_t() if p else None)
    return calls


def same_bits(a, b):
    a, b = [t for t in a if t is not None], [t for t in b if t is not None]
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
                                    for x, y in zip(a, b))


def bits_section(parent, dev, line):
    import run_edges

    total = unequal = 0
    for gname in ("edges", "one-row", "whole-batches"):
        n, m, rowptr, col = run_edges.graph(gname)
        g = attention.EdgeGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), (n, m))
        for h in (3, 32, 256, 520):
            for name, dtype in DTYPES.items():
                calls = {}
                for heads in (1, 4) if name in ("f32", "bf16") else ():
                    if h % heads:
                        line(section="bits", graph=gname, h=h, x_dtype=name, heads=heads, skipped=f"heads = {heads} does not divide h = {h}: heads = {h} instead")
                        heads = h
                    calls.update(forward_calls(g, h, heads, dtype, dev, plain=False))
                    if h // heads <= 256:
                        calls.update(backward_calls(g, h, heads, dtype, dev))
                    else:
                        line(section="bits", graph=gname, h=h, x_dtype=name, heads=heads,
                             skipped="sparse_attention, gatv2_aggregate, gatv2_backward: a head wider than 256 features is rejected by the entry points")
                calls.update(forward_calls(g, h, 1, dtype, dev, with_heads=False))
                for what, fn in calls.items():
                    mine = fn()
                    with parent:
                        theirs = fn()
                    torch.cuda.synchronize()
                    eq = same_bits(mine, theirs)
                    total += 1
                    unequal += not eq
                    line(section="bits", graph=gname, h=h, x_dtype=name, call=what, outputs=sum(t is not None for t in mine), equal=eq)
    line(section="bits", calls=total, unequal=unequal)
    return unequal


def time_section(parent, dev, line, iters, shape):
    n, nnz, d_max = synth.SHAPES[shape]
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    g = attention.EdgeGraph(rowptr, col, (n, n))
    g.transposed()
    g.entry_ids_t()
    h, recs = 256, []
    G32 = features(n, h, torch.float32, 8, dev)
    for name in ("f32", "bf16"):
        dtype = DTYPES[name]
        G = G32.to(dtype)
        for heads in (1, 8):
            calls = forward_calls(g, h, heads, dtype, dev, plain=heads == 1)
            ct = attention._compute_dtype(dtype)
            att0 = torch.randn(h, dtype=ct, device=dev, generator=torch.Generator(device=dev).manual_seed(4)) * (h // heads) ** -0.5
            leaves = [t.requires_grad_() for t in (features(n, h, dtype, 6, dev), features(n, h, dtype, 5, dev), att0)]

            def step():
                for t in leaves:
                    t.grad = None
                attention.gatv2_aggregate(g, *leaves, heads=heads, negative_slope=SLOPE).backward(G)

            calls[f"gatv2_aggregate forward + backward heads={heads}"] = step
            for what, fn in calls.items():
                k = max(2, iters // 3) if "backward" in what else iters
                timed(fn, k)   # one discarded pass per build (profiles/exp_dropout.txt, first run)
                with parent:
                    timed(fn, k)
                rec = dict(section="time", graph=shape, h=h, nnz=nnz, x_dtype=name, call=what, iters=k)
                for rnd in range(2):
                    rec[f"new_ms_{rnd}"] = round(timed(fn, k), 4)
                    with parent:
                        rec[f"parent_ms_{rnd}"] = round(timed(fn, k), 4)
                rec["parent_spread"] = round(abs(rec["parent_ms_0"] - rec["parent_ms_1"]) / min(rec["parent_ms_0"], rec["parent_ms_1"]), 5)
                recs.append(rec)
                line(**rec)
            del calls, leaves
            torch.cuda.empty_cache()
    s = max(r["parent_spread"] for r in recs)
    slower = [dict(x_dtype=r["x_dtype"], call=r["call"], round=rnd, new_ms=r[f"new_ms_{rnd}"], parent_ms=r[f"parent_ms_{rnd}"])
              for r in recs for rnd in range(2) if r[f"new_ms_{rnd}"] > r[f"parent_ms_{rnd}"] * (1 + s)]
    ratio = [r[f"new_ms_{rnd}"] / r[f"parent_ms_{rnd}"] for r in recs for rnd in range(2)]
    line(section="time", calls=len(recs), s=s, new_over_parent_min=round(min(ratio), 4), new_over_parent_max=round(max(ratio), 4), not_passing=slower)
    return len(slower)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libpygim_hip.so")
    ap.add_argument("--section", default="all", choices=["all", "bits", "time"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shape", default="reddit")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    parent = ParentBuild(args.parent_lib)

    def line(**kw):
        print(json.dumps(kw), flush=True)

    bad = 0
    if args.section in ("all", "bits"):
        bad += bits_section(parent, dev, line)
    if args.section in ("all", "time"):
        bad += time_section(parent, dev, line, args.iters, args.shape)
    with parent:
        _lib.release()
    torch.ops.pim_ops.dpu_release()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
