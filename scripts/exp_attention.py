"""Products and softmax with per-call edge values on the Reddit-shaped graph (h = 256, FLT32), one process, device events after a
warm-up.  JSON lines:
  spmm_values with heads = 1 and heads = 8 (time, gather rate: every stored entry reads one X row of h * 4 bytes), next to
    (a) the only other way to apply new values: free the group, create it again with the new values, mul -- per step, host clock;
    (b) pygim_sddmm on the same graph (it gathers a G row and an X row per entry where spmm_values gathers the X row);
    (c) the frozen-values product mul: the code stream, and the sweep (lds_mode = 2);
  edge_softmax forward and backward at heads = 8 (time, bytes moved / time) next to the torch composite (index_reduce_ amax, exp,
    index_add_, divide);
  the bytes both *_workspace functions return for this shape;
  the fused GAT aggregation, after everything above (heads = 8, the same graph, two rounds in the same run):
    (a) gat_aggregate forward; (b) the unfused sequence of GATConv for the same inputs -- score composite + edge_softmax +
    spmm_values -- and each part on its own; (c) spmm_values heads = 8 alone, the floor of the gather; (d) forward + backward of
    both paths with torch.cuda.max_memory_allocated for each.
  16-bit features (--section half, on its own: profiles/exp_half.txt), per storage type of X (FLT32, BF16, FLT16; values, node terms
    and sums float32 throughout), two rounds: spmm_values heads = 1 and 8, gat_aggregate heads = 8, spmm_reduce mean and sddmm (time,
    gather rate: every stored entry reads one X row of h * 4 or h * 2 bytes); then forward + backward of a fused GATConv layer
    (h -> 8 heads of h / 8) in FLT32 and BF16.  --dtypes f32 restricts it to calls that exist without the 16-bit codes.
  sparse dot-product attention (--section dot, on its own: profiles/exp_sparse_attention.txt), heads = 1 and 8, FLT32 and BF16 storage of
    Q, K, V (--dtypes), two rounds: (a) sparse_attention forward without and with lse; (b) the three-pass composition -- one pygim_sddmm
    per head, edge_softmax, spmm_values; (c) gat_aggregate at the same heads; (d) spmm_values twice, the floor of the gather (every
    entry reads one K row and one V row); then forward + backward of both paths with torch.cuda.max_memory_allocated for each.
  the GATv2 aggregation (--section v2, on its own: profiles/exp_gatv2.txt), heads = 1 and 8, FLT32 and BF16 storage of x_dst, x_src
    (--dtypes), two rounds: (a) gatv2_aggregate forward without and with lse; (b) gat_aggregate and (c) sparse_attention at the same
    heads, from the same run; then forward + backward of the fused path with torch.cuda.max_memory_allocated, and each of the two
    pygim_gatv2_backward calls on its own.  There is no composition to compare with on this graph (one [nnz, h] float32 tensor is
    nnz * h * 4 bytes = 117 GB); fused against fused=False runs on --small-shape (products-mini: 1 000 000 entries, one [nnz, h] float32
    tensor = 1.02 GB, so the handful the composition and its autograd graph hold fit beside everything else).
  attention dropout (--section dropout, on its own: profiles/exp_dropout.txt), heads = 1 and 8, FLT32 and BF16 (--dtypes), two rounds:
    forward, and forward + backward, of gat_aggregate, sparse_attention and gatv2_aggregate at p = 0 and p = 0.5, and -- with
    --parent-lib PATH, the parent commit's libpygim_hip.so loaded beside this build -- the parent's p = 0 calls between them.
  edge terms (--section edge, on its own: profiles/exp_edge_term.txt), heads = 1 and 8, FLT32 and BF16 (--dtypes), two rounds: forward,
    and forward + backward with torch.cuda.max_memory_allocated, of gat_aggregate and sparse_attention without a term, with a term
    ([nnz, heads] float32, inside the gather) and as the fused=False composition with the same term; with --parent-lib PATH the parent
    build's calls without a term between them.
    python scripts/exp_attention.py [--iters 10] [--section all|base|fused|half|dot|v2|dropout|edge] [--forward-only] [--dtypes f32,bf16,f16]
  --section base runs everything but the fused part (the record in profiles/exp_attention.txt), --section fused that part alone
  (profiles/exp_gat_fused.txt); all = base + fused."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pygim_amd import _lib, attention, autograd, pim_ops, synth  # noqa: E402
from pygim_amd.backend_pim import spmm as spmm_mod  # noqa: E402
from pygim_amd.sparse_tensor import SparseTensorShim  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def fused_section(g, x, n, nnz, h, iters, dev, line, backward=True):
    """the fused GAT aggregation next to the three passes it replaces, heads = 8"""
    import torch.nn.functional as F

    heads, slope = 8, 0.2
    gen = torch.Generator(device=dev).manual_seed(2)
    a_dst = torch.randn(n, heads, device=dev, generator=gen) * 2
    a_src = torch.randn(n, heads, device=dev, generator=gen) * 2
    row, col = g.row.long(), g.col.long()

    def score():
        return F.leaky_relu(a_dst.index_select(0, row) + a_src.index_select(0, col), slope)

    def unfused():
        return attention._run_spmm_values(g, attention._run_edge_softmax(g, score(), None, heads), x, heads)

    s = score()
    P = attention._run_edge_softmax(g, s, None, heads)
    got = attention._run_gat_aggregate(g, a_dst, a_src, x, heads, slope, False)[0]
    agree = bool(torch.allclose(got, attention._run_spmm_values(g, P, x, heads), rtol=1e-4, atol=1e-5))
    del got
    for rnd in range(2):
        ta = timed(lambda: attention._run_gat_aggregate(g, a_dst, a_src, x, heads, slope, False), iters)
        tl = timed(lambda: attention._run_gat_aggregate(g, a_dst, a_src, x, heads, slope, True), iters)
        tb = timed(unfused, iters)
        ts = timed(score, iters)
        te = timed(lambda: attention._run_edge_softmax(g, s, None, heads), iters)
        tc = timed(lambda: attention._run_spmm_values(g, P, x, heads), iters)
        line(what="gat fused vs unfused forward, heads=8", round=rnd, a_gat_aggregate_ms=round(ta, 3), a_with_lse_ms=round(tl, 3), b_unfused_ms=round(tb, 3),
             b_score_composite_ms=round(ts, 3), b_edge_softmax_ms=round(te, 3), c_spmm_values_heads8_ms=round(tc, 3), a_over_b=round(ta / tb, 4),
             a_over_c=round(ta / tc, 4), gather_tb_s=round(nnz * h * 4 / ta / 1e9, 2), same_result=agree)
    del s, P
    line(what="gat workspace bytes", gat_aggregate=_lib.gat_aggregate_workspace(_lib.FLT32, n, nnz, h, heads),
         spmm_values=_lib.spmm_values_workspace(_lib.FLT32, n, nnz, h, heads))

    if not backward:
        return

    # ---- (d) forward + backward of both paths, peak memory of each ----
    G = synth.features(n, h, torch.float32, seed=2, device=dev, kind="uniform")
    leaves = [t.clone().requires_grad_() for t in (a_dst, a_src, x)]
    g.transposed()   # built once per graph, before either path is measured

    def fused_step():
        for t in leaves:
            t.grad = None
        attention.gat_aggregate(g, *leaves, slope).backward(G)

    def unfused_step():   # gnn.GATConv.forward between the two reductions and the concat
        for t in leaves:
            t.grad = None
        r, c = g.row.long(), g.col.long()
        sc = F.leaky_relu(leaves[0].index_select(0, r) + leaves[1].index_select(0, c), slope)
        attention.spmm_values(g, attention.edge_softmax(g, sc), leaves[2], heads=heads).backward(G)

    del row, col
    res = {}
    for name, step in (("fused", fused_step), ("unfused", unfused_step)):
        step()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = timed(step, max(2, iters // 3))
        res[name] = (ms, base, torch.cuda.max_memory_allocated())
    line(what="gat forward + backward, heads=8", fused_ms=round(res["fused"][0], 2), unfused_ms=round(res["unfused"][0], 2),
         fused_peak_bytes=res["fused"][2], unfused_peak_bytes=res["unfused"][2], allocated_before_bytes=res["fused"][1],
         fused_peak_above_start_gb=round((res["fused"][2] - res["fused"][1]) / 1e9, 2),
         unfused_peak_above_start_gb=round((res["unfused"][2] - res["unfused"][1]) / 1e9, 2), nnz_heads_tensor_gb=round(nnz * heads * 4 / 1e9, 2))


HALF_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def half_section(g, n, nnz, h, iters, dev, line, names):
    """the gather family per storage type of X, then a fused GAT layer forward + backward"""
    from pygim_amd import gnn, reduce

    heads, slope = 8, 0.2
    gen = torch.Generator(device=dev).manual_seed(3)
    v1 = torch.rand(nnz, 1, device=dev, generator=gen)
    v8 = torch.rand(nnz, heads, device=dev, generator=gen)
    a_dst = torch.randn(n, heads, device=dev, generator=gen) * 2
    a_src = torch.randn(n, heads, device=dev, generator=gen) * 2
    x32 = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform")
    g32 = synth.features(n, h, torch.float32, seed=1, device=dev, kind="uniform")
    for name in names:
        dt = HALF_DTYPES[name]
        x, gr = x32.to(dt), g32.to(dt)
        gathered = nnz * h * x.element_size()
        for rnd in range(2):
            t1 = timed(lambda: attention._run_spmm_values(g, v1, x, 1), iters)
            t8 = timed(lambda: attention._run_spmm_values(g, v8, x, heads), iters)
            tg = timed(lambda: attention._run_gat_aggregate(g, a_dst, a_src, x, heads, slope, False), iters)
            tm = timed(lambda: reduce._run_spmm_reduce(g, None, x, reduce.REDUCE_CODE["mean"], False), iters)
            sd = timed(lambda: autograd.sddmm(g.rowptr, g.col, gr, x), iters)
            ms = dict(spmm_values_heads1=t1, spmm_values_heads8=t8, gat_aggregate_heads8=tg, mean=tm, sddmm=sd)
            line(what="16-bit features: the gather family", x_dtype=name, round=rnd, bytes_per_x_row=h * x.element_size(),
                 **{k + "_ms": round(v, 3) for k, v in ms.items()}, **{k + "_gather_tb_s": round(gathered / v / 1e9, 2) for k, v in ms.items()})
        del x, gr
    del v1, v8, a_dst, a_src, g32
    g.transposed()
    for name in [k for k in names if k in ("f32", "bf16")]:
        dt = HALF_DTYPES[name]
        torch.manual_seed(0)
        conv = gnn.GATConv(h, h // heads, heads=heads, fused=True).to(dev, dt)
        x = x32.to(dt)

        def step():
            conv.zero_grad(set_to_none=True)
            conv(x, g).float().square().mean().backward()

        step()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = [timed(step, max(2, iters // 3)) for _ in range(2)]
        line(what="fused GATConv forward + backward, heads=8", x_dtype=name, ms_round0=round(ms[0], 2), ms_round1=round(ms[1], 2),
             peak_above_start_gb=round((torch.cuda.max_memory_allocated() - base) / 1e9, 2))
        del conv, x


def dot_section(g, n, nnz, h, iters, dev, line, names, backward=True):
    """the fused dot-product attention next to the three passes it replaces, to gat_aggregate and to two plain gathers"""
    g.transposed()   # built once per graph, before any backward is measured
    q32, k32, v32, g32 = (synth.features(n, h, torch.float32, seed=sd, device=dev, kind="uniform") for sd in (5, 6, 7, 8))
    for name in names:
        dt = HALF_DTYPES[name]
        Q, K, V, G = (t.to(dt) for t in (q32, k32, v32, g32))
        for heads in (1, 8):
            scale = (h // heads) ** -0.5
            gen = torch.Generator(device=dev).manual_seed(4)
            a_dst = torch.randn(n, heads, device=dev, generator=gen) * 2
            a_src = torch.randn(n, heads, device=dev, generator=gen) * 2

            def composition():
                sc = attention._head_dots(g, Q, K, heads).mul_(scale)
                return attention._run_spmm_values(g, attention._run_edge_softmax(g, sc, None, heads), V, heads)

            P = attention._run_edge_softmax(g, attention._head_dots(g, Q, K, heads).mul_(scale), None, heads)
            got = attention._run_sparse_attention(g, Q, K, V, heads, scale, False)[0]
            tol = dict(rtol=1e-4, atol=1e-5) if dt == torch.float32 else dict(rtol=2e-2, atol=1e-3)
            agree = bool(torch.allclose(got.float(), attention._run_spmm_values(g, P, V, heads).float(), **tol))
            del got
            for rnd in range(2):
                ta = timed(lambda: attention._run_sparse_attention(g, Q, K, V, heads, scale, False), iters)
                tl = timed(lambda: attention._run_sparse_attention(g, Q, K, V, heads, scale, True), iters)
                tb = timed(composition, iters)
                tg = timed(lambda: attention._run_gat_aggregate(g, a_dst, a_src, V, heads, 0.2, False), iters)
                t2 = timed(lambda: (attention._run_spmm_values(g, P, K, heads), attention._run_spmm_values(g, P, V, heads)), iters)
                line(what="sparse_attention fused vs composition forward", x_dtype=name, heads=heads, round=rnd, a_sparse_attention_ms=round(ta, 3),
                     a_with_lse_ms=round(tl, 3), b_composition_ms=round(tb, 3), c_gat_aggregate_ms=round(tg, 3), d_two_spmm_values_ms=round(t2, 3),
                     a_over_b=round(ta / tb, 4), a_over_c=round(ta / tg, 4), a_over_d=round(ta / t2, 4),
                     gather_tb_s=round(2 * nnz * h * Q.element_size() / ta / 1e9, 2), same_result=agree)
            del P
            if not backward:
                continue
            leaves = [t.clone().requires_grad_() for t in (Q, K, V)]
            res = {}
            for path, fused in (("fused", True), ("unfused", False)):
                def step():
                    for t in leaves:
                        t.grad = None
                    attention.sparse_attention(g, *leaves, heads=heads, fused=fused).backward(G)

                step()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ms = timed(step, max(2, iters // 3))
                res[path] = (ms, base, torch.cuda.max_memory_allocated())
            del leaves
            line(what="sparse_attention forward + backward", x_dtype=name, heads=heads, fused_ms=round(res["fused"][0], 2),
                 unfused_ms=round(res["unfused"][0], 2), fused_peak_above_start_gb=round((res["fused"][2] - res["fused"][1]) / 1e9, 2),
                 unfused_peak_above_start_gb=round((res["unfused"][2] - res["unfused"][1]) / 1e9, 2), nnz_heads_tensor_gb=round(nnz * heads * 4 / 1e9, 2))
        del Q, K, V, G
    line(what="sparse_attention workspace bytes", heads8=_lib.sparse_attention_workspace(_lib.FLT32, n, nnz, h, 8))


def v2_section(g, n, nnz, h, iters, dev, line, names, small_shape, backward=True):
    """the GATv2 aggregation next to gat_aggregate and sparse_attention; fused against the composition on a graph where that fits"""
    g.transposed()   # built once per graph, before any backward is measured
    slope = 0.2
    d32, s32, g32 = (synth.features(n, h, torch.float32, seed=sd, device=dev, kind="uniform") for sd in (5, 6, 8))
    for name in names:
        dt = HALF_DTYPES[name]
        Xd, Xs, G = (t.to(dt) for t in (d32, s32, g32))
        for heads in (1, 8):
            hd = h // heads
            gen = torch.Generator(device=dev).manual_seed(4)
            a_dst = torch.randn(n, heads, device=dev, generator=gen) * 2
            a_src = torch.randn(n, heads, device=dev, generator=gen) * 2
            att = torch.randn(h, device=dev, generator=gen) * hd ** -0.5
            for rnd in range(2):
                ta = timed(lambda: attention._run_gatv2_aggregate(g, Xd, Xs, att, heads, slope, False), iters)
                tl = timed(lambda: attention._run_gatv2_aggregate(g, Xd, Xs, att, heads, slope, True), iters)
                tg = timed(lambda: attention._run_gat_aggregate(g, a_dst, a_src, Xs, heads, slope, False), iters)
                ts = timed(lambda: attention._run_sparse_attention(g, Xd, Xs, Xs, heads, hd ** -0.5, False), iters)
                line(what="gatv2_aggregate forward", x_dtype=name, heads=heads, round=rnd, a_gatv2_aggregate_ms=round(ta, 3), a_with_lse_ms=round(tl, 3),
                     b_gat_aggregate_ms=round(tg, 3), c_sparse_attention_ms=round(ts, 3), a_over_b=round(ta / tg, 4), a_over_c=round(ta / ts, 4),
                     gather_tb_s=round(nnz * h * Xs.element_size() / ta / 1e9, 2))
            if not backward:
                continue
            out, lse = attention._run_gatv2_aggregate(g, Xd, Xs, att, heads, slope, True)
            delta = (G.float() * out.float()).view(n, heads, hd).sum(-1).contiguous()
            gt, _ = g.transposed()
            nb = max(2, iters // 3)
            t_row = timed(lambda: attention._run_gatv2_backward(g, False, Xd, Xs, att, heads, slope, G, lse, delta, True), nb)
            t_col = timed(lambda: attention._run_gatv2_backward(gt, True, Xs, Xd, att, heads, slope, G, lse, delta, False), nb)
            del out, lse, delta
            leaves = [t.clone().requires_grad_() for t in (Xd, Xs, att)]

            def step():
                for t in leaves:
                    t.grad = None
                attention.gatv2_aggregate(g, *leaves, heads=heads, negative_slope=slope).backward(G)

            step()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ms = timed(step, nb)
            peak = torch.cuda.max_memory_allocated()
            del leaves
            line(what="gatv2_aggregate forward + backward", x_dtype=name, heads=heads, fused_ms=round(ms, 2), backward_row_side_ms=round(t_row, 2),
                 backward_transposed_ms=round(t_col, 2), fused_peak_above_start_gb=round((peak - base) / 1e9, 2),
                 one_nnz_h_float32_tensor_gb=round(nnz * h * 4 / 1e9, 2),
                 backward_workspace_gb=round(_lib.gatv2_backward_workspace(_lib.FLT32, n, nnz, h, heads) / 1e9, 2))
        del Xd, Xs, G
    del d32, s32, g32
    line(what="gatv2 workspace bytes", aggregate_heads8=_lib.gatv2_aggregate_workspace(_lib.FLT32, n, nnz, h, 8),
         backward_heads8=_lib.gatv2_backward_workspace(_lib.FLT32, n, nnz, h, 8))
    if not backward:
        return
    # fused against the composition, where the composition fits
    ns, nnzs, d_max = synth.SHAPES[small_shape]
    rowptr, col = synth.make_csr(ns, nnzs, d_max, seed=0, device=dev)
    gs = attention.EdgeGraph(rowptr, col, (ns, ns))
    gs.transposed()
    d32, s32, g32 = (synth.features(ns, h, torch.float32, seed=sd, device=dev, kind="uniform") for sd in (5, 6, 8))
    for name in names:
        dt = HALF_DTYPES[name]
        for heads in (1, 8):
            att = torch.randn(h, device=dev, generator=torch.Generator(device=dev).manual_seed(4)) * (h // heads) ** -0.5
            leaves = [t.clone().requires_grad_() for t in (d32.to(dt), s32.to(dt), att)]
            G = g32.to(dt)
            res, outs = {}, {}
            for path, fused in (("fused", True), ("unfused", False)):
                def step():
                    for t in leaves:
                        t.grad = None
                    out = attention.gatv2_aggregate(gs, *leaves, heads=heads, negative_slope=slope, fused=fused)
                    out.backward(G)
                    return out

                outs[path] = [step().detach().float()] + [t.grad.float().clone() for t in leaves]
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ms = timed(step, max(2, iters // 3))
                res[path] = (ms, base, torch.cuda.max_memory_allocated())
            # largest difference between the two paths per tensor, relative to the tensor's largest magnitude
            diff = {k: float("%.2e" % ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item())
                    for k, a, b in zip(("out", "dx_dst", "dx_src", "datt"), outs["fused"], outs["unfused"])}
            del leaves, outs
            line(what="gatv2_aggregate fused vs composition, forward + backward", graph=small_shape, nnz=nnzs, x_dtype=name, heads=heads,
                 fused_ms=round(res["fused"][0], 2), unfused_ms=round(res["unfused"][0], 2),
                 fused_peak_above_start_gb=round((res["fused"][2] - res["fused"][1]) / 1e9, 3),
                 unfused_peak_above_start_gb=round((res["unfused"][2] - res["unfused"][1]) / 1e9, 3),
                 one_nnz_h_float32_tensor_gb=round(nnzs * h * 4 / 1e9, 2), max_diff_over_max_magnitude=diff)


def base_section(g, x, rowptr, col, n, nnz, h, iters, dev, line):
    """spmm_values, edge_softmax, the workspaces, new values through a new group: the record in profiles/exp_attention.txt"""
    gen = torch.Generator(device=dev).manual_seed(1)
    gathered = nnz * h * 4

    # ---- spmm_values, alternating with pygim_sddmm (two rounds: the spread) ----
    v1 = torch.rand(nnz, 1, device=dev, generator=gen)
    v8 = torch.rand(nnz, 8, device=dev, generator=gen)
    gr = synth.features(n, h, torch.float32, seed=1, device=dev, kind="uniform")
    for rnd in range(2):
        t1 = timed(lambda: attention._run_spmm_values(g, v1, x, 1), iters)
        sd = timed(lambda: autograd.sddmm(g.rowptr, g.col, gr, x), iters)
        t8 = timed(lambda: attention._run_spmm_values(g, v8, x, 8), iters)
        line(what="spmm_values vs sddmm", round=rnd, spmm_values_heads1_ms=round(t1, 3), spmm_values_heads8_ms=round(t8, 3), sddmm_ms=round(sd, 3),
             heads1_gather_tb_s=round(gathered / t1 / 1e9, 2), heads8_gather_tb_s=round(gathered / t8 / 1e9, 2),
             sddmm_x_gather_tb_s=round(gathered / sd / 1e9, 2))
    del gr, v8
    line(what="workspace bytes", spmm_values=_lib.spmm_values_workspace(_lib.FLT32, n, nnz, h, 8),
         edge_softmax_heads8=_lib.edge_softmax_workspace(_lib.FLT32, n, nnz, 8))

    # ---- edge_softmax forward / backward at heads = 8 against the torch composite ----
    heads = 8
    s = torch.randn(nnz, heads, device=dev, generator=gen) * 3
    dP = torch.randn(nnz, heads, device=dev, generator=gen)
    row = g.row.long()
    P = attention._run_edge_softmax(g, s, None, heads)
    fwd = timed(lambda: attention._run_edge_softmax(g, s, None, heads), iters)
    bwd = timed(lambda: attention._run_edge_softmax(g, P, dP, heads), iters)

    def torch_fwd():
        m = torch.full((n, heads), -float("inf"), device=dev).index_reduce_(0, row, s, "amax", include_self=True)
        e = torch.exp(s - m[row])
        return e / torch.zeros(n, heads, device=dev).index_add_(0, row, e)[row]

    def torch_bwd():
        t = torch.zeros(n, heads, device=dev).index_add_(0, row, P * dP)
        return P * (dP - t[row])

    tf, tb = timed(torch_fwd, max(2, iters // 3)), timed(torch_bwd, max(2, iters // 3))
    elems = nnz * heads * 4
    line(what="edge_softmax heads=8", forward_ms=round(fwd, 3), backward_ms=round(bwd, 3), torch_forward_ms=round(tf, 3), torch_backward_ms=round(tb, 3),
         forward_min_bytes_tb_s=round(2 * elems / fwd / 1e9, 2), backward_min_bytes_tb_s=round(3 * elems / bwd / 1e9, 2),
         note="rates count one read of every input and one write; rows longer than a 64-entry batch are read twice")
    del s, dP, P, row

    # ---- (a) new values through a new group, (c) the frozen-values product ----
    val = v1[:, 0].contiguous()
    adj = SparseTensorShim(rowptr=rowptr.long(), col=col.long(), value=val, sparse_sizes=(n, n))

    def regroup_step(A):
        A.free_group()
        A.csr = []
        A.to_pim_group_csr(h, 1)
        return A.mul(x)

    A = spmm_mod.SparseTensorCOO(adj, dtype=torch.float32, format="CSR")
    A.to_pim_group_csr(h, 1)
    ref = A.mul(x)
    got = attention._run_spmm_values(g, v1, x, 1)
    agree = bool(torch.allclose(got, ref, rtol=1e-4, atol=1e-3))
    torch.cuda.synchronize()
    steps = 3
    t0 = time.perf_counter()
    for _ in range(steps):
        regroup_step(A)
    torch.cuda.synchronize()
    regroup_ms = (time.perf_counter() - t0) * 1e3 / steps
    t1 = timed(lambda: attention._run_spmm_values(g, v1, x, 1), iters)
    mul_code = timed(lambda: A.mul(x), iters)
    note = _lib.group_lds_note(A.sp_info_ptr)
    A.free_group()
    old = _lib.set_tunable("lds_mode", 2)
    A.csr = []
    A.to_pim_group_csr(h, 1)
    mul_sweep = timed(lambda: A.mul(x), iters)
    A.free_group()
    _lib.set_tunable("lds_mode", old)
    line(what="new values per step", regroup_then_mul_ms=round(regroup_ms, 2), spmm_values_heads1_ms=round(t1, 3), ratio=round(regroup_ms / t1, 2),
         same_product=agree, frozen_mul_ms=round(mul_code, 3), frozen_mul_form=note[:120], frozen_mul_sweep_ms=round(mul_sweep, 3))


class OtherBuild:
    """another build of the library (the parent commit's libpygim_hip.so) loaded beside this one: inside ``with other:`` every call of
    pygim_amd._lib goes to it, so the two builds are timed alternately in one process on the same tensors.  Only the entry points the
    dropout section calls get their argument types, copied from this build's."""
    NAMES = ("pygim_init_ranks", "pygim_release", "pygim_last_error", "pygim_spmm_values", "pygim_spmm_values_workspace", "pygim_sddmm",
             "pygim_gat_aggregate", "pygim_gat_aggregate_workspace", "pygim_sparse_attention", "pygim_sparse_attention_workspace",
             "pygim_gatv2_aggregate", "pygim_gatv2_aggregate_workspace", "pygim_gatv2_backward", "pygim_gatv2_backward_workspace")

    def __init__(self, path):
        import ctypes

        self.mine = _lib.lib()
        self.handle = ctypes.CDLL(os.path.abspath(path))
        for name in self.NAMES:
            src, dst = getattr(self.mine, name), getattr(self.handle, name)
            dst.argtypes, dst.restype = src.argtypes, src.restype
        with self:
            _lib.init_ranks(1)

    def __enter__(self):
        _lib._lib = self.handle

    def __exit__(self, *exc):
        _lib._lib = self.mine


def dropout_section(g, n, nnz, h, iters, dev, line, names, parent):
    """what attention dropout costs: forward, and forward + backward, of gat_aggregate, sparse_attention and gatv2_aggregate at p = 0 and
    p = 0.5, heads = 1 and 8, and the p = 0 calls of the parent build (--parent-lib) in the same run, alternating, two rounds"""
    g.transposed()
    g.entry_ids_t()
    slope = 0.2
    a32, b32, g32 = (synth.features(n, h, torch.float32, seed=sd, device=dev, kind="uniform") for sd in (5, 6, 8))
    nb = max(2, iters // 3)
    for name in names:
        dt = HALF_DTYPES[name]
        A, B, G = (t.to(dt) for t in (a32, b32, g32))
        for heads in (1, 8):
            hd = h // heads
            gen = torch.Generator(device=dev).manual_seed(4)
            a_dst = torch.randn(n, heads, device=dev, generator=gen) * 2
            a_src = torch.randn(n, heads, device=dev, generator=gen) * 2
            att = torch.randn(h, device=dev, generator=gen) * hd ** -0.5
            calls = {
                "gat_aggregate": (lambda p: attention._run_gat_aggregate(g, a_dst, a_src, B, heads, slope, False, p, 9),
                                  lambda p, t: attention.gat_aggregate(g, *t, slope, dropout=p, seed=9), (a_dst, a_src, B)),
                "sparse_attention": (lambda p: attention._run_sparse_attention(g, A, B, B, heads, hd ** -0.5, False, p, 9),
                                     lambda p, t: attention.sparse_attention(g, *t, heads=heads, dropout=p, seed=9), (A, B, B)),
                "gatv2_aggregate": (lambda p: attention._run_gatv2_aggregate(g, A, B, att, heads, slope, False, p, 9),
                                    lambda p, t: attention.gatv2_aggregate(g, *t, heads=heads, negative_slope=slope, dropout=p, seed=9), (A, B, att)),
            }
            for fn_name, (fwd, full, operands) in calls.items():
                leaves = [t.clone().requires_grad_() for t in operands]

                def step(p):
                    for t in leaves:
                        t.grad = None
                    full(p, leaves).backward(G)

                # one discarded pass per build: without it the first timing after a shape's tensors are allocated came out 2 - 3 % slow
                # (profiles/exp_dropout.txt, first run)
                timed(lambda: fwd(0.0), iters)
                if parent is not None:
                    with parent:
                        timed(lambda: fwd(0.0), iters)
                for rnd in range(2):
                    rec = dict(what=f"{fn_name} dropout", x_dtype=name, heads=heads, round=rnd)
                    rec["fwd_p0_ms"] = round(timed(lambda: fwd(0.0), iters), 3)
                    if parent is not None:
                        with parent:
                            rec["fwd_parent_ms"] = round(timed(lambda: fwd(0.0), iters), 3)
                    rec["fwd_p05_ms"] = round(timed(lambda: fwd(0.5), iters), 3)
                    rec["fwdbwd_p0_ms"] = round(timed(lambda: step(0.0), nb), 2)
                    if parent is not None:
                        with parent:
                            rec["fwdbwd_parent_ms"] = round(timed(lambda: step(0.0), nb), 2)
                    rec["fwdbwd_p05_ms"] = round(timed(lambda: step(0.5), nb), 2)
                    rec["fwd_p05_over_p0"] = round(rec["fwd_p05_ms"] / rec["fwd_p0_ms"], 4)
                    rec["fwdbwd_p05_over_p0"] = round(rec["fwdbwd_p05_ms"] / rec["fwdbwd_p0_ms"], 4)
                    if parent is not None:
                        rec["fwd_p0_over_parent"] = round(rec["fwd_p0_ms"] / rec["fwd_parent_ms"], 4)
                        rec["fwdbwd_p0_over_parent"] = round(rec["fwdbwd_p0_ms"] / rec["fwdbwd_parent_ms"], 4)
                    line(**rec)
                del leaves
                torch.cuda.empty_cache()
        del A, B, G


def edge_section(g, n, nnz, h, iters, dev, line, names, parent):
    """what a per-entry term of the score costs: gat_aggregate(a_edge=) and sparse_attention(bias=) next to the calls without a term (this
    build and, with --parent-lib, the parent's, alternating) and next to the fused=False composition with the same term; forward, and
    forward + backward with the peak of torch.cuda.max_memory_allocated over one step; heads = 1 and 8, two rounds"""
    import torch.nn.functional as F

    g.transposed()
    slope = 0.2
    a32, b32, g32 = (synth.features(n, h, torch.float32, seed=sd, device=dev, kind="uniform") for sd in (5, 6, 8))
    nb = max(2, iters // 3)
    row, col = g.row.long(), g.col.long()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)

    for name in names:
        dt = HALF_DTYPES[name]
        A, B, G = (t.to(dt) for t in (a32, b32, g32))
        for heads in (1, 8):
            hd = h // heads
            gen = torch.Generator(device=dev).manual_seed(4)
            a_dst = torch.randn(n, heads, device=dev, generator=gen) * 2
            a_src = torch.randn(n, heads, device=dev, generator=gen) * 2
            term = torch.rand(nnz, heads, device=dev, generator=gen) * 4 - 2

            def gat_composed(a, b, x, e):   # the fused=False path of gnn.GATConv with the term on the scores
                score = F.leaky_relu(a.index_select(0, row) + b.index_select(0, col) + e, slope)
                return attention.spmm_values(g, attention.edge_softmax(g, score), x, heads)

            calls = {
                "gat_aggregate": (lambda e: attention._run_gat_aggregate(g, a_dst, a_src, B, heads, slope, False, 0.0, 0, e),
                                  lambda t, e: attention.gat_aggregate(g, *t, slope, a_edge=e), gat_composed, (a_dst, a_src, B)),
                "sparse_attention": (lambda e: attention._run_sparse_attention(g, A, B, B, heads, hd ** -0.5, False, 0.0, 0, e),
                                     lambda t, e: attention.sparse_attention(g, *t, heads=heads, bias=e),
                                     lambda q, k, v, e: attention.sparse_attention(g, q, k, v, heads=heads, fused=False, bias=e), (A, B, B)),
            }
            for fn_name, (fwd, full, composed, operands) in calls.items():
                leaves = [t.clone().requires_grad_() for t in operands]
                eterm = term.clone().requires_grad_()

                def step(kind):
                    for t in leaves + [eterm]:
                        t.grad = None
                    out = full(leaves, None) if kind == "none" else full(leaves, eterm) if kind == "term" else composed(*leaves, eterm)
                    out.backward(G)

                def fwd_composed():
                    with torch.no_grad():
                        return composed(*operands, term)

                # one discarded pass per build, as in the dropout section, of the forward and of forward + backward: without the second the
                # first forward + backward after a storage type's tensors are allocated came out 1.5 % slow once (profiles/exp_edge_term.txt)
                timed(lambda: fwd(None), iters)
                timed(lambda: step("none"), 1)
                if parent is not None:
                    with parent:
                        timed(lambda: fwd(None), iters)
                        timed(lambda: step("none"), 1)
                for rnd in range(2):
                    rec = dict(what=f"{fn_name} edge term", x_dtype=name, heads=heads, round=rnd)
                    rec["fwd_none_ms"] = round(timed(lambda: fwd(None), iters), 3)
                    if parent is not None:
                        with parent:
                            rec["fwd_parent_ms"] = round(timed(lambda: fwd(None), iters), 3)
                    rec["fwd_term_ms"] = round(timed(lambda: fwd(term), iters), 3)
                    rec["fwd_composed_ms"] = round(timed(fwd_composed, nb), 2)
                    rec["fwdbwd_none_ms"] = round(timed(lambda: step("none"), nb), 2)
                    if parent is not None:
                        with parent:
                            rec["fwdbwd_parent_ms"] = round(timed(lambda: step("none"), nb), 2)
                    rec["fwdbwd_term_ms"] = round(timed(lambda: step("term"), nb), 2)
                    rec["fwdbwd_composed_ms"] = round(timed(lambda: step("composed"), nb), 2)
                    for kind in ("none", "term", "composed"):
                        rec[f"fwdbwd_{kind}_peak_gib"] = peak(lambda: step(kind))
                    rec["fwd_term_over_none"] = round(rec["fwd_term_ms"] / rec["fwd_none_ms"], 4)
                    rec["fwd_composed_over_term"] = round(rec["fwd_composed_ms"] / rec["fwd_term_ms"], 3)
                    rec["fwdbwd_composed_over_term"] = round(rec["fwdbwd_composed_ms"] / rec["fwdbwd_term_ms"], 3)
                    if parent is not None:
                        rec["fwd_none_over_parent"] = round(rec["fwd_none_ms"] / rec["fwd_parent_ms"], 4)
                        rec["fwdbwd_none_over_parent"] = round(rec["fwdbwd_none_ms"] / rec["fwdbwd_parent_ms"], 4)
                    line(**rec)
                del leaves, eterm
                for t in operands:
                    t.grad = None
                torch.cuda.empty_cache()
            del term
        del A, B, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--section", default="all", choices=["all", "base", "fused", "half", "dot", "v2", "dropout", "edge"])
    ap.add_argument("--parent-lib", default=None, help="--section dropout / edge: the parent commit's libpygim_hip.so, timed alternately in the same run")
    ap.add_argument("--small-shape", default="products-mini", help="--section v2: the graph on which fused=False fits in memory")
    ap.add_argument("--dtypes", default="f32,bf16,f16", help="--section half / dot: the storage types of the features to measure")
    ap.add_argument("--forward-only", action="store_true", help="skip (d) of the fused part: for a kernel trace of the forward kernels alone")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, nnz, d_max = synth.SHAPES[args.shape]
    h, iters = args.h, args.iters
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    g = attention.EdgeGraph(rowptr, col, (n, n))
    x = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform")

    def line(**kw):
        print(json.dumps({"graph": args.shape, "h": h, "nnz": nnz, **kw}), flush=True)

    if args.section in ("all", "base"):
        base_section(g, x, rowptr, col, n, nnz, h, iters, dev, line)
    if args.section in ("all", "fused"):   # after the recorded parts, which keep the allocator and cache state they were taken under
        fused_section(g, x, n, nnz, h, iters, dev, line, backward=not args.forward_only)
    if args.section == "half":
        del x
        half_section(g, n, nnz, h, iters, dev, line, args.dtypes.split(","))
    if args.section == "dot":
        del x
        dot_section(g, n, nnz, h, iters, dev, line, [k for k in args.dtypes.split(",") if k in ("f32", "bf16")], backward=not args.forward_only)
    if args.section == "v2":
        del x
        v2_section(g, n, nnz, h, iters, dev, line, [k for k in args.dtypes.split(",") if k in ("f32", "bf16")], args.small_shape,
                   backward=not args.forward_only)
    if args.section == "dropout":
        del x
        dropout_section(g, n, nnz, h, iters, dev, line, [k for k in args.dtypes.split(",") if k in ("f32", "bf16")],
                        OtherBuild(args.parent_lib) if args.parent_lib else None)
    if args.section == "edge":
        del x
        edge_section(g, n, nnz, h, iters, dev, line, [k for k in args.dtypes.split(",") if k in ("f32", "bf16")],
                     OtherBuild(args.parent_lib) if args.parent_lib else None)
    torch.ops.pim_ops.dpu_release()


if __name__ == "__main__":
    main()
