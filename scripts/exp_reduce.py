"""Mean / max / min aggregation on the Reddit-shaped graph (h = 256, FLT32), one process, device events after a warm-up.  JSON lines:
  spmm_reduce mean, max without arg and max with arg next to spmm_values with one head in the same run (time, gather rate: every
    stored entry reads one X row of h * 4 bytes), two rounds: the spread;
  the gradient of max with respect to X (pygim_spmm_reduce_backward: an arg row beside every G row);
  the torch composite for scale: index_reduce_ amax over the per-entry messages, in blocks of 2^23 entries (the messages of the whole
    graph would be 117 GB);
  the bytes pygim_spmm_reduce_workspace returns for this shape.
    python scripts/exp_reduce.py [--iters 10]
--section multi: several statistics in one gather (pygim_spmm_multi_reduce) on the same graph, float32 and bfloat16, two rounds in one
process, written to profiles/exp_multi_reduce.txt (--out) as JSON lines:
  spmm_values with one head (the yardstick) and spmm_reduce mean in the same round;
  spmm_multi_reduce for ("mean",), ("max", "min") with args, ("mean", "std"), ("mean", "min", "max", "std") with and without args;
  the fused=False composition of the last (one spmm_reduce per statistic, two for std);
  forward + backward of the four-statistic call, fused against composed, with the peak of allocated memory;
  the bytes pygim_spmm_multi_reduce_workspace returns.
    python scripts/exp_reduce.py --section multi [--iters 10] [--out profiles/exp_multi_reduce.txt]
--section softmax: softmax aggregation per feature in one gather (pygim_spmm_softmax and its backward), float32 and bfloat16, two rounds
in one process, written to profiles/exp_softmax.txt (--out) as JSON lines:
  on the Reddit-shaped graph spmm_values with one head and unit weights (the yardstick), the fused forward with and without lse, and
    forward + backward (one backward gather on the transposed structure) with t requiring a gradient, with the peak of allocated memory;
  on products-mini the same beside the fused=False composition (X[col], edge_softmax and spmm_values with heads = h: it fits there),
    forward and forward + backward, with peak memory;
  the bytes the two workspace functions return.
    python scripts/exp_reduce.py --section softmax [--iters 10] [--out profiles/exp_softmax.txt]
--section edge: messages with a feature-wide edge feature (pygim_spmm_edge, pygim_spmm_edge_softmax, pygim_spmm_edge_backward), float32 and
bfloat16, sum and softmax, two rounds in one process, written to profiles/exp_edge_message.txt (--out) as JSON lines:
  on the Reddit-shaped graph at --edge-h (default 32: E and dE are [nnz, h], 14.7 GB each in float32 there; at h = 256 one of them would
    be 117 GB) and on products-mini at --h: the plain gather of the same fold (spmm_values with unit weights / spmm_softmax), the fused
    forward relu(X[col] + E) + eps, the fused=False composition through the [nnz, h] message tensor, and forward + backward of both
    (gradients of X, E and t), each with the peak of allocated memory; e_stream_tb_s is the rate of the E bytes alone;
  with --parent-lib PATH (the parent commit's libpygim_hip.so loaded beside this build) the calls that existed before -- spmm_values,
    spmm_reduce mean and max, spmm_softmax, each forward and forward + backward -- on both builds, alternating: the parity of what did not change.
    python scripts/exp_reduce.py --section edge [--iters 10] [--edge-h 32] [--parent-lib PATH] [--out profiles/exp_edge_message.txt]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pygim_amd import _lib, attention, pim_ops, reduce as red, synth  # noqa: E402


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


def section_multi(args):
    dev = torch.device("cuda", 0)
    n, nnz, d_max = synth.SHAPES[args.shape]
    h, iters = args.h, args.iters
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    g = attention.EdgeGraph(rowptr, col, (n, n))
    g.transposed()   # built once, outside the timings
    out_path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exp_multi_reduce.txt")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    sink = open(out_path, "w")

    def line(**kw):
        text = json.dumps({"graph": args.shape, "h": h, "nnz": nnz, **kw})
        print(text, flush=True)
        sink.write(text + "\n")
        sink.flush()

    S = red.STAT_CODE
    four = ("mean", "min", "max", "std")
    codes = lambda names: [S[s] for s in names]
    ones = torch.ones(nnz, 1, device=dev)
    for dtype, name, code in ((torch.float32, "float32", _lib.FLT32), (torch.bfloat16, "bfloat16", _lib.BF16)):
        x = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform").to(dtype)
        gathered = nnz * h * x.element_size()
        multi = lambda names, arg: red._run_multi_reduce(g, x, codes(names), 1e-5, arg and "max" in names, arg and "min" in names)
        for rnd in range(2):
            t = {"spmm_values_heads1": timed(lambda: attention._run_spmm_values(g, ones, x, 1), iters),
                 "spmm_reduce_mean": timed(lambda: red._run_spmm_reduce(g, None, x, red.REDUCE_CODE["mean"], False), iters),
                 "multi_mean": timed(lambda: multi(("mean",), False), iters),
                 "multi_max_min_args": timed(lambda: multi(("max", "min"), True), iters),
                 "multi_mean_std": timed(lambda: multi(("mean", "std"), False), iters),
                 "multi_four": timed(lambda: multi(four, False), iters),
                 "multi_four_args": timed(lambda: multi(four, True), iters)}
            with torch.no_grad():
                t["composed_four"] = timed(lambda: red.spmm_multi_reduce(g, x, four, fused=False), max(iters // 2, 1))
            sv = t["spmm_values_heads1"]
            line(what="forward", dtype=name, round=rnd, **{k + "_ms": round(v, 3) for k, v in t.items()},
                 **{k + "_over_values": round(v / sv, 3) for k, v in t.items() if k != "spmm_values_heads1"},
                 multi_four_gather_tb_s=round(gathered / t["multi_four"] / 1e9, 2), composed_over_fused=round(t["composed_four"] / t["multi_four"], 2))
        G = synth.features(n, 4 * h, torch.float32, seed=1, device=dev, kind="uniform").to(dtype)

        def step(fused):
            xx = x.detach().requires_grad_()
            red.spmm_multi_reduce(g, xx, four, fused=fused).backward(G)
            return xx.grad

        for rnd in range(2):
            res = {}
            for fused in (True, False):
                step(fused)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                ms = timed(lambda: step(fused), max(iters // 2, 1))
                res["fused" if fused else "composed"] = (ms, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20)
            line(what="forward + backward, four statistics", dtype=name, round=rnd, fused_ms=round(res["fused"][0], 3), composed_ms=round(res["composed"][0], 3),
                 composed_over_fused=round(res["composed"][0] / res["fused"][0], 2), fused_peak_mib=round(res["fused"][1], 1),
                 composed_peak_mib=round(res["composed"][1], 1))
        d_f, d_c = step(True).float(), step(False).float()
        line(what="gradient check", dtype=name, max_abs_fused_minus_composed=float((d_f - d_c).abs().max()), max_abs=float(d_c.abs().max()))
        line(what="workspace bytes", dtype=name, **{"_".join(k): _lib.spmm_multi_reduce_workspace(code, codes(k), n, nnz, h)
                                                    for k in (("mean",), ("max", "min"), ("mean", "std"), four)},
             spmm_reduce_mean=_lib.spmm_reduce_workspace(code, red.REDUCE_CODE["mean"], n, nnz, h))
        del x, G, d_f, d_c
    sink.close()
    torch.ops.pim_ops.dpu_release()


def section_softmax(args):
    dev = torch.device("cuda", 0)
    h, iters = args.h, args.iters
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    out_path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exp_softmax.txt")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    sink = open(out_path, "w")

    def peak(fn, reps):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        ms = timed(fn, reps)
        return ms, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    for shape, composed in (("reddit", False), ("products-mini", True)):
        n, nnz, d_max = synth.SHAPES[shape]
        rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
        g = attention.EdgeGraph(rowptr, col, (n, n))
        g.transposed()   # built once, outside the timings

        def line(**kw):
            text = json.dumps({"graph": shape, "h": h, "nnz": nnz, **kw})
            print(text, flush=True)
            sink.write(text + "\n")
            sink.flush()

        ones = torch.ones(nnz, 1, device=dev)
        for dtype, name, code in ((torch.float32, "float32", _lib.FLT32), (torch.bfloat16, "bfloat16", _lib.BF16)):
            x = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform").to(dtype)
            G = synth.features(n, h, torch.float32, seed=1, device=dev, kind="uniform").to(dtype)
            tv = torch.linspace(0.5, 2.0, h, device=dev)
            gathered = nnz * h * x.element_size()

            def step(fused):
                xx, tt = x.detach().requires_grad_(), tv.detach().requires_grad_()
                red.spmm_softmax(g, xx, tt, fused=fused).backward(G)
                return xx.grad, tt.grad

            for rnd in range(2):
                t = {"spmm_values_heads1": timed(lambda: attention._run_spmm_values(g, ones, x, 1), iters),
                     "softmax": timed(lambda: red._run_spmm_softmax(g, x, tv, False), iters),
                     "softmax_lse": timed(lambda: red._run_spmm_softmax(g, x, tv, True), iters)}
                fb_ms, fb_mib = peak(lambda: step(True), max(iters // 2, 1))
                sv = t["spmm_values_heads1"]
                extra = {}
                if composed:
                    with torch.no_grad():
                        c_ms, c_mib = peak(lambda: red.spmm_softmax(g, x, tv, fused=False), max(iters // 2, 1))
                    cfb_ms, cfb_mib = peak(lambda: step(False), 1)   # its spmm_values gradient is one sddmm per head: h launches
                    extra = dict(composed_forward_ms=round(c_ms, 3), composed_forward_peak_mib=round(c_mib, 1),
                                 composed_forward_over_fused=round(c_ms / t["softmax"], 2), composed_fwd_bwd_ms=round(cfb_ms, 3),
                                 composed_fwd_bwd_peak_mib=round(cfb_mib, 1), composed_fwd_bwd_over_fused=round(cfb_ms / fb_ms, 2))
                line(dtype=name, round=rnd, **{k + "_ms": round(v, 3) for k, v in t.items()},
                     softmax_over_values=round(t["softmax"] / sv, 3), softmax_lse_over_values=round(t["softmax_lse"] / sv, 3),
                     softmax_gather_tb_s=round(gathered / t["softmax"] / 1e9, 2), fwd_bwd_ms=round(fb_ms, 3), fwd_bwd_peak_mib=round(fb_mib, 1),
                     fwd_bwd_over_values=round(fb_ms / sv, 3), backward_over_values=round((fb_ms - t["softmax_lse"]) / sv, 3), **extra)
            if composed:
                (dx_f, dt_f), (dx_c, dt_c) = step(True), step(False)
                line(what="gradient check", dtype=name, dx_max_abs_fused_minus_composed=float((dx_f.float() - dx_c.float()).abs().max()),
                     dx_max_abs=float(dx_c.float().abs().max()), dt_max_abs_fused_minus_composed=float((dt_f - dt_c).abs().max()),
                     dt_max_abs=float(dt_c.abs().max()))
                del dx_f, dx_c
            line(what="workspace bytes", dtype=name, forward=_lib.spmm_softmax_workspace(code, n, nnz, h),
                 backward=_lib.spmm_softmax_backward_workspace(code, n, nnz, h), spmm_values=_lib.spmm_values_workspace(code, n, nnz, h, 1))
            del x, G
        del g, ones, rowptr, col
        torch.cuda.empty_cache()
    sink.close()
    torch.ops.pim_ops.dpu_release()


class OtherBuild:
    """another build of the library (the parent commit's libpygim_hip.so) loaded beside this one: inside ``with other:`` every call of
    pygim_amd._lib goes to it, so the two builds are timed alternately in one process on the same tensors (as scripts/exp_attention.py does)"""
    NAMES = ("pygim_init_ranks", "pygim_release", "pygim_last_error", "pygim_spmm_values", "pygim_spmm_values_workspace", "pygim_spmm_reduce",
             "pygim_spmm_reduce_workspace", "pygim_spmm_reduce_backward", "pygim_sddmm", "pygim_spmm_softmax", "pygim_spmm_softmax_workspace", "pygim_spmm_softmax_backward",
             "pygim_spmm_softmax_backward_workspace")

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


def section_edge(args):
    dev = torch.device("cuda", 0)
    iters = args.iters
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    parent = OtherBuild(args.parent_lib) if args.parent_lib else None
    out_path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exp_edge_message.txt")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    sink = open(out_path, "w")
    eps = 1e-7

    def peak(fn, reps):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        ms = timed(fn, reps)
        return ms, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    for shape, h in (("reddit", args.edge_h), ("products-mini", args.h)):
        n, nnz, d_max = synth.SHAPES[shape]
        rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
        g = attention.EdgeGraph(rowptr, col, (n, n))
        g.transposed()   # built once, outside the timings
        g.entry_ids_t()

        def line(**kw):
            text = json.dumps({"graph": shape, "h": h, "nnz": nnz, **kw})
            print(text, flush=True)
            sink.write(text + "\n")
            sink.flush()

        ones = torch.ones(nnz, 1, device=dev)
        for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
            x = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform").to(dtype)
            G = synth.features(n, h, torch.float32, seed=1, device=dev, kind="uniform").to(dtype)
            E = (torch.rand((nnz, h), device=dev, dtype=torch.float32) - 0.5).to(dtype)
            tv = torch.linspace(0.5, 2.0, h, device=dev)
            streamed = nnz * h * x.element_size()   # the bytes of E (and of dE); e_stream_tb_s counts these alone, not the gathered rows of X

            def step(fold, fused):
                xx, ee, tt = x.detach().requires_grad_(), E.detach().requires_grad_(), tv.detach().requires_grad_()
                red.spmm_edge(g, xx, ee, fold, "relu", eps, tt, fused=fused).backward(G)
                return xx.grad, ee.grad, tt.grad

            for rnd in range(2):
                for fold in ("sum", "softmax"):
                    if fold == "sum":
                        plain = timed(lambda: attention._run_spmm_values(g, ones, x, 1), iters)
                    else:
                        plain = timed(lambda: red._run_spmm_softmax(g, x, tv, False), iters)
                    fused, f_mib = peak(lambda: red._run_spmm_edge(g, x, E, fold, 1, eps, tv, False, False), iters)
                    with torch.no_grad():
                        c_ms, c_mib = peak(lambda: red.spmm_edge(g, x, E, fold, "relu", eps, tv, fused=False), max(iters // 2, 1))
                    fb_ms, fb_mib = peak(lambda: step(fold, True), max(iters // 2, 1))
                    # the composed softmax backward is one sddmm per feature (h launches): one repetition
                    cfb_ms, cfb_mib = peak(lambda: step(fold, False), 1 if fold == "softmax" else max(iters // 2, 1))
                    line(fold=fold, dtype=name, round=rnd, plain_gather_ms=round(plain, 3), fused_forward_ms=round(fused, 3),
                         fused_over_plain=round(fused / plain, 3), fused_forward_peak_mib=round(f_mib, 1), e_stream_tb_s=round(streamed / fused / 1e9, 2),
                         composed_forward_ms=round(c_ms, 3), composed_forward_peak_mib=round(c_mib, 1), composed_forward_over_fused=round(c_ms / fused, 2),
                         fused_fwd_bwd_ms=round(fb_ms, 3), fused_fwd_bwd_peak_mib=round(fb_mib, 1), composed_fwd_bwd_ms=round(cfb_ms, 3),
                         composed_fwd_bwd_peak_mib=round(cfb_mib, 1), composed_fwd_bwd_over_fused=round(cfb_ms / fb_ms, 2),
                         e_or_de_mib=round(streamed / 2 ** 20, 1))
            for fold in ("sum", "softmax"):
                (dx_f, de_f, dt_f), (dx_c, de_c, dt_c) = step(fold, True), step(fold, False)
                rec = dict(dx_max_abs_fused_minus_composed=float((dx_f.float() - dx_c.float()).abs().max()), dx_max_abs=float(dx_c.float().abs().max()),
                           de_max_abs_fused_minus_composed=float((de_f.float() - de_c.float()).abs().max()), de_max_abs=float(de_c.float().abs().max()))
                if fold == "softmax":
                    rec.update(dt_max_abs_fused_minus_composed=float((dt_f - dt_c).abs().max()), dt_max_abs=float(dt_c.abs().max()))
                line(what="gradient check", fold=fold, dtype=name, **rec)
                del dx_f, de_f, dx_c, de_c
            del E
            torch.cuda.empty_cache()
            if parent is not None:   # what existed before, this build and the parent's alternately
                def sm_step():
                    xx, tt = x.detach().requires_grad_(), tv.detach().requires_grad_()
                    red.spmm_softmax(g, xx, tt).backward(G)

                def grad_step(fn):
                    def run():
                        xx = x.detach().requires_grad_()
                        fn(xx).backward(G)
                    return run

                calls = {"spmm_values": lambda: attention._run_spmm_values(g, ones, x, 1),
                         "spmm_values_fwd_bwd": grad_step(lambda xx: attention.spmm_values(g, ones, xx)),
                         "spmm_reduce_mean_fwd_bwd": grad_step(lambda xx: red.spmm_reduce(g, xx, "mean")),
                         "spmm_reduce_mean": lambda: red._run_spmm_reduce(g, None, x, red.REDUCE_CODE["mean"], False),
                         "spmm_softmax": lambda: red._run_spmm_softmax(g, x, tv, True), "spmm_softmax_fwd_bwd": sm_step}
                if dtype == torch.float32:
                    calls["spmm_reduce_max_arg"] = lambda: red._run_spmm_reduce(g, None, x, red.REDUCE_CODE["max"], True)
                    calls["spmm_reduce_max_fwd_bwd"] = grad_step(lambda xx: red.spmm_reduce(g, xx, "max"))
                for rnd in range(2):
                    rec = {}
                    for key, fn in calls.items():
                        with parent:
                            a = timed(fn, iters)
                        b = timed(fn, iters)
                        with parent:
                            a2 = timed(fn, iters)
                        b2 = timed(fn, iters)
                        rec[key] = dict(parent_ms=[round(a, 3), round(a2, 3)], this_ms=[round(b, 3), round(b2, 3)],
                                        this_over_parent=round((b + b2) / (a + a2), 4))
                    line(what="parity with the parent build", dtype=name, round=rnd, **rec)
            del x, G
        del g, ones, rowptr, col
        torch.cuda.empty_cache()
    sink.close()
    if parent is not None:
        with parent:
            _lib.release()
    torch.ops.pim_ops.dpu_release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--section", default="reduce", choices=("reduce", "multi", "softmax", "edge"))
    ap.add_argument("--edge-h", type=int, default=32, help="--section edge: the width on the Reddit-shaped graph (E and dE are [nnz, h])")
    ap.add_argument("--parent-lib", default=None, help="--section edge: the parent commit's libpygim_hip.so, timed beside this build")
    ap.add_argument("--out", default=None, help="--section multi / softmax: where the JSON lines go (default profiles/exp_multi_reduce.txt / exp_softmax.txt)")
    args = ap.parse_args()
    if args.section == "multi":
        return section_multi(args)
    if args.section == "softmax":
        return section_softmax(args)
    if args.section == "edge":
        return section_edge(args)
    dev = torch.device("cuda", 0)
    n, nnz, d_max = synth.SHAPES[args.shape]
    h, iters = args.h, args.iters
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    g = attention.EdgeGraph(rowptr, col, (n, n))
    x = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform")
    gen = torch.Generator(device=dev).manual_seed(1)
    gathered = nnz * h * 4

    def line(**kw):
        print(json.dumps({"graph": args.shape, "h": h, "nnz": nnz, **kw}), flush=True)

    v1 = torch.rand(nnz, 1, device=dev, generator=gen)
    w = v1[:, 0].contiguous()
    MEAN, MAX = red.REDUCE_CODE["mean"], red.REDUCE_CODE["max"]
    for rnd in range(2):
        sv = timed(lambda: attention._run_spmm_values(g, v1, x, 1), iters)
        mean = timed(lambda: red._run_spmm_reduce(g, w, x, MEAN, False), iters)
        mx = timed(lambda: red._run_spmm_reduce(g, w, x, MAX, False), iters)
        mxa = timed(lambda: red._run_spmm_reduce(g, w, x, MAX, True), iters)
        mx1 = timed(lambda: red._run_spmm_reduce(g, None, x, MAX, True), iters)
        line(what="spmm_reduce vs spmm_values", round=rnd, spmm_values_heads1_ms=round(sv, 3), mean_ms=round(mean, 3), max_ms=round(mx, 3),
             max_arg_ms=round(mxa, 3), max_arg_unit_weights_ms=round(mx1, 3), mean_over_values=round(mean / sv, 3), max_over_values=round(mx / sv, 3),
             max_arg_over_values=round(mxa / sv, 3), max_arg_gather_tb_s=round(gathered / mxa / 1e9, 2))
    line(what="workspace bytes", mean=_lib.spmm_reduce_workspace(_lib.FLT32, MEAN, n, nnz, h), max=_lib.spmm_reduce_workspace(_lib.FLT32, MAX, n, nnz, h))

    # ---- the gradient of max with respect to X ----
    out, arg = red._run_spmm_reduce(g, w, x, MAX, True)
    gt, perm32 = red._transposed32(g)
    G = synth.features(n, h, torch.float32, seed=1, device=dev, kind="uniform")
    dX = torch.empty((n, h), device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def bwd():
        _lib.spmm_reduce_backward(_lib.FLT32, n, gt.rowptr.data_ptr(), gt.col.data_ptr(), perm32.data_ptr(), nnz, w.data_ptr(), G.data_ptr(), h,
                                  arg.data_ptr(), h, dX.data_ptr(), h, st)

    for rnd in range(2):
        sv = timed(lambda: attention._run_spmm_values(g, v1, x, 1), iters)
        tb = timed(bwd, iters)
        line(what="max backward", round=rnd, backward_ms=round(tb, 3), spmm_values_heads1_ms=round(sv, 3), backward_over_values=round(tb / sv, 3),
             gather_tb_s=round(2 * gathered / tb / 1e9, 2), note="the rate counts a G row and an arg row per stored entry")
    # every (row, feature) of a non-empty row has exactly one winner: the column sums of dX and of the rows' G * w[arg] agree
    won = torch.gather(w, 0, arg.clamp(min=0).long().reshape(-1)).reshape(n, h) * (arg >= 0)
    line(what="max backward check", sum_dx=float(dX.double().sum()), sum_w_g=float((won.double() * G.double()).sum()))
    del dX, G, won

    # ---- the torch composite ----
    row = g.row.long()
    colL = g.col.long()
    step = 1 << 23

    def composite():
        o = torch.full((n, h), -float("inf"), device=dev)
        for s in range(0, nnz, step):
            o.index_reduce_(0, row[s:s + step], w[s:s + step].unsqueeze(1) * x[colL[s:s + step]], "amax", include_self=True)
        return o

    tc = timed(composite, 1)
    comp = composite()
    same = bool(torch.equal(torch.where(torch.isinf(comp), torch.zeros_like(out), comp), out))
    del comp
    mxa = timed(lambda: red._run_spmm_reduce(g, w, x, MAX, True), iters)
    line(what="torch composite", index_reduce_amax_ms=round(tc, 2), max_arg_ms=round(mxa, 3), ratio=round(tc / mxa, 1), same_result=same)
    torch.ops.pim_ops.dpu_release()


if __name__ == "__main__":
    main()
