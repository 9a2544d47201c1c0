"""The backward of the aggregation on the Reddit-shaped graph (h = 256, FLT32), timed with device events after a warm-up:
creation of the A^T group, the backward product mul_t against the forward mul, and the edge-value SDDMM with the gather rate
it implies (every stored entry reads one X row of h * 4 bytes).  One JSON line.
    python scripts/exp_backward.py [--iters 20]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pygim_amd import autograd, pim_ops, synth  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--h", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, nnz, d_max = synth.SHAPES["reddit"]
    h = args.h
    rowptr, col = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    adj = SparseTensorShim(rowptr=rowptr.long(), col=col.long(), sparse_sizes=(n, n))
    A = spmm_mod.SparseTensorCOO(adj, dtype=torch.float32, format="CSR")
    A.to_pim_group(h, 1)
    x = synth.features(n, h, torch.float32, seed=0, device=dev, kind="uniform")
    g = synth.features(n, h, torch.float32, seed=1, device=dev, kind="uniform")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    A.prepare_backward(h)
    torch.cuda.synchronize()
    create_ms = (time.perf_counter() - t0) * 1e3
    fwd = timed(lambda: A.mul(x), args.iters)
    bwd = timed(lambda: A.mul_t(g), args.iters)
    rp, ci = rowptr.int().contiguous(), col.int().contiguous()
    sd = timed(lambda: autograd.sddmm(rp, ci, g, x), args.iters)
    gathered = nnz * h * 4
    print(json.dumps({"graph": "reddit", "h": h, "nnz": nnz, "create_transposed_ms": round(create_ms, 1), "forward_mul_ms": round(fwd, 3),
                      "backward_mul_t_ms": round(bwd, 3), "sddmm_ms": round(sd, 3), "sddmm_gather_tb_s": round(gathered / sd / 1e9, 2)}))
    A.free_group()
    torch.ops.pim_ops.dpu_release()


if __name__ == "__main__":
    main()
