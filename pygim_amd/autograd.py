"""Gradients through the aggregation: ``SparseTensorCOO.mul`` of the three ``backend_pim`` wrappers as a
``torch.autograd.Function``.

The CPU path's ``_shim_matmul`` (``torch.sparse_csr_tensor(...) @ other``) and ``torch_sparse.matmul`` are differentiable in
both operands; the ops this package registers under ``torch.ops.pim_ops`` have no autograd formula.  ``mul`` therefore goes
through :class:`Aggregate` when a gradient is wanted, and its backward returns

* ``dB = A^T . G`` -- one more product on the device, through the wrapper's group of A^T (``SparseGroupBase.mul_t``), with the
  shape of the ``B`` that ``mul`` was given (padding, feature windows and row blocks of the variants stay inside the forward);
* ``dvalue[e] = G[row(e)] . B[col(e)]`` -- :func:`sddmm` on the raw tensor's CSR, in its entry order -- when the raw tensor's
  ``value`` requires grad (default ``spmm`` wrapper only: grande and spmv take ``coo.int()`` in their constructors, as the
  reference does, which cuts the values off the graph).

The forward is the wrapper's plain product, unchanged: the same kernels and bits, and no A^T group until the first backward.

Not covered: ``mul_quantized`` and ``message_and_aggregate`` (``round()`` has a zero gradient there, in the reference too),
``RowShardAdj``, the C++ ``libbackend_pim.so`` shims and the raw ``torch.ops.pim_ops`` ops, double backward, and capturing the
backward into a graph.
"""
from __future__ import annotations

import torch

FLOAT_TYPES = (torch.float32, torch.float64)


def wants_grad(A, B: torch.Tensor, value) -> bool:
    """the routing rule of ``mul``: grad mode on, the dense operand (or the value) requires grad, a float group"""
    if not torch.is_grad_enabled() or A.dtype not in FLOAT_TYPES:
        return False
    return bool(B.requires_grad or (value is not None and value.requires_grad))


class Aggregate(torch.autograd.Function):
    """out = A.mul(B) (the wrapper's product); value: the raw tensor's edge values when they take part in the graph, else None"""

    @staticmethod
    def forward(ctx, A, B, value):
        ctx.A = A
        ctx.b_shape = B.shape
        ctx.save_for_backward(B if value is not None else None)
        return A._mul(B)

    @staticmethod
    def backward(ctx, G):
        A = ctx.A
        (B,) = ctx.saved_tensors
        dB = dvalue = None
        if ctx.needs_input_grad[1]:
            dB = A.mul_t(G.to(A.dtype)).reshape(ctx.b_shape)
        if ctx.needs_input_grad[2]:
            value = A.raw.storage.value()
            rowptr, col, _ = A.raw.csr()
            dvalue = sddmm(rowptr, col, G.to(A.dtype), B.to(A.dtype)).to(value.device, value.dtype)
        return None, dB, dvalue


def aggregate(A, B: torch.Tensor, value=None):
    return Aggregate.apply(A, B, value)


def sddmm(rowptr: torch.Tensor, col: torch.Tensor, G: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """``out[e] = G[row(e)] . X[col[e]]`` for every stored entry ``e`` of the CSR (rowptr [nrows + 1], col [nnz]), in stored order.

    G [nrows, h] and X [ncols, h] float32 or float64 (the same type), or both bfloat16 / both float16: the products and sums are then
    float32 and so is the result (nothing is rounded to 16 bits).  Runs on the device (pygim_sddmm: hand-written for gfx950,
    no atomics, the same bits on every run); CPU tensors are staged there and the result comes back to G's device."""
    from . import pim_ops
    from .attention import HALF_TYPES, _compute_dtype, _gather_code

    if G.dtype not in FLOAT_TYPES + HALF_TYPES or X.dtype != G.dtype:
        raise TypeError(f"sddmm: G and X must both be float32, float64, bfloat16 or float16, got {G.dtype} and {X.dtype}")
    if G.dim() != 2 or X.dim() != 2 or G.size(1) != X.size(1):
        raise ValueError(f"sddmm: G {tuple(G.shape)} and X {tuple(X.shape)} must be [*, h] with the same h")
    nrows, nnz = rowptr.numel() - 1, col.numel()
    if nrows < 0 or G.size(0) != nrows:
        raise ValueError(f"sddmm: G has {G.size(0)} rows, the CSR {nrows}")
    home = G.device
    dev = G.device
    if not G.is_cuda and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    rowptr = rowptr.to(dev, torch.int32).contiguous()
    col = col.to(dev, torch.int32).contiguous()
    # the kernel trusts its CSR (a column past X would be read out of bounds): checked here, a few small reductions
    if nnz > 0:
        bad = (rowptr[0] != 0) | (rowptr[-1] != nnz) | (rowptr[1:] < rowptr[:-1]).any() | (col.min() < 0) | (col.max() >= X.size(0))
        if bool(bad):
            raise ValueError("sddmm: rowptr must rise from 0 to nnz and every column must index a row of X")
    G = G.to(dev).contiguous()
    X = X.to(dev).contiguous()
    out = torch.empty(nnz, dtype=_compute_dtype(G.dtype), device=dev)
    if nnz > 0:
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
        pim_ops._lib.sddmm(_gather_code(G.dtype), nrows, rowptr.data_ptr(), col.data_ptr(), nnz, G.data_ptr(), G.size(1),
                           X.data_ptr(), X.size(1), G.size(1), out.data_ptr(), stream)
    return out.to(home)
