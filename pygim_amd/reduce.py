"""Aggregation with a reduction other than the sum: ``spmm_reduce`` (mean / max / min over the stored entries of every row).

``torch_sparse.matmul(adj, x, reduce=...)`` with ``"mean"``, ``"max"`` or ``"min"``: GraphSAGE's mean, max-pool SAGE, PNA- and GIN-style
layers.  A reduction other than the sum cannot be compiled into a device group, so this is a functional entry point on the plain CSR
like ``spmm_values`` (pygim_spmm_reduce, pygim_spmm_reduce_backward: hand-written gfx950 kernels, no atomics, the same bits on every
run).  Sums stay with ``mul`` / ``spmm_values``.

* mean: the sum divided by the row's number of stored entries (duplicates count; not the sum of the values); float32 / float64;
  differentiable in X and value (``spmm_values`` on the transposed structure, ``pygim_sddmm``).  X may also be bfloat16 / float16
  (value float32 or X's dtype, taken as float32): float32 sums and division, the quotient rounded once into X's dtype.
* max / min: all six element types; among equal products the lowest entry index wins and ``return_arg`` hands out that index per
  (row, feature), -1 for empty rows; differentiable in X (float32 / float64): the gradient goes to the entry that won.

Not covered: the gradient of max / min with respect to ``value`` (it needs a masked SDDMM), double backward, integer mean,
multi-head values, ``RowShardAdj`` / multi-GPU.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .attention import FLOAT_TYPES, HALF_TYPES, EdgeGraph, _backend, _compute_dtype, _gather_code, _run_spmm_values, _stream, _workspace

REDUCE_CODE = {"mean": 1, "max": 2, "min": 3}   # PYGIM_REDUCE_*


def _run_spmm_reduce(g: EdgeGraph, value, X: torch.Tensor, op: int, want_arg: bool):
    """value [nnz] (float32 beside 16-bit X) or None and X [ncols, h] contiguous on g.device -> (out [nrows, h], arg int32 [nrows, h] or None)"""
    L, _ = _backend()
    dt = _gather_code(X.dtype)
    h = X.size(1)
    out = torch.empty((g.nrows, h), dtype=X.dtype, device=g.device)
    arg = torch.empty((g.nrows, h), dtype=torch.int32, device=g.device) if want_arg else None
    if g.nrows == 0:
        return out, arg
    ws = _workspace(L.spmm_reduce_workspace(dt, op, g.nrows, g.nnz, h), g.device)
    L.spmm_reduce(dt, op, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, 0 if value is None else value.data_ptr(), X.data_ptr(),
                  X.stride(0), h, out.data_ptr(), h, 0 if arg is None else arg.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g.device))
    return out, arg


def _counts(g: EdgeGraph, dtype) -> torch.Tensor:
    """stored entries per row, at least 1 (an empty row's sum and gradient are zero whatever it is divided by)"""
    return (g.rowptr[1:] - g.rowptr[:-1]).clamp_(min=1).to(dtype)


def _transposed32(g: EdgeGraph):
    """(graph of A^T, perm as int32): what pygim_spmm_reduce_backward reads"""
    gt, perm = g.transposed()
    if getattr(gt, "_perm32", None) is None:
        gt._perm32 = perm.to(torch.int32).contiguous()
    return gt, gt._perm32


class SpmmMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, value, X):
        ctx.g = g
        ctx.save_for_backward(value, X)
        return _run_spmm_reduce(g, value, X, REDUCE_CODE["mean"], False)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        g = ctx.g
        value, X = ctx.saved_tensors
        ct = _compute_dtype(X.dtype)   # float32 beside 16-bit X and G: counts and weights are never held in 16 bits
        cnt = _counts(g, ct)
        dvalue = dX = None
        if ctx.needs_input_grad[2]:   # A_mean^T . G: the sum kernel on the transposed structure with values w / count
            gt, perm = g.transposed()
            w = 1.0 / cnt.index_select(0, g.row.long())
            if value is not None:
                w = w * value
            dX = _run_spmm_values(gt, w.index_select(0, perm).unsqueeze(1).contiguous(), G.contiguous(), 1)
        if value is not None and ctx.needs_input_grad[1]:
            L, _ = _backend()
            dvalue = torch.empty(g.nnz, dtype=ct, device=g.device)
            if g.nnz > 0:
                # 16-bit G: the dot products of G itself (float32 out), divided afterwards -- G / count would be rounded to 16 bits
                Gc = G.contiguous() if X.dtype in HALF_TYPES else (G / cnt.unsqueeze(1)).contiguous()
                L.sddmm(_gather_code(X.dtype), g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, Gc.data_ptr(), Gc.size(1), X.data_ptr(), X.stride(0),
                        X.size(1), dvalue.data_ptr(), _stream(g.device))
                if X.dtype in HALF_TYPES:
                    dvalue.div_(cnt.index_select(0, g.row.long()))
        return None, dvalue, dX


class SpmmArgReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, value, X, op, want_arg):
        need = want_arg or ctx.needs_input_grad[2]
        out, arg = _run_spmm_reduce(g, value, X, op, need)
        ctx.g = g
        ctx.save_for_backward(value, arg)
        if arg is None:
            arg = torch.empty(0, dtype=torch.int32, device=g.device)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        g = ctx.g
        value, arg = ctx.saved_tensors
        if not ctx.needs_input_grad[2]:
            return None, None, None, None, None
        L, code = _backend()
        G = G.contiguous()
        h = G.size(1)
        gt, perm32 = _transposed32(g)
        dX = torch.empty((g.ncols, h), dtype=G.dtype, device=g.device)
        if g.ncols > 0:
            L.spmm_reduce_backward(code[G.dtype], g.ncols, gt.rowptr.data_ptr(), gt.col.data_ptr(), perm32.data_ptr(), g.nnz,
                                   0 if value is None else value.data_ptr(), G.data_ptr(), h, arg.data_ptr(), h, dX.data_ptr(), h, _stream(g.device))
        return None, None, dX, None, None


def spmm_reduce(graph, X: torch.Tensor, reduce: str, value=None, return_arg: bool = False):
    """``out[r, f] = REDUCE over the stored entries e of row r of value[e] * X[col[e], f]`` (unit weights without ``value``)

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; X [columns, h]; reduce: ``"mean"`` (float32 / float64, or
    bfloat16 / float16 features: float32 arithmetic, one rounding of the result) or ``"max"`` / ``"min"`` (any of the six element
    types; no 16-bit floats); value [nnz] in X's dtype (float32 or X's dtype beside 16-bit X), in CSR entry order.  Empty rows give 0.
    ``return_arg`` (max / min): also the int32 [rows, h] index of the entry that won, -1 for empty rows; ties go to the lowest index.
    Differentiable in X (and in value for mean) for float types.  Runs on the device; CPU tensors are staged there and the results
    come back to X's device."""
    if reduce not in REDUCE_CODE:
        raise ValueError(f"spmm_reduce: reduce must be 'mean', 'max' or 'min', got {reduce!r} (sums: mul / spmm_values)")
    g = EdgeGraph.of(graph)
    op = REDUCE_CODE[reduce]
    _, code = _backend()
    half = X.dtype in HALF_TYPES
    if X.dtype not in code and not (half and reduce == "mean"):
        raise TypeError(f"spmm_reduce: unsupported element type {X.dtype}" + (" for max / min (16-bit features: mean only)" if half else ""))
    if reduce == "mean" and X.dtype not in FLOAT_TYPES and not half:
        raise TypeError(f"spmm_reduce: mean needs float32, float64, bfloat16 or float16, got {X.dtype}")
    if value is not None and value.dtype != X.dtype and not (half and value.dtype == torch.float32):
        raise TypeError(f"spmm_reduce: value and X must have one dtype (float32 values are fine beside 16-bit X), got {value.dtype} and {X.dtype}")
    if X.dim() != 2 or X.size(0) != g.ncols or X.size(1) < 1:
        raise ValueError(f"spmm_reduce: X must be [{g.ncols}, h], got {tuple(X.shape)}")
    if value is not None and (value.dim() != 1 or value.size(0) != g.nnz):
        raise ValueError(f"spmm_reduce: value must be [{g.nnz}], got {tuple(value.shape)}")
    if return_arg and reduce == "mean":
        raise ValueError("spmm_reduce: return_arg is for max / min")
    if reduce != "mean" and value is not None and value.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("spmm_reduce: the gradient of max / min with respect to value is not implemented (detach value)")
    home = X.device
    Xd = X.to(g.device).contiguous()
    vd = None if value is None else value.to(g.device, _compute_dtype(X.dtype)).contiguous()
    if reduce == "mean":
        return SpmmMean.apply(g, vd, Xd).to(home)
    out, arg = SpmmArgReduce.apply(g, vd, Xd, op, bool(return_arg))
    return (out.to(home), arg.to(home)) if return_arg else out.to(home)


def matmul_reduce(adj, B: torch.Tensor, reduce: str):
    """``torch_sparse.matmul(adj, B, reduce)`` for mean / max / min on the device: adj a SparseTensor or a ``backend_pim`` wrapper;
    its stored values (cast to B's dtype; to float32 beside 16-bit B) weigh the entries when it has them, unit weights otherwise"""
    raw = adj.raw if hasattr(adj, "raw") and hasattr(adj.raw, "csr") else adj
    value = raw.storage.value() if hasattr(raw, "storage") else None
    if value is not None:
        value = (value if reduce == "mean" else value.detach()).to(_compute_dtype(B.dtype) if reduce == "mean" else B.dtype)
    return spmm_reduce(EdgeGraph.of(adj), B, reduce, value=value)
