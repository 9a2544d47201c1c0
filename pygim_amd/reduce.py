"""Aggregation with a reduction other than the sum: ``spmm_reduce`` (mean / max / min over the stored entries of every row),
``spmm_multi_reduce`` (several statistics of the same neighbourhood -- sum, mean, min, max, var, std -- from ONE gather) and
``spmm_softmax`` (PyG's SoftmaxAggregation: a softmax per row and feature with the feature as its own score, in ONE gather).

``torch_sparse.matmul(adj, x, reduce=...)`` with ``"mean"``, ``"max"`` or ``"min"``: GraphSAGE's mean, max-pool SAGE, PNA- and GIN-style
layers.  A reduction other than the sum cannot be compiled into a device group, so this is a functional entry point on the plain CSR
like ``spmm_values`` (pygim_spmm_reduce, pygim_spmm_reduce_backward: hand-written gfx950 kernels, no atomics, the same bits on every
run).  Sums stay with ``mul`` / ``spmm_values``.

* mean: the sum divided by the row's number of stored entries (duplicates count; not the sum of the values); float32 / float64;
  differentiable in X and value (``spmm_values`` on the transposed structure, ``pygim_sddmm``).  X may also be bfloat16 / float16
  (value float32 or X's dtype, taken as float32): float32 sums and division, the quotient rounded once into X's dtype.
* max / min: all six element types; among equal products the lowest entry index wins and ``return_arg`` hands out that index per
  (row, feature), -1 for empty rows; differentiable in X (float32 / float64): the gradient goes to the entry that won.

* ``spmm_multi_reduce``: PyG's ``MultiAggregation`` / ``PNAConv`` list ``["mean", "min", "max", "std"]`` (any of ``sum``, ``mean``,
  ``min``, ``max``, ``var``, ``std``) concatenated as ``[rows, k * h]``, unit weights (pygim_spmm_multi_reduce: the sums of x and of
  x * x and the two (best, entry) pairs are held in registers beside one gather of X).  float32 / float64 / bfloat16 / float16
  (float32 arithmetic, one rounding per stored value); sum / mean and max / min have the bits of the single-statistic calls;
  var = max(mean(x^2) - mean(x)^2, 0), std = sqrt(var + eps); differentiable in X through kernels that exist (``spmm_values`` on the
  transposed structure, pygim_spmm_reduce_backward); ``fused=False`` composes the same result from ``spmm_reduce`` calls.

* ``spmm_softmax``: ``out[r, f] = sum_e softmax_e(t[f] * x[e, f]) * x[e, f]`` with a temperature per feature (pygim_spmm_softmax: the
  online-softmax triple per feature beside one gather of X; pygim_spmm_softmax_backward: one gather on the transposed structure that
  takes the probabilities again from the saved log-sum-exp).  float32 / float64 / bfloat16 / float16; differentiable in X and t;
  ``fused=False`` composes it from ``edge_softmax`` and ``spmm_values`` with ``heads = h`` through ``[nnz, h]`` tensors.

* ``spmm_edge``: messages with a feature-wide edge feature, ``msg[e, f] = act(X[col[e], f] + E[e, f]) + eps`` (GINEConv; GENConv with
  ``edge_dim``), folded per row with sum, mean, max, min or the softmax above (pygim_spmm_edge / pygim_spmm_edge_softmax: the gather of the
  same fold with ``E [nnz, h]`` read as a stream beside it; pygim_spmm_edge_backward: ``dE`` in one entry-order kernel, and ``dX`` as the
  sum of the ``dE`` rows per column through ``pygim_spmm_values`` on the transposed structure).  float32 / float64 / bfloat16 / float16
  (max / min: float32 / float64); differentiable in X, E and t; ``fused=False`` composes it through ``X[col] + E``.

Not covered: the gradient of max / min with respect to ``value`` (it needs a masked SDDMM), double backward, integer mean,
multi-head values, edge weights or integer types in ``spmm_multi_reduce``, ``spmm_softmax`` and ``spmm_edge``, forming ``E = edge_attr @ W``
inside the kernel, ``powermean``, ``RowShardAdj`` / multi-GPU.
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


# ---- several statistics of a row's stored entries in one gather ----
STAT_CODE = {"sum": 0, "mean": 1, "min": 2, "max": 3, "var": 4, "std": 5}   # PYGIM_STAT_*


def _run_multi_reduce(g: EdgeGraph, X: torch.Tensor, stats, eps: float, want_max: bool, want_min: bool):
    """X [ncols, h] contiguous on g.device, stats: PYGIM_STAT_* codes -> (out [nrows, k * h], arg_max, arg_min: int32 [nrows, h] or None)"""
    L, _ = _backend()
    dt = _gather_code(X.dtype)
    h, k = X.size(1), len(stats)
    out = torch.empty((g.nrows, k * h), dtype=X.dtype, device=g.device)
    amax = torch.empty((g.nrows, h), dtype=torch.int32, device=g.device) if want_max else None
    amin = torch.empty((g.nrows, h), dtype=torch.int32, device=g.device) if want_min else None
    if g.nrows == 0:
        return out, amax, amin
    ws = _workspace(L.spmm_multi_reduce_workspace(dt, stats, g.nrows, g.nnz, h), g.device)
    L.spmm_multi_reduce(dt, stats, eps, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, X.data_ptr(), X.stride(0), h, out.data_ptr(), k * h,
                        0 if amax is None else amax.data_ptr(), 0 if amin is None else amin.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g.device))
    return out, amax, amin


def _unit_values_t(g: EdgeGraph, dtype):
    """(graph of A^T, ones [nnz, 1]): unit-weight sums on the transposed structure through pygim_spmm_values; the ones are kept with the graph"""
    gt, _ = g.transposed()
    held = getattr(gt, "_ones", None)
    if held is None:
        held = gt._ones = {}
    if dtype not in held:
        held[dtype] = torch.ones((g.nnz, 1), dtype=dtype, device=g.device)
    return gt, held[dtype]


class SpmmMultiReduce(torch.autograd.Function):
    """forward: one pygim_spmm_multi_reduce.  backward, with n = the counts clamped to 1 and G_s the gradient block of statistic s:
        U  = (2 / n) [var > 0] (G_var + G_std / (2 std))          P = G_sum + G_mean / n - U * mean
        dX = A^T P + X * (A^T U) + spmm_reduce_backward(arg_max, G_max) + spmm_reduce_backward(arg_min, G_min)
    ([var > 0]: the subgradient of PyG's relu).  Saved: X, the mean and var-or-std blocks and the two arg tensors; nothing of size nnz."""

    @staticmethod
    def forward(ctx, g, X, names, eps, want_arg):
        stats = [STAT_CODE[s] for s in names]
        grad = ctx.needs_input_grad[1]
        out, amax, amin = _run_multi_reduce(g, X, stats, eps, "max" in names and (want_arg or grad), "min" in names and (want_arg or grad))
        ctx.g, ctx.names, ctx.eps = g, names, eps
        h = X.size(1)
        block = lambda s: out[:, names.index(s) * h:(names.index(s) + 1) * h] if s in names else None
        spread = "std" if "std" in names else ("var" if "var" in names else None)
        ctx.spread = spread
        half = X.dtype in HALF_TYPES   # 16-bit blocks are rounded: the backward takes mean and var again in float32 instead
        keep_spread = None if (spread is None or half) else block(spread)
        keep_mean = None if (spread is None or half) else block("mean")
        ctx.save_for_backward(X, keep_mean, keep_spread, amax, amin)
        empty = lambda a: torch.empty(0, dtype=torch.int32, device=g.device) if a is None else a
        amax_o, amin_o = empty(amax), empty(amin)
        ctx.mark_non_differentiable(amax_o, amin_o)
        return out, amax_o, amin_o

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _a, _b):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        g, names, eps, spread = ctx.g, ctx.names, ctx.eps, ctx.spread
        X, mean, sp, amax, amin = ctx.saved_tensors
        ct = _compute_dtype(X.dtype)
        h = X.size(1)
        Gb = lambda s: G[:, names.index(s) * h:(names.index(s) + 1) * h].to(ct) if s in names else None
        n = _counts(g, ct).unsqueeze(1)
        U = P = None
        if spread is not None:
            if sp is None:   # 16-bit X: mean and var of the forward again, in float32
                mv, _, _ = _run_multi_reduce(g, X.to(ct), [STAT_CODE["mean"], STAT_CODE["var"]], 0.0, False, False)
                mean, var = mv[:, :h], mv[:, h:]
                live, std = var > 0, torch.sqrt(var + eps)
            else:
                if mean is None:
                    mean = _run_spmm_reduce(g, None, X, REDUCE_CODE["mean"], False)[0]
                if spread == "std":   # var > 0 exactly where sqrt(var + eps) lies above sqrt(eps), up to the rounding of the sum
                    std, live = sp, sp > torch.sqrt(torch.tensor(eps, dtype=ct, device=g.device))
                else:
                    std, live = None, sp > 0
            t = Gb("var")
            if "std" in names:
                t = Gb("std") / (2 * std) if t is None else t + Gb("std") / (2 * std)
            U = (2.0 / n) * live.to(ct) * t
            P = -U * mean
        for s, w in (("sum", None), ("mean", n)):
            if s in names:
                t = Gb(s) if w is None else Gb(s) / w
                P = t if P is None else P + t
        dX = None
        if P is not None:
            gt, ones = _unit_values_t(g, ct)
            if U is None:
                dX = _run_spmm_values(gt, ones, P.contiguous(), 1)
            else:   # both products as one call on [P | U]
                both = _run_spmm_values(gt, ones, torch.cat([P, U], 1), 1)
                dX = both[:, :h] + X.to(ct) * both[:, h:]
        for s, arg in (("max", amax), ("min", amin)):
            if s in names:
                L, code = _backend()
                gt, perm32 = _transposed32(g)
                Gs = Gb(s).contiguous()
                d = torch.empty((g.ncols, h), dtype=ct, device=g.device)
                if g.ncols > 0:
                    L.spmm_reduce_backward(code[ct], g.ncols, gt.rowptr.data_ptr(), gt.col.data_ptr(), perm32.data_ptr(), g.nnz, 0, Gs.data_ptr(), h,
                                           arg.data_ptr(), h, d.data_ptr(), h, _stream(g.device))
                dX = d if dX is None else dX + d
        return None, dX.to(X.dtype), None, None, None


def _multi_reduce_composed(g: EdgeGraph, X: torch.Tensor, names, eps: float, want_arg: bool):
    """the same statistics from one spmm_reduce call each (two for var / std): the comparison of the fused call, and differentiable
    through the single calls' own gradients.  16-bit X is taken up to float32 and the result rounded once."""
    ct = _compute_dtype(X.dtype)
    Xc = X.to(ct)
    n = _counts(g, ct).unsqueeze(1)
    mean = spmm_reduce(g, Xc, "mean") if {"sum", "mean", "var", "std"} & set(names) else None
    var = None
    if {"var", "std"} & set(names):
        var = torch.relu(spmm_reduce(g, Xc * Xc, "mean") - mean * mean)
    blocks, args = [], {"max": None, "min": None}
    for s in names:
        if s in ("max", "min"):
            v, args[s] = spmm_reduce(g, Xc, s, return_arg=True)
            blocks.append(v)
        else:
            blocks.append({"sum": lambda: mean * n, "mean": lambda: mean, "var": lambda: var, "std": lambda: torch.sqrt(var + eps)}[s]())
    out = torch.cat(blocks, 1).to(X.dtype)
    return (out, args["max"], args["min"]) if want_arg else out


def spmm_multi_reduce(graph, X: torch.Tensor, reduces=("mean", "min", "max", "std"), eps: float = 1e-5, return_arg: bool = False, fused: bool = True):
    """``out[r, j * h + f] = reduces[j] over the stored entries e of row r of X[col[e], f]``: several statistics of one neighbourhood,
    concatenated in the order of ``reduces``, from one pass over the stored entries (unit weights)

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; X [columns, h] in float32, float64, bfloat16 or float16 (16-bit:
    float32 arithmetic, every stored value rounded once); reduces: distinct names among ``"sum"``, ``"mean"``, ``"min"``, ``"max"``,
    ``"var"`` (``max(mean(x^2) - mean(x)^2, 0)``, PyG's VarAggregation) and ``"std"`` (``sqrt(var + eps)``, PNAConv's formula).  Empty
    rows give 0, and ``sqrt(eps)`` for std.  ``return_arg``: returns ``(out, arg_max, arg_min)``, the int32 [rows, h] indices of the
    entries that won (-1 for empty rows; the lowest index wins a tie), ``None`` for a statistic not asked for.  Differentiable in X;
    no double backward.  ``fused=False`` composes the same result from one ``spmm_reduce`` call per statistic (two for var / std).
    Runs on the device; CPU tensors are staged there and the results come back to X's device."""
    names = tuple(reduces)
    if not names or any(s not in STAT_CODE for s in names):
        raise ValueError(f"spmm_multi_reduce: reduces must be names among {sorted(STAT_CODE)}, got {reduces!r}")
    if len(set(names)) != len(names):
        raise ValueError(f"spmm_multi_reduce: a statistic is listed twice in {reduces!r}")
    if X.dtype not in FLOAT_TYPES and X.dtype not in HALF_TYPES:
        raise TypeError(f"spmm_multi_reduce: X must be float32, float64, bfloat16 or float16, got {X.dtype}")
    g = EdgeGraph.of(graph)
    if X.dim() != 2 or X.size(0) != g.ncols or X.size(1) < 1:
        raise ValueError(f"spmm_multi_reduce: X must be [{g.ncols}, h], got {tuple(X.shape)}")
    eps = float(eps)
    if "std" in names and not (0.0 < eps < float("inf")):
        raise ValueError(f"spmm_multi_reduce: std needs a finite eps > 0, got {eps}")
    home = X.device
    Xd = X.to(g.device).contiguous()
    back = lambda a: None if a is None else a.to(home)
    if not fused:
        res = _multi_reduce_composed(g, Xd, names, eps, bool(return_arg))
        return (res[0].to(home), back(res[1]), back(res[2])) if return_arg else res.to(home)
    out, amax, amin = SpmmMultiReduce.apply(g, Xd, names, eps, bool(return_arg))
    if not return_arg:
        return out.to(home)
    return out.to(home), (amax.to(home) if "max" in names else None), (amin.to(home) if "min" in names else None)


def matmul_multi_reduce(adj, B: torch.Tensor, reduces=("mean", "min", "max", "std"), eps: float = 1e-5, fused: bool = True):
    """``spmm_multi_reduce`` on the structure of a SparseTensor or a ``backend_pim`` wrapper (its stored values are not used: unit weights)"""
    return spmm_multi_reduce(EdgeGraph.of(adj), B, reduces, eps, fused=fused)


# ---- softmax aggregation per feature in one gather ----
def _run_spmm_softmax(g: EdgeGraph, X: torch.Tensor, tv: torch.Tensor, want_lse: bool):
    """X [ncols, h] contiguous and tv [h] (compute dtype) on g.device -> (out [nrows, h] in X's dtype, lse [nrows, h] in the compute dtype or None)"""
    L, _ = _backend()
    dt = _gather_code(X.dtype)
    h = X.size(1)
    out = torch.empty((g.nrows, h), dtype=X.dtype, device=g.device)
    lse = torch.empty((g.nrows, h), dtype=tv.dtype, device=g.device) if want_lse else None
    if g.nrows == 0:
        return out, lse
    ws = _workspace(L.spmm_softmax_workspace(dt, g.nrows, g.nnz, h), g.device)
    L.spmm_softmax(dt, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, X.data_ptr(), X.stride(0), tv.data_ptr(), h, out.data_ptr(), h,
                   0 if lse is None else lse.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g.device))
    return out, lse


class SpmmSoftmax(torch.autograd.Function):
    """forward: one pygim_spmm_softmax; backward: one pygim_spmm_softmax_backward on the transposed structure, which takes the
    probabilities again from the saved log-sum-exp.  Saved: X, t, out and lse -- node-sized, nothing of size nnz."""

    @staticmethod
    def forward(ctx, g, X, tv):
        grad = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        out, lse = _run_spmm_softmax(g, X, tv, grad)
        ctx.g = g
        if grad:
            ctx.save_for_backward(X, tv, out, lse)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        g = ctx.g
        X, tv, out, lse = ctx.saved_tensors
        L, _ = _backend()
        dt = _gather_code(X.dtype)
        h = X.size(1)
        G = G.to(X.dtype).contiguous()
        gt, _ = g.transposed()
        dX = torch.empty((g.ncols, h), dtype=X.dtype, device=g.device)
        dT = torch.empty((g.ncols, h), dtype=tv.dtype, device=g.device) if ctx.needs_input_grad[2] else None
        if g.ncols > 0:
            ws = _workspace(L.spmm_softmax_backward_workspace(dt, g.ncols, g.nnz, h), g.device)
            L.spmm_softmax_backward(dt, g.ncols, gt.rowptr.data_ptr(), gt.col.data_ptr(), g.nnz, X.data_ptr(), X.stride(0), tv.data_ptr(), h, G.data_ptr(), h,
                                    out.data_ptr(), h, lse.data_ptr(), dX.data_ptr(), h, 0 if dT is None else dT.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream(g.device))
        return None, (dX if ctx.needs_input_grad[1] else None), (None if dT is None else dT.sum(0))


def _softmax_composed(g: EdgeGraph, X: torch.Tensor, tv: torch.Tensor):
    """the same aggregation from functions that exist: X[col], edge_softmax with heads = h, spmm_values with heads = h.  It holds
    several [nnz, h] tensors: the CPU-checkable and small-graph reference of the fused call.  16-bit X is taken up to float32 and the result
    rounded once."""
    from .attention import edge_softmax, spmm_values

    Xc = X.to(tv.dtype)
    p = edge_softmax(g, Xc.index_select(0, g.col.long()) * tv)
    return spmm_values(g, p, Xc, heads=X.size(1)).to(X.dtype)


def spmm_softmax(graph, X: torch.Tensor, t=1.0, fused: bool = True):
    """``out[r, f] = sum over the stored entries e of row r of softmax_e(t[f] * X[col[e], f]) * X[col[e], f]``: PyG's
    ``SoftmaxAggregation`` (``aggr="softmax"``, GENConv / DeeperGCN), a softmax per (row, feature) with the feature itself as the score

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; X [columns, h] in float32, float64, bfloat16 or float16 (16-bit:
    float32 arithmetic, the result rounded once); t: the temperature, a float, a 0-d tensor or an ``[h]`` tensor (``t = 0``: the mean;
    large ``t``: towards the max), taken to the compute dtype on the device.  Unit weights; duplicates count separately; empty rows
    give 0.  Differentiable in X and in t (one backward gather on the transposed structure, nothing of size nnz is kept or allocated);
    no double backward.  ``fused=False`` composes the same result from ``edge_softmax`` and ``spmm_values`` with ``heads = h`` and
    holds ``[nnz, h]`` tensors.  Runs on the device; CPU tensors are staged there and the result comes back to X's device."""
    if X.dtype not in FLOAT_TYPES and X.dtype not in HALF_TYPES:
        raise TypeError(f"spmm_softmax: X must be float32, float64, bfloat16 or float16, got {X.dtype}")
    g = EdgeGraph.of(graph)
    if X.dim() != 2 or X.size(0) != g.ncols or X.size(1) < 1:
        raise ValueError(f"spmm_softmax: X must be [{g.ncols}, h], got {tuple(X.shape)}")
    h = X.size(1)
    ct = _compute_dtype(X.dtype)
    if torch.is_tensor(t):
        if not t.is_floating_point():
            raise TypeError(f"spmm_softmax: t must be a float or a floating-point tensor, got {t.dtype}")
        if t.dim() > 1 or (t.dim() == 1 and t.size(0) != h):
            raise ValueError(f"spmm_softmax: t must be a scalar or [{h}], got {tuple(t.shape)}")
        tv = t.to(g.device, ct).expand(h).contiguous()   # autograd takes the gradient back to t's shape and dtype
    else:
        tv = torch.full((h,), float(t), dtype=ct, device=g.device)
    home = X.device
    Xd = X.to(g.device).contiguous()
    if not fused:
        return _softmax_composed(g, Xd, tv).to(home)
    return SpmmSoftmax.apply(g, Xd, tv).to(home)


def matmul_softmax(adj, B: torch.Tensor, t=1.0, fused: bool = True):
    """``spmm_softmax`` on the structure of a SparseTensor or a ``backend_pim`` wrapper (its stored values are not used: unit weights)"""
    if getattr(adj, "row_sharded", False):
        raise NotImplementedError("matmul_softmax is not available on a RowShardAdj (one GPU only)")
    return spmm_softmax(EdgeGraph.of(adj), B, t, fused=fused)


# ---- messages with a feature-wide edge feature: act(X[col] + E) + eps, folded per row ----
EDGE_REDUCE_CODE = {"sum": 4, "mean": 1, "max": 2, "min": 3, "softmax": 5}   # PYGIM_REDUCE_* (softmax: pygim_spmm_edge_backward's code)
ACT_CODE = {None: 0, "relu": 1}                                               # PYGIM_ACT_*


def _run_spmm_edge(g: EdgeGraph, X, E, reduce: str, act: int, eps: float, tv, want_arg: bool, want_lse: bool):
    """X [ncols, h], E [nnz, h] contiguous on g.device, tv [h] (compute dtype) for the softmax -> (out [nrows, h], arg int32 or None, lse or None)"""
    L, _ = _backend()
    dt = _gather_code(X.dtype)
    h = X.size(1)
    out = torch.empty((g.nrows, h), dtype=X.dtype, device=g.device)
    arg = torch.empty((g.nrows, h), dtype=torch.int32, device=g.device) if want_arg else None
    lse = torch.empty((g.nrows, h), dtype=_compute_dtype(X.dtype), device=g.device) if want_lse else None
    if g.nrows == 0:
        return out, arg, lse
    if reduce == "softmax":
        ws = _workspace(L.spmm_edge_softmax_workspace(dt, g.nrows, g.nnz, h), g.device)
        L.spmm_edge_softmax(dt, act, eps, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, X.data_ptr(), X.stride(0), E.data_ptr(), E.stride(0),
                            tv.data_ptr(), h, out.data_ptr(), h, 0 if lse is None else lse.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g.device))
    else:
        op = EDGE_REDUCE_CODE[reduce]
        ws = _workspace(L.spmm_edge_workspace(dt, op, g.nrows, g.nnz, h), g.device)
        L.spmm_edge(dt, op, act, eps, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, X.data_ptr(), X.stride(0), E.data_ptr(), E.stride(0), h,
                    out.data_ptr(), h, 0 if arg is None else arg.data_ptr(), ws.data_ptr(), ws.numel(), _stream(g.device))
    return out, arg, lse


def _sum_entries_per_column(g: EdgeGraph, dE: torch.Tensor) -> torch.Tensor:
    """dX[c] = the sum of the rows dE[e] over the entries e of column c, in the order of A^T: pygim_spmm_values on the transposed row
    pointer with perm as column ids, unit weights and X := dE"""
    L, _ = _backend()
    gt, ones = _unit_values_t(g, _compute_dtype(dE.dtype))
    h = dE.size(1)
    dX = torch.empty((g.ncols, h), dtype=dE.dtype, device=g.device)
    if g.ncols == 0:
        return dX
    dt = _gather_code(dE.dtype)
    ws = _workspace(L.spmm_values_workspace(dt, g.ncols, g.nnz, h, 1), g.device)
    L.spmm_values(dt, g.ncols, gt.rowptr.data_ptr(), g.entry_ids_t().data_ptr(), g.nnz, ones.data_ptr(), 1, dE.data_ptr(), h, h, dX.data_ptr(), h,
                  ws.data_ptr(), ws.numel(), _stream(g.device))
    return dX


class SpmmEdge(torch.autograd.Function):
    """forward: one pygim_spmm_edge / pygim_spmm_edge_softmax.  backward: one pygim_spmm_edge_backward writes dE in entry order -- the only
    [nnz, h] tensor it allocates -- and, the message being additive in x and e, dX is the sum of the dE rows per column (pygim_spmm_values
    on the transposed structure); dt is the column sum of the runs' partial results.  Saved: X, E and arg, or out and lse."""

    @staticmethod
    def forward(ctx, g, X, E, tv, reduce, act, eps, want_arg):
        grad = ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or (tv is not None and ctx.needs_input_grad[3])
        best = reduce in ("max", "min")
        out, arg, lse = _run_spmm_edge(g, X, E, reduce, act, eps, tv, best and (want_arg or grad), reduce == "softmax" and grad)
        ctx.g, ctx.reduce, ctx.act, ctx.eps = g, reduce, act, eps
        if grad:
            ctx.save_for_backward(X, E, tv, arg, out if reduce == "softmax" else None, lse)
        arg_o = torch.empty(0, dtype=torch.int32, device=g.device) if arg is None else arg
        ctx.mark_non_differentiable(arg_o)
        return out, arg_o

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        g, reduce = ctx.g, ctx.reduce
        X, E, tv, arg, out, lse = ctx.saved_tensors
        L, _c = _backend()
        dt = _gather_code(X.dtype)
        h = X.size(1)
        G = G.to(X.dtype).contiguous()
        op = EDGE_REDUCE_CODE[reduce]
        dE = torch.empty((g.nnz, h), dtype=X.dtype, device=g.device)
        want_dt = reduce == "softmax" and ctx.needs_input_grad[3]
        part = None
        if g.nnz > 0:
            if want_dt:
                part = torch.empty((L.spmm_edge_backward_workspace(dt, op, g.nrows, g.nnz, h), h), dtype=tv.dtype, device=g.device)
            ptr = lambda a: 0 if a is None else a.data_ptr()
            L.spmm_edge_backward(dt, op, ctx.act, ctx.eps, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, X.data_ptr(), X.stride(0), E.data_ptr(),
                                 E.stride(0), G.data_ptr(), h, ptr(arg), ptr(tv), ptr(out), h, ptr(lse), h, dE.data_ptr(), h, ptr(part), _stream(g.device))
        dX = _sum_entries_per_column(g, dE) if ctx.needs_input_grad[1] else None
        dT = None
        if want_dt:
            dT = part.sum(0) if part is not None else torch.zeros(h, dtype=tv.dtype, device=g.device)
        return None, dX, (dE if ctx.needs_input_grad[2] else None), dT, None, None, None, None


def _edge_composed(g: EdgeGraph, X, E, tv, reduce: str, act, eps: float, want_arg: bool):
    """the same aggregation through the [nnz, h] message tensor: X[col] + E, then spmm_values with ones on an identity of the entries'
    columns, spmm_reduce, or edge_softmax + spmm_values with heads = h.  16-bit operands are taken up to float32 and the result rounded once."""
    from .attention import edge_softmax, spmm_values

    ct = _compute_dtype(X.dtype)
    msg = X.to(ct).index_select(0, g.col.long()) + E.to(ct)
    if act == "relu":
        msg = torch.relu(msg)
    if eps != 0.0:
        msg = msg + eps
    # the messages as the "feature matrix" of a graph whose entry e gathers row e: the structure of A with col = arange(nnz)
    ge = EdgeGraph._bare(g.rowptr, torch.arange(g.nnz, dtype=torch.int32, device=g.device), g.row, g.nrows, g.nnz)
    arg = None
    if reduce == "sum":
        out = spmm_values(ge, torch.ones(g.nnz, dtype=ct, device=g.device), msg)
    elif reduce == "softmax":
        out = spmm_values(ge, edge_softmax(ge, msg * tv), msg, heads=msg.size(1))
    elif want_arg:
        out, arg = spmm_reduce(ge, msg, reduce, return_arg=True)
    else:
        out = spmm_reduce(ge, msg, reduce)
    return out.to(X.dtype), arg


def spmm_edge(graph, X: torch.Tensor, E: torch.Tensor, reduce: str = "sum", act=None, eps: float = 0.0, t=1.0, fused: bool = True,
              return_arg: bool = False):
    """``out[r, f] = REDUCE over the stored entries e of row r of act(X[col[e], f] + E[e, f]) + eps``: aggregation of messages that carry a
    feature-wide edge feature (PyG's GINEConv and GENConv with ``edge_dim``), without the ``[nnz, h]`` message tensor

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; X [columns, h] and E [nnz, h] of one dtype -- float32, float64,
    bfloat16 or float16 (16-bit: float32 arithmetic, the result rounded once; max / min take float32 / float64 only) -- with the rows of
    E in the stored order of the graph (``EdgeGraph.row`` / ``.col``); reduce: ``"sum"``, ``"mean"``, ``"max"``, ``"min"`` or ``"softmax"``
    (``softmax_e(t[f] * msg[e, f])`` per row and feature, ``t`` as in :func:`spmm_softmax`); act: ``None`` or ``"relu"``; eps: a float added
    after the activation.  Unit weights; empty rows give 0.  ``return_arg`` (max / min): also the int32 [rows, h] index of the entry that won,
    -1 for empty rows; ties go to the lowest index.  Differentiable in X, E and (softmax) t: the backward writes ``dE`` in one kernel -- the
    only ``[nnz, h]`` tensor it allocates -- and sums its rows per column for ``dX``; no double backward.  ``fused=False`` composes the same
    result from ``X[col] + E`` and the functions that exist.  Runs on the device; CPU tensors are staged there and the results come back
    to X's device."""
    if reduce not in EDGE_REDUCE_CODE:
        raise ValueError(f"spmm_edge: reduce must be 'sum', 'mean', 'max', 'min' or 'softmax', got {reduce!r}")
    if act not in ACT_CODE:
        raise ValueError(f"spmm_edge: act must be None or 'relu', got {act!r}")
    if X.dtype not in FLOAT_TYPES and X.dtype not in HALF_TYPES:
        raise TypeError(f"spmm_edge: X must be float32, float64, bfloat16 or float16, got {X.dtype}")
    if reduce in ("max", "min") and X.dtype in HALF_TYPES:
        raise TypeError(f"spmm_edge: unsupported element type {X.dtype} for max / min (16-bit features: sum, mean and softmax)")
    if not torch.is_tensor(E) or E.dtype != X.dtype:
        raise TypeError(f"spmm_edge: X and E must have one dtype, got {X.dtype} and {E.dtype if torch.is_tensor(E) else type(E).__name__}")
    g = EdgeGraph.of(graph)
    if X.dim() != 2 or X.size(0) != g.ncols or X.size(1) < 1:
        raise ValueError(f"spmm_edge: X must be [{g.ncols}, h], got {tuple(X.shape)}")
    h = X.size(1)
    if E.dim() != 2 or E.size(0) != g.nnz or E.size(1) != h:
        raise ValueError(f"spmm_edge: E must be [{g.nnz}, {h}] (one row per stored entry, in the order of the graph's row / col), got {tuple(E.shape)}")
    eps = float(eps)
    if eps != eps:
        raise ValueError("spmm_edge: eps is NaN")
    if return_arg and reduce not in ("max", "min"):
        raise ValueError("spmm_edge: return_arg is for max / min")
    ct = _compute_dtype(X.dtype)
    tv = None
    if reduce == "softmax":
        if torch.is_tensor(t):
            if not t.is_floating_point():
                raise TypeError(f"spmm_edge: t must be a float or a floating-point tensor, got {t.dtype}")
            if t.dim() > 1 or (t.dim() == 1 and t.size(0) != h):
                raise ValueError(f"spmm_edge: t must be a scalar or [{h}], got {tuple(t.shape)}")
            tv = t.to(g.device, ct).expand(h).contiguous()   # autograd takes the gradient back to t's shape and dtype
        else:
            tv = torch.full((h,), float(t), dtype=ct, device=g.device)
    home = X.device
    Xd = X.to(g.device).contiguous()
    Ed = E.to(g.device)
    if Ed.stride(1) != 1 or (g.nnz > 1 and Ed.stride(0) < h):
        Ed = Ed.contiguous()
    if not fused:
        out, arg = _edge_composed(g, Xd, Ed, tv, reduce, act, eps, bool(return_arg))
    else:
        out, arg = SpmmEdge.apply(g, Xd, Ed, tv, reduce, ACT_CODE[act], eps, bool(return_arg))
    return (out.to(home), arg.to(home)) if return_arg else out.to(home)


def matmul_edge(adj, B: torch.Tensor, E: torch.Tensor, reduce: str = "sum", act=None, eps: float = 0.0, t=1.0, fused: bool = True):
    """``spmm_edge`` on the structure of a SparseTensor or a ``backend_pim`` wrapper (its stored values are not used: unit weights)"""
    if getattr(adj, "row_sharded", False):
        raise NotImplementedError("matmul_edge is not available on a RowShardAdj (one GPU only)")
    return spmm_edge(EdgeGraph.of(adj), B, E, reduce, act, eps, t, fused=fused)
