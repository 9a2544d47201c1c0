"""Aggregation with edge values that are an operand of the call: ``spmm_values``, ``edge_softmax``, the fused ``gat_aggregate``,
``sparse_attention`` and ``gatv2_aggregate``, and the structure they share.

A device group (``to_pim_group``) freezes its edge values when it is created -- on the fast path they are compiled into the code
stream -- so ``mul`` multiplies by those values for as long as the group lives.  Values that change between calls (attention
weights, gates, a normalisation derived from learned quantities, or simply edge weights after ``optimizer.step()``) go through the
functions here instead: hand-written gfx950 kernels on the plain CSR (pygim_spmm_values, pygim_edge_softmax,
pygim_edge_softmax_backward: no atomics, the same bits on every run), differentiable in every floating operand.

* :class:`EdgeGraph` holds the structure once, on the device: int32 ``rowptr`` / ``col``, the row of every entry, and -- built on the
  first backward -- the transposed structure with the permutation that carries per-entry values over to it.
* :func:`spmm_values` ``out[r] = sum_e value[e, head] * X[col[e]]``; backward ``dX`` = the same kernel on the transposed structure,
  ``dvalue`` = one ``pygim_sddmm`` per head on strided views of ``G`` and ``X``.
* :func:`edge_softmax` the softmax of per-entry scores over the stored entries of every row, per head.
* :func:`gat_aggregate` the aggregation of a GAT layer in one pass (pygim_gat_aggregate): the score of an entry is
  ``leaky_relu(a_dst[row] + a_src[col])``, a function of two per-node numbers, so scores, an online softmax and the product with ``X``
  run inside the gather of ``spmm_values``.  Nothing of size nnz is written by the forward or kept for the backward (it saves
  ``a_dst``, ``a_src``, ``X``, ``out`` and the per-row ``lse``); the backward recomputes the probabilities from them.
* :func:`sparse_attention` scaled dot-product attention over the stored entries in one pass (pygim_sparse_attention): the score of an
  entry is ``scale * Q[row] . K[col]`` per head, reduced across the lanes of a head inside the gather; the forward saves ``Q``, ``K``,
  ``V``, ``out`` and ``lse``, the backward recomputes the probabilities and runs on ``pygim_sddmm`` and ``spmm_values``.
* :func:`gatv2_aggregate` the aggregation of a GATv2 layer in one pass (pygim_gatv2_aggregate): the score of an entry is
  ``sum_f att[f] * leaky_relu(x_dst[row, f] + x_src[col, f])`` per head, which no composition forms without an ``[nnz, h]`` tensor; the
  backward is fused as well (pygim_gatv2_backward, one gather on the CSR and one on the transposed CSR), nothing of size nnz is allocated.

16-bit features: ``X`` of ``spmm_values`` and ``gat_aggregate``, ``Q`` / ``K`` / ``V`` of ``sparse_attention``, ``x_dst`` / ``x_src`` of ``gatv2_aggregate`` (and of ``spmm_reduce(..., "mean")``, ``autograd.sddmm``) may be
bfloat16 or float16 -- what ``model.to(torch.bfloat16)`` and ``torch.autocast`` hand a layer.  Only the feature matrices are stored
in 16 bits: edge values, ``a_dst`` / ``a_src``, ``lse``, every partial sum and the softmax state are float32 (the wrappers upcast
16-bit values and node terms), and a result row is rounded once, to nearest even, where it is stored.  ``edge_softmax`` stays float32 /
float64.

Attention dropout (``dropout=`` of PyG's GATConv, GATv2Conv and TransformerConv): ``gat_aggregate``, ``sparse_attention`` and
``gatv2_aggregate`` take ``dropout=0.0, seed=None``.  The coefficients are dropped after the softmax and before the product with the
gathered row, inside the gather: ``out[r] = sum_e pr[e] * w[e] * v[e]`` with ``w = 1 / (1 - dropout)`` for a kept (entry, head) and 0 for a
dropped one, while the maximum, the normalisation and ``lse`` run over all entries.  The mask is a stateless hash of ``(seed, entry index
in A, head)`` (include/pygim_hip.h states it bit for bit; :func:`dropout_mask` returns it), so the fused forward, the composed and fused
backwards and the ``fused=False`` compositions drop the same entries for one seed; ``seed=None`` draws one per call from torch's default
CPU generator (``torch.manual_seed`` reproduces a run) and the backward reuses it.  ``dropout=0`` launches exactly what the call without
the argument launches.  Not covered by attention dropout: a captured graph replays the seed it was captured with; multi-GPU; heads wider
than 256 features get it through the unfused composition only.

Edge terms: ``gat_aggregate(..., a_edge=)`` and ``sparse_attention(..., bias=)`` take one scalar per stored entry and head, ``[nnz, heads]`` in
the stored order of the graph (``g.row``, ``g.col``), inside the score: ``leaky_relu(a_dst[row] + a_src[col] + a_edge[e])`` -- the edge features of
PyG's ``GATConv(edge_dim=)``, reduced to ``(lin_edge(edge_attr).view(-1, H, C) * att_edge).sum(-1)`` -- and ``scale * Q[row] . K[col] + bias[e]``, the
learned attention bias of graph transformers.  A term of ``-inf`` is a mask: probability 0, gradient 0.  The kernels read the term at the entry's
index beside the gathered row (pygim_gat_aggregate_edge, pygim_sparse_attention_bias: ``heads / h`` of the gathered bytes); the forward saves it
as the input it is and creates nothing of size nnz; the composed backwards add it when they recompute the probabilities and return its gradient, the
``ds`` they form anyway (after the leaky-ReLU factor for GAT, before the factor ``scale`` for the bias).  It combines with attention dropout; its dtype
is that of the node terms (the compute dtype, or the features' 16-bit dtype, which is upcast).  ``None`` calls exactly what the call without it calls.

Not covered: integer types, ``RowShardAdj`` / multi-GPU, double backward, capturing the backward into a graph, 16-bit device groups
(``mul``), 16-bit ``edge_softmax`` and 16-bit max / min; for ``sparse_attention`` also a fused backward kernel, the feature-wide edge embeddings
(``key_j + e``, ``value_j + e``) / ``beta`` of PyG's TransformerConv, and heads wider than 256 features in the fused kernel (they run as the three-pass
composition); for ``gatv2_aggregate`` edge features, ``fill_value`` / self loops, and heads wider than 256 features when fused.
"""
from __future__ import annotations

import torch

FLOAT_TYPES = (torch.float32, torch.float64)
HALF_TYPES = (torch.float16, torch.bfloat16)
HALF_CODE = {torch.float16: 6, torch.bfloat16: 7}   # PYGIM_FLT16 / PYGIM_BF16: feature types of the gather family only, never a group's


def _backend():
    from . import pim_ops

    L = pim_ops._lib
    if not L.is_initialized():
        L.init_ranks(1)
    return L, pim_ops.DTYPE_CODE


def _gather_code(dtype) -> int:
    """the pygim_dtype of a feature matrix of the gather family (sddmm, spmm_values, gat_aggregate, spmm_reduce mean)"""
    if dtype in HALF_CODE:
        return HALF_CODE[dtype]
    return _backend()[1][dtype]


def _compute_dtype(dtype):
    """what values, node terms, partial sums and lse are held in beside features of ``dtype``: float32 for the 16-bit types"""
    return torch.float32 if dtype in HALF_TYPES else dtype


def _device_for(t: torch.Tensor) -> torch.device:
    if t.is_cuda or not torch.cuda.is_available():
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


class EdgeGraph:
    """the CSR structure of an adjacency, on the device, for :func:`spmm_values` and :func:`edge_softmax`

    ``rowptr`` [nrows + 1] and ``col`` [nnz] (any integer type, entries in stored order; duplicates and empty rows allowed);
    ``sparse_sizes`` = (rows, columns).  The CSR is checked here, once: the kernels trust it."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, sparse_sizes):
        nrows, ncols = int(sparse_sizes[0]), int(sparse_sizes[1])
        if rowptr.dim() != 1 or col.dim() != 1 or rowptr.numel() != nrows + 1 or nrows < 0 or ncols < 0:
            raise ValueError(f"EdgeGraph: rowptr must have {nrows + 1} elements (sparse_sizes {tuple(sparse_sizes)}), got {tuple(rowptr.shape)}")
        nnz = col.numel()
        if nnz > 2 ** 31 - 1:
            raise ValueError("EdgeGraph: more than 2^31 - 1 entries")
        dev = _device_for(col)
        rp = rowptr.to(dev, torch.int64)
        cc = col.to(dev, torch.int64)
        bad = (rp[0] != 0) | (rp[-1] != nnz) | (rp[1:] < rp[:-1]).any()
        if nnz > 0:
            bad = bad | (cc.min() < 0) | (cc.max() >= ncols)
        if bool(bad):
            raise ValueError("EdgeGraph: rowptr must rise from 0 to nnz and every column must lie inside sparse_sizes")
        self.nrows, self.ncols, self.nnz, self.device = nrows, ncols, nnz, dev
        self.rowptr = rp.to(torch.int32).contiguous()
        self.col = cc.to(torch.int32).contiguous()
        self.row = torch.repeat_interleave(torch.arange(nrows, device=dev, dtype=torch.int32), rp[1:] - rp[:-1])
        self._t = None

    @classmethod
    def _bare(cls, rowptr, col, row, nrows, ncols):
        g = cls.__new__(cls)
        g.nrows, g.ncols, g.nnz, g.device = nrows, ncols, col.numel(), col.device
        g.rowptr, g.col, g.row, g._t = rowptr, col, row, None
        return g

    @classmethod
    def of(cls, adj) -> "EdgeGraph":
        """the graph of a SparseTensor / SparseTensorShim, of a ``backend_pim`` wrapper (its ``.raw``) or of an EdgeGraph; cached on
        the object it was made from"""
        if isinstance(adj, cls):
            return adj
        held = getattr(adj, "_edge_graph", None)
        if isinstance(held, cls):
            return held
        raw = adj.raw if hasattr(adj, "raw") and hasattr(adj.raw, "csr") else adj
        if not hasattr(raw, "csr"):
            raise TypeError(f"EdgeGraph.of: expected a SparseTensor, a backend_pim wrapper or an EdgeGraph, got {type(adj).__name__}")
        rowptr, col, _ = raw.csr()
        g = cls(rowptr, col, (raw.size(0), raw.size(1)))
        try:
            adj._edge_graph = g
        except AttributeError:
            pass
        return g

    def transposed(self):
        """(graph of A^T, perm): entry i of A^T is entry perm[i] of A -- the stable sort of the entries by column, the order
        pygim_group_create_transposed defines"""
        if self._t is None:
            perm = torch.argsort(self.col.long(), stable=True)
            counts = torch.bincount(self.col.long(), minlength=self.ncols)
            rowptr_t = torch.zeros(self.ncols + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(counts, 0, out=rowptr_t[1:])
            col_t = self.row[perm].contiguous()
            row_t = self.col[perm].contiguous()
            self._t = (EdgeGraph._bare(rowptr_t.to(torch.int32), col_t, row_t, self.ncols, self.nrows), perm)
        return self._t

    def entry_ids_t(self) -> torch.Tensor:
        """``perm`` of :meth:`transposed` as int32, cached: the index in A of every entry of A^T, what pygim_gatv2_backward_dropout and
        pygim_attention_dropout_mask take as ``entry_ids``"""
        if getattr(self, "_perm32", None) is None:
            self._perm32 = self.transposed()[1].to(torch.int32).contiguous()
        return self._perm32


def _workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


def _dropout_rate(name: str, p) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:   # NaN included
        raise ValueError(f"{name}: dropout must lie in [0, 1), got {p}")
    return p


def _dropout_seed(seed) -> int:
    """the 64-bit seed of a call: the caller's, or two 32-bit draws from torch's default CPU generator (``torch.manual_seed`` reproduces it)"""
    if seed is not None:
        return int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


def _edge_term(name: str, arg: str, t, g: "EdgeGraph", heads: int, feat_dtype) -> torch.Tensor:
    """the per-entry term of a score (``a_edge`` of gat_aggregate, ``bias`` of sparse_attention) checked and brought to [nnz, heads] in the
    compute dtype, contiguous, on the graph's device"""
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise TypeError(f"{name}: {arg} must be a floating-point tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    allowed = (torch.float32, feat_dtype) if feat_dtype in HALF_TYPES else (feat_dtype,)
    if t.dtype not in allowed:
        raise TypeError(f"{name}: {arg} must be {' or '.join(str(d) for d in allowed)} beside {feat_dtype} features, got {t.dtype}")
    if t.dim() == 1 and heads == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2 or t.size(0) != g.nnz or t.size(1) != heads:
        raise ValueError(f"{name}: {arg} must be [{g.nnz}, {heads}]" + (f" or [{g.nnz}]" if heads == 1 else "") +
                         f" (one row per stored entry, in the order of the graph's row / col), got {tuple(t.shape)}")
    return t.to(g.device, _compute_dtype(feat_dtype)).contiguous()


def dropout_mask(graph, heads: int, p: float, seed: int, dtype=torch.float32, transposed: bool = False) -> torch.Tensor:
    """the weights of attention dropout, ``[nnz, heads]`` on the graph's device: ``1 / (1 - p)`` where (entry, head) is kept, 0 where it
    is dropped (pygim_attention_dropout_mask; the mask function is specified in include/pygim_hip.h).  A pure function of
    ``(seed, entry index in A, head)``: the fused kernels with the same ``p`` and ``seed`` drop the same entries.  ``transposed=True``
    gives the rows in the order of ``EdgeGraph.transposed()`` (row i belongs to entry ``perm[i]`` of A).  float32 or float64."""
    p = _dropout_rate("dropout_mask", p)
    g = EdgeGraph.of(graph)
    heads = int(heads)
    if heads < 1:
        raise ValueError(f"dropout_mask: heads must be at least 1, got {heads}")
    if dtype not in FLOAT_TYPES:
        raise TypeError(f"dropout_mask: dtype must be float32 or float64, got {dtype}")
    L, code = _backend()
    w = torch.empty((g.nnz, heads), dtype=dtype, device=g.device)
    if g.nnz > 0:
        ids = g.entry_ids_t().data_ptr() if transposed else 0
        L.attention_dropout_mask(code[dtype], g.nnz, heads, ids, p, _dropout_seed(seed), w.data_ptr(), _stream(g.device))
    return w


def _run_spmm_values(g: EdgeGraph, value: torch.Tensor, X: torch.Tensor, heads: int) -> torch.Tensor:
    """value [nnz, heads] (float32 beside 16-bit X, else X's dtype) and X [ncols, h] contiguous on g.device -> [nrows, h] in X's dtype"""
    L, _ = _backend()
    dt = _gather_code(X.dtype)
    h = X.size(1)
    out = torch.empty((g.nrows, h), dtype=X.dtype, device=g.device)
    if g.nrows == 0:
        return out
    nbytes = L.spmm_values_workspace(dt, g.nrows, g.nnz, h, heads)
    ws = _workspace(nbytes, g.device)
    L.spmm_values(dt, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, value.data_ptr(), heads, X.data_ptr(), X.stride(0), h,
                  out.data_ptr(), h, ws.data_ptr(), ws.numel(), _stream(g.device))
    return out


class SpmmValues(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, value, X, heads):
        ctx.g, ctx.heads = g, heads
        ctx.save_for_backward(value, X)
        return _run_spmm_values(g, value, X, heads)

    @staticmethod
    def backward(ctx, G):
        g, heads = ctx.g, ctx.heads
        value, X = ctx.saved_tensors
        G = G.contiguous()
        dvalue = dX = None
        if ctx.needs_input_grad[2]:
            gt, perm = g.transposed()
            dX = _run_spmm_values(gt, value.index_select(0, perm), G, heads)
        if ctx.needs_input_grad[1]:
            L, _ = _backend()
            h = X.size(1)
            hd, es = h // heads, X.element_size()
            per_head = torch.empty((heads, g.nnz), dtype=value.dtype, device=g.device)   # float32 beside 16-bit G and X
            if g.nnz > 0:
                for k in range(heads):   # G[:, k * hd:(k + 1) * hd] . X[:, k * hd:(k + 1) * hd] per entry: strided views of both
                    L.sddmm(_gather_code(X.dtype), g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, G.data_ptr() + k * hd * es, h,
                            X.data_ptr() + k * hd * es, X.stride(0), hd, per_head[k].data_ptr(), _stream(g.device))
            dvalue = per_head.t().contiguous()
        return None, dvalue, dX, None


def spmm_values(graph, value: torch.Tensor, X: torch.Tensor, heads: int = 1) -> torch.Tensor:
    """``out[r, f] = sum over the stored entries e of row r of value[e, f // (h // heads)] * X[col[e], f]``

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; value [nnz] (heads = 1) or [nnz, heads]; X [columns, h] with
    ``h % heads == 0``; value and X both float32 or both float64.  X may also be bfloat16 / float16 with value float32 or X's dtype:
    the values are then taken as float32, the sums are float32 and ``out`` (X's dtype) is rounded once per element.  Differentiable
    in value and X, each gradient in its operand's dtype (``dX``: the same kernel on the transposed structure; ``dvalue``: a float32
    ``pygim_sddmm``).  Runs on the device; CPU tensors are staged there and the result comes back to X's device."""
    g = EdgeGraph.of(graph)
    heads = int(heads)
    if X.dtype in HALF_TYPES:
        if value.dtype not in (torch.float32, X.dtype):
            raise TypeError(f"spmm_values: beside {X.dtype} features value must be float32 or {X.dtype}, got {value.dtype}")
    elif X.dtype not in FLOAT_TYPES or value.dtype != X.dtype:
        raise TypeError(f"spmm_values: value and X must both be float32 or float64 (or X bfloat16 / float16), got {value.dtype} and {X.dtype}")
    if X.dim() != 2 or X.size(0) != g.ncols:
        raise ValueError(f"spmm_values: X must be [{g.ncols}, h], got {tuple(X.shape)}")
    if heads < 1 or X.size(1) < 1 or X.size(1) % heads != 0:
        raise ValueError(f"spmm_values: heads = {heads} must divide h = {X.size(1)}")
    if value.dim() == 1 and heads == 1:
        value = value.unsqueeze(1)
    if value.dim() != 2 or value.size(0) != g.nnz or value.size(1) != heads:
        raise ValueError(f"spmm_values: value must be [{g.nnz}] or [{g.nnz}, {heads}], got {tuple(value.shape)}")
    home = X.device
    out = SpmmValues.apply(g, value.to(g.device, _compute_dtype(X.dtype)).contiguous(), X.to(g.device).contiguous(), heads)
    return out.to(home)


def _run_edge_softmax(g: EdgeGraph, a: torch.Tensor, b, heads: int) -> torch.Tensor:
    L, code = _backend()
    out = torch.empty_like(a)
    if g.nnz == 0:
        return out
    ws = _workspace(L.edge_softmax_workspace(code[a.dtype], g.nrows, g.nnz, heads), g.device)
    if b is None:
        L.edge_softmax(code[a.dtype], g.nrows, g.rowptr.data_ptr(), g.nnz, a.data_ptr(), heads, out.data_ptr(), ws.data_ptr(), ws.numel(),
                       _stream(g.device))
    else:
        L.edge_softmax_backward(code[a.dtype], g.nrows, g.rowptr.data_ptr(), g.nnz, a.data_ptr(), b.data_ptr(), heads, out.data_ptr(),
                                ws.data_ptr(), ws.numel(), _stream(g.device))
    return out


class EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, scores, heads):
        ctx.g, ctx.heads = g, heads
        P = _run_edge_softmax(g, scores, None, heads)
        ctx.save_for_backward(P)
        return P

    @staticmethod
    def backward(ctx, dP):
        (P,) = ctx.saved_tensors
        return None, _run_edge_softmax(ctx.g, P, dP.contiguous(), ctx.heads), None


def edge_softmax(graph, scores: torch.Tensor) -> torch.Tensor:
    """softmax of ``scores`` ([nnz] or [nnz, heads], float32 / float64, one score per stored entry and head) over the stored entries
    of every row, per head: ``exp(s - max) / sum exp(s - max)``; duplicates are separate entries.  Differentiable; same shape as
    ``scores``, on its device."""
    g = EdgeGraph.of(graph)
    if scores.dtype not in FLOAT_TYPES:
        raise TypeError(f"edge_softmax: scores must be float32 or float64, got {scores.dtype}")
    if scores.dim() not in (1, 2) or scores.size(0) != g.nnz or (scores.dim() == 2 and scores.size(1) < 1):
        raise ValueError(f"edge_softmax: scores must be [{g.nnz}] or [{g.nnz}, heads], got {tuple(scores.shape)}")
    heads = 1 if scores.dim() == 1 else scores.size(1)
    home = scores.device
    P = EdgeSoftmax.apply(g, scores.to(g.device).reshape(g.nnz, heads).contiguous(), heads)
    return P.reshape(scores.shape).to(home)


def _run_gat_aggregate(g: EdgeGraph, a_dst, a_src, X, heads: int, slope: float, want_lse: bool, p: float = 0.0, seed: int = 0, a_edge=None):
    """a_dst [nrows, heads], a_src [ncols, heads] (float32 beside 16-bit X, else X's dtype), X [ncols, h] contiguous on g.device ->
    (out [nrows, h] in X's dtype, lse [nrows, heads] in a_dst's or None).  a_edge: None, or the per-entry term [nnz, heads] in a_dst's
    dtype, contiguous (pygim_gat_aggregate_edge)"""
    L, _ = _backend()
    dt = _gather_code(X.dtype)
    h = X.size(1)
    out = torch.empty((g.nrows, h), dtype=X.dtype, device=g.device)
    lse = torch.empty((g.nrows, heads), dtype=a_dst.dtype, device=g.device) if want_lse else None   # float32 beside 16-bit X
    if g.nrows == 0:
        return out, lse
    ws = _workspace(L.gat_aggregate_workspace(dt, g.nrows, g.nnz, h, heads), g.device)
    args = (dt, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, a_dst.data_ptr(), a_src.data_ptr(), heads, slope,
            X.data_ptr(), X.stride(0), h, out.data_ptr(), h, lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(), _stream(g.device))
    if a_edge is not None:
        L.gat_aggregate_edge(*args, a_edge.data_ptr(), p, seed)
    elif p > 0.0:
        L.gat_aggregate_dropout(*args, p, seed)
    else:   # exactly the call without the argument
        L.gat_aggregate(*args)
    return out, lse


class GatAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, a_dst, a_src, X, slope, p, seed, a_edge=None):
        heads = a_src.size(1)
        need = any(ctx.needs_input_grad[1:4]) or (a_edge is not None and ctx.needs_input_grad[7])
        out, lse = _run_gat_aggregate(g, a_dst, a_src, X, heads, slope, need, p, seed, a_edge)
        if need:
            ctx.g, ctx.heads, ctx.slope, ctx.p, ctx.seed = g, heads, slope, p, seed
            if a_edge is None:
                ctx.save_for_backward(a_dst, a_src, X, out, lse)   # node-sized, all of them
            else:
                ctx.save_for_backward(a_dst, a_src, X, out, lse, a_edge)   # and the term: an input of the call, nothing new of size nnz
        return out

    @staticmethod
    def backward(ctx, G):
        g, heads, slope = ctx.g, ctx.heads, ctx.slope
        a_dst, a_src, X, out, lse = ctx.saved_tensors[:5]
        a_edge = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        want_edge = a_edge is not None and ctx.needs_input_grad[7]
        G = G.contiguous()
        h = X.size(1)
        hd = h // heads
        row, col = g.row.long(), g.col.long()
        gt, perm = g.transposed()
        # the probabilities again, from the node terms and the row's log-sum-exp: [nnz, heads], transient; in place where a tensor is done
        # with.  The peak is at dp.t().contiguous(): p, dp, ds and the byte mask neg, beside the int64 row / col / perm indices
        p = a_dst.index_select(0, row).add_(a_src.index_select(0, col))
        if a_edge is not None:
            p.add_(a_edge)   # the term of the entry, before the leaky ReLU as in the kernel; -inf gives p = 0 and ds = 0
        neg = p < 0
        torch.nn.functional.leaky_relu_(p, slope)
        p.sub_(lse.index_select(0, row)).exp_()
        # attention dropout: w per (entry, head) again from the seed; dX gathers p * w, dp below becomes w * G . x
        w = dropout_mask(g, heads, ctx.p, ctx.seed, p.dtype) if ctx.p > 0.0 else None
        if ctx.needs_input_grad[3]:
            dX = _run_spmm_values(gt, (p if w is None else p * w).index_select(0, perm), G, heads)
        else:
            dX = None
        da_dst = da_src = da_edge = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or want_edge:
            L, _ = _backend()
            es = X.element_size()
            ct = a_dst.dtype   # float32 beside 16-bit G, X and out: p, dp, delta and ds are never held in 16 bits
            dp = torch.empty((heads, g.nnz), dtype=ct, device=g.device)
            if g.nnz > 0:
                for k in range(heads):   # G[:, k * hd:(k + 1) * hd] . X[:, k * hd:(k + 1) * hd] per entry, as SpmmValues.backward does
                    L.sddmm(_gather_code(X.dtype), g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, G.data_ptr() + k * hd * es, h,
                            X.data_ptr() + k * hd * es, X.stride(0), hd, dp[k].data_ptr(), _stream(g.device))
            ds = dp.t().contiguous()
            del dp
            if w is not None:
                ds.mul_(w)
            del w
            if X.dtype in HALF_TYPES:
                # out was rounded to 16 bits when it was stored: G . out would carry that rounding (2^-9 of sum |G . out|) into every
                # gradient of a row.  sum_e p * dp itself, as a float32 row sum per head (the gather of da_dst below)
                delta = _run_spmm_values(g, p * ds, torch.ones((g.ncols, heads), dtype=ct, device=g.device), heads)
            else:
                delta = (G * out).view(g.nrows, heads, hd).sum(-1)   # = sum_e p * dp per (row, head), without a pass over the entries
            ds.sub_(delta.index_select(0, row)).mul_(p)
            del p
            one = torch.ones((), dtype=ct, device=g.device)
            ds.mul_(torch.where(neg, one * slope, one))   # ds = p * (dp - delta[row]) * leaky_relu'(z)
            del neg
            # the two sums per head run on ones of the compute type (FLT32 beside 16-bit features: a 16-bit call would round a sum over
            # a whole row to 8 or 11 bits)
            if ctx.needs_input_grad[1]:   # row sums per head
                da_dst = _run_spmm_values(g, ds, torch.ones((g.ncols, heads), dtype=ct, device=g.device), heads)
            if ctx.needs_input_grad[2]:   # column sums per head
                da_src = _run_spmm_values(gt, ds.index_select(0, perm), torch.ones((g.nrows, heads), dtype=ct, device=g.device), heads)
            if want_edge:   # z is linear in the term: its gradient is ds itself
                da_edge = ds
        return None, da_dst, da_src, dX, None, None, None, da_edge


def gat_aggregate(graph, a_dst: torch.Tensor, a_src: torch.Tensor, X: torch.Tensor, negative_slope: float = 0.2, dropout: float = 0.0,
                  seed=None, a_edge=None) -> torch.Tensor:
    """the aggregation of a GAT layer, fused: with ``k = f // (h // heads)`` and e over the stored entries of row r

    ``out[r, f] = sum_e softmax_e(leaky_relu(a_dst[r, k] + a_src[col[e], k], negative_slope)) * X[col[e], f]``

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; a_dst [rows, heads] and a_src [columns, heads] (1-D: one head);
    X [columns, h] with ``h % heads == 0``; all three float32 or all float64.  X may also be bfloat16 / float16, with a_dst and a_src
    both float32 or both X's dtype: they are taken as float32, the softmax state and the sums are float32 and ``out`` (X's dtype) is
    rounded once per element; every gradient comes back in its operand's dtype.  Empty rows give 0; duplicates are separate entries.
    One kernel, one pass over the entries; what ``edge_softmax`` + ``spmm_values`` on the composed scores give, without the
    ``[nnz, heads]`` score and probability tensors.  Differentiable in ``a_dst``, ``a_src`` and ``X``: the forward saves only
    node-sized tensors, the backward recomputes the probabilities and runs on ``spmm_values`` and ``pygim_sddmm`` (deterministic; its
    ``[nnz, heads]`` tensors are transient, a fused backward kernel is not part of this).  Runs on the device; CPU tensors are staged
    there and the result comes back to X's device.  No double backward.

    ``dropout`` in [0, 1): attention dropout, PyG's ``GATConv(dropout=)`` -- every coefficient is dropped with that probability after the
    softmax, the kept ones are scaled by ``1 / (1 - dropout)``, inside the gather (see the module docstring).  ``seed``: 64 bits; ``None``
    draws one per call from torch's default CPU generator.  0 is the call without the argument, bit for bit.

    ``a_edge``: a term per stored entry and head, ``[nnz, heads]`` (1-D: one head) in the stored order of the graph (``g.row``, ``g.col``):
    the score becomes ``leaky_relu(a_dst[r, k] + a_src[col[e], k] + a_edge[e, k])`` -- the edge features of PyG's ``GATConv(edge_dim=)``
    (``a_edge = (lin_edge(edge_attr).view(-1, H, C) * att_edge).sum(-1)``); ``-inf`` masks an (entry, head): probability 0, gradient 0.
    Its dtype follows ``a_dst`` / ``a_src``.  Read inside the gather (pygim_gat_aggregate_edge); it is saved for the backward as the input
    it is, and its gradient is the ``ds`` the backward forms anyway.  ``None`` is the call without the argument."""
    dropout = _dropout_rate("gat_aggregate", dropout)
    g = EdgeGraph.of(graph)
    if X.dtype in HALF_TYPES:
        if a_dst.dtype != a_src.dtype or a_dst.dtype not in (torch.float32, X.dtype):
            raise TypeError(f"gat_aggregate: beside {X.dtype} features a_dst and a_src must both be float32 or both {X.dtype}, "
                            f"got {a_dst.dtype} and {a_src.dtype}")
    elif X.dtype not in FLOAT_TYPES or a_dst.dtype != X.dtype or a_src.dtype != X.dtype:
        raise TypeError(f"gat_aggregate: a_dst, a_src and X must all be float32 or float64 (or X bfloat16 / float16), "
                        f"got {a_dst.dtype}, {a_src.dtype} and {X.dtype}")
    if a_src.dim() == 1 and a_dst.dim() == 1:
        a_src, a_dst = a_src.unsqueeze(1), a_dst.unsqueeze(1)
    if a_src.dim() != 2 or a_dst.dim() != 2 or a_src.size(1) < 1 or a_dst.size(1) != a_src.size(1):
        raise ValueError(f"gat_aggregate: a_dst and a_src must both be 1-D or both [nodes, heads], got {tuple(a_dst.shape)} and {tuple(a_src.shape)}")
    heads = a_src.size(1)
    if a_dst.size(0) != g.nrows or a_src.size(0) != g.ncols:
        raise ValueError(f"gat_aggregate: a_dst must be [{g.nrows}, {heads}] and a_src [{g.ncols}, {heads}], got {tuple(a_dst.shape)} and {tuple(a_src.shape)}")
    if X.dim() != 2 or X.size(0) != g.ncols:
        raise ValueError(f"gat_aggregate: X must be [{g.ncols}, h], got {tuple(X.shape)}")
    if X.size(1) < 1 or X.size(1) % heads != 0:
        raise ValueError(f"gat_aggregate: heads = {heads} must divide h = {X.size(1)}")
    home = X.device
    ct = _compute_dtype(X.dtype)
    operands = (g, a_dst.to(g.device, ct).contiguous(), a_src.to(g.device, ct).contiguous(), X.to(g.device).contiguous(),
                float(negative_slope), dropout, _dropout_seed(seed) if dropout > 0.0 else 0)
    if a_edge is None:
        out = GatAggregate.apply(*operands)
    else:
        out = GatAggregate.apply(*operands, _edge_term("gat_aggregate", "a_edge", a_edge, g, heads, X.dtype))
    return out.to(home)


SA_MAX_HEAD = 256   # features of one head the fused kernel takes (include/pygim_hip.h); wider heads run as the three-pass composition


def _head_dots(g: EdgeGraph, A: torch.Tensor, B: torch.Tensor, heads: int) -> torch.Tensor:
    """[nnz, heads]: ``A[row(e), head k] . B[col[e], head k]`` for every stored entry, one ``pygim_sddmm`` per head on strided views of
    A [nrows, h] and B [ncols, h] (contiguous, on g.device, one dtype); float32 beside 16-bit operands, else their dtype"""
    L, _ = _backend()
    h = A.size(1)
    hd, es = h // heads, A.element_size()
    per_head = torch.empty((heads, g.nnz), dtype=_compute_dtype(A.dtype), device=g.device)
    if g.nnz > 0:
        for k in range(heads):
            L.sddmm(_gather_code(A.dtype), g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, A.data_ptr() + k * hd * es, A.stride(0),
                    B.data_ptr() + k * hd * es, B.stride(0), hd, per_head[k].data_ptr(), _stream(g.device))
    return per_head.t().contiguous()


class HeadScores(torch.autograd.Function):
    """``s[e, k] = scale * Q[row(e), head k] . K[col[e], head k]``: the scores of the three-pass composition"""

    @staticmethod
    def forward(ctx, g, Q, K, heads, scale):
        ctx.g, ctx.heads, ctx.scale = g, heads, scale
        ctx.save_for_backward(Q, K)
        return _head_dots(g, Q, K, heads).mul_(scale)

    @staticmethod
    def backward(ctx, dS):
        g, heads = ctx.g, ctx.heads
        Q, K = ctx.saved_tensors
        dS = dS * ctx.scale
        dQ = _run_spmm_values(g, dS, K, heads) if ctx.needs_input_grad[1] else None
        dK = None
        if ctx.needs_input_grad[2]:
            gt, perm = g.transposed()
            dK = _run_spmm_values(gt, dS.index_select(0, perm), Q, heads)
        return None, dQ, dK, None, None


def _run_sparse_attention(g: EdgeGraph, Q, K, V, heads: int, scale: float, want_lse: bool, p: float = 0.0, seed: int = 0, bias=None):
    """Q [nrows, h], K and V [ncols, h] contiguous on g.device, one dtype -> (out [nrows, h] in that dtype, lse [nrows, heads] in the
    compute dtype or None).  bias: None, or the per-entry term [nnz, heads] in the compute dtype, contiguous (pygim_sparse_attention_bias)"""
    L, _ = _backend()
    dt = _gather_code(Q.dtype)
    h = Q.size(1)
    out = torch.empty((g.nrows, h), dtype=Q.dtype, device=g.device)
    lse = torch.empty((g.nrows, heads), dtype=_compute_dtype(Q.dtype), device=g.device) if want_lse else None
    if g.nrows == 0:
        return out, lse
    ws = _workspace(L.sparse_attention_workspace(dt, g.nrows, g.nnz, h, heads), g.device)
    args = (dt, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0),
            V.data_ptr(), V.stride(0), h, heads, scale, out.data_ptr(), h, lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(),
            _stream(g.device))
    if bias is not None:
        L.sparse_attention_bias(*args, bias.data_ptr(), p, seed)
    elif p > 0.0:
        L.sparse_attention_dropout(*args, p, seed)
    else:
        L.sparse_attention(*args)
    return out, lse


class SparseAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, Q, K, V, heads, scale, p, seed, bias=None):
        need = any(ctx.needs_input_grad[1:4]) or (bias is not None and ctx.needs_input_grad[8])
        out, lse = _run_sparse_attention(g, Q, K, V, heads, scale, need, p, seed, bias)
        if need:
            ctx.g, ctx.heads, ctx.scale, ctx.p, ctx.seed = g, heads, scale, p, seed
            if bias is None:
                ctx.save_for_backward(Q, K, V, out, lse)   # node-sized, all of them
            else:
                ctx.save_for_backward(Q, K, V, out, lse, bias)   # and the term: an input of the call, nothing new of size nnz
        return out

    @staticmethod
    def backward(ctx, G):
        g, heads, scale = ctx.g, ctx.heads, ctx.scale
        Q, K, V, out, lse = ctx.saved_tensors[:5]
        bias = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        want_bias = bias is not None and ctx.needs_input_grad[8]
        G = G.contiguous()
        hd = Q.size(1) // heads
        row = g.row.long()
        gt, perm = g.transposed()
        # the probabilities again, from the scores and the row's log-sum-exp: [nnz, heads], transient, in the compute dtype
        p = _head_dots(g, Q, K, heads).mul_(scale)
        if bias is not None:
            p.add_(bias)   # the term of the entry, after the scaling as in the kernel; -inf gives p = 0 and ds = 0
        p.sub_(lse.index_select(0, row)).exp_()
        # attention dropout: w per (entry, head) again from the seed; dV gathers p * w, dP becomes w * G . v
        w = dropout_mask(g, heads, ctx.p, ctx.seed, p.dtype) if ctx.p > 0.0 else None
        dV = _run_spmm_values(gt, (p if w is None else p * w).index_select(0, perm), G, heads) if ctx.needs_input_grad[3] else None
        dQ = dK = dbias = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or want_bias:
            ds = _head_dots(g, G, V, heads)   # dP
            if w is not None:
                ds.mul_(w)
            del w
            if Q.dtype in HALF_TYPES:
                # out was rounded to 16 bits when it was stored (GatAggregate.backward): sum_e p * dp itself, as a float32 row sum per head
                delta = _run_spmm_values(g, p * ds, torch.ones((g.ncols, heads), dtype=p.dtype, device=g.device), heads)
            else:
                delta = (G * out).view(g.nrows, heads, hd).sum(-1)   # = sum_e p * dp per (row, head), without a pass over the entries
            ds.sub_(delta.index_select(0, row)).mul_(p)   # P * (dP - delta[row]): the gradient of the score, and of the term
            del p
            if want_bias:
                dbias = ds.clone() if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] else ds
            if dbias is not ds:
                ds.mul_(scale)   # dS = scale * P * (dP - delta[row])
            if ctx.needs_input_grad[1]:
                dQ = _run_spmm_values(g, ds, K, heads)
            if ctx.needs_input_grad[2]:
                dK = _run_spmm_values(gt, ds.index_select(0, perm), Q, heads)
        return None, dQ, dK, dV, None, None, None, None, dbias


def sparse_attention(graph, Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, heads: int = 1, scale=None, fused: bool = True, dropout: float = 0.0,
                     seed=None, bias=None) -> torch.Tensor:
    """scaled dot-product attention over the stored entries: with ``hd = h // heads``, ``k = f // hd`` and e over the entries of row r

    ``out[r, f] = sum_e softmax_e(scale * Q[r, head k] . K[col[e], head k]) * V[col[e], f]``

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; Q [rows, h], K and V [columns, h] with ``h % heads == 0``; all
    float32, all float64, or all three the same 16-bit type (products, scores, softmax state and sums are then float32 and ``out`` is
    rounded once per element).  ``scale`` defaults to ``1 / sqrt(h // heads)``.  Empty rows give 0; duplicates are separate entries.
    ``fused=True``: one kernel, one pass over the entries (pygim_sparse_attention), nothing of size nnz written or saved -- the
    backward recomputes the probabilities from ``Q``, ``K`` and the per-row ``lse`` and runs on ``pygim_sddmm`` and ``spmm_values``
    (deterministic; its ``[nnz, heads]`` tensors are transient).  ``fused=False``: the three-pass composition -- per-head sddmm scores,
    ``edge_softmax``, ``spmm_values`` -- which heads wider than 256 features take in either case.  Differentiable in Q, K and V, each
    gradient in its operand's dtype; no double backward.  Runs on the device; CPU tensors are staged there and the result comes back
    to Q's device.

    ``dropout`` in [0, 1), ``seed``: attention dropout as in :func:`gat_aggregate` (PyG's ``TransformerConv(dropout=)``).  With one seed
    ``fused=True`` and ``fused=False`` drop the same entries: the composition multiplies the ``edge_softmax`` result by
    :func:`dropout_mask`.

    ``bias``: a term per stored entry and head, ``[nnz, heads]`` (1-D: one head) in the stored order of the graph (``g.row``, ``g.col``):
    the score becomes ``scale * Q[r, head k] . K[col[e], head k] + bias[e, k]`` -- the learned attention bias of graph transformers
    (Graphormer, SAN, GPS); ``-inf`` masks an (entry, head): probability 0, gradient 0.  float32 / float64 like Q, float32 or Q's dtype beside
    16-bit Q.  ``fused=True`` reads it inside the gather (pygim_sparse_attention_bias) and saves it as the input it is; its gradient is
    ``P * (dP - delta[row])``, the gradient of the score before the factor ``scale``.  ``fused=False`` and wide heads add it to the composed
    scores.  The feature-wide edge embeddings of PyG's ``TransformerConv(edge_dim=)`` are not covered.  ``None`` is the call without it."""
    dropout = _dropout_rate("sparse_attention", dropout)
    g = EdgeGraph.of(graph)
    heads = int(heads)
    if Q.dtype not in FLOAT_TYPES + HALF_TYPES or K.dtype != Q.dtype or V.dtype != Q.dtype:
        raise TypeError(f"sparse_attention: Q, K and V must all be float32, float64, bfloat16 or float16, got {Q.dtype}, {K.dtype} and {V.dtype}")
    if Q.dim() != 2 or Q.size(0) != g.nrows:
        raise ValueError(f"sparse_attention: Q must be [{g.nrows}, h], got {tuple(Q.shape)}")
    h = Q.size(1)
    if K.dim() != 2 or V.dim() != 2 or tuple(K.shape) != (g.ncols, h) or tuple(V.shape) != (g.ncols, h):
        raise ValueError(f"sparse_attention: K and V must be [{g.ncols}, {h}], got {tuple(K.shape)} and {tuple(V.shape)}")
    if heads < 1 or h < 1 or h % heads != 0:
        raise ValueError(f"sparse_attention: heads = {heads} must divide h = {h}")
    hd = h // heads
    scale = hd ** -0.5 if scale is None else float(scale)
    home = Q.device
    q, k, v = (t.to(g.device).contiguous() for t in (Q, K, V))
    seed = _dropout_seed(seed) if dropout > 0.0 else 0
    if bias is not None:
        bias = _edge_term("sparse_attention", "bias", bias, g, heads, Q.dtype)
    if fused and hd <= SA_MAX_HEAD:
        if bias is None:
            out = SparseAttention.apply(g, q, k, v, heads, scale, dropout, seed)
        else:
            out = SparseAttention.apply(g, q, k, v, heads, scale, dropout, seed, bias)
    else:
        s = HeadScores.apply(g, q, k, heads, scale)
        p = EdgeSoftmax.apply(g, s if bias is None else s + bias, heads)
        if dropout > 0.0:
            p = p * dropout_mask(g, heads, dropout, seed, p.dtype)
        out = SpmmValues.apply(g, p, v, heads)
    return out.to(home)


def _run_gatv2_aggregate(g: EdgeGraph, x_dst, x_src, att, heads: int, slope: float, want_lse: bool, p: float = 0.0, seed: int = 0):
    """x_dst [nrows, h] and x_src [ncols, h] contiguous on g.device, one dtype; att [h] in the compute dtype -> (out [nrows, h] in the
    feature dtype, lse [nrows, heads] in the compute dtype or None)"""
    L, _ = _backend()
    dt = _gather_code(x_src.dtype)
    h = x_src.size(1)
    out = torch.empty((g.nrows, h), dtype=x_src.dtype, device=g.device)
    lse = torch.empty((g.nrows, heads), dtype=att.dtype, device=g.device) if want_lse else None
    if g.nrows == 0:
        return out, lse
    ws = _workspace(L.gatv2_aggregate_workspace(dt, g.nrows, g.nnz, h, heads), g.device)
    args = (dt, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, x_dst.data_ptr(), x_dst.stride(0), x_src.data_ptr(),
            x_src.stride(0), att.data_ptr(), h, heads, slope, out.data_ptr(), h, lse.data_ptr() if want_lse else 0, ws.data_ptr(), ws.numel(),
            _stream(g.device))
    if p > 0.0:
        L.gatv2_aggregate_dropout(*args, p, seed)
    else:
        L.gatv2_aggregate(*args)
    return out, lse


def _run_gatv2_backward(g: EdgeGraph, transposed: bool, own, oth, att, heads: int, slope: float, G, lse, delta, want_datt: bool, p: float = 0.0,
                        seed: int = 0, entry_ids=None):
    """one pygim_gatv2_backward call on ``g`` (the graph of A, or of A^T when ``transposed``) -> (d_own [g.nrows, h] in the feature dtype,
    datt [h] in the compute dtype or None).  p > 0: the forward ran with attention dropout (p, seed); entry_ids is the int32 index in A of
    every entry of ``g`` (None: ``g`` is the graph of A)"""
    L, _ = _backend()
    dt = _gather_code(own.dtype)
    h = own.size(1)
    d_own = torch.empty((g.nrows, h), dtype=own.dtype, device=g.device)
    datt = torch.empty(h, dtype=att.dtype, device=g.device) if want_datt else None
    if g.nrows == 0:
        return d_own, None if datt is None else datt.zero_()
    ws = _workspace(L.gatv2_backward_workspace(dt, g.nrows, g.nnz, h, heads), g.device)
    args = (dt, 1 if transposed else 0, g.nrows, g.rowptr.data_ptr(), g.col.data_ptr(), g.nnz, own.data_ptr(), own.stride(0), oth.data_ptr(),
            oth.stride(0), att.data_ptr(), h, heads, slope, G.data_ptr(), G.stride(0), lse.data_ptr(), delta.data_ptr(), d_own.data_ptr(), h,
            datt.data_ptr() if want_datt else 0, ws.data_ptr(), ws.numel(), _stream(g.device))
    if p > 0.0:
        L.gatv2_backward_dropout(*args, 0 if entry_ids is None else entry_ids.data_ptr(), p, seed)
    else:
        L.gatv2_backward(*args)
    return d_own, datt


class GatV2Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x_dst, x_src, att, heads, slope, p, seed):
        need = any(ctx.needs_input_grad[1:4])
        out, lse = _run_gatv2_aggregate(g, x_dst, x_src, att, heads, slope, need, p, seed)
        if need:
            ctx.g, ctx.heads, ctx.slope, ctx.p, ctx.seed = g, heads, slope, p, seed
            ctx.save_for_backward(x_dst, x_src, att, out, lse)   # node-sized, all of them
        return out

    @staticmethod
    def backward(ctx, G):
        g, heads, slope = ctx.g, ctx.heads, ctx.slope
        x_dst, x_src, att, out, lse = ctx.saved_tensors
        G = G.contiguous()
        h = x_src.size(1)
        # delta[r, k] = sum_{f in head k} G out = sum_e p dp, in the compute dtype; beside 16-bit features from the stored, once-rounded out
        delta = (G.to(att.dtype) * out.to(att.dtype)).view(g.nrows, heads, h // heads).sum(-1).contiguous()
        dx_dst = dx_src = datt = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            dx_dst, datt = _run_gatv2_backward(g, False, x_dst, x_src, att, heads, slope, G, lse, delta, ctx.needs_input_grad[3], ctx.p, ctx.seed)
            if not ctx.needs_input_grad[1]:
                dx_dst = None
        if ctx.needs_input_grad[2]:
            gt, _ = g.transposed()   # the permutation is needed only by attention dropout: the mask is a function of the entry's index in A
            dx_src, _ = _run_gatv2_backward(gt, True, x_src, x_dst, att, heads, slope, G, lse, delta, False, ctx.p, ctx.seed,
                                            g.entry_ids_t() if ctx.p > 0.0 else None)
        return None, dx_dst, dx_src, datt, None, None, None, None


def gatv2_aggregate(graph, x_dst: torch.Tensor, x_src: torch.Tensor, att: torch.Tensor, heads: int = 1, negative_slope: float = 0.2,
                    fused: bool = True, dropout: float = 0.0, seed=None) -> torch.Tensor:
    """the aggregation of a GATv2 layer (Brody et al.; PyG's GATv2Conv): with ``hd = h // heads``, ``k = f // hd`` and e over the entries of row r

    ``s[e, k] = sum_{f in head k} att[f] * leaky_relu(x_dst[r, f] + x_src[col[e], f], negative_slope)``
    ``out[r, f] = sum_e softmax_e(s[., k]) * x_src[col[e], f]``

    graph: an :class:`EdgeGraph` or anything ``EdgeGraph.of`` takes; x_dst [rows, h] and x_src [columns, h] with ``h % heads == 0``, both
    float32, both float64 or both the same 16-bit type; att [h] or [heads, hd] in the feature dtype, or float32 beside 16-bit features
    (att, the sums ``z``, the scores, the softmax state and every sum are then float32 and ``out`` is rounded once per element).  Empty rows
    give 0; duplicates are separate entries.
    ``fused=True``: one kernel, one pass over the entries (pygim_gatv2_aggregate), one gathered row per entry; nothing of size nnz is
    written, saved or allocated -- the forward saves ``x_dst``, ``x_src``, ``att``, ``out`` and the per-row ``lse``, the backward takes
    ``delta = sum over a head of G * out`` in the compute dtype (beside 16-bit features from the stored, once-rounded ``out``, as
    FlashAttention's backward does) and makes at most two pygim_gatv2_backward calls that recompute the probabilities: one on the CSR for
    ``dx_dst`` and ``datt``, one on the transposed CSR for ``dx_src`` (no atomics, the same bits on every run).
    ``fused=False``, and heads wider than 256 features in either case: PyG's composition -- ``z = x_dst[row] + x_src[col]``, the scores in
    torch, ``edge_softmax``, ``spmm_values`` -- which materialises ``[nnz, h]`` tensors and keeps them for the backward.
    Differentiable in x_dst, x_src and att, each gradient in its operand's dtype; no double backward.  Runs on the device; CPU tensors are
    staged there and the result comes back to x_src's device.

    ``dropout`` in [0, 1), ``seed``: attention dropout as in :func:`gat_aggregate` (PyG's ``GATv2Conv(dropout=)``), in the forward gather
    and in both backward gathers (pygim_gatv2_backward_dropout; the transposed one reads the entry's index in A from an int32 copy of
    ``perm`` cached on the graph).  ``fused=False`` multiplies the ``edge_softmax`` result by :func:`dropout_mask`: the same entries."""
    dropout = _dropout_rate("gatv2_aggregate", dropout)
    g = EdgeGraph.of(graph)
    heads = int(heads)
    if x_src.dtype not in FLOAT_TYPES + HALF_TYPES or x_dst.dtype != x_src.dtype:
        raise TypeError(f"gatv2_aggregate: x_dst and x_src must both be float32, float64, bfloat16 or float16, got {x_dst.dtype} and {x_src.dtype}")
    if att.dtype != x_src.dtype and not (x_src.dtype in HALF_TYPES and att.dtype == torch.float32):
        raise TypeError(f"gatv2_aggregate: att must be {x_src.dtype}" + (" or float32" if x_src.dtype in HALF_TYPES else "") + f", got {att.dtype}")
    if x_dst.dim() != 2 or x_dst.size(0) != g.nrows:
        raise ValueError(f"gatv2_aggregate: x_dst must be [{g.nrows}, h], got {tuple(x_dst.shape)}")
    h = x_dst.size(1)
    if x_src.dim() != 2 or tuple(x_src.shape) != (g.ncols, h):
        raise ValueError(f"gatv2_aggregate: x_src must be [{g.ncols}, {h}], got {tuple(x_src.shape)}")
    if heads < 1 or h < 1 or h % heads != 0:
        raise ValueError(f"gatv2_aggregate: heads = {heads} must divide h = {h}")
    hd = h // heads
    if tuple(att.shape) not in ((h,), (heads, hd)):
        raise ValueError(f"gatv2_aggregate: att must be [{h}] or [{heads}, {hd}], got {tuple(att.shape)}")
    slope = float(negative_slope)
    home = x_src.device
    ct = _compute_dtype(x_src.dtype)
    xd, xs = x_dst.to(g.device).contiguous(), x_src.to(g.device).contiguous()
    a = att.to(g.device, ct).reshape(h).contiguous()
    seed = _dropout_seed(seed) if dropout > 0.0 else 0
    if fused and hd <= SA_MAX_HEAD:
        out = GatV2Aggregate.apply(g, xd, xs, a, heads, slope, dropout, seed)
    else:
        row, col = g.row.long(), g.col.long()
        z = xd.to(ct).index_select(0, row) + xs.to(ct).index_select(0, col)   # [nnz, h]
        s = (torch.nn.functional.leaky_relu(z, slope) * a).view(g.nnz, heads, hd).sum(-1)
        pr = EdgeSoftmax.apply(g, s.contiguous(), heads)
        if dropout > 0.0:
            pr = pr * dropout_mask(g, heads, dropout, seed, pr.dtype)
        out = SpmmValues.apply(g, pr, xs, heads)
    return out.to(home)
