"""GCN / SAGE / GIN inference stacks whose aggregation runs on the HIP backend.

Same structure and call pattern as the reference's models/models.py:12-131 and the three
``message_and_aggregate`` conv layers (pyg_gcn_conv.py:116-137, pyg_gin_conv.py:74-101,
pyg_sage_conv.py:122-155), written on plain torch.nn (torch_geometric is not installable here):

    Linear -> BN -> ReLU -> [conv -> BN -> ReLU] x L -> Linear          (dropout is identity in eval)
    GCNConv : lin(x) (no bias) -> aggregate -> + bias        (no degree normalisation in the reference)
    SAGEConv: lin_l(aggregate(x)) + lin_r(x)                  (sum aggregation through adj_t.mul; aggr="mean" / "max": spmm_reduce)
    GINConv : nn((1 + eps) * x + aggregate(x)),  nn = Linear -> BN -> ReLU -> Linear  (PyG MLP([h, h, h]))
with aggregate = quantise -> adj_t.mul -> dequantise (pygim_amd/quantize.py).  ``adj_t`` is a
SparseTensor (cpu path), a backend_pim SparseTensorCOO, or a pygim_amd.dist.RowShardAdj (multi-GPU:
x and the result are then this rank's row block).

GATConv / GAT are the attention layer on top of pygim_amd.attention: its edge weights are computed on every call, so its aggregation
is ``spmm_values`` (values as an operand) instead of ``adj_t.mul`` (values frozen in the group); float32 / float64, trainable, and
bfloat16 / float16 features after ``model.to(torch.bfloat16)`` or under ``torch.autocast`` (so is ``SAGEConv(aggr="mean")``).
``GATConv(..., fused=True)`` / ``GAT(..., fused=True)`` aggregate with ``gat_aggregate`` instead: scores, softmax and product in one
kernel, no ``[nnz, heads]`` tensor written or kept for the backward.  The default (``fused=False``) is the layer as before.
``GATConv(..., edge_dim=d)`` takes PyG's edge features: ``forward(x, adj_t, edge_attr)`` with ``edge_attr`` [nnz, d] in the stored order of
the adjacency; they enter the score as one scalar per entry and head, inside the fused kernel (``gat_aggregate(a_edge=)``) or on the composed scores.

TransformerConv / GraphTransformer are the dot-product attention layer (PyG's TransformerConv without edge features or ``beta``) on
``pygim_amd.attention.sparse_attention``: one kernel per layer when ``fused`` is set, the three-pass composition otherwise; the same
dtypes as GATConv.

GATv2Conv / GATv2 are PyG's GATv2Conv (Brody et al.) without self loops or edge features on ``pygim_amd.attention.gatv2_aggregate``: fused by
default -- one forward kernel and two backward kernels per layer, nothing of size nnz -- because the composition holds ``[nnz, heads * out]``
tensors; the same dtypes as GATConv.

PNAConv / PNA are PyG's PNAConv with one tower, one linear pre-layer and no edge features on ``pygim_amd.reduce.spmm_multi_reduce``:
mean, min, max and std (or any of sum / mean / min / max / var / std) of the neighbours' messages come from one gather per layer, no
``[E, F]`` message tensor is formed; identity / amplification / attenuation scalers; float32 / float64, bfloat16 like ``SAGEConv(aggr="mean")``.

GENConv / GEN are PyG's GENConv (DeeperGCN, Li et al.) on ``pygim_amd.reduce.spmm_softmax``: the softmax aggregation
of the neighbours' messages per feature, with a fixed or learnable temperature, is one gather per layer forward and one backward, no
``[E, F]`` tensor; ``aggr="mean"`` / ``"max"`` / ``"sum"`` go through the functions that exist; the same dtypes as PNAConv.
``GENEConv(in, out, edge_dim, ...)`` is GENConv with PyG's edge features, ``forward(x, adj_t, edge_attr)``: the message ``relu(x_j + e_ij) + eps`` is formed
inside the gather (``pygim_amd.reduce.spmm_edge``), the edge features read as a stream beside it.

GINEConv / GINE are PyG's GINEConv (Hu et al.): ``nn((1 + eps) * x_i + sum_j relu(x_j + e_ij))`` on ``spmm_edge`` with the sum fold.
"""
import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d, Linear, ReLU, Sequential

from .quantize import message_and_aggregate


TRANSFORMER_FUSED_DEFAULT = True   # the fused forward beat the composition in both rounds of profiles/exp_sparse_attention.txt
PNA_FUSED_DEFAULT = True           # the fused call beat the composition 3.4 x (float32) / 4.0 x (bfloat16) forward in both rounds of profiles/exp_multi_reduce.txt


class GCNConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, bias=True, **_):
        super().__init__()
        self.lin = Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None

    def forward(self, x, adj_t):
        out = message_and_aggregate(adj_t, self.lin(x))
        return out if self.bias is None else out + self.bias


class SAGEConv(torch.nn.Module):
    """``aggr="sum"``: the reference's layer (quantise -> adj_t.mul -> dequantise).  ``"mean"`` / ``"max"`` / ``"min"``: PyG's other
    aggregators through pygim_amd.reduce on the adjacency's plain CSR: float32 / float64, trainable, no quantisation, one GPU."""

    def __init__(self, in_channels, out_channels, bias=True, aggr="sum", **_):
        super().__init__()
        if aggr not in ("sum", "add", "mean", "max", "min"):
            raise ValueError(f"SAGEConv: aggr must be 'sum', 'mean', 'max' or 'min', got {aggr!r}")
        self.aggr = "sum" if aggr == "add" else aggr
        self.lin_l = Linear(in_channels, out_channels, bias=bias)
        self.lin_r = Linear(in_channels, out_channels, bias=False)

    def forward(self, x, adj_t):
        if self.aggr == "sum":
            return self.lin_l(message_and_aggregate(adj_t, x)) + self.lin_r(x)
        if getattr(adj_t, "row_sharded", False):
            raise NotImplementedError(f"SAGEConv: aggr={self.aggr!r} is not available on a RowShardAdj (one GPU only); use aggr='sum'")
        from .reduce import matmul_reduce

        return self.lin_l(matmul_reduce(adj_t, x, self.aggr)) + self.lin_r(x)


class GINConv(torch.nn.Module):
    def __init__(self, nn, eps=0.0):
        super().__init__()
        self.nn = nn
        self.register_buffer("eps", torch.tensor([float(eps)]))

    def forward(self, x, adj_t):
        return self.nn(message_and_aggregate(adj_t, x) + (1 + self.eps) * x)


class GINEConv(torch.nn.Module):
    """PyG's GINEConv: ``out_i = nn((1 + eps) * x_i + sum_j relu(x_j + e_ij))`` over the stored entries (i, j) of the adjacency as given.
    ``forward(x, adj_t, edge_attr)`` takes ``edge_attr`` [nnz, edge_dim] (or [nnz, in_channels] without ``edge_dim``) in the stored order of
    the adjacency (``EdgeGraph.of(adj_t).row`` / ``.col``: row-major CSR order); with ``edge_dim`` a ``Linear(edge_dim, in_channels)`` maps it
    to the node width first (``in_channels``: that of ``nn``'s first Linear, as in PyG).  The sum runs in ONE ``spmm_edge`` gather
    (``fused=True``, the default) that reads the edge features as a stream -- no ``[nnz, F]`` message tensor -- or through the composition
    ``relu(x[col] + e)`` (``fused=False``).  ``train_eps``: eps is a parameter.  float32 / float64, trainable; bfloat16 after
    ``.to(torch.bfloat16)`` or under ``torch.autocast``; one GPU."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None, fused=True, **_):
        super().__init__()
        self.nn, self.fused = nn, bool(fused)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.tensor(float(eps)))
        else:
            self.register_buffer("eps", torch.tensor(float(eps)))
        self.lin = None
        if edge_dim is not None:
            first = nn[0] if isinstance(nn, Sequential) else nn
            width = getattr(first, "in_features", getattr(first, "in_channels", None))
            if width is None:
                raise ValueError("GINEConv: could not infer the input width from nn (its first module needs in_features or in_channels)")
            if int(edge_dim) < 1:
                raise ValueError(f"GINEConv: edge_dim must be at least 1, got {edge_dim}")
            self.lin = Linear(int(edge_dim), int(width))

    def forward(self, x, adj_t, edge_attr):
        if getattr(adj_t, "row_sharded", False):
            raise NotImplementedError("GINEConv is not available on a RowShardAdj (one GPU only)")
        from .reduce import matmul_edge

        if self.lin is not None and (edge_attr.dim() != 2 or edge_attr.size(1) != self.lin.in_features):
            raise ValueError(f"GINEConv: edge_attr must be [nnz, {self.lin.in_features}], got {tuple(edge_attr.shape)}")
        e = edge_attr if self.lin is None else self.lin(edge_attr)
        if e.dim() != 2 or e.size(1) != x.size(1):
            raise ValueError(f"GINEConv: node features of width {x.size(1)} need edge features of that width (set edge_dim), got {tuple(e.shape)}")
        if e.dtype != x.dtype:   # under autocast lin gives 16 bits beside float32 x: the wider of the two
            wide = torch.promote_types(e.dtype, x.dtype)
            x, e = x.to(wide), e.to(wide)
        agg = matmul_edge(adj_t, x, e, "sum", "relu", 0.0, fused=self.fused)
        return self.nn(agg + (1 + self.eps).to(agg.dtype) * x)


class GATConv(torch.nn.Module):
    """PyG's GATConv arithmetic on the adjacency as given (no self loops are inserted, like the other layers here):
    x' = lin(x) as [N, H, F];  score of stored entry (i, j) = leaky_relu(a_dst[i] + a_src[j]) with a = (x' * att).sum(-1);
    p = softmax of the scores over the entries of row i;  out[i] = sum_j p[(i, j)] * x'[j] per head; heads concatenated or averaged.
    ``fused=True``: everything after the two reductions ``a`` is one ``gat_aggregate`` call.
    ``dropout``: PyG's attention dropout on ``p`` (a fresh mask per forward while training, none in ``eval()``), inside the fused kernel
    or on the ``edge_softmax`` result.
    ``edge_dim``: PyG's edge features.  ``forward(x, adj_t, edge_attr)`` takes ``edge_attr`` [nnz, edge_dim] in the stored order of the
    adjacency (``EdgeGraph.of(adj_t).row`` / ``.col``: row-major CSR order) and adds ``a_edge = (lin_edge(edge_attr).view(-1, H, F) *
    att_edge).sum(-1)`` to the score before the leaky ReLU.  ``a_edge`` is formed as ``edge_attr @ M`` with ``M[d, k] = sum_c
    lin_edge.weight[k F + c, d] * att_edge[0, k, c]`` -- the same function of the same parameters without the [nnz, H F] tensor -- and goes
    into ``gat_aggregate(a_edge=)`` (fused) or onto the composed scores.  Without ``edge_dim``, or with ``edge_attr=None``, the layer is
    the one above."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, fused=False, dropout=0.0, edge_dim=None,
                 **_):
        super().__init__()
        self.fused, self.dropout = bool(fused), _att_dropout("GATConv", dropout)
        self.heads, self.out_channels, self.concat, self.negative_slope = int(heads), int(out_channels), bool(concat), float(negative_slope)
        self.lin = Linear(in_channels, self.heads * self.out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.empty(1, self.heads, self.out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, self.heads, self.out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(self.heads * self.out_channels if self.concat else self.out_channels)) if bias else None
        torch.nn.init.xavier_uniform_(self.lin.weight)
        torch.nn.init.xavier_uniform_(self.att_src)
        torch.nn.init.xavier_uniform_(self.att_dst)
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        if self.edge_dim is not None:   # created last, so that the other parameters draw what they drew without edge_dim
            if self.edge_dim < 1:
                raise ValueError(f"GATConv: edge_dim must be at least 1, got {edge_dim}")
            self.lin_edge = Linear(self.edge_dim, self.heads * self.out_channels, bias=False)
            self.att_edge = torch.nn.Parameter(torch.empty(1, self.heads, self.out_channels))
            torch.nn.init.xavier_uniform_(self.lin_edge.weight)
            torch.nn.init.xavier_uniform_(self.att_edge)

    def edge_term(self, edge_attr):
        """``a_edge`` [nnz, heads] of ``edge_attr`` [nnz, edge_dim]: PyG's ``(lin_edge(edge_attr).view(-1, H, F) * att_edge).sum(-1)`` as one
        [nnz, edge_dim] x [edge_dim, H] product"""
        if self.edge_dim is None:
            raise ValueError("GATConv: edge_attr was given, but the layer was built without edge_dim")
        if edge_attr.dim() == 1 and self.edge_dim == 1:
            edge_attr = edge_attr.unsqueeze(1)
        if edge_attr.dim() != 2 or edge_attr.size(1) != self.edge_dim:
            raise ValueError(f"GATConv: edge_attr must be [nnz, {self.edge_dim}], got {tuple(edge_attr.shape)}")
        M = (self.lin_edge.weight.view(self.heads, self.out_channels, self.edge_dim) * self.att_edge.view(self.heads, self.out_channels, 1)).sum(1)
        return F.linear(edge_attr, M)   # edge_attr @ M^T, M [H, edge_dim]; under autocast a 16-bit matmul

    def forward(self, x, adj_t, edge_attr=None):
        from .attention import EdgeGraph, _dropout_seed, dropout_mask, edge_softmax, gat_aggregate, spmm_values

        g = EdgeGraph.of(adj_t)
        H, F_ = self.heads, self.out_channels
        drop = self.dropout if self.training else 0.0
        xp = self.lin(x).view(-1, H, F_)
        a_src = (xp * self.att_src).sum(-1)
        a_dst = (xp * self.att_dst).sum(-1)
        a_edge = None
        if edge_attr is not None:
            if edge_attr.size(0) != g.nnz:
                raise ValueError(f"GATConv: edge_attr must have one row per stored entry ({g.nnz}), got {tuple(edge_attr.shape)}")
            a_edge = self.edge_term(edge_attr.to(x.device))
        if self.fused:
            if a_edge is None:
                out = gat_aggregate(g, a_dst, a_src, xp.reshape(-1, H * F_), self.negative_slope, dropout=drop)
            else:   # beside 16-bit features (model.to(bfloat16), autocast) the term goes to float32, what the kernel reads
                a_edge = a_edge.float() if xp.dtype in (torch.float16, torch.bfloat16) else a_edge.to(xp.dtype)
                out = gat_aggregate(g, a_dst, a_src, xp.reshape(-1, H * F_), self.negative_slope, dropout=drop, a_edge=a_edge)
        else:
            row, col = g.row.long().to(x.device), g.col.long().to(x.device)
            z = a_dst.index_select(0, row) + a_src.index_select(0, col)
            score = F.leaky_relu(z if a_edge is None else z + a_edge.to(z.dtype), self.negative_slope)
            if score.dtype in (torch.float16, torch.bfloat16):   # edge_softmax is float32 / float64: 16-bit scores go up, and
                score = score.float()                             # spmm_values takes the float32 probabilities beside 16-bit features
            p = edge_softmax(g, score)
            if drop > 0.0:
                p = p * dropout_mask(g, H, drop, _dropout_seed(None), p.dtype).to(p.device)
            out = spmm_values(g, p, xp.reshape(-1, H * F_), heads=H)
        if not self.concat:
            out = out.view(-1, H, F_).mean(1)
        return out if self.bias is None else out + self.bias


class TransformerConv(torch.nn.Module):
    """PyG's TransformerConv arithmetic without edge features or ``beta``, on the adjacency as given: q = lin_query(x), k = lin_key(x),
    v = lin_value(x) as [N, H, F];  score of stored entry (i, j) = q[i] . k[j] / sqrt(F) per head;  p = softmax of the scores over the
    entries of row i;  out[i] = sum_j p[(i, j)] * v[j] per head; heads concatenated or averaged;  + lin_skip(x) with ``root_weight``.
    ``fused=True``: scores, softmax and product are one ``sparse_attention`` kernel (heads wider than 256 features run unfused).
    ``dropout``: PyG's attention dropout on ``p``, active while training.
    A per-entry, per-head attention bias or mask goes through ``pygim_amd.sparse_attention(bias=)`` directly; PyG's ``edge_dim`` here is the
    feature-wide form (``key_j + e``, ``value_j + e``) and is not covered."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, root_weight=True, bias=True, fused=TRANSFORMER_FUSED_DEFAULT, dropout=0.0,
                 **_):
        super().__init__()
        self.fused, self.dropout = bool(fused), _att_dropout("TransformerConv", dropout)
        self.heads, self.out_channels, self.concat, self.root_weight = int(heads), int(out_channels), bool(concat), bool(root_weight)
        width = self.heads * self.out_channels
        self.lin_key = Linear(in_channels, width, bias=bias)
        self.lin_query = Linear(in_channels, width, bias=bias)
        self.lin_value = Linear(in_channels, width, bias=bias)
        self.lin_skip = Linear(in_channels, width if self.concat else self.out_channels, bias=bias) if self.root_weight else None

    def forward(self, x, adj_t):
        from .attention import EdgeGraph, sparse_attention

        g = EdgeGraph.of(adj_t)
        out = sparse_attention(g, self.lin_query(x), self.lin_key(x), self.lin_value(x), heads=self.heads, fused=self.fused,
                               dropout=self.dropout if self.training else 0.0)
        if not self.concat:
            out = out.view(-1, self.heads, self.out_channels).mean(1)
        return out if self.lin_skip is None else out + self.lin_skip(x)


class GATv2Conv(torch.nn.Module):
    """PyG's GATv2Conv arithmetic on the adjacency as given (no self loops are inserted, no edge features): x_l = lin_l(x) (the source /
    value side) and x_r = lin_r(x) (the target side) as [N, H, F], ``lin_r is lin_l`` with ``share_weights``;  score of stored entry
    (i, j) = (att * leaky_relu(x_r[i] + x_l[j])).sum(-1) per head;  p = softmax of the scores over the entries of row i;
    out[i] = sum_j p[(i, j)] * x_l[j] per head; heads concatenated or averaged; + bias.
    ``fused=True`` (the default): everything after the two linear maps is ``gatv2_aggregate``'s fused forward and backward (heads wider
    than 256 features run unfused); ``fused=False`` materialises ``[nnz, H * F]``.
    ``dropout``: PyG's attention dropout on ``p``, active while training; fused, it lives in the forward and both backward gathers."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, share_weights=False, fused=True,
                 dropout=0.0, **_):
        super().__init__()
        self.fused, self.share_weights, self.dropout = bool(fused), bool(share_weights), _att_dropout("GATv2Conv", dropout)
        self.heads, self.out_channels, self.concat, self.negative_slope = int(heads), int(out_channels), bool(concat), float(negative_slope)
        self.lin_l = Linear(in_channels, self.heads * self.out_channels, bias=bias)
        self.lin_r = self.lin_l if self.share_weights else Linear(in_channels, self.heads * self.out_channels, bias=bias)
        self.att = torch.nn.Parameter(torch.empty(self.heads, self.out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(self.heads * self.out_channels if self.concat else self.out_channels)) if bias else None
        torch.nn.init.xavier_uniform_(self.lin_l.weight)
        if not self.share_weights:
            torch.nn.init.xavier_uniform_(self.lin_r.weight)
        torch.nn.init.xavier_uniform_(self.att)

    def forward(self, x, adj_t):
        from .attention import EdgeGraph, gatv2_aggregate

        g = EdgeGraph.of(adj_t)
        x_l = self.lin_l(x)
        x_r = x_l if self.share_weights else self.lin_r(x)
        att = self.att if self.att.dtype == x_l.dtype else self.att.float()   # autocast: 16-bit features beside the float32 parameter
        out = gatv2_aggregate(g, x_r, x_l, att, heads=self.heads, negative_slope=self.negative_slope, fused=self.fused,
                              dropout=self.dropout if self.training else 0.0)
        if not self.concat:
            out = out.view(-1, self.heads, self.out_channels).mean(1)
        return out if self.bias is None else out + self.bias


class PNAConv(torch.nn.Module):
    """PyG's PNAConv (Corso et al.) with ``towers=1``, ``pre_layers=1`` and no edge features, on the adjacency as given:
    message of stored entry (i, j) = pre_nn(cat[x_i, x_j]);  every aggregator over the entries of row i;  every scaler on the
    concatenated aggregates;  out = lin(post_nn(cat[x, scaled aggregates])).

    With one linear pre-layer the message is ``W . [x_i || x_j] + b = a_i + m_j`` with ``a = W_dst . x + b`` and ``m = W_src . x``
    (W_dst, W_src: the two halves of pre_nn's weight), so no ``[E, F]`` tensor is formed -- with d the stored entries of row i:
        mean_i = a_i + mean_j m_j      min_i = a_i + min_j m_j      max_i = a_i + max_j m_j
        std_i  = std_j m_j             var_i = var_j m_j            sum_i = d_i a_i + sum_j m_j
    and all the statistics of m are ONE ``spmm_multi_reduce`` (``fused=True``) or one ``spmm_reduce`` per statistic (``fused=False``).
    Rows with d = 0 keep the kernel's empty-row values (0, and sqrt(eps) for std) without a_i, as PyG's scatter gives them.
    std = sqrt(relu(var) + 1e-5), var = mean of squares minus squared mean.
    Scalers (PyG's DegreeScalerAggregation, d clamped to 1): ``identity``; ``amplification``: ``log(d + 1) / avg_log``; ``attenuation``:
    ``avg_log / log(d + 1)``.  ``avg_log`` = the mean of log(d + 1) over the nodes, from ``deg`` (a degree histogram, as PyG takes it) or,
    without it, from the adjacency of the first forward (kept as a buffer).
    float32 / float64, trainable; bfloat16 after ``.to(torch.bfloat16)`` or under ``torch.autocast``; one GPU."""

    EPS = 1e-5

    def __init__(self, in_channels, out_channels, aggregators=("mean", "min", "max", "std"), scalers=("identity", "amplification", "attenuation"),
                 deg=None, post_layers=1, fused=None, towers=1, pre_layers=1, edge_dim=None, divide_input=False, **_):
        super().__init__()
        if towers != 1 or pre_layers != 1 or edge_dim is not None or divide_input:
            raise NotImplementedError("PNAConv: only towers=1, pre_layers=1 and no edge features are implemented")
        self.aggregators, self.scalers = tuple(aggregators), tuple(scalers)
        if not self.aggregators or len(set(self.aggregators)) != len(self.aggregators) or any(
                a not in ("sum", "mean", "min", "max", "var", "std") for a in self.aggregators):
            raise ValueError(f"PNAConv: aggregators must be distinct names among sum, mean, min, max, var, std, got {aggregators!r}")
        if not self.scalers or any(s not in ("identity", "amplification", "attenuation") for s in self.scalers):
            raise ValueError(f"PNAConv: scalers must be among identity, amplification, attenuation, got {scalers!r}")
        self.fused = PNA_FUSED_DEFAULT if fused is None else bool(fused)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        F_ = self.in_channels
        self.pre_nn = Linear(2 * F_, F_)
        layers = [Linear((len(self.aggregators) * len(self.scalers) + 1) * F_, self.out_channels)]
        for _i in range(int(post_layers) - 1):
            layers += [ReLU(), Linear(self.out_channels, self.out_channels)]
        self.post_nn = Sequential(*layers)
        self.lin = Linear(self.out_channels, self.out_channels)
        avg_log = float("nan")
        if deg is not None:
            deg = torch.as_tensor(deg).to(torch.float64)
            avg_log = float((torch.log(torch.arange(deg.numel(), dtype=torch.float64) + 1) * deg).sum() / deg.sum())
        self.register_buffer("avg_log", torch.tensor(avg_log, dtype=torch.float64))

    def forward(self, x, adj_t):
        if getattr(adj_t, "row_sharded", False):
            raise NotImplementedError("PNAConv is not available on a RowShardAdj (one GPU only)")
        from .attention import EdgeGraph
        from .reduce import spmm_multi_reduce

        g = EdgeGraph.of(adj_t)
        F_ = self.in_channels
        W, b = self.pre_nn.weight, self.pre_nn.bias
        a = F.linear(x, W[:, :F_], b)   # the target's half of the message, with the bias
        m = F.linear(x, W[:, F_:])      # the source's half: what is aggregated
        agg = spmm_multi_reduce(g, m, self.aggregators, self.EPS, fused=self.fused)
        d = (g.rowptr[1:] - g.rowptr[:-1]).to(x.device)
        has = (d > 0).to(agg.dtype).unsqueeze(1)
        own = {"mean": has, "min": has, "max": has, "sum": d.to(agg.dtype).unsqueeze(1)}
        a = a.to(agg.dtype)
        agg = torch.cat([agg[:, j * F_:(j + 1) * F_] + own[s] * a if s in own else agg[:, j * F_:(j + 1) * F_]
                         for j, s in enumerate(self.aggregators)], 1)
        logd = torch.log(d.clamp(min=1).to(torch.float64) + 1)
        if torch.isnan(self.avg_log):   # no histogram was given: the first adjacency's own (rows without entries count as log(0 + 1) = 0, as in a histogram)
            self.avg_log.copy_(torch.log(d.to(torch.float64) + 1).mean() if d.numel() else torch.tensor(1.0))
        avg = self.avg_log.to(torch.float64)
        scale = {"identity": None, "amplification": (logd / avg), "attenuation": (avg / logd)}
        outs = [agg if scale[s] is None else agg * scale[s].to(agg.dtype).unsqueeze(1) for s in self.scalers]
        return self.lin(self.post_nn(torch.cat([x, torch.cat(outs, 1)], 1)))


class GENConv(torch.nn.Module):
    """PyG's GENConv (Li et al., DeeperGCN) on the adjacency as given:
    message of stored entry (i, j) = relu(x_src[j]) + eps;  agg_i = the aggregation of the messages over the entries of row i;
    out = mlp(agg + x_dst),  x_src = lin_src(x) and x_dst = lin_dst(x) when ``in_channels != out_channels`` (else x itself),
    mlp = Linear -> norm -> ReLU -> Linear (``num_layers`` linear maps, hidden width ``expansion * out_channels``).

    Without edge features the message depends on the source node alone, so it is formed per node and no ``[E, F]`` tensor exists.
    ``aggr="softmax"``: ``agg_i[f] = sum_j softmax_j(t * msg_j[f]) * msg_j[f]`` with the temperature ``t`` (a parameter with
    ``learn_t``), ONE ``spmm_softmax`` gather (``fused=True``, the default: the composition holds ``[nnz, out_channels]`` tensors) or its
    composition from ``edge_softmax`` and ``spmm_values`` (``fused=False``).  ``"mean"``, ``"max"``, ``"sum"``: ``spmm_reduce`` /
    ``spmm_values`` with unit weights.  Rows without entries aggregate to 0.
    This class takes no edge features (``edge_dim`` and ``edge_attr`` raise NotImplementedError, as they always did): :class:`GENEConv` is
    the layer with them.
    float32 / float64, trainable; bfloat16 after ``.to(torch.bfloat16)`` or under ``torch.autocast`` (softmax, mean, sum); one GPU."""

    EDGE_FEATURES = False   # GENEConv: True

    def __init__(self, in_channels, out_channels, aggr="softmax", t=1.0, learn_t=False, eps=1e-7, num_layers=2, expansion=2, norm="batch", bias=True,
                 fused=True, edge_dim=None, learn_p=False, msg_norm=False, **_):
        super().__init__()
        if aggr in ("powermean", "power"):
            raise NotImplementedError("GENConv: aggr='powermean' is not implemented (softmax, mean, max and sum are)")
        if edge_dim is not None and not self.EDGE_FEATURES:
            raise NotImplementedError("GENConv: edge features (edge_dim) are not implemented in this class; GENEConv(in, out, edge_dim) is the layer with them")
        if edge_dim is not None and int(edge_dim) < 1:
            raise ValueError(f"GENEConv: edge_dim must be at least 1, got {edge_dim}")
        if learn_p or msg_norm:
            raise NotImplementedError("GENConv: learn_p and msg_norm are not implemented")
        if aggr not in ("softmax", "mean", "max", "sum", "add"):
            raise ValueError(f"GENConv: aggr must be 'softmax', 'mean', 'max' or 'sum', got {aggr!r}")
        if norm not in ("batch", "layer", None):
            raise ValueError(f"GENConv: norm must be 'batch', 'layer' or None, got {norm!r}")
        self.aggr = "sum" if aggr == "add" else aggr
        self.in_channels, self.out_channels, self.eps, self.fused = int(in_channels), int(out_channels), float(eps), bool(fused)
        self.lin_src = self.lin_dst = None
        if self.in_channels != self.out_channels:
            self.lin_src = Linear(self.in_channels, self.out_channels, bias=bias)
            self.lin_dst = Linear(self.in_channels, self.out_channels, bias=bias)
        if learn_t and self.aggr == "softmax":
            self.t = torch.nn.Parameter(torch.tensor(float(t)))
        else:
            self.t = float(t)
        widths = [self.out_channels] + [self.out_channels * int(expansion)] * (int(num_layers) - 1) + [self.out_channels]
        layers = []
        for i in range(len(widths) - 1):
            layers.append(Linear(widths[i], widths[i + 1], bias=bias))
            if i < len(widths) - 2:
                if norm is not None:
                    layers.append(BatchNorm1d(widths[i + 1]) if norm == "batch" else torch.nn.LayerNorm(widths[i + 1]))
                layers.append(ReLU())
        self.mlp = Sequential(*layers)
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        self.lin_edge = None
        if self.edge_dim is not None and self.edge_dim != self.out_channels:   # created last, so that the other parameters draw what they drew without edge_dim
            self.lin_edge = Linear(self.edge_dim, self.out_channels, bias=bias)

    def forward(self, x, adj_t, edge_attr=None):
        if edge_attr is not None and self.edge_dim is None:
            raise NotImplementedError("GENConv: edge features are not implemented in this class; GENEConv(in, out, edge_dim) is the layer with them")
        if getattr(adj_t, "row_sharded", False):
            raise NotImplementedError("GENConv is not available on a RowShardAdj (one GPU only)")
        from .attention import EdgeGraph, _compute_dtype, spmm_values
        from .reduce import spmm_edge, spmm_reduce, spmm_softmax

        g = EdgeGraph.of(adj_t)
        src = x if self.lin_src is None else self.lin_src(x)
        if edge_attr is not None:
            if edge_attr.dim() != 2 or edge_attr.size(1) != self.edge_dim:
                raise ValueError(f"GENEConv: edge_attr must be [nnz, {self.edge_dim}], got {tuple(edge_attr.shape)}")
            e = edge_attr if self.lin_edge is None else self.lin_edge(edge_attr)
            if e.dtype != src.dtype:   # under autocast the two Linears give 16 bits beside float32 operands: the wider of the two
                wide = torch.promote_types(e.dtype, src.dtype)
                src, e = src.to(wide), e.to(wide)
            agg = spmm_edge(g, src, e, self.aggr, "relu", self.eps, self.t, fused=self.fused)
            dst = x if self.lin_dst is None else self.lin_dst(x)
            return self.mlp(agg + dst.to(agg.dtype))
        msg = F.relu(src) + self.eps
        if self.aggr == "softmax":
            agg = spmm_softmax(g, msg, self.t, fused=self.fused)
        elif self.aggr == "sum":
            agg = spmm_values(g, torch.ones(g.nnz, dtype=_compute_dtype(msg.dtype), device=msg.device), msg)
        else:
            agg = spmm_reduce(g, msg, self.aggr)
        dst = x if self.lin_dst is None else self.lin_dst(x)
        return self.mlp(agg + dst.to(agg.dtype))


class GENEConv(GENConv):
    """GENConv with PyG's edge features (PyG's ``GENConv(edge_dim=)``; a class of its own, as GINEConv is beside GINConv).
    ``forward(x, adj_t, edge_attr)`` takes ``edge_attr`` [nnz, edge_dim] in the stored order of the adjacency (``EdgeGraph.of(adj_t).row`` /
    ``.col``: row-major CSR order); the message is ``relu(x_src[j] + e_ij) + eps`` with ``e = lin_edge(edge_attr)`` (a Linear when
    ``edge_dim != out_channels``, as in PyG, else ``edge_attr`` itself), formed inside ONE ``spmm_edge`` gather for every ``aggr`` -- softmax
    with ``learn_t``, mean, max, sum -- that reads the edge features as a stream (``fused=False``: through the ``[nnz, out_channels]``
    message tensor).  ``edge_attr=None`` gives GENConv's own forward.  The other arguments, the dtypes and the parameters drawn before
    ``lin_edge`` are GENConv's."""

    EDGE_FEATURES = True

    def __init__(self, in_channels, out_channels, edge_dim, **kw):
        if edge_dim is None:
            raise ValueError("GENEConv: edge_dim is needed (GENConv is the layer without edge features)")
        super().__init__(in_channels, out_channels, edge_dim=edge_dim, **kw)


def _att_dropout(name, p):
    """a layer's ``dropout=`` (attention dropout, as in PyG): a rate in [0, 1), active only while the layer is training"""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}: dropout must lie in [0, 1), got {p}")
    return p


def folded_epilogue(conv_bias, bn):
    """bias + eval-mode BatchNorm as ONE affine map per feature: bn(y + bias) = a * y + b with
    a = weight / sqrt(running_var + eps), b = (bias - running_mean) * a + bn.bias"""
    a = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    bias = conv_bias if conv_bias is not None else torch.zeros_like(bn.running_mean)
    return a, (bias - bn.running_mean) * a + bn.bias


class _Stack(torch.nn.Module):
    fuse_post = False  # True: a GCN layer's "+ bias -> BatchNorm (eval) -> ReLU" runs in the aggregation's last store

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, make_conv):
        super().__init__()
        self.ln1 = Linear(in_channels, hidden_channels)
        self.bn0 = BatchNorm1d(hidden_channels)
        self.convs = torch.nn.ModuleList([make_conv(hidden_channels) for _ in range(num_layers)])
        self.bns = torch.nn.ModuleList([BatchNorm1d(hidden_channels) for _ in range(num_layers)])
        self.ln2 = Linear(hidden_channels, out_channels)
        self.dropout = dropout

    def forward(self, x, adj_t, edge_attr=None):
        x = F.dropout(F.relu(self.bn0(self.ln1(x))), p=self.dropout, training=self.training)
        for conv, bn in zip(self.convs, self.bns):
            if (self.fuse_post and not self.training and isinstance(conv, GCNConv) and x.is_cuda
                    and hasattr(adj_t, "mul_quantized") and not getattr(adj_t, "row_sharded", False)
                    and adj_t.dtype in (torch.int8, torch.int16, torch.int32, torch.float32)):
                # same mathematics as the three torch ops below, one rounding sequence instead of three passes over [N, h]
                a, b = folded_epilogue(conv.bias, bn)
                x, _ = adj_t.mul_quantized(conv.lin(x), post=(a, b, True))
                continue
            out = conv(x, adj_t) if edge_attr is None else conv(x, adj_t, edge_attr)
            x = F.dropout(F.relu(bn(out)), p=self.dropout, training=self.training)
        return self.ln2(x)


class GCN(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5):
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout, lambda h: GCNConv(h, h))


class SAGE(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, aggr="sum"):
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout, lambda h: SAGEConv(h, h, aggr=aggr))


class GIN(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5):
        mlp = lambda h: Sequential(Linear(h, h), BatchNorm1d(h), ReLU(), Linear(h, h))
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout, lambda h: GINConv(mlp(h)))


class GINE(_Stack):
    """a stack of GINEConv layers; ``forward(x, adj_t, edge_attr)`` hands the same ``edge_attr`` [nnz, edge_dim] to every layer"""

    def __init__(self, in_channels, hidden_channels, out_channels, edge_dim, num_layers=2, dropout=0.5, train_eps=False, fused=True):
        mlp = lambda h: Sequential(Linear(h, h), BatchNorm1d(h), ReLU(), Linear(h, h))
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout,
                         lambda h: GINEConv(mlp(h), train_eps=train_eps, edge_dim=edge_dim, fused=fused))


class GAT(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=1, fused=False, att_dropout=0.0):
        assert hidden_channels % heads == 0, "GAT: heads must divide hidden_channels (the heads are concatenated)"
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout,
                         lambda h: GATConv(h, h // heads, heads=heads, concat=True, fused=fused, dropout=att_dropout))


class GATv2(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=1, share_weights=False, fused=True,
                 att_dropout=0.0):
        assert hidden_channels % heads == 0, "GATv2: heads must divide hidden_channels (the heads are concatenated)"
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout,
                         lambda h: GATv2Conv(h, h // heads, heads=heads, concat=True, share_weights=share_weights, fused=fused,
                                             dropout=att_dropout))


class PNA(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, aggregators=("mean", "min", "max", "std"),
                 scalers=("identity", "amplification", "attenuation"), deg=None, post_layers=1, fused=None):
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout,
                         lambda h: PNAConv(h, h, aggregators=aggregators, scalers=scalers, deg=deg, post_layers=post_layers, fused=fused))


class GEN(_Stack):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, aggr="softmax", t=1.0, learn_t=False, norm="batch",
                 fused=True, edge_dim=None):
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout,
                         lambda h: (GENConv(h, h, aggr=aggr, t=t, learn_t=learn_t, norm=norm, fused=fused) if edge_dim is None else
                                    GENEConv(h, h, edge_dim, aggr=aggr, t=t, learn_t=learn_t, norm=norm, fused=fused)))


class GraphTransformer(_Stack):
    """a stack of TransformerConv layers.  A learned per-edge, per-head attention bias (Graphormer, SAN, GPS) is ``pygim_amd.sparse_attention(bias=)``;
    the layers here take no edge features."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, heads=1, fused=TRANSFORMER_FUSED_DEFAULT,
                 att_dropout=0.0):
        assert hidden_channels % heads == 0, "GraphTransformer: heads must divide hidden_channels (the heads are concatenated)"
        super().__init__(in_channels, hidden_channels, out_channels, num_layers, dropout,
                         lambda h: TransformerConv(h, h // heads, heads=heads, concat=True, fused=fused, dropout=att_dropout))
