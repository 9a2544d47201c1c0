"""Edge terms inside the fused attention kernels: the cases, the operands and the float64 reference shared by test_edge_term_cpu.py (the
reference alone, no device) and test_edge_term_gpu.py (pygim_gat_aggregate_edge / pygim_sparse_attention_bias against it).  Host helpers
take the torch device they compute on, so one reference serves both files.

    gat:  z[e, k] = a_dst[r, k] + a_src[col[e], k] + term[e, k],  s = z >= 0 ? z : slope * z
    sa:   s[e, k] = scale * Q[r, head k] . K[col[e], head k] + term[e, k]
then the softmax over the stored entries of a row and the product with the gathered row, as in the base calls.

Bounds, those of the base calls' own GPU tests:
    gat:  |out - ref| <= TOL * sum_e p |x|,  |lse - ref| <= TOL * (1 + |lse|),  TOL = 2e-5 (FLT32) / 2e-12 (DBL64).  The node terms are drawn
          from uniform(-3, 3) and the edge term from uniform(-2, 2), so |z| <= 8 and the one extra float32 addition stays under 1e-6
          relative per probability: the bound holds as it stands.
    sa:   |out - ref| <= (2 EPS + 2 Delta[r, k]) * sum_e p |v|,  |lse - ref| <= 2 EPS * (1 + |lse|) + Delta,  EPS = 1e-5 / 1e-12,
          Delta[r, k] = EPS * max_e (|scale| * sum_f |Q K| + |term[e, k]|): the bias counts as one more magnitude of the score.
    16-bit features: u * |ref| more on out, u = 2^-8 (BF16) / 2^-11 (FLT16)."""
import numpy as np
import torch

import attn_dropout_ref as ad

GAT_WIDTHS = (1, 9, 32, 100, 256, 300, 512)   # test_gat_fused_gpu.test_gat_aggregate_parity: every lane layout
GAT_HEADS = (1, 4, 8)                          # where they divide the width
SA_SHAPES = [(4, 4), (9, 3), (32, 1), (32, 4), (32, 8), (100, 4), (256, 1), (256, 8), (512, 2), (1024, 16)]   # test_sparse_attention_gpu.SHAPES
GRAPH_NAMES = ("edges", "small")               # run_edges.edges_graph, test_attention_gpu.small_graph (attn_dropout_ref.graph caches them)
SLOPE = 0.2
GAT_TOL = {torch.float32: 2e-5, torch.float64: 2e-12, torch.bfloat16: 2e-5, torch.float16: 2e-5}
SA_EPS = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 1e-5, torch.float16: 1e-5}
U = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF = (torch.bfloat16, torch.float16)

graph = ad.graph


def gat_cases():
    return [(h, heads) for h in GAT_WIDTHS for heads in GAT_HEADS if h % heads == 0]


def compute_type(dtype):
    return torch.float32 if dtype in HALF else dtype


def operands(kind, n, m, nnz, h, heads, dtype, seed=11):
    """host tensors -> dict(A, B, V, term, scalar): A the row operand (a_dst, Q), B the gathered one the score reads (a_src, K), V the
    gathered values, term [nnz, heads] from uniform(-2, 2) in the compute type, scalar the slope or the scale.  gat: node terms from
    uniform(-3, 3), so |z| <= 8.  16-bit values: |v| in [0.5, 2) with random signs, as in the existing 16-bit tests."""
    r = np.random.default_rng(seed)
    ct = compute_type(dtype)
    half = dtype in HALF
    V = torch.from_numpy(r.uniform(0.5, 2, size=(m, h)) * r.choice([-1.0, 1.0], size=(m, h)) if half else r.uniform(-1, 1, size=(m, h))).to(dtype)
    term = torch.from_numpy(r.uniform(-2, 2, size=(nnz, heads))).to(ct)
    if kind == "gat":
        return dict(A=torch.from_numpy(r.uniform(-3, 3, size=(n, heads))).to(ct), B=torch.from_numpy(r.uniform(-3, 3, size=(m, heads))).to(ct),
                    V=V, term=term, scalar=SLOPE)
    Q, K = (torch.from_numpy(r.uniform(-2, 2, size=(k, h))).to(dtype) for k in (n, m))
    return dict(A=Q, B=K, V=V, term=term, scalar=(h // heads) ** -0.5)


def as_float64(ops, device):
    return {k: (v.to(device).double() if torch.is_tensor(v) else v) for k, v in ops.items()}


def reference(kind, dtype, n, rowptr, col, ops, h, heads, device, term="own", w=None):
    """float64 on `device` from float64 operands (as_float64 of the operands as stored) -> dict(ref, mag = sum_e p w |v| per output, lse (0
    for empty rows), delta per (row, head) -- 0 for gat --, pr [nnz, heads], row).  term: "own" (ops["term"]), None (left out) or a float64
    tensor [nnz, heads]; w: float64 numpy dropout weights [nnz, heads] or None."""
    hd = h // heads
    row = ad.entry_rows(n, rowptr, device)
    cc = torch.from_numpy(col).long().to(device)
    t = ops["term"] if isinstance(term, str) else term
    zeros = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=device)
    if kind == "gat":
        z = ops["A"][row] + ops["B"][cc]
        if t is not None:
            z = z + t
        s = torch.where(z >= 0, z, ops["scalar"] * z)
        sabs = torch.zeros_like(s)
    else:
        prod = (ops["A"][row] * ops["B"][cc]).view(-1, heads, hd)
        s = ops["scalar"] * prod.sum(-1)
        sabs = abs(ops["scalar"]) * prod.abs().sum(-1)
        if t is not None:
            s = s + t
            sabs = sabs + t.abs()
    delta = SA_EPS[dtype] * zeros(n, heads).index_reduce_(0, row, sabs, "amax", include_self=True)
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=device).index_reduce_(0, row, s, "amax", include_self=True)
    e = torch.exp(s - mx[row])
    l = zeros(n, heads).index_add_(0, row, e)
    pr = e / l[row]
    pw = pr if w is None else pr * torch.from_numpy(w).to(device)
    msg = pw.repeat_interleave(hd, dim=1) * ops["V"][cc]
    ref = zeros(n, h).index_add_(0, row, msg)
    mag = zeros(n, h).index_add_(0, row, msg.abs())
    lse = torch.where(l > 0, mx + torch.log(l.clamp_min(1e-300)), torch.zeros_like(l))
    return dict(ref=ref, mag=mag, lse=lse, delta=delta, pr=pr, row=row)


def out_bound(kind, dtype, r, h, heads):
    if kind == "gat":
        return GAT_TOL[dtype] * r["mag"] + U[dtype] * r["ref"].abs()
    return (2 * SA_EPS[dtype] + 2 * r["delta"].repeat_interleave(h // heads, dim=1)) * r["mag"] + U[dtype] * r["ref"].abs()


def lse_bound(kind, dtype, r):
    if kind == "gat":
        return GAT_TOL[dtype] * (1 + r["lse"].abs())
    return 2 * SA_EPS[dtype] * (1 + r["lse"].abs()) + r["delta"]


def remove_entries(n, rowptr, col, gone):
    """the CSR without the entries where `gone` (bool [nnz]) is set -> (rowptr, col)"""
    row = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    keep = ~gone
    rp = np.zeros(n + 1, dtype=rowptr.dtype)
    rp[1:] = np.cumsum(np.bincount(row[keep], minlength=n))
    return rp, col[keep].copy()
