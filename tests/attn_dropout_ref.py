"""Attention dropout: the numpy mirror of the mask, the cases, the operands and the float64 reference shared by test_attn_dropout_cpu.py
(the reference alone, no device) and test_attn_dropout_gpu.py (the kernels against it).  Host helpers take the torch device they compute
on, so one reference serves both files.

The mask, from the text of include/pygim_hip.h ("attention dropout"), all arithmetic uint32:
    fmix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
    u(e, k) = fmix(fmix(e ^ seed_lo) + seed_hi + k * 0x9E3779B9)
    keep(e, k) = u(e, k) >= T,  T = min(2^32 - 1, floor(p * 2^32))
The forward bound is the kernels' own with p[e] read as pr * w: |out - ref| <= (2 EPS + 2 Delta[r, k]) * sum_e pr w |v| + u |ref|, EPS = 1e-5
(FLT32 and the 16-bit types) / 1e-12 (DBL64), Delta the pygim_sddmm bound on a score (0 for gat_aggregate, whose scores are sums of two
numbers: its existing bound is 2 EPS * sum), u = 2^-8 (BF16)."""
import numpy as np
import torch

import launch_shapes as ls
import run_edges

CASES = [(4, 4), (9, 3), (32, 8), (100, 4), (256, 8), (512, 2)]   # (h, heads); the two-launch case is TWO_LAUNCH below
HALF_CASES = [(32, 8), (256, 8)]                                   # BF16
TWO_LAUNCH = ls.TWO_LAUNCHES                                       # heads across two launches of the head-wise kernels: head0
PS = (0.3, 0.5)
SEED = (0x9E3779B9 << 32) | 0x1234ABCD                             # both halves in use
KINDS = ("gat", "sa", "gatv2")
SLOPE = 0.2
EPS = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 1e-5}
U = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8}


def fmix(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def threshold(p):
    return min(2 ** 32 - 1, int(np.floor(p * 2.0 ** 32)))


def keep_mirror(entries, heads, p, seed):
    """bool [len(entries), heads]: entries are indices into A (any integer array)"""
    e = np.asarray(entries).astype(np.uint32)
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    k = np.arange(heads, dtype=np.uint32)
    with np.errstate(over="ignore"):
        inner = fmix(e ^ lo)
        u = fmix(inner[:, None] + hi + k[None, :] * np.uint32(0x9E3779B9))
    return u >= np.uint32(threshold(p))


def weights(nnz, heads, p, seed, entries=None):
    """float64 [nnz, heads]: 1 / (1 - p) where kept, 0 where dropped"""
    keep = keep_mirror(np.arange(nnz) if entries is None else entries, heads, p, seed)
    return np.where(keep, 1.0 / (1.0 - p), 0.0)


def small():
    """small_graph of test_attention_gpu.py with the suite's generator"""
    from test_attention_gpu import small_graph

    return small_graph(np.random.default_rng(1234))


GRAPHS = {"edges": run_edges.edges_graph, "small": small}
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def operands(kind, n, m, h, heads, dtype, seed=7):
    """host tensors in the ranges of the kernels' own parity tests -> dict(A, B, V, att, scalar): A is the row operand (a_dst, Q, x_dst), B
    the gathered one the score reads (a_src, K, x_src), V the gathered values (X, V, x_src), scalar the slope or the scale.  16-bit values:
    |v| in [0.5, 2) with random signs, as in the existing 16-bit tests (the bound has no absolute term)"""
    r = np.random.default_rng(seed)
    hd = h // heads
    ct = torch.float32 if dtype == torch.bfloat16 else dtype
    half = dtype == torch.bfloat16
    vals = lambda rows, lim: torch.from_numpy(r.uniform(0.5, 2, size=(rows, h)) * r.choice([-1.0, 1.0], size=(rows, h)) if half
                                              else r.uniform(-lim, lim, size=(rows, h))).to(dtype)
    if kind == "gat":
        return dict(A=torch.from_numpy(r.uniform(-4, 4, size=(n, heads))).to(ct), B=torch.from_numpy(r.uniform(-4, 4, size=(m, heads))).to(ct),
                    V=vals(m, 1), att=None, scalar=SLOPE)
    if kind == "sa":
        Q, K = (torch.from_numpy(r.uniform(-2, 2, size=(k, h))).to(dtype) for k in (n, m))
        return dict(A=Q, B=K, V=vals(m, 1), att=None, scalar=hd ** -0.5)
    Xd = torch.from_numpy(r.uniform(-2, 2, size=(n, h))).to(dtype)
    Xs = vals(m, 2)
    att = torch.from_numpy(r.uniform(-1, 1, size=h) * hd ** -0.5).to(ct)
    return dict(A=Xd, B=Xs, V=Xs, att=att, scalar=SLOPE)


def two_launch_operands(kind):
    """launch_shapes.two_launch_operands for the head-wise kernels, float32"""
    Q, K, V, att = (torch.from_numpy(t) for t in ls.two_launch_operands())
    hd = TWO_LAUNCH[0] // TWO_LAUNCH[1]
    if kind == "sa":
        return dict(A=Q, B=K, V=V, att=None, scalar=hd ** -0.5)
    return dict(A=Q, B=K, V=K, att=att, scalar=SLOPE)


def entry_rows(n, rowptr, device):
    return torch.repeat_interleave(torch.arange(n, device=device), torch.diff(torch.from_numpy(rowptr).long().to(device)))


def scores(kind, ops, row, cc, h, heads):
    """float64 (s, sum of the magnitudes a score is made of) per entry and head, from operands already on the device and in float64"""
    hd = h // heads
    if kind == "gat":
        z = ops["A"][row] + ops["B"][cc]
        return torch.where(z >= 0, z, ops["scalar"] * z), torch.zeros_like(z)
    if kind == "sa":
        prod = (ops["A"][row] * ops["B"][cc]).view(-1, heads, hd)
        return ops["scalar"] * prod.sum(-1), abs(ops["scalar"]) * prod.abs().sum(-1)
    terms = (torch.nn.functional.leaky_relu(ops["A"][row] + ops["B"][cc], ops["scalar"]) * ops["att"]).view(-1, heads, hd)
    return terms.sum(-1), terms.abs().sum(-1)


def reference(kind, dtype, n, rowptr, col, ops, h, heads, w, device):
    """float64 on `device`, from the operands as stored: dict(ref, mag = sum_e pr w |v| per output, lse (0 for empty rows), delta per row
    and head, pr [nnz, heads], row).  w: float64 numpy [nnz, heads] or None (no dropout: w = 1).  Differentiable in the float64 operands
    when they require grad (w is a constant)."""
    hd = h // heads
    row = entry_rows(n, rowptr, device)
    cc = torch.from_numpy(col).long().to(device)
    s, sabs = scores(kind, ops, row, cc, h, heads)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=device)
    delta = EPS[dtype] * z(n, heads).index_reduce_(0, row, sabs.detach(), "amax", include_self=True)
    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=device).index_reduce_(0, row, s.detach(), "amax", include_self=True)
    e = torch.exp(s - mx[row])
    l = z(n, heads).index_add(0, row, e)
    pr = e / l[row]
    pw = pr if w is None else pr * torch.from_numpy(w).to(device)
    msg = pw.repeat_interleave(hd, dim=1) * ops["V"][cc]
    ref = z(n, h).index_add(0, row, msg)
    mag = z(n, h).index_add(0, row, msg.detach().abs())
    lse = torch.where(l > 0, mx + torch.log(l.detach().clamp_min(1e-300)), torch.zeros_like(l)).detach()
    return dict(ref=ref, mag=mag, lse=lse, delta=delta, pr=pr.detach(), row=row)


def out_bound(dtype, r, h, heads):
    return (2 * EPS[dtype] + 2 * r["delta"].repeat_interleave(h // heads, dim=1)) * r["mag"] + U[dtype] * r["ref"].detach().abs()


def as_float64(ops, device):
    return {k: (v.to(device).double() if torch.is_tensor(v) else v) for k, v in ops.items()}
