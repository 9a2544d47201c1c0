"""Attention dropout without a device: the mask function of include/pygim_hip.h (pygim_attention_dropout_host, the function the kernels
call) against a numpy mirror written from the header's text, its statistics, the argument checks of every layer, and the sharpness of the
GPU file's forward bound on the float64 reference alone.

Statistics: a mask of N = nnz * heads independent bits that are kept with probability q = 1 - p has a keep rate within
5 * sqrt(p (1 - p) / N) of q except with probability 6e-7 (the binomial's normal approximation), and the sample correlation of two
independent such bit vectors times sqrt(N) is standard normal: 5 standard deviations again."""
import numpy as np
import pytest
import torch

import attn_dropout_ref as ad
import launch_shapes as ls
from pygim_amd import _lib, attention, gnn

SEEDS = (0, 1, 2 ** 32, 2 ** 63 + 7)
RATES = (0.0, 0.3, 0.5, 0.9)
HEADS = (1, 3, 8)
E0 = (0, 5000)
NNZ = 5121


@pytest.mark.parametrize("seed", SEEDS)
def test_host_mask_equals_the_numpy_mirror(seed):
    for p in RATES:
        for heads in HEADS:
            for e0 in E0:
                got = _lib.attention_dropout_host(NNZ, heads, e0, p, seed)
                want = ad.keep_mirror(np.arange(e0, e0 + NNZ), heads, p, seed)
                assert got.shape == (NNZ, heads) and got.dtype == np.uint8
                assert np.array_equal(got.astype(bool), want), f"seed {seed} p {p} heads {heads} e0 {e0}"
    # the entry index is taken mod 2^32 nowhere below 2^32: the last entries a CSR can hold
    top = _lib.attention_dropout_host(4, 2, 2 ** 31 - 5, 0.5, seed)
    assert np.array_equal(top.astype(bool), ad.keep_mirror(np.arange(2 ** 31 - 5, 2 ** 31 - 1), 2, 0.5, seed))


def corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("seed", SEEDS)
def test_mask_statistics(seed):
    for p in RATES[1:]:
        for heads in HEADS:
            for e0 in E0:
                keep = _lib.attention_dropout_host(NNZ, heads, e0, p, seed).astype(bool)
                N = keep.size
                rate = keep.mean()
                tag = f"seed {seed} p {p} heads {heads} e0 {e0}"
                figures = [abs(rate - (1 - p)) / np.sqrt(p * (1 - p) / N), abs(corr(keep[1:], keep[:-1])) * np.sqrt(keep[1:].size)]
                if heads > 1:
                    figures.append(abs(corr(keep[:, 1:], keep[:, :-1])) * np.sqrt(keep[:, 1:].size))
                print(f"mask statistics {tag}: keep rate, entry and head correlation in standard deviations = {[round(f, 2) for f in figures]}")
                assert all(f < 5 for f in figures), tag


def test_seeds_that_differ_in_one_bit_give_unrelated_masks():
    base = _lib.attention_dropout_host(NNZ, 8, 0, 0.5, 0x0123456789ABCDEF).astype(bool)
    for bit in (0, 31, 32, 63):
        other = _lib.attention_dropout_host(NNZ, 8, 0, 0.5, 0x0123456789ABCDEF ^ (1 << bit)).astype(bool)
        agree = (base == other).mean()
        assert abs(agree - 0.5) < 5 * 0.5 / np.sqrt(base.size), f"bit {bit}: {agree}"


def test_rate_zero_keeps_everything():
    for seed in SEEDS:
        assert _lib.attention_dropout_host(NNZ, 8, 0, 0.0, seed).all()
    assert ad.threshold(0.0) == 0 and ad.threshold(1 - 2.0 ** -40) == 2 ** 32 - 1


BAD_RATES = (-0.1, 1.0, 1.5, float("nan"))


def test_functions_and_layers_reject_a_rate_outside_the_unit_interval():
    x = torch.zeros(2, 4)
    for p in BAD_RATES:
        with pytest.raises(ValueError):
            attention.gat_aggregate(None, x, x, x, dropout=p)
        with pytest.raises(ValueError):
            attention.sparse_attention(None, x, x, x, dropout=p)
        with pytest.raises(ValueError):
            attention.gatv2_aggregate(None, x, x, x[0], dropout=p)
        with pytest.raises(ValueError):
            attention.dropout_mask(None, 1, p, 0)
        for layer in (gnn.GATConv, gnn.TransformerConv, gnn.GATv2Conv):
            with pytest.raises(ValueError):
                layer(4, 4, dropout=p)
        for stack in (gnn.GAT, gnn.GATv2, gnn.GraphTransformer):
            with pytest.raises(ValueError):
                stack(4, 4, 2, att_dropout=p)


def test_layers_keep_the_rate_and_the_defaults():
    for layer in (gnn.GATConv, gnn.TransformerConv, gnn.GATv2Conv):
        assert layer(4, 4).dropout == 0.0 and layer(4, 4, dropout=0.6).dropout == 0.6
    for stack in (gnn.GAT, gnn.GATv2, gnn.GraphTransformer):
        assert all(c.dropout == 0.0 for c in stack(4, 4, 2).convs) and all(c.dropout == 0.25 for c in stack(4, 4, 2, att_dropout=0.25).convs)
        assert stack(4, 4, 2, dropout=0.5, att_dropout=0.25).dropout == 0.5, "the feature dropout of the stack is another argument"


def test_c_entry_points_reject_a_bad_rate_before_anything_else():
    """no device, no initialisation and no valid pointer is needed for this answer"""
    for p in BAD_RATES:
        calls = (
            lambda: _lib.gat_aggregate_dropout(_lib.FLT32, 1, 0, 0, 0, 0, 0, 1, 0.2, 0, 4, 4, 0, 4, 0, 0, 0, 0, p, 1),
            lambda: _lib.sparse_attention_dropout(_lib.FLT32, 1, 0, 0, 0, 0, 4, 0, 4, 0, 4, 4, 1, 1.0, 0, 4, 0, 0, 0, 0, p, 1),
            lambda: _lib.gatv2_aggregate_dropout(_lib.FLT32, 1, 0, 0, 0, 0, 4, 0, 4, 0, 4, 1, 0.2, 0, 4, 0, 0, 0, 0, p, 1),
            lambda: _lib.gatv2_backward_dropout(_lib.FLT32, 0, 1, 0, 0, 0, 0, 4, 0, 4, 0, 4, 1, 0.2, 0, 4, 0, 0, 0, 4, 0, 0, 0, 0, 0, p, 1),
            lambda: _lib.attention_dropout_mask(_lib.FLT32, 1, 1, 0, p, 1, 0),
            lambda: _lib.attention_dropout_host(1, 1, 0, p, 1),
        )
        for call in calls:
            with pytest.raises(_lib.PygimError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID and "dropout" in str(e.value)
    with pytest.raises(_lib.PygimError):   # an entry index past 2^32 has no mask
        _lib.attention_dropout_host(2, 1, 2 ** 32 - 1, 0.5, 1)


def test_launch_shapes_answer_as_before():
    """the dropout entry points launch the base kernel's shape: no new PYGIM_SHAPE_* kind, and the existing kinds answer what the tables
    of launch_shapes.py state"""
    with pytest.raises(_lib.PygimError):
        _lib.gather_launch_shape(9, _lib.FLT32, 32, 4)
    for family in ("walker", "head"):
        for case in ls.TABLES[family]:
            for kind in ls.FAMILIES[family]["kinds"]:
                got = ls.query(family, case.h, case.heads, case.dtype, case.mis is None, kind)
                assert tuple(got[f] for f in _lib.SHAPE_FIELDS) == tuple(case.shape), (family, case, kind)


# ---- sharpness of the GPU file's forward bound, on the float64 reference alone ----
def sharp(kind, dtype, gname, n, rowptr, col, ops, h, heads, p):
    """the reference WITHOUT the mask against the reference with it: outside the bound in at least one output of every row that has a
    dropped entry of non-zero probability -- a kernel that ignored the mask could not pass the GPU test"""
    nnz = len(col)
    ops64 = ad.as_float64(ops, "cpu")
    w = ad.weights(nnz, heads, p, ad.SEED)
    masked = ad.reference(kind, dtype, n, rowptr, col, ops64, h, heads, w, "cpu")
    plain = ad.reference(kind, dtype, n, rowptr, col, ops64, h, heads, None, "cpu")
    outside = ((plain["ref"] - masked["ref"]).abs() > ad.out_bound(dtype, masked, h, heads)).any(dim=1)
    dropped = torch.from_numpy(w == 0) & (masked["pr"] > 0)
    rows = torch.zeros(n, dtype=torch.float64).index_add_(0, masked["row"], dropped.any(dim=1).double()) > 0
    assert rows.any(), "no dropped entry at all"
    assert bool(outside[rows].all()), f"{kind} {dtype} {gname} h={h} heads={heads} p={p}: rows {torch.nonzero(rows & ~outside).flatten().tolist()}"
    return int(rows.sum())


@pytest.mark.parametrize("kind", ad.KINDS)
@pytest.mark.parametrize("gname", list(ad.GRAPHS))
def test_the_forward_bound_tells_a_mask_that_is_ignored(kind, gname):
    n, m, rowptr, col = ad.graph(gname)
    for p in ad.PS:
        for dtype in (torch.float32, torch.float64, torch.bfloat16):
            for h, heads in (ad.HALF_CASES if dtype == torch.bfloat16 else ad.CASES):
                sharp(kind, dtype, gname, n, rowptr, col, ad.operands(kind, n, m, h, heads, dtype), h, heads, p)


@pytest.mark.parametrize("kind", ["sa", "gatv2"])
def test_the_forward_bound_tells_a_mask_that_is_ignored_two_launches(kind):
    n, m, rowptr, col = ls.two_launch_graph()
    h, heads = ad.TWO_LAUNCH
    for p in ad.PS:
        sharp(kind, torch.float32, "two-launch", n, rowptr, col, ad.two_launch_operands(kind), h, heads, p)
    # ... and a mask that took the second launch's heads for the first ones: head k of the second launch read as head k - 65535
    w = ad.weights(len(col), heads, 0.5, ad.SEED)
    assert (w[:, 65535:] != w[:, :2]).any(), "head0 matters to the mask of this case"
