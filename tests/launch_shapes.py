"""The launch shapes of the gather kernels, on purpose instead of by luck of a list: for every kernel family a table of cases (h, heads,
storage type, what is misaligned) with the shape each case is there for -- which instantiation and lane layout the launch_* function of
the family picks, as pygim_gather_launch_shape (include/pygim_hip.h) reports it.  The counterpart of run_edges.py on the feature / head
axis.  test_launch_shapes_cpu.py proves the tables complete and free of redundant cases from the query alone; test_launch_shapes_gpu.py
runs every case through the existing GPU files' own checks.  Host only.

A family is a set of entry points (or folds) that share one *_shape() function and one set of storage types (the CPU test asserts
that their kinds answer alike):
  walker        spmm_values, gat_aggregate               row_gather_shape, a piece must not lie across two heads
  mean          spmm_reduce MEAN                         row_gather_shape, no heads; FLT32, DBL64 and the 16-bit types
  maxmin        spmm_reduce MAX / MIN                    the same; FLT32, DBL64 and the four integer types
  reduce_bwd    spmm_reduce_backward                     the same with L lanes up to 64 pieces
  head          sparse_attention, gatv2 forward/backward head_gather_shape
  sddmm         sddmm
  edge_softmax  edge_softmax forward and backward
The storage types of a family come in groups (FLT32 | DBL64 | the 16-bit types | the integers): the kernels are templates over the
type, so every class a group reaches has to run in that group -- a one-element class that FLT32 covers is repeated in DBL64, in a
16-bit type and in an integer type ("second type of the same class").

To regenerate a table after a deliberate change of a launch function: print(table_text(family)) and paste it over the family's rows.
"""
from collections import namedtuple

import numpy as np
import torch

from pygim_amd import _lib

# mis: None (contiguous, aligned), "stride" (a row stride that is no multiple of a 16-byte piece) or "base" (a base pointer one element
# into a 16-byte aligned buffer while the strides stay multiples of a piece); the GPU tests misalign every operand in turn
Case = namedtuple("Case", "h heads dtype mis shape why")
# the stated shape, in the order of _lib.SHAPE_FIELDS: vec, pieces, LH, L, per, chunks, launches, flags
FLAG_NAMES = ((_lib.SHAPE_PART_PIECE, "last piece on some lanes only"), (_lib.SHAPE_PART_CHUNK, "last chunk partly filled"),
              (_lib.SHAPE_PART_HEADS, "a block's heads partly filled"), (_lib.SHAPE_SCALAR_SIZE, "scalar: the width fills no whole pieces"),
              (_lib.SHAPE_SCALAR_ALIGN, "scalar: misaligned"))

CODE = {"i8": _lib.INT8, "i16": _lib.INT16, "i32": _lib.INT32, "i64": _lib.INT64, "f32": _lib.FLT32, "f64": _lib.DBL64, "f16": _lib.FLT16,
        "bf16": _lib.BF16}
GROUP = {"f32": "FLT32", "f64": "DBL64", "bf16": "16-bit", "f16": "16-bit", "i8": "integer", "i16": "integer", "i32": "integer", "i64": "integer"}
GATHER_TYPES = ("f32", "f64", "bf16", "f16")
BIG_HEADS = (17, 33, 65, 130)          # "a few larger": the head counts at which 1, 2 and 4 lanes per head spill over blockIdx.y
TWO_LAUNCHES = (65537 * 33, 65537)     # (h, heads): one head per block and 65 537 chunks, the second launch holds two of them
ALL_MIS = (None, "stride", "base")

FAMILIES = {
    "walker": dict(kinds=(_lib.SHAPE_SPMM_VALUES, _lib.SHAPE_GAT_AGGREGATE), dtypes=GATHER_TYPES, mis=ALL_MIS),
    "mean": dict(kinds=(_lib.SHAPE_SPMM_REDUCE,), dtypes=GATHER_TYPES, mis=ALL_MIS),
    "maxmin": dict(kinds=(_lib.SHAPE_SPMM_REDUCE,), dtypes=("f32", "f64", "i8", "i16", "i32", "i64"), mis=ALL_MIS),
    "reduce_bwd": dict(kinds=(_lib.SHAPE_SPMM_REDUCE_BACKWARD,), dtypes=("f32", "f64"), mis=ALL_MIS),
    "head": dict(kinds=(_lib.SHAPE_SPARSE_ATTENTION, _lib.SHAPE_GATV2_AGGREGATE, _lib.SHAPE_GATV2_BACKWARD), dtypes=GATHER_TYPES, mis=ALL_MIS),
    "sddmm": dict(kinds=(_lib.SHAPE_SDDMM,), dtypes=GATHER_TYPES, mis=ALL_MIS),
    "edge_softmax": dict(kinds=(_lib.SHAPE_EDGE_SOFTMAX,), dtypes=("f32", "f64"), mis=(None, "base")),   # [nnz, heads] contiguous: no stride
}


def domain(family, dtype="f32"):
    """the (h, heads) a family is swept over: h in 1 .. 1100, heads in 1 .. 16 and BIG_HEADS where the family has heads, a head at most
    256 wide for the head-wise kernels, and for them (in FLT32, the type the GPU case runs in) the one shape that needs a second
    launch: the launches differ in head0 alone"""
    if family == "edge_softmax":
        return [(k, k) for k in range(1, 17)]
    if family in ("mean", "maxmin", "reduce_bwd", "sddmm"):
        return [(h, 1) for h in range(1, 1101)]
    out = [(h, k) for k in tuple(range(1, 17)) + BIG_HEADS for h in range(k, 1101, k) if family == "walker" or h // k <= 256]
    return out + ([TWO_LAUNCHES] if family == "head" and dtype == "f32" else [])


def query(family, h, heads, dtype, aligned, kind=None):
    return _lib.gather_launch_shape(FAMILIES[family]["kinds"][0] if kind is None else kind, CODE[dtype], h, heads, aligned)


def shape_class(family, shape):
    """what two cases must share to count as the same launch shape: every value of the piece width, the pieces per lane, LH and L;
    one head per block or several; one chunk or several; one launch or several; each of the three "partly filled" flags; and for
    edge_softmax why a scalar path is scalar (elsewhere the two reasons launch the same kernel with the same arguments: the
    misaligned calls are required per storage type instead, see requirements)"""
    flags = shape["flags"] if family == "edge_softmax" else shape["flags"] & (_lib.SHAPE_PART_PIECE | _lib.SHAPE_PART_CHUNK | _lib.SHAPE_PART_HEADS)
    return (shape["vec"], shape["pieces"], shape["LH"], shape["L"], shape["per"] > 1, shape["chunks"] > 1, shape["launches"] > 1, flags)


def requirements(family):
    """what the family's table has to cover: every class a group of storage types reaches, in a type of that group, and every storage
    type with every kind of misalignment"""
    fam = FAMILIES[family]
    need = {("type", d, m) for d in fam["dtypes"] for m in fam["mis"]}
    for d in fam["dtypes"]:
        for h, heads in domain(family, d):
            for aligned in (True, False):
                need.add(("class", GROUP[d]) + shape_class(family, query(family, h, heads, d, aligned)))
    return need


def satisfies(family, case):
    """the requirements a case covers: its class in its group of types, and its (type, misalignment) pair when the alignment is what
    decides -- an aligned case that takes 16-byte pieces, a misaligned one whose width would have filled whole pieces"""
    shape = query(family, case.h, case.heads, case.dtype, case.mis is None)
    decides = shape["vec"] > 1 if case.mis is None else bool(shape["flags"] & _lib.SHAPE_SCALAR_ALIGN)
    return {("class", GROUP[case.dtype]) + shape_class(family, shape)} | ({("type", case.dtype, case.mis)} if decides else set())


def describe(shape):
    s = (f"{shape['vec']}-element pieces, {shape['pieces']} per lane, LH {shape['LH']}, L {shape['L']}, {shape['per']} head(s) per block, "
         f"{shape['chunks']} chunk(s), {shape['launches']} launch(es)")
    return s + "".join("; " + name for bit, name in FLAG_NAMES if shape["flags"] & bit)


def C(h, heads, dtype, mis, *shape):
    """a case and the shape it is there for; its one-line statement is that shape in words"""
    return Case(h, heads, dtype, mis, shape, describe(dict(zip(_lib.SHAPE_FIELDS, shape))))


def select_cases(family):
    """a minimal table for requirements(family): greedy over the domain (the case that covers most of what is left, the narrowest
    first), then every case that is not the only one to cover something is dropped"""
    fam = FAMILIES[family]
    cands = {}
    for d in fam["dtypes"]:
        for h, heads in domain(family, d):
            for mis in fam["mis"]:
                c = Case(h, heads, d, mis, None, "")
                cands[c] = satisfies(family, c)
    order = sorted(cands, key=lambda c: (c.h, -c.heads))
    left, chosen = requirements(family), []
    while left:
        best = max(order, key=lambda c: (len(cands[c] & left), -c.h))
        assert cands[best] & left, sorted(left, key=str)[:3]
        chosen.append(best)
        left -= cands[best]
    for c in list(chosen):
        if not cands[c] - set().union(*(cands[o] for o in chosen if o != c)):
            chosen.remove(c)
    return sorted(chosen, key=lambda c: (fam["dtypes"].index(c.dtype), fam["mis"].index(c.mis), c.h, c.heads))


def table_text(family):
    """the source text of TABLES[family] for select_cases(family)"""
    out, key = [], None
    for c in select_cases(family):
        if (c.dtype, c.mis) != key:
            key = (c.dtype, c.mis)
            out.append(('""") + ' if out else f'TABLES["{family}"] = ') + f'rows("{c.dtype}", {c.mis!r}, """'.replace("'", '"'))
        shape = query(family, c.h, c.heads, c.dtype, c.mis is None)
        out.append(f"{c.h} {c.heads} | " + " ".join(str(shape[k]) for k in _lib.SHAPE_FIELDS))
    return "\n".join(out + ['""")'])


# ---- the deep cases: the reduction depth of the GATv2 datt, and the head-wise kernels' second launch ----
DATT_CASES = ((256, 8, 2), (257, 8, 2), (513, 8, 2), (65537, 1, 1))   # (runs, h, heads); GV2_RED = 256 partials are added per level
SLOPE = 0.2


def datt_levels(runs):
    """levels of k_gatv2_datt_reduce (gatv2_dev.hpp): 256 partials per thread and level"""
    levels = 1
    while runs > 256:
        runs, levels = (runs + 255) // 256, levels + 1
    return levels


def datt_graph(runs, device="cpu"):
    """64 rows of equal length over `runs` runs of 512 entries, columns e % 61; whole runs, except for the three-level graph, whose
    last run holds one entry (nnz = 512 * 65 536 + 1).  Built where it is used: nothing of size nnz crosses the bus"""
    nnz = 512 * runs if runs < 65537 else 512 * (runs - 1) + 1
    n, m = 64, 61
    rowptr = (torch.arange(n + 1, device=device, dtype=torch.int64) * (nnz // n)).clamp(max=nnz)
    rowptr[-1] = nnz
    col = (torch.arange(nnz, device=device, dtype=torch.int64) % m).to(torch.int32)
    assert (nnz + 511) // 512 == runs
    return n, m, rowptr.to(torch.int32), col


def datt_operands(runs, h, heads, dtype):
    """x_dst, x_src, G, att in (0.5, 1.5), att / sqrt(hd): one sign, so that datt is a sum of positive row terms G[r] * Var_p(x_src) (one
    head of one feature) and no run's part of it is lost in a cancellation"""
    gen = torch.Generator().manual_seed(runs)
    Xd, Xs, G = (torch.rand(r, h, dtype=torch.float64, generator=gen).add(0.5).to(dtype) for r in (64, 61, 64))
    att = (torch.rand(h, dtype=torch.float64, generator=gen).add(0.5) * (h // heads) ** -0.5).to(dtype)
    return Xd, Xs, G, att


def datt_reference(rowptr, col, Xd, Xs, att, G, h, heads, slope=SLOPE, chunk=1 << 22, per_run=False):
    """float64 on the operands' device, closed form (include/pygim_hip.h): datt[f] = sum_e ds[e, head of f] * lrelu(z[e, f]), with lse
    and delta from the same pass -> (datt, lse, delta, every run's part of datt [runs, h] when per_run).  The entries go in chunks, so
    that the [nnz, h] terms of the three-level graph never exist at once"""
    dev = Xd.device
    n, hd = rowptr.numel() - 1, h // heads
    row = torch.repeat_interleave(torch.arange(n, device=dev), torch.diff(rowptr.long()))
    cc = col.long()
    xd, xs, a, Gd = Xd.double(), Xs.double(), att.double(), G.double()
    nnz = cc.numel()

    def scores(lo):
        z = torch.nn.functional.leaky_relu(xd[row[lo:lo + chunk]] + xs[cc[lo:lo + chunk]], slope)
        return z, (z * a).view(-1, heads, hd).sum(-1)

    mx = torch.full((n, heads), -float("inf"), dtype=torch.float64, device=dev)
    for lo in range(0, nnz, chunk):
        mx.index_reduce_(0, row[lo:lo + chunk], scores(lo)[1], "amax", include_self=True)
    l = torch.zeros(n, heads, dtype=torch.float64, device=dev)
    out = torch.zeros(n, h, dtype=torch.float64, device=dev)
    for lo in range(0, nnz, chunk):
        r = row[lo:lo + chunk]
        e = torch.exp(scores(lo)[1] - mx[r])
        l.index_add_(0, r, e)
        out.index_add_(0, r, e.repeat_interleave(hd, dim=1) * xs[cc[lo:lo + chunk]])
    out = out / l.repeat_interleave(hd, dim=1)
    lse = mx + torch.log(l)
    delta = (Gd * out).view(n, heads, hd).sum(-1)
    datt = torch.zeros(h, dtype=torch.float64, device=dev)
    parts = []
    for lo in range(0, nnz, chunk):
        r, c = row[lo:lo + chunk], cc[lo:lo + chunk]
        z, s = scores(lo)
        ds = torch.exp(s - lse[r]) * ((Gd[r] * xs[c]).view(-1, heads, hd).sum(-1) - delta[r])
        t = ds.repeat_interleave(hd, dim=1) * z
        datt += t.sum(0)
        if per_run:
            pad = (-t.size(0)) % 512
            parts.append(torch.cat([t, t.new_zeros(pad, h)]).view(-1, 512, h).sum(1))
    return datt, lse, delta, (torch.cat(parts) if per_run else None)


def two_launch_graph():
    """three rows (one empty), five entries, two columns"""
    return 3, 2, np.array([0, 3, 3, 5], dtype=np.int32), np.array([0, 1, 1, 0, 1], dtype=np.int32)


def two_launch_operands():
    """float32 Q / x_dst [3, h], K / x_src [2, h], V [2, h] and att [h] for TWO_LAUNCHES, in the ranges of the parity tests"""
    h, heads = TWO_LAUNCHES
    r = np.random.default_rng(65537)
    Q, K = (r.uniform(-2, 2, size=(k, h)).astype(np.float32) for k in (3, 2))
    V = r.uniform(-1, 1, size=(2, h)).astype(np.float32)
    att = (r.uniform(-1, 1, size=h) * (h // heads) ** -0.5).astype(np.float32)
    return Q, K, V, att


def rows(dtype, mis, text):
    """one case per line: h heads | vec pieces LH L per chunks launches flags"""
    return [C(*(int(v) for v in line.split()[:2]), dtype, mis, *(int(v) for v in line.split()[3:])) for line in text.strip().splitlines()]


# Every table is minimal for requirements(): test_launch_shapes_cpu.py fails when a case is removed, and when a launch function changes
# so that a stated shape is no longer what it picks.  flags: 1 last piece on some lanes only, 2 last chunk partly filled, 4 a block's
# heads partly filled, 8 scalar because of the width, 16 scalar because of the misalignment alone.
TABLES = {}
TABLES["walker"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 2 | 1 1 2 2 1 1 1 8
3 3 | 1 1 4 4 1 1 1 9
4 1 | 4 1 1 1 1 1 1 0
5 5 | 1 1 8 8 1 1 1 9
8 2 | 4 1 2 2 1 1 1 0
9 9 | 1 1 16 16 1 1 1 9
12 3 | 4 1 4 4 1 1 1 1
16 4 | 4 1 4 4 1 1 1 0
16 16 | 1 1 16 16 1 1 1 8
17 17 | 1 1 32 32 1 1 1 9
20 5 | 4 1 8 8 1 1 1 1
32 8 | 4 1 8 8 1 1 1 0
32 16 | 1 1 32 32 1 1 1 8
33 33 | 1 1 64 64 1 1 1 9
36 9 | 4 1 16 16 1 1 1 1
64 16 | 4 1 16 16 1 1 1 0
65 65 | 1 2 64 64 1 1 1 9
68 17 | 4 1 32 32 1 1 1 1
128 16 | 4 1 32 32 1 1 1 0
129 3 | 1 2 64 64 1 2 1 11
132 33 | 4 1 64 64 1 1 1 1
256 16 | 4 1 64 64 1 1 1 0
260 65 | 4 2 64 64 1 1 1 1
512 16 | 4 2 64 64 1 1 1 0
516 3 | 4 2 64 64 1 2 1 3
768 16 | 4 2 64 64 1 2 1 2
1024 16 | 4 2 64 64 1 2 1 0
""") + rows("f32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
64 16 | 1 1 64 64 1 1 1 16
128 16 | 1 2 64 64 1 1 1 16
192 16 | 1 2 64 64 1 2 1 18
256 16 | 1 2 64 64 1 2 1 16
""") + rows("f32", "base", """
8 2 | 1 1 8 8 1 1 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 2 1 1 1 1 1 1 0
3 3 | 1 1 4 4 1 1 1 9
4 2 | 2 1 2 2 1 1 1 0
5 5 | 1 1 8 8 1 1 1 9
6 3 | 2 1 4 4 1 1 1 1
8 4 | 2 1 4 4 1 1 1 0
8 8 | 1 1 8 8 1 1 1 8
9 9 | 1 1 16 16 1 1 1 9
10 5 | 2 1 8 8 1 1 1 1
16 8 | 2 1 8 8 1 1 1 0
16 16 | 1 1 16 16 1 1 1 8
17 17 | 1 1 32 32 1 1 1 9
18 9 | 2 1 16 16 1 1 1 1
32 16 | 2 1 16 16 1 1 1 0
33 33 | 1 1 64 64 1 1 1 9
34 17 | 2 1 32 32 1 1 1 1
64 16 | 2 1 32 32 1 1 1 0
65 65 | 1 2 64 64 1 1 1 9
66 33 | 2 1 64 64 1 1 1 1
128 16 | 2 1 64 64 1 1 1 0
129 3 | 1 2 64 64 1 2 1 11
130 65 | 2 2 64 64 1 1 1 1
256 16 | 2 2 64 64 1 1 1 0
258 3 | 2 2 64 64 1 2 1 3
384 16 | 2 2 64 64 1 2 1 2
512 16 | 2 2 64 64 1 2 1 0
""") + rows("f64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
32 16 | 1 1 32 32 1 1 1 16
64 16 | 1 1 64 64 1 1 1 16
128 16 | 1 2 64 64 1 1 1 16
192 16 | 1 2 64 64 1 2 1 18
256 16 | 1 2 64 64 1 2 1 16
""") + rows("f64", "base", """
4 2 | 1 1 4 4 1 1 1 16
""") + rows("bf16", None, """
1 1 | 1 1 1 1 1 1 1 8
2 2 | 1 1 2 2 1 1 1 8
3 3 | 1 1 4 4 1 1 1 9
4 4 | 1 1 4 4 1 1 1 8
5 5 | 1 1 8 8 1 1 1 9
8 1 | 8 1 1 1 1 1 1 0
9 9 | 1 1 16 16 1 1 1 9
24 3 | 8 1 4 4 1 1 1 1
32 4 | 8 1 4 4 1 1 1 0
33 33 | 1 1 64 64 1 1 1 9
40 5 | 8 1 8 8 1 1 1 1
64 8 | 8 1 8 8 1 1 1 0
64 16 | 1 1 64 64 1 1 1 8
65 65 | 1 2 64 64 1 1 1 9
72 9 | 8 1 16 16 1 1 1 1
128 16 | 8 1 16 16 1 1 1 0
129 3 | 1 2 64 64 1 2 1 11
136 17 | 8 1 32 32 1 1 1 1
192 16 | 1 2 64 64 1 2 1 10
256 16 | 8 1 32 32 1 1 1 0
264 33 | 8 1 64 64 1 1 1 1
512 16 | 8 1 64 64 1 1 1 0
520 65 | 8 2 64 64 1 1 1 1
1024 16 | 8 2 64 64 1 1 1 0
1032 3 | 8 2 64 64 1 2 1 3
""") + rows("bf16", "stride", """
8 1 | 1 1 8 8 1 1 1 16
128 16 | 1 2 64 64 1 1 1 16
256 16 | 1 2 64 64 1 2 1 16
""") + rows("bf16", "base", """
16 2 | 1 1 16 16 1 1 1 16
""") + rows("f16", None, """
16 2 | 8 1 2 2 1 1 1 0
""") + rows("f16", "stride", """
24 3 | 1 1 32 32 1 1 1 17
""") + rows("f16", "base", """
32 4 | 1 1 32 32 1 1 1 16
""")

TABLES["mean"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
4 1 | 4 1 1 1 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
8 1 | 4 1 2 2 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
12 1 | 4 1 4 4 1 1 1 1
16 1 | 4 1 4 4 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
20 1 | 4 1 8 8 1 1 1 1
32 1 | 4 1 8 8 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
36 1 | 4 1 16 16 1 1 1 1
64 1 | 4 1 16 16 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
68 1 | 4 1 32 32 1 1 1 1
128 1 | 4 1 32 32 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
132 1 | 4 1 64 64 1 1 1 1
256 1 | 4 1 64 64 1 1 1 0
260 1 | 4 2 64 64 1 1 1 1
512 1 | 4 2 64 64 1 1 1 0
516 1 | 4 2 64 64 1 2 1 3
768 1 | 4 2 64 64 1 2 1 2
1024 1 | 4 2 64 64 1 2 1 0
""") + rows("f32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("f32", "base", """
8 1 | 1 1 8 8 1 1 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 2 1 1 1 1 1 1 0
3 1 | 1 1 4 4 1 1 1 9
4 1 | 2 1 2 2 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
6 1 | 2 1 4 4 1 1 1 1
8 1 | 2 1 4 4 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
10 1 | 2 1 8 8 1 1 1 1
16 1 | 2 1 8 8 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
18 1 | 2 1 16 16 1 1 1 1
32 1 | 2 1 16 16 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
34 1 | 2 1 32 32 1 1 1 1
64 1 | 2 1 32 32 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
66 1 | 2 1 64 64 1 1 1 1
128 1 | 2 1 64 64 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
130 1 | 2 2 64 64 1 1 1 1
256 1 | 2 2 64 64 1 1 1 0
258 1 | 2 2 64 64 1 2 1 3
384 1 | 2 2 64 64 1 2 1 2
512 1 | 2 2 64 64 1 2 1 0
""") + rows("f64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
8 1 | 1 1 8 8 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("f64", "base", """
4 1 | 1 1 4 4 1 1 1 16
""") + rows("bf16", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
4 1 | 1 1 4 4 1 1 1 8
5 1 | 1 1 8 8 1 1 1 9
8 1 | 8 1 1 1 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
24 1 | 8 1 4 4 1 1 1 1
32 1 | 8 1 4 4 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
40 1 | 8 1 8 8 1 1 1 1
64 1 | 8 1 8 8 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
72 1 | 8 1 16 16 1 1 1 1
128 1 | 8 1 16 16 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
136 1 | 8 1 32 32 1 1 1 1
256 1 | 8 1 32 32 1 1 1 0
264 1 | 8 1 64 64 1 1 1 1
512 1 | 8 1 64 64 1 1 1 0
520 1 | 8 2 64 64 1 1 1 1
1024 1 | 8 2 64 64 1 1 1 0
1032 1 | 8 2 64 64 1 2 1 3
""") + rows("bf16", "stride", """
8 1 | 1 1 8 8 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("bf16", "base", """
16 1 | 1 1 16 16 1 1 1 16
""") + rows("f16", None, """
16 1 | 8 1 2 2 1 1 1 0
""") + rows("f16", "stride", """
24 1 | 1 1 32 32 1 1 1 17
""") + rows("f16", "base", """
32 1 | 1 1 32 32 1 1 1 16
""")

TABLES["maxmin"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
4 1 | 4 1 1 1 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
8 1 | 4 1 2 2 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
12 1 | 4 1 4 4 1 1 1 1
16 1 | 4 1 4 4 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
20 1 | 4 1 8 8 1 1 1 1
32 1 | 4 1 8 8 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
36 1 | 4 1 16 16 1 1 1 1
64 1 | 4 1 16 16 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
68 1 | 4 1 32 32 1 1 1 1
128 1 | 4 1 32 32 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
132 1 | 4 1 64 64 1 1 1 1
256 1 | 4 1 64 64 1 1 1 0
260 1 | 4 2 64 64 1 1 1 1
512 1 | 4 2 64 64 1 1 1 0
516 1 | 4 2 64 64 1 2 1 3
768 1 | 4 2 64 64 1 2 1 2
1024 1 | 4 2 64 64 1 2 1 0
""") + rows("f32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("f32", "base", """
8 1 | 1 1 8 8 1 1 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 2 1 1 1 1 1 1 0
3 1 | 1 1 4 4 1 1 1 9
4 1 | 2 1 2 2 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
6 1 | 2 1 4 4 1 1 1 1
8 1 | 2 1 4 4 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
10 1 | 2 1 8 8 1 1 1 1
16 1 | 2 1 8 8 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
18 1 | 2 1 16 16 1 1 1 1
32 1 | 2 1 16 16 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
34 1 | 2 1 32 32 1 1 1 1
64 1 | 2 1 32 32 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
66 1 | 2 1 64 64 1 1 1 1
128 1 | 2 1 64 64 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
130 1 | 2 2 64 64 1 1 1 1
256 1 | 2 2 64 64 1 1 1 0
258 1 | 2 2 64 64 1 2 1 3
384 1 | 2 2 64 64 1 2 1 2
512 1 | 2 2 64 64 1 2 1 0
""") + rows("f64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
8 1 | 1 1 8 8 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("f64", "base", """
4 1 | 1 1 4 4 1 1 1 16
""") + rows("i8", None, """
1 1 | 1 1 1 1 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
16 1 | 16 1 1 1 1 1 1 0
32 1 | 16 1 2 2 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
48 1 | 16 1 4 4 1 1 1 1
64 1 | 16 1 4 4 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
80 1 | 16 1 8 8 1 1 1 1
128 1 | 16 1 8 8 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
144 1 | 16 1 16 16 1 1 1 1
256 1 | 16 1 16 16 1 1 1 0
272 1 | 16 1 32 32 1 1 1 1
512 1 | 16 1 32 32 1 1 1 0
528 1 | 16 1 64 64 1 1 1 1
1024 1 | 16 1 64 64 1 1 1 0
1040 1 | 16 2 64 64 1 1 1 1
""") + rows("i8", "stride", """
16 1 | 1 1 16 16 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("i8", "base", """
32 1 | 1 1 32 32 1 1 1 16
""") + rows("i16", None, """
8 1 | 8 1 1 1 1 1 1 0
16 1 | 8 1 2 2 1 1 1 0
24 1 | 8 1 4 4 1 1 1 1
32 1 | 8 1 4 4 1 1 1 0
40 1 | 8 1 8 8 1 1 1 1
64 1 | 8 1 8 8 1 1 1 0
72 1 | 8 1 16 16 1 1 1 1
128 1 | 8 1 16 16 1 1 1 0
136 1 | 8 1 32 32 1 1 1 1
256 1 | 8 1 32 32 1 1 1 0
264 1 | 8 1 64 64 1 1 1 1
512 1 | 8 1 64 64 1 1 1 0
520 1 | 8 2 64 64 1 1 1 1
1024 1 | 8 2 64 64 1 1 1 0
1032 1 | 8 2 64 64 1 2 1 3
""") + rows("i16", "stride", """
8 1 | 1 1 8 8 1 1 1 16
""") + rows("i16", "base", """
24 1 | 1 1 32 32 1 1 1 17
""") + rows("i32", None, """
4 1 | 4 1 1 1 1 1 1 0
8 1 | 4 1 2 2 1 1 1 0
12 1 | 4 1 4 4 1 1 1 1
16 1 | 4 1 4 4 1 1 1 0
20 1 | 4 1 8 8 1 1 1 1
32 1 | 4 1 8 8 1 1 1 0
36 1 | 4 1 16 16 1 1 1 1
64 1 | 4 1 16 16 1 1 1 0
68 1 | 4 1 32 32 1 1 1 1
128 1 | 4 1 32 32 1 1 1 0
132 1 | 4 1 64 64 1 1 1 1
256 1 | 4 1 64 64 1 1 1 0
260 1 | 4 2 64 64 1 1 1 1
512 1 | 4 2 64 64 1 1 1 0
516 1 | 4 2 64 64 1 2 1 3
768 1 | 4 2 64 64 1 2 1 2
1024 1 | 4 2 64 64 1 2 1 0
""") + rows("i32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
""") + rows("i32", "base", """
12 1 | 1 1 16 16 1 1 1 17
""") + rows("i64", None, """
2 1 | 2 1 1 1 1 1 1 0
4 1 | 2 1 2 2 1 1 1 0
6 1 | 2 1 4 4 1 1 1 1
8 1 | 2 1 4 4 1 1 1 0
10 1 | 2 1 8 8 1 1 1 1
16 1 | 2 1 8 8 1 1 1 0
18 1 | 2 1 16 16 1 1 1 1
32 1 | 2 1 16 16 1 1 1 0
34 1 | 2 1 32 32 1 1 1 1
64 1 | 2 1 32 32 1 1 1 0
66 1 | 2 1 64 64 1 1 1 1
128 1 | 2 1 64 64 1 1 1 0
130 1 | 2 2 64 64 1 1 1 1
256 1 | 2 2 64 64 1 1 1 0
258 1 | 2 2 64 64 1 2 1 3
384 1 | 2 2 64 64 1 2 1 2
512 1 | 2 2 64 64 1 2 1 0
""") + rows("i64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
""") + rows("i64", "base", """
6 1 | 1 1 8 8 1 1 1 17
""")

TABLES["reduce_bwd"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
4 1 | 4 1 1 1 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
8 1 | 4 1 2 2 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
12 1 | 4 1 4 4 1 1 1 1
16 1 | 4 1 4 4 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
20 1 | 4 1 8 8 1 1 1 1
32 1 | 4 1 8 8 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
36 1 | 4 1 16 16 1 1 1 1
64 1 | 4 1 16 16 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
68 1 | 4 1 32 32 1 1 1 1
128 1 | 4 1 32 32 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
132 1 | 4 1 64 64 1 1 1 1
256 1 | 4 1 64 64 1 1 1 0
260 1 | 4 2 64 64 1 1 1 1
512 1 | 4 2 64 64 1 1 1 0
516 1 | 4 2 64 64 1 2 1 3
768 1 | 4 2 64 64 1 2 1 2
1024 1 | 4 2 64 64 1 2 1 0
""") + rows("f32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("f32", "base", """
8 1 | 1 1 8 8 1 1 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 2 1 1 1 1 1 1 0
3 1 | 1 1 4 4 1 1 1 9
4 1 | 2 1 2 2 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
6 1 | 2 1 4 4 1 1 1 1
8 1 | 2 1 4 4 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
10 1 | 2 1 8 8 1 1 1 1
16 1 | 2 1 8 8 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
18 1 | 2 1 16 16 1 1 1 1
32 1 | 2 1 16 16 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
34 1 | 2 1 32 32 1 1 1 1
64 1 | 2 1 32 32 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
66 1 | 2 1 64 64 1 1 1 1
128 1 | 2 1 64 64 1 1 1 0
129 1 | 1 2 64 64 1 2 1 11
130 1 | 2 2 64 64 1 1 1 1
256 1 | 2 2 64 64 1 1 1 0
258 1 | 2 2 64 64 1 2 1 3
384 1 | 2 2 64 64 1 2 1 2
512 1 | 2 2 64 64 1 2 1 0
""") + rows("f64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
8 1 | 1 1 8 8 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 2 64 64 1 2 1 18
256 1 | 1 2 64 64 1 2 1 16
""") + rows("f64", "base", """
4 1 | 1 1 4 4 1 1 1 16
""")

TABLES["head"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
2 2 | 1 1 1 2 2 1 1 8
3 1 | 1 1 4 4 1 1 1 9
3 3 | 1 1 1 4 4 1 1 12
4 1 | 4 1 1 1 1 1 1 0
4 2 | 1 1 2 4 2 1 1 8
4 4 | 1 1 1 4 4 1 1 8
5 1 | 1 1 8 8 1 1 1 9
5 5 | 1 1 1 8 8 1 1 12
6 2 | 1 1 4 8 2 1 1 9
6 3 | 1 1 2 8 4 1 1 12
8 1 | 4 1 2 2 1 1 1 0
8 2 | 4 1 1 2 2 1 1 0
8 4 | 1 1 2 8 4 1 1 8
8 8 | 1 1 1 8 8 1 1 8
9 1 | 1 1 16 16 1 1 1 9
9 3 | 1 1 4 16 4 1 1 13
9 9 | 1 1 1 16 16 1 1 12
10 2 | 1 1 8 16 2 1 1 9
10 5 | 1 1 2 16 8 1 1 12
12 1 | 4 1 4 4 1 1 1 1
12 3 | 4 1 1 4 4 1 1 4
12 4 | 1 1 4 16 4 1 1 9
15 3 | 1 1 8 32 4 1 1 13
15 5 | 1 1 4 32 8 1 1 13
16 1 | 4 1 4 4 1 1 1 0
16 2 | 4 1 2 4 2 1 1 0
16 4 | 4 1 1 4 4 1 1 0
16 8 | 1 1 2 16 8 1 1 8
16 16 | 1 1 1 16 16 1 1 8
17 1 | 1 1 32 32 1 1 1 9
17 17 | 1 1 1 32 32 1 1 12
18 2 | 1 1 16 32 2 1 1 9
18 9 | 1 1 2 32 16 1 1 12
20 1 | 4 1 8 8 1 1 1 1
20 4 | 1 1 8 32 4 1 1 9
20 5 | 4 1 1 8 8 1 1 4
24 2 | 4 1 4 8 2 1 1 1
24 3 | 4 1 2 8 4 1 1 4
24 8 | 1 1 4 32 8 1 1 9
25 5 | 1 1 8 64 8 1 1 13
27 3 | 1 1 16 64 4 1 1 13
27 9 | 1 1 4 64 16 1 1 13
32 1 | 4 1 8 8 1 1 1 0
32 2 | 4 1 4 8 2 1 1 0
32 4 | 4 1 2 8 4 1 1 0
32 8 | 4 1 1 8 8 1 1 0
32 16 | 1 1 2 32 16 1 1 8
33 1 | 1 1 64 64 1 1 1 9
33 33 | 1 1 1 64 64 1 1 12
34 2 | 1 1 32 64 2 1 1 9
34 17 | 1 1 2 64 32 1 1 12
36 1 | 4 1 16 16 1 1 1 1
36 3 | 4 1 4 16 4 1 1 5
36 4 | 1 1 16 64 4 1 1 9
36 9 | 4 1 1 16 16 1 1 4
40 2 | 4 1 8 16 2 1 1 1
40 5 | 4 1 2 16 8 1 1 4
40 8 | 1 1 8 64 8 1 1 9
45 5 | 1 1 16 64 4 2 1 15
45 9 | 1 1 8 64 8 2 1 15
48 3 | 4 1 4 16 4 1 1 4
48 4 | 4 1 4 16 4 1 1 1
48 16 | 1 1 4 64 16 1 1 9
51 3 | 1 1 32 64 2 2 1 15
51 17 | 1 1 4 64 16 2 1 15
60 3 | 4 1 8 32 4 1 1 5
60 5 | 4 1 4 32 8 1 1 5
64 1 | 4 1 16 16 1 1 1 0
64 2 | 4 1 8 16 2 1 1 0
64 4 | 4 1 4 16 4 1 1 0
64 8 | 4 1 2 16 8 1 1 0
64 16 | 4 1 1 16 16 1 1 0
65 1 | 1 2 64 64 1 1 1 9
65 65 | 1 1 1 64 64 2 1 14
66 2 | 1 1 64 64 1 2 1 9
66 33 | 1 1 2 64 32 2 1 14
68 1 | 4 1 32 32 1 1 1 1
68 4 | 1 1 32 64 2 2 1 9
68 17 | 4 1 1 32 32 1 1 4
72 2 | 4 1 16 32 2 1 1 1
72 8 | 1 1 16 64 4 2 1 9
72 9 | 4 1 2 32 16 1 1 4
80 4 | 4 1 8 32 4 1 1 1
80 5 | 4 1 4 32 8 1 1 4
80 16 | 1 1 8 64 8 2 1 9
96 3 | 4 1 8 32 4 1 1 4
96 8 | 4 1 4 32 8 1 1 1
100 5 | 4 1 8 64 8 1 1 5
108 3 | 4 1 16 64 4 1 1 5
108 9 | 4 1 4 64 16 1 1 5
128 1 | 4 1 32 32 1 1 1 0
128 2 | 4 1 16 32 2 1 1 0
128 4 | 4 1 8 32 4 1 1 0
128 8 | 4 1 4 32 8 1 1 0
128 16 | 4 1 2 32 16 1 1 0
129 1 | 1 4 64 64 1 1 1 9
130 2 | 1 2 64 64 1 2 1 9
132 1 | 4 1 64 64 1 1 1 1
132 33 | 4 1 1 64 64 1 1 4
136 2 | 4 1 32 64 2 1 1 1
136 17 | 4 1 2 64 32 1 1 4
144 4 | 4 1 16 64 4 1 1 1
144 9 | 4 1 4 64 16 1 1 4
160 5 | 4 1 8 64 8 1 1 4
160 8 | 4 1 8 64 8 1 1 1
180 5 | 4 1 16 64 4 2 1 7
180 9 | 4 1 8 64 8 2 1 7
192 3 | 4 1 16 64 4 1 1 4
192 16 | 4 1 4 64 16 1 1 1
204 3 | 4 1 32 64 2 2 1 7
204 17 | 4 1 4 64 16 2 1 7
256 1 | 4 1 64 64 1 1 1 0
256 2 | 4 1 32 64 2 1 1 0
256 4 | 4 1 16 64 4 1 1 0
256 8 | 4 1 8 64 8 1 1 0
256 16 | 4 1 4 64 16 1 1 0
258 2 | 1 4 64 64 1 2 1 9
260 65 | 4 1 1 64 64 2 1 6
264 2 | 4 1 64 64 1 2 1 1
264 33 | 4 1 2 64 32 2 1 6
272 4 | 4 1 32 64 2 2 1 1
272 17 | 4 1 4 64 16 2 1 6
288 8 | 4 1 16 64 4 2 1 1
288 9 | 4 1 8 64 8 2 1 6
320 5 | 4 1 16 64 4 2 1 6
320 16 | 4 1 8 64 8 2 1 1
384 3 | 4 1 32 64 2 2 1 6
512 2 | 4 1 64 64 1 2 1 0
512 4 | 4 1 32 64 2 2 1 0
512 8 | 4 1 16 64 4 2 1 0
512 16 | 4 1 8 64 8 2 1 0
2162721 65537 | 1 1 64 64 1 65537 2 9
""") + rows("f32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
8 1 | 1 1 8 8 1 1 1 16
12 3 | 1 1 4 16 4 1 1 20
16 1 | 1 1 16 16 1 1 1 16
16 2 | 1 1 8 16 2 1 1 16
16 4 | 1 1 4 16 4 1 1 16
20 5 | 1 1 4 32 8 1 1 20
24 3 | 1 1 8 32 4 1 1 20
32 1 | 1 1 32 32 1 1 1 16
32 2 | 1 1 16 32 2 1 1 16
32 4 | 1 1 8 32 4 1 1 16
32 8 | 1 1 4 32 8 1 1 16
36 9 | 1 1 4 64 16 1 1 20
40 5 | 1 1 8 64 8 1 1 20
48 3 | 1 1 16 64 4 1 1 20
64 1 | 1 1 64 64 1 1 1 16
64 2 | 1 1 32 64 2 1 1 16
64 4 | 1 1 16 64 4 1 1 16
64 8 | 1 1 8 64 8 1 1 16
64 16 | 1 1 4 64 16 1 1 16
68 17 | 1 1 4 64 16 2 1 22
72 9 | 1 1 8 64 8 2 1 22
80 5 | 1 1 16 64 4 2 1 22
96 3 | 1 1 32 64 2 2 1 22
128 1 | 1 2 64 64 1 1 1 16
128 2 | 1 1 64 64 1 2 1 16
128 4 | 1 1 32 64 2 2 1 16
128 8 | 1 1 16 64 4 2 1 16
128 16 | 1 1 8 64 8 2 1 16
256 1 | 1 4 64 64 1 1 1 16
256 2 | 1 2 64 64 1 2 1 16
512 2 | 1 4 64 64 1 2 1 16
""") + rows("f32", "base", """
8 2 | 1 1 4 8 2 1 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 2 1 1 1 1 1 1 0
2 2 | 1 1 1 2 2 1 1 8
3 1 | 1 1 4 4 1 1 1 9
3 3 | 1 1 1 4 4 1 1 12
4 1 | 2 1 2 2 1 1 1 0
4 2 | 2 1 1 2 2 1 1 0
4 4 | 1 1 1 4 4 1 1 8
5 1 | 1 1 8 8 1 1 1 9
5 5 | 1 1 1 8 8 1 1 12
6 1 | 2 1 4 4 1 1 1 1
6 2 | 1 1 4 8 2 1 1 9
6 3 | 2 1 1 4 4 1 1 4
8 1 | 2 1 4 4 1 1 1 0
8 2 | 2 1 2 4 2 1 1 0
8 4 | 2 1 1 4 4 1 1 0
8 8 | 1 1 1 8 8 1 1 8
9 1 | 1 1 16 16 1 1 1 9
9 3 | 1 1 4 16 4 1 1 13
9 9 | 1 1 1 16 16 1 1 12
10 1 | 2 1 8 8 1 1 1 1
10 2 | 1 1 8 16 2 1 1 9
10 5 | 2 1 1 8 8 1 1 4
12 2 | 2 1 4 8 2 1 1 1
12 3 | 2 1 2 8 4 1 1 4
12 4 | 1 1 4 16 4 1 1 9
15 3 | 1 1 8 32 4 1 1 13
15 5 | 1 1 4 32 8 1 1 13
16 1 | 2 1 8 8 1 1 1 0
16 2 | 2 1 4 8 2 1 1 0
16 4 | 2 1 2 8 4 1 1 0
16 8 | 2 1 1 8 8 1 1 0
16 16 | 1 1 1 16 16 1 1 8
17 1 | 1 1 32 32 1 1 1 9
17 17 | 1 1 1 32 32 1 1 12
18 1 | 2 1 16 16 1 1 1 1
18 2 | 1 1 16 32 2 1 1 9
18 3 | 2 1 4 16 4 1 1 5
18 9 | 2 1 1 16 16 1 1 4
20 2 | 2 1 8 16 2 1 1 1
20 4 | 1 1 8 32 4 1 1 9
20 5 | 2 1 2 16 8 1 1 4
24 3 | 2 1 4 16 4 1 1 4
24 4 | 2 1 4 16 4 1 1 1
24 8 | 1 1 4 32 8 1 1 9
25 5 | 1 1 8 64 8 1 1 13
27 3 | 1 1 16 64 4 1 1 13
27 9 | 1 1 4 64 16 1 1 13
30 3 | 2 1 8 32 4 1 1 5
30 5 | 2 1 4 32 8 1 1 5
32 1 | 2 1 16 16 1 1 1 0
32 2 | 2 1 8 16 2 1 1 0
32 4 | 2 1 4 16 4 1 1 0
32 8 | 2 1 2 16 8 1 1 0
32 16 | 2 1 1 16 16 1 1 0
33 1 | 1 1 64 64 1 1 1 9
33 33 | 1 1 1 64 64 1 1 12
34 1 | 2 1 32 32 1 1 1 1
34 2 | 1 1 32 64 2 1 1 9
34 17 | 2 1 1 32 32 1 1 4
36 2 | 2 1 16 32 2 1 1 1
36 4 | 1 1 16 64 4 1 1 9
36 9 | 2 1 2 32 16 1 1 4
40 4 | 2 1 8 32 4 1 1 1
40 5 | 2 1 4 32 8 1 1 4
40 8 | 1 1 8 64 8 1 1 9
45 5 | 1 1 16 64 4 2 1 15
45 9 | 1 1 8 64 8 2 1 15
48 3 | 2 1 8 32 4 1 1 4
48 8 | 2 1 4 32 8 1 1 1
48 16 | 1 1 4 64 16 1 1 9
50 5 | 2 1 8 64 8 1 1 5
51 3 | 1 1 32 64 2 2 1 15
51 17 | 1 1 4 64 16 2 1 15
54 3 | 2 1 16 64 4 1 1 5
54 9 | 2 1 4 64 16 1 1 5
64 1 | 2 1 32 32 1 1 1 0
64 2 | 2 1 16 32 2 1 1 0
64 4 | 2 1 8 32 4 1 1 0
64 8 | 2 1 4 32 8 1 1 0
64 16 | 2 1 2 32 16 1 1 0
65 1 | 1 2 64 64 1 1 1 9
65 65 | 1 1 1 64 64 2 1 14
66 1 | 2 1 64 64 1 1 1 1
66 2 | 1 1 64 64 1 2 1 9
66 33 | 2 1 1 64 64 1 1 4
68 2 | 2 1 32 64 2 1 1 1
68 4 | 1 1 32 64 2 2 1 9
68 17 | 2 1 2 64 32 1 1 4
72 4 | 2 1 16 64 4 1 1 1
72 8 | 1 1 16 64 4 2 1 9
72 9 | 2 1 4 64 16 1 1 4
80 5 | 2 1 8 64 8 1 1 4
80 8 | 2 1 8 64 8 1 1 1
80 16 | 1 1 8 64 8 2 1 9
90 5 | 2 1 16 64 4 2 1 7
90 9 | 2 1 8 64 8 2 1 7
96 3 | 2 1 16 64 4 1 1 4
96 16 | 2 1 4 64 16 1 1 1
102 3 | 2 1 32 64 2 2 1 7
102 17 | 2 1 4 64 16 2 1 7
128 1 | 2 1 64 64 1 1 1 0
128 2 | 2 1 32 64 2 1 1 0
128 4 | 2 1 16 64 4 1 1 0
128 8 | 2 1 8 64 8 1 1 0
128 16 | 2 1 4 64 16 1 1 0
129 1 | 1 4 64 64 1 1 1 9
130 1 | 2 2 64 64 1 1 1 1
130 2 | 1 2 64 64 1 2 1 9
130 65 | 2 1 1 64 64 2 1 6
132 2 | 2 1 64 64 1 2 1 1
132 33 | 2 1 2 64 32 2 1 6
136 4 | 2 1 32 64 2 2 1 1
136 17 | 2 1 4 64 16 2 1 6
144 8 | 2 1 16 64 4 2 1 1
144 9 | 2 1 8 64 8 2 1 6
160 5 | 2 1 16 64 4 2 1 6
160 16 | 2 1 8 64 8 2 1 1
192 3 | 2 1 32 64 2 2 1 6
256 1 | 2 2 64 64 1 1 1 0
256 2 | 2 1 64 64 1 2 1 0
256 4 | 2 1 32 64 2 2 1 0
256 8 | 2 1 16 64 4 2 1 0
256 16 | 2 1 8 64 8 2 1 0
258 2 | 1 4 64 64 1 2 1 9
260 2 | 2 2 64 64 1 2 1 1
512 2 | 2 2 64 64 1 2 1 0
""") + rows("f64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
4 1 | 1 1 4 4 1 1 1 16
6 3 | 1 1 2 8 4 1 1 20
8 1 | 1 1 8 8 1 1 1 16
8 2 | 1 1 4 8 2 1 1 16
8 4 | 1 1 2 8 4 1 1 16
10 5 | 1 1 2 16 8 1 1 20
12 3 | 1 1 4 16 4 1 1 20
16 1 | 1 1 16 16 1 1 1 16
16 2 | 1 1 8 16 2 1 1 16
16 4 | 1 1 4 16 4 1 1 16
16 8 | 1 1 2 16 8 1 1 16
18 9 | 1 1 2 32 16 1 1 20
20 5 | 1 1 4 32 8 1 1 20
24 3 | 1 1 8 32 4 1 1 20
32 1 | 1 1 32 32 1 1 1 16
32 2 | 1 1 16 32 2 1 1 16
32 4 | 1 1 8 32 4 1 1 16
32 8 | 1 1 4 32 8 1 1 16
32 16 | 1 1 2 32 16 1 1 16
34 17 | 1 1 2 64 32 1 1 20
36 9 | 1 1 4 64 16 1 1 20
40 5 | 1 1 8 64 8 1 1 20
48 3 | 1 1 16 64 4 1 1 20
64 1 | 1 1 64 64 1 1 1 16
64 2 | 1 1 32 64 2 1 1 16
64 4 | 1 1 16 64 4 1 1 16
64 8 | 1 1 8 64 8 1 1 16
64 16 | 1 1 4 64 16 1 1 16
66 33 | 1 1 2 64 32 2 1 22
68 17 | 1 1 4 64 16 2 1 22
72 9 | 1 1 8 64 8 2 1 22
80 5 | 1 1 16 64 4 2 1 22
96 3 | 1 1 32 64 2 2 1 22
128 1 | 1 2 64 64 1 1 1 16
128 2 | 1 1 64 64 1 2 1 16
128 4 | 1 1 32 64 2 2 1 16
128 8 | 1 1 16 64 4 2 1 16
128 16 | 1 1 8 64 8 2 1 16
256 1 | 1 4 64 64 1 1 1 16
256 2 | 1 2 64 64 1 2 1 16
512 2 | 1 4 64 64 1 2 1 16
""") + rows("f64", "base", """
4 2 | 1 1 2 4 2 1 1 16
""") + rows("bf16", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
2 2 | 1 1 1 2 2 1 1 8
3 1 | 1 1 4 4 1 1 1 9
3 3 | 1 1 1 4 4 1 1 12
4 1 | 1 1 4 4 1 1 1 8
4 2 | 1 1 2 4 2 1 1 8
4 4 | 1 1 1 4 4 1 1 8
5 1 | 1 1 8 8 1 1 1 9
5 5 | 1 1 1 8 8 1 1 12
6 2 | 1 1 4 8 2 1 1 9
6 3 | 1 1 2 8 4 1 1 12
8 1 | 8 1 1 1 1 1 1 0
8 2 | 1 1 4 8 2 1 1 8
8 4 | 1 1 2 8 4 1 1 8
8 8 | 1 1 1 8 8 1 1 8
9 1 | 1 1 16 16 1 1 1 9
9 3 | 1 1 4 16 4 1 1 13
9 9 | 1 1 1 16 16 1 1 12
10 2 | 1 1 8 16 2 1 1 9
10 5 | 1 1 2 16 8 1 1 12
12 3 | 1 1 4 16 4 1 1 12
12 4 | 1 1 4 16 4 1 1 9
15 3 | 1 1 8 32 4 1 1 13
15 5 | 1 1 4 32 8 1 1 13
16 1 | 8 1 2 2 1 1 1 0
16 4 | 1 1 4 16 4 1 1 8
16 8 | 1 1 2 16 8 1 1 8
16 16 | 1 1 1 16 16 1 1 8
17 1 | 1 1 32 32 1 1 1 9
17 17 | 1 1 1 32 32 1 1 12
18 2 | 1 1 16 32 2 1 1 9
18 9 | 1 1 2 32 16 1 1 12
20 4 | 1 1 8 32 4 1 1 9
20 5 | 1 1 4 32 8 1 1 12
24 1 | 8 1 4 4 1 1 1 1
24 3 | 8 1 1 4 4 1 1 4
24 8 | 1 1 4 32 8 1 1 9
25 5 | 1 1 8 64 8 1 1 13
27 3 | 1 1 16 64 4 1 1 13
27 9 | 1 1 4 64 16 1 1 13
32 1 | 8 1 4 4 1 1 1 0
32 2 | 8 1 2 4 2 1 1 0
32 4 | 8 1 1 4 4 1 1 0
32 8 | 1 1 4 32 8 1 1 8
32 16 | 1 1 2 32 16 1 1 8
33 1 | 1 1 64 64 1 1 1 9
33 33 | 1 1 1 64 64 1 1 12
34 2 | 1 1 32 64 2 1 1 9
34 17 | 1 1 2 64 32 1 1 12
36 4 | 1 1 16 64 4 1 1 9
36 9 | 1 1 4 64 16 1 1 12
40 1 | 8 1 8 8 1 1 1 1
40 5 | 8 1 1 8 8 1 1 4
40 8 | 1 1 8 64 8 1 1 9
45 5 | 1 1 16 64 4 2 1 15
45 9 | 1 1 8 64 8 2 1 15
48 2 | 8 1 4 8 2 1 1 1
48 3 | 8 1 2 8 4 1 1 4
48 16 | 1 1 4 64 16 1 1 9
51 3 | 1 1 32 64 2 2 1 15
51 17 | 1 1 4 64 16 2 1 15
64 1 | 8 1 8 8 1 1 1 0
64 2 | 8 1 4 8 2 1 1 0
64 4 | 8 1 2 8 4 1 1 0
64 8 | 8 1 1 8 8 1 1 0
64 16 | 1 1 4 64 16 1 1 8
65 1 | 1 2 64 64 1 1 1 9
65 65 | 1 1 1 64 64 2 1 14
66 2 | 1 1 64 64 1 2 1 9
66 33 | 1 1 2 64 32 2 1 14
68 4 | 1 1 32 64 2 2 1 9
68 17 | 1 1 4 64 16 2 1 14
72 1 | 8 1 16 16 1 1 1 1
72 3 | 8 1 4 16 4 1 1 5
72 8 | 1 1 16 64 4 2 1 9
72 9 | 8 1 1 16 16 1 1 4
80 2 | 8 1 8 16 2 1 1 1
80 5 | 8 1 2 16 8 1 1 4
80 16 | 1 1 8 64 8 2 1 9
96 3 | 8 1 4 16 4 1 1 4
96 4 | 8 1 4 16 4 1 1 1
120 3 | 8 1 8 32 4 1 1 5
120 5 | 8 1 4 32 8 1 1 5
128 1 | 8 1 16 16 1 1 1 0
128 2 | 8 1 8 16 2 1 1 0
128 4 | 8 1 4 16 4 1 1 0
128 8 | 8 1 2 16 8 1 1 0
128 16 | 8 1 1 16 16 1 1 0
129 1 | 1 4 64 64 1 1 1 9
130 2 | 1 2 64 64 1 2 1 9
136 1 | 8 1 32 32 1 1 1 1
136 17 | 8 1 1 32 32 1 1 4
144 2 | 8 1 16 32 2 1 1 1
144 9 | 8 1 2 32 16 1 1 4
160 4 | 8 1 8 32 4 1 1 1
160 5 | 8 1 4 32 8 1 1 4
192 3 | 8 1 8 32 4 1 1 4
192 8 | 8 1 4 32 8 1 1 1
200 5 | 8 1 8 64 8 1 1 5
216 3 | 8 1 16 64 4 1 1 5
216 9 | 8 1 4 64 16 1 1 5
256 1 | 8 1 32 32 1 1 1 0
256 2 | 8 1 16 32 2 1 1 0
256 4 | 8 1 8 32 4 1 1 0
256 8 | 8 1 4 32 8 1 1 0
256 16 | 8 1 2 32 16 1 1 0
258 2 | 1 4 64 64 1 2 1 9
264 33 | 8 1 1 64 64 1 1 4
272 2 | 8 1 32 64 2 1 1 1
272 17 | 8 1 2 64 32 1 1 4
288 4 | 8 1 16 64 4 1 1 1
288 9 | 8 1 4 64 16 1 1 4
320 5 | 8 1 8 64 8 1 1 4
320 8 | 8 1 8 64 8 1 1 1
360 5 | 8 1 16 64 4 2 1 7
360 9 | 8 1 8 64 8 2 1 7
384 3 | 8 1 16 64 4 1 1 4
384 16 | 8 1 4 64 16 1 1 1
408 3 | 8 1 32 64 2 2 1 7
408 17 | 8 1 4 64 16 2 1 7
512 2 | 8 1 32 64 2 1 1 0
512 4 | 8 1 16 64 4 1 1 0
512 8 | 8 1 8 64 8 1 1 0
512 16 | 8 1 4 64 16 1 1 0
520 65 | 8 1 1 64 64 2 1 6
528 33 | 8 1 2 64 32 2 1 6
544 4 | 8 1 32 64 2 2 1 1
544 17 | 8 1 4 64 16 2 1 6
576 8 | 8 1 16 64 4 2 1 1
576 9 | 8 1 8 64 8 2 1 6
640 5 | 8 1 16 64 4 2 1 6
640 16 | 8 1 8 64 8 2 1 1
768 3 | 8 1 32 64 2 2 1 6
1024 4 | 8 1 32 64 2 2 1 0
1024 8 | 8 1 16 64 4 2 1 0
1024 16 | 8 1 8 64 8 2 1 0
""") + rows("bf16", "stride", """
8 1 | 1 1 8 8 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
32 2 | 1 1 16 32 2 1 1 16
32 4 | 1 1 8 32 4 1 1 16
40 5 | 1 1 8 64 8 1 1 20
48 3 | 1 1 16 64 4 1 1 20
64 1 | 1 1 64 64 1 1 1 16
64 2 | 1 1 32 64 2 1 1 16
64 4 | 1 1 16 64 4 1 1 16
64 8 | 1 1 8 64 8 1 1 16
72 9 | 1 1 8 64 8 2 1 22
80 5 | 1 1 16 64 4 2 1 22
96 3 | 1 1 32 64 2 2 1 22
128 1 | 1 2 64 64 1 1 1 16
128 2 | 1 1 64 64 1 2 1 16
128 4 | 1 1 32 64 2 2 1 16
128 8 | 1 1 16 64 4 2 1 16
128 16 | 1 1 8 64 8 2 1 16
256 1 | 1 4 64 64 1 1 1 16
256 2 | 1 2 64 64 1 2 1 16
512 2 | 1 4 64 64 1 2 1 16
""") + rows("bf16", "base", """
16 2 | 1 1 8 16 2 1 1 16
""") + rows("f16", None, """
16 2 | 8 1 1 2 2 1 1 0
""") + rows("f16", "stride", """
16 1 | 1 1 16 16 1 1 1 16
""") + rows("f16", "base", """
24 3 | 1 1 8 32 4 1 1 20
""")

TABLES["sddmm"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
4 1 | 4 1 1 1 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
8 1 | 4 1 2 2 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
12 1 | 4 1 4 4 1 1 1 1
16 1 | 4 1 4 4 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
20 1 | 4 1 8 8 1 1 1 1
32 1 | 4 1 8 8 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
36 1 | 4 1 16 16 1 1 1 1
64 1 | 4 1 16 16 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
68 1 | 4 1 32 32 1 1 1 1
128 1 | 4 1 32 32 1 1 1 0
129 1 | 1 3 64 64 1 1 1 9
132 1 | 4 1 64 64 1 1 1 1
193 1 | 1 4 64 64 1 1 1 9
256 1 | 4 1 64 64 1 1 1 0
257 1 | 1 4 64 64 1 2 1 11
260 1 | 4 2 64 64 1 1 1 1
449 1 | 1 4 64 64 1 2 1 9
512 1 | 4 2 64 64 1 1 1 0
516 1 | 4 3 64 64 1 1 1 1
768 1 | 4 3 64 64 1 1 1 0
772 1 | 4 4 64 64 1 1 1 1
1024 1 | 4 4 64 64 1 1 1 0
1028 1 | 4 4 64 64 1 2 1 3
""") + rows("f32", "stride", """
4 1 | 1 1 4 4 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 3 64 64 1 1 1 16
256 1 | 1 4 64 64 1 1 1 16
320 1 | 1 4 64 64 1 2 1 18
512 1 | 1 4 64 64 1 2 1 16
""") + rows("f32", "base", """
8 1 | 1 1 8 8 1 1 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 2 1 1 1 1 1 1 0
3 1 | 1 1 4 4 1 1 1 9
4 1 | 2 1 2 2 1 1 1 0
5 1 | 1 1 8 8 1 1 1 9
6 1 | 2 1 4 4 1 1 1 1
8 1 | 2 1 4 4 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
10 1 | 2 1 8 8 1 1 1 1
16 1 | 2 1 8 8 1 1 1 0
17 1 | 1 1 32 32 1 1 1 9
18 1 | 2 1 16 16 1 1 1 1
32 1 | 2 1 16 16 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
34 1 | 2 1 32 32 1 1 1 1
64 1 | 2 1 32 32 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
66 1 | 2 1 64 64 1 1 1 1
128 1 | 2 1 64 64 1 1 1 0
129 1 | 1 3 64 64 1 1 1 9
130 1 | 2 2 64 64 1 1 1 1
193 1 | 1 4 64 64 1 1 1 9
256 1 | 2 2 64 64 1 1 1 0
257 1 | 1 4 64 64 1 2 1 11
258 1 | 2 3 64 64 1 1 1 1
384 1 | 2 3 64 64 1 1 1 0
386 1 | 2 4 64 64 1 1 1 1
449 1 | 1 4 64 64 1 2 1 9
512 1 | 2 4 64 64 1 1 1 0
514 1 | 2 4 64 64 1 2 1 3
640 1 | 2 4 64 64 1 2 1 2
898 1 | 2 4 64 64 1 2 1 1
1024 1 | 2 4 64 64 1 2 1 0
""") + rows("f64", "stride", """
2 1 | 1 1 2 2 1 1 1 16
8 1 | 1 1 8 8 1 1 1 16
16 1 | 1 1 16 16 1 1 1 16
32 1 | 1 1 32 32 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 3 64 64 1 1 1 16
256 1 | 1 4 64 64 1 1 1 16
320 1 | 1 4 64 64 1 2 1 18
512 1 | 1 4 64 64 1 2 1 16
""") + rows("f64", "base", """
4 1 | 1 1 4 4 1 1 1 16
""") + rows("bf16", None, """
1 1 | 1 1 1 1 1 1 1 8
2 1 | 1 1 2 2 1 1 1 8
3 1 | 1 1 4 4 1 1 1 9
4 1 | 1 1 4 4 1 1 1 8
5 1 | 1 1 8 8 1 1 1 9
8 1 | 8 1 1 1 1 1 1 0
9 1 | 1 1 16 16 1 1 1 9
24 1 | 8 1 4 4 1 1 1 1
32 1 | 8 1 4 4 1 1 1 0
33 1 | 1 1 64 64 1 1 1 9
40 1 | 8 1 8 8 1 1 1 1
64 1 | 8 1 8 8 1 1 1 0
65 1 | 1 2 64 64 1 1 1 9
72 1 | 8 1 16 16 1 1 1 1
128 1 | 8 1 16 16 1 1 1 0
129 1 | 1 3 64 64 1 1 1 9
136 1 | 8 1 32 32 1 1 1 1
193 1 | 1 4 64 64 1 1 1 9
256 1 | 8 1 32 32 1 1 1 0
257 1 | 1 4 64 64 1 2 1 11
264 1 | 8 1 64 64 1 1 1 1
449 1 | 1 4 64 64 1 2 1 9
512 1 | 8 1 64 64 1 1 1 0
520 1 | 8 2 64 64 1 1 1 1
1024 1 | 8 2 64 64 1 1 1 0
1032 1 | 8 3 64 64 1 1 1 1
""") + rows("bf16", "stride", """
8 1 | 1 1 8 8 1 1 1 16
64 1 | 1 1 64 64 1 1 1 16
128 1 | 1 2 64 64 1 1 1 16
192 1 | 1 3 64 64 1 1 1 16
256 1 | 1 4 64 64 1 1 1 16
320 1 | 1 4 64 64 1 2 1 18
512 1 | 1 4 64 64 1 2 1 16
""") + rows("bf16", "base", """
16 1 | 1 1 16 16 1 1 1 16
""") + rows("f16", None, """
16 1 | 8 1 2 2 1 1 1 0
""") + rows("f16", "stride", """
24 1 | 1 1 32 32 1 1 1 17
""") + rows("f16", "base", """
32 1 | 1 1 32 32 1 1 1 16
""")

TABLES["edge_softmax"] = rows("f32", None, """
1 1 | 1 1 1 1 1 1 1 8
2 2 | 1 1 1 1 1 2 1 8
4 4 | 4 1 1 1 1 1 1 0
8 8 | 4 1 1 1 1 2 1 0
""") + rows("f32", "base", """
4 4 | 1 1 1 1 1 4 1 16
""") + rows("f64", None, """
1 1 | 1 1 1 1 1 1 1 8
2 2 | 2 1 1 1 1 1 1 0
3 3 | 1 1 1 1 1 3 1 8
4 4 | 2 1 1 1 1 2 1 0
""") + rows("f64", "base", """
2 2 | 1 1 1 1 1 2 1 16
""")
