"""NaN, +-inf, -0.0 and subnormal features and values through every form of the group product (pygim_spmm_run_group, pygim_block_run,
pygim_grande_run_group, pygim_spmv_run_group) against the CPU loop, through the C ABI.

tests/group_nonfinite.py holds the graph, the operands, the rule (compare: NaN exactly where the CPU loop has NaN, every other element its
bits, no -0.0) and the table of forms; tests/test_group_nonfinite_cpu.py proves that fixture without a device.  Here every case sets its
knobs, creates the group, asks the group's own queries whether the product runs in the form the case is there for (a case whose query names
another form FAILS), multiplies into an output filled with 77, compares, frees the group and puts every knob back.

What a wrong kernel looks like here: a masked lane or a padding token that is added (column 0 is all NaN: a NaN in a row that does not hold
column 0), a sum that lands in the neighbouring row, feature, slice, panel or chunk (the infinities at their edges), an explicit zero that is
dropped (0 x inf must be NaN), an accumulator seeded with its first term (a row of -0.0 features would return -0.0).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from group_nonfinite import CASES, NP_DTYPES, coalesced, column_blocks, compare, expected, graph, operands, overwrite_rows, params
from pygim_amd import _lib

pytestmark = pytest.mark.gpu
CODE_OF = {np.float32: _lib.FLT32, np.float64: _lib.DBL64}
PARAMS, IDS = params()
ALL_KNOBS = sorted({k for c in CASES for k in list(c.knobs) + list(c.create_knobs)})


def knob_values():
    out = {}
    for k in ALL_KNOBS:
        out[k] = _lib.set_tunable(k, 0)
        _lib.set_tunable(k, out[k])
    return out


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    before = knob_values()
    yield
    after = knob_values()
    _lib.release()
    assert after == before, f"a case leaked a knob: {[(k, before[k], after[k]) for k in before if before[k] != after[k]]}"


@contextlib.contextmanager
def knobs(values):
    """the knobs are process-wide: every one a case sets goes back to the value set_tunable returned, whatever happens in between"""
    old = []
    try:
        for k, v in values.items():
            prev = _lib.set_tunable(k, v)
            assert prev != -1, f"unknown tunable {k}"
            old.append((k, prev))
        yield
    finally:
        for k, prev in reversed(old):
            _lib.set_tunable(k, prev)


def _ptr(a):
    return a.ctypes.data


def queries(hd):
    return {"info": _lib.group_info(hd), "plan": _lib.group_plan(hd), "lds_plan": _lib.group_lds_plan(hd), "lds_code": _lib.group_lds_code(hd),
            "lds_geometry": _lib.group_lds_geometry(hd), "lds_note": _lib.group_lds_note(hd)}


def prove(c, q):
    """the product ran in the form the case is there for, by the group's own account"""
    for query, field, op, value in c.proof:
        got = q[query] if field is None else q[query][field]
        ok = {"==": lambda: got == value, ">=": lambda: got >= value, "has": lambda: value in got, "lacks": lambda: value not in got}[op]()
        assert ok, f"{c.form}: not the form the case is for -- {query}{'' if field is None else '.' + field} is {got!r}, wanted {op} {value!r}; the group says {q}"


@functools.lru_cache(maxsize=None)
def hybrid_graph():
    """the community graph of tests/test_hybrid_gpu.py (its float case) with the fixed rows written in"""
    from test_hybrid_gpu import _graph

    rowptr, col = _graph(torch.device("cuda", 0), seed=13)
    n = rowptr.numel() - 1
    rp, ci = overwrite_rows(rowptr.cpu().numpy(), col.cpu().numpy(), n)
    return rp, ci, n


def transpose(rowptr, col, vals, nrows, ncols):
    from test_autograd_gpu import np_transpose

    return np_transpose([(rowptr, col, vals, ncols)], nrows)


class Setup:
    """what a case multiplies: the structure the CPU loop walks (rowptr, col), how the group is created from it, and the operands"""

    def __init__(self, c, npdt, weights, h, seed):
        self.c, self.npdt, self.h = c, npdt, h
        self.exp_fmt, self.fmt, counts = "CSR", _lib.CSR, None
        if c.fmt == "COO":
            row, self.col, counts, self.rowptr, self.ncols = coalesced(c.graph)
            self.idx0, self.exp_fmt, self.fmt = np.ascontiguousarray(row, np.int32), "COO", _lib.COO
        else:
            self.rowptr, self.col, self.ncols = hybrid_graph() if c.graph == "hybrid" else graph(c.graph)
            self.idx0 = self.rowptr
        self.nrows = len(self.rowptr) - 1
        small = 2.0 ** -149 if c.entry == "narrow" else None      # (a float32 subnormal: it survives the round trip through 4 bytes)
        self.make = lambda edge=(): operands(seed, self.rowptr, self.ncols, h, npdt, weights, nnz=len(self.col), edge_cols=edge, counts=counts, small_subnormal=small)
        self.ops0 = self.make()
        self.widths = [len(w) for w in np.array_split(np.arange(h), 3)] if c.entry in ("windows", "grande") else [h]
        self.parts = column_blocks(self.rowptr, self.col, self.ops0.vals, [0, 170, 171, self.ncols]) if c.entry == "parts" else None
        if c.entry == "transposed":   # the fixture graph is A^T: the group is created from A, the CPU loop walks the host transpose of A
            clean = np.arange(len(self.col), dtype=np.float64) if self.ops0.vals is None else self.ops0.vals_clean
            self.a = transpose(self.rowptr, self.col, self.ops0.vals, self.nrows, self.ncols)
            a_clean = transpose(self.rowptr, self.col, clean, self.nrows, self.ncols)
            t = transpose(self.a[0], self.a[1], self.a[2], self.ncols, self.nrows)
            t_clean = transpose(a_clean[0], a_clean[1], a_clean[2], self.ncols, self.nrows)
            assert np.array_equal(t[0], self.rowptr) and np.array_equal(t[1], self.col)
            self.t_vals, self.t_clean = t[2], (None if self.ops0.vals is None else t_clean[2])

    def create(self):
        c, h = self.c, self.h
        v = self.ops0.vals
        if c.entry == "parts":
            ps = self.parts
            return _lib.group_create(_lib.CSR, CODE_OF[self.npdt], [_ptr(p[0]) for p in ps], [_ptr(p[1]) for p in ps], None if v is None else [_ptr(p[2]) for p in ps],
                                     [self.nrows] * 3, [p[3] for p in ps], [len(p[1]) for p in ps], [1] * 3, [h] * 3, h)
        if c.entry == "transposed":
            rp, ci, av = self.a
            self.keep = [np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), None if av is None else np.ascontiguousarray(av, self.npdt)]
            return _lib.group_create_transposed(_lib.CSR, CODE_OF[self.npdt], [_ptr(self.keep[0])], [_ptr(self.keep[1])], None if av is None else [_ptr(self.keep[2])],
                                                [self.ncols], [self.nrows], [len(ci)], [1], [h], h)
        n_dense, dense_cols = ([h], [1] * h) if c.entry == "spmv" else ([len(self.widths)], self.widths)
        return _lib.group_create(self.fmt, CODE_OF[self.npdt], [_ptr(self.idx0)], [_ptr(self.col)], None if v is None else [_ptr(v)], [self.nrows], [self.ncols],
                                 [len(self.col)], n_dense, dense_cols, h)

    def want(self, ops):
        if self.c.entry == "transposed":
            entries = [] if ops.vals is None else np.nonzero(self.t_vals.view(np.uint8).reshape(len(self.col), -1) != self.t_clean.view(np.uint8).reshape(len(self.col), -1))[0]
            ops = ops._replace(vals=self.t_vals, vals_clean=self.t_clean, entries=[int(e) for e in np.unique(entries)])
        return expected(self.rowptr, self.col, ops, fmt="GROUP" if self.parts else self.exp_fmt, parts=self.parts)[0]


def out_of(n, h, npdt):
    return np.full((n, h), 77, dtype=npdt)


def run_spmm(hd, s, ops):
    out = out_of(s.nrows, s.h, s.npdt)
    _lib.spmm_run_group(hd, [_ptr(ops.x)], _ptr(out))
    return out


def run_pinned(hd, s, ops):
    out = torch.full((s.nrows, s.h), 77, dtype=torch.from_numpy(ops.x).dtype, pin_memory=True)
    _lib.spmm_run_group(hd, [_ptr(ops.x)], out.data_ptr())
    return out.numpy().copy()


def run_device(hd, s, ops):
    """device operands; X inside a larger allocation, so that a one-slice product may read the caller's matrix in place"""
    x = torch.from_numpy(ops.x)
    big = torch.zeros((s.ncols + 4096) * s.h, dtype=x.dtype, device="cuda")
    xv = big[:s.ncols * s.h].view(s.ncols, s.h)
    xv.copy_(x)
    out = torch.full((s.nrows, s.h), 77, dtype=x.dtype, device="cuda")
    _lib.spmm_run_group(hd, [xv.data_ptr()], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_spmv(hd, s, ops):
    vecs = [np.ascontiguousarray(ops.x[:, j]) for j in range(s.h)]
    out = out_of(s.nrows, s.h, s.npdt)
    _lib.spmv_run_group(hd, [_ptr(v) for v in vecs], _ptr(out))
    return out


def run_windows(hd, s, ops):
    chunks = [np.ascontiguousarray(a) for a in np.array_split(ops.x, 3, axis=1)]
    out = out_of(s.nrows, s.h, s.npdt)
    _lib.spmm_run_group(hd, [_ptr(a) for a in chunks], _ptr(out))
    return out


def run_grande(hd, s, ops):
    """per-unit windows with strides padded to 8 bytes (backend_pim/grande.py); the padding holds NaN"""
    per8 = 8 // ops.x.itemsize
    wins, lds, a = [], [], 0
    for w in s.widths:
        ld = -(-w // per8) * per8
        buf = np.full((s.ncols, ld), np.nan, dtype=s.npdt)
        buf[:, :w] = ops.x[:, a:a + w]
        wins.append(buf)
        lds.append(ld)
        a += w
    out = out_of(s.nrows, s.h, s.npdt)
    _lib.grande_run_group(hd, [_ptr(b) for b in wins], lds, _ptr(out))
    return out


def poisoned_c(nrows, h, npdt):
    """what C holds before the two adding block runs: 7 everywhere but a NaN in an empty row and in an ordinary one, -0.0 over row 3, infinities in rows 7 and 21.
    (-0.0 only where the row adds a term that is not -0.0: `C += A.X` read as a loop that continues from C and as a finished sum added to C then agree)"""
    c0 = np.full((nrows, h), 7, dtype=npdt)
    c0[4, 1] = c0[20, 5] = np.nan
    c0[3, :] = -0.0
    c0[7, h - 1] = c0[21, 0] = np.inf
    c0[7, 0] = -np.inf
    return c0


def run_block2(hd, s, ops):
    """pygim_block_run twice with accumulate on device operands inside larger buffers: base pointers one element off, row strides h + 3 and h + 1, NaN in X's padding"""
    h, ldx, ldc = s.h, s.h + 3, s.h + 1
    tdt, es = torch.from_numpy(ops.x).dtype, ops.x.itemsize
    xb = torch.full((s.ncols * ldx + 1,), float("nan"), dtype=tdt, device="cuda")
    xb[1:].view(s.ncols, ldx)[:, :h] = torch.from_numpy(ops.x).cuda()
    c0 = poisoned_c(s.nrows, h, s.npdt)
    cb = torch.full((s.nrows * ldc + 1,), 7, dtype=tdt, device="cuda")
    cb[1:].view(s.nrows, ldc)[:, :h] = torch.from_numpy(c0).cuda()
    st = torch.cuda.current_stream().cuda_stream
    _lib.block_run(hd, 0, xb.data_ptr() + es, ldx, cb.data_ptr() + es, ldc, h, True, st)
    _lib.block_run(hd, 0, xb.data_ptr() + es, ldx, cb.data_ptr() + es, ldc, h, True, st)
    torch.cuda.synchronize()
    got = cb[1:].view(s.nrows, ldc).cpu().numpy()
    assert (got[:, h:] == 7).all() and float(cb[0]) == 7, "wrote outside the window"
    return np.ascontiguousarray(got[:, :h])


RUNNERS = {"spmm": run_spmm, "narrow": run_spmm, "parts": run_spmm, "transposed": run_spmm, "pinned": run_pinned, "device": run_device, "spmv": run_spmv,
           "windows": run_windows, "grande": run_grande, "block2": run_block2}


def run_case(c, dt, weights, h):
    npdt = NP_DTYPES[dt]
    s = Setup(c, npdt, weights, h, seed=1000 + h)
    with knobs(c.knobs):
        with knobs(c.create_knobs):
            hd = s.create()
        try:
            q = queries(hd)
            edge = ()
            if c.edge:      # the last column of one panel / chunk and the first of the next
                w = q[c.edge[0]][c.edge[1]]
                if c.edge[1] == "chunk_cols" and w == 0 and q["lds_plan"]["tiles"] > 0:
                    w = 320     # (a token plan that names no chunk width stages 320 columns, lds_launch.hpp lds_rows_pad)
                assert 1 < w < s.ncols, f"{c.form}: {c.edge} is {w}; the group says {q}"
                edge = (w - 1, w)
            ops = s.make(edge)
            want = s.want(ops)
            if c.entry == "block2":
                with np.errstate(invalid="ignore"):
                    c0 = poisoned_c(s.nrows, h, npdt)
                    want = (c0 + want) + want
            got = RUNNERS[c.entry](hd, s, ops)
            q["lds_runs"], q["host_windows"] = _lib.group_lds_runs(hd), _lib.group_host_windows(hd)
            prove(c, q)
            compare(got, want, f"{c.form}, {dt}, {weights}, h = {h}")
        finally:
            _lib.group_free(hd)


@pytest.mark.parametrize("c,dt,weights", PARAMS, ids=IDS)
def test_nonfinite_operands_follow_the_cpu_loop(c, dt, weights):
    for h in c.hs:
        run_case(c, dt, weights, h)
