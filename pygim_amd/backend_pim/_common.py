"""Shared machinery of the three ``backend_pim`` wrappers.

Mirrors what backend_pim/spmm.py, grande.py and spmv.py of the reference each
re-implement: holding the raw SparseTensor, cutting it into ``sp_parts`` column
blocks (spmm.py:127-136), materialising per-part int32 CSR / coalesced COO arrays
(spmm.py:31-55) and calling ``torch.ops.pim_ops``.
"""
from __future__ import annotations

import torch

TORCH_TYPES = {"INT64": torch.int64, "INT32": torch.int32, "INT16": torch.int16, "INT8": torch.int8,
               "FLT32": torch.float32, "DBL64": torch.float64}


class CSRPart:
    """int32 CSR arrays of one column block (what the reference reads back from a
    torch.sparse_csr_tensor: crow_indices / col_indices / values)."""

    def __init__(self, crow, col, values, shape):
        self._crow, self._col, self._values, self._shape = crow, col, values, tuple(shape)

    def crow_indices(self):
        return self._crow

    def col_indices(self):
        return self._col

    def values(self):
        return self._values

    def size(self, dim):
        return self._shape[dim]


def part_values(item, dtype):
    """Edge values of a part in the compute dtype; all ones when the adjacency has none
    (spmm.py:36-39, 48-51)."""
    value = item.storage.value()
    if value is None:
        return torch.ones(item.nnz(), dtype=dtype, device=item.device())
    return value.type(dtype)


def split_widths(total, nparts):
    """ceil-sized blocks with the remainder in the last one (spmm.py:62-72, 129-133)."""
    width = (total + nparts - 1) // nparts
    sizes = [width] * nparts
    if nparts * width != total:
        sizes[-1] = total - (nparts - 1) * width
    return sizes


class SparseGroupBase:
    def __init__(self, coo, dtype=torch.int32, format=""):
        self.raw = coo
        self.dtype = dtype
        self.format = format
        self._handle = None  # (handle, generation) of the device group this object owns
        self._handle_t = None  # (handle, serial, h) of the group of A^T (mul_t), made on the first backward
        self.sp_info_ptr = None
        self.result = None
        self.parts = [self.raw]
        self.csr, self.coo = [], []
        self.dense_parts = 0
        self.hidden_size = 0
        self.nparts = 1

    # -- the device group's lifetime ----------------------------------------------
    # The reference leaves spmm_free_group (spmm_default/pytorch_api.cpp:198-201) to the caller and its wrappers never call
    # it: a DPU group is a few arrays.  Here a group owns its CSR, its plans and -- for the LDS-staged product -- up to a GB of
    # executable code, so the wrapper frees what it created: when the handle is replaced (to_pim_group again) and when the
    # object dies.  A handle is an address: after dpu_release (every group freed) or a spmm_free_group by the caller it may
    # belong to a later group, so the wrapper remembers the group's creation serial (pygim_group_serial, never reused) and
    # frees only while the handle still names THAT group.
    @property
    def sp_info_ptr(self):
        return self._handle[0] if self._handle is not None else None

    @sp_info_ptr.setter
    def sp_info_ptr(self, handle):
        self.free_group()
        if handle is not None:
            from .. import _lib

            try:
                self._handle = (int(handle), _lib.group_serial(handle))
            except _lib.PygimError:   # not a group of this library (another pim_ops backend registered under the same names): not ours to free
                self._handle = (int(handle), None)

    def free_group(self):
        """spmm_free_group on the group this object created, if it is still alive (and on its A^T group, see mul_t)."""
        from .. import _lib

        self._free_transposed()
        held, self._handle = getattr(self, "_handle", None), None
        if held is None or held[1] is None or not _lib.is_initialized():
            return
        try:
            alive = _lib.group_serial(held[0]) == held[1]
        except _lib.PygimError:  # freed by the caller or by dpu_release
            alive = False
        if alive:
            torch.ops.pim_ops.spmm_free_group(held[0])

    def __del__(self):
        try:
            self.free_group()
        except Exception:  # interpreter shutdown: torch.ops or the library may be gone already
            pass

    # -- the backward product: A^T . G (pygim_amd/autograd.py) ------------------------------------------
    # A second device group, of A^T, built from the same per-part arrays the wrapper handed to *_to_device_group (self.csr /
    # self.coo) and transposed on the device (pygim_group_create_transposed).  It is a compiled group like the forward's: on a
    # Reddit-like graph about 1 GB of code plus the transient memory of creation (README: about 1.0 GB and 5 GB for the forward
    # group), paid on the first backward -- or up front with prepare_backward() -- and never by a model that only runs forward.
    # Owned like the forward group: freed by free_group, by to_pim_group* and when the object dies, guarded by its serial.
    def _free_transposed(self):
        from .. import pim_ops

        held, self._handle_t = getattr(self, "_handle_t", None), None
        if held is None:
            return
        L = pim_ops._lib
        if not L.is_initialized():
            return
        try:
            alive = L.group_serial(held[0]) == held[1]
        except L.PygimError:  # freed by dpu_release
            alive = False
        if alive:
            L.group_free(held[0])

    def _group_arrays(self):
        """(format code, idx0, col, values, nrows, ncols) per part: what to_pim_group* passed to the library"""
        from .. import _lib

        if self.format == "CSR":
            return (_lib.CSR, [p.crow_indices() for p in self.csr], [p.col_indices() for p in self.csr],
                    [p.values() for p in self.csr], [p.size(0) for p in self.csr], [p.size(1) for p in self.csr])
        if self.format == "COO":
            return (_lib.COO, self.row_indices, self.col_indices, self.values, [c.size(0) for c in self.coo],
                    [c.size(1) for c in self.coo])
        raise RuntimeError("mul_t: no device group (call to_pim_group first)")

    def _transposed(self, h):
        """handle of the A^T group for h features (made here on first use)"""
        from .. import pim_ops

        L = pim_ops._lib
        held = self._handle_t
        if held is not None:
            try:
                if held[2] == h and L.group_serial(held[0]) == held[1]:
                    return held[0]
            except L.PygimError:  # freed by dpu_release: build again
                self._handle_t = None
        self._free_transposed()
        fmt, idx0, cols, vals, nrows, ncols = self._group_arrays()
        n = len(cols)
        handle = L.group_create_transposed(fmt, pim_ops.DTYPE_CODE[self.dtype], [t.data_ptr() for t in idx0], [t.data_ptr() for t in cols],
                                           [v.contiguous().data_ptr() for v in vals], nrows, ncols, [v.numel() for v in vals], [1] * n,
                                           [int(h)] * n, int(h))
        self._handle_t = (handle, L.group_serial(handle), int(h))
        return handle

    def prepare_backward(self, h=None):
        """build the A^T group now instead of on the first backward (h: feature width of the gradients, default hidden_size)"""
        self._transposed(int(h if h is not None else self.hidden_size))

    def mul_t(self, G: torch.Tensor):
        """A^T . G for every dtype: G [rows of A, h] (CPU or device tensor, the group's dtype), result [columns of A, h] on G's
        device, like mul.  The gradient of ``mul`` with respect to its dense operand."""
        from .. import pim_ops

        assert G.dim() == 2 and G.dtype == self.dtype, "mul_t: G must be [rows, h] in the group's dtype"
        fmt, idx0, cols, vals, nrows, ncols = self._group_arrays()
        rows, total_cols = int(nrows[0]), int(sum(ncols))
        if G.size(0) < rows:  # (spmv pads the matrix: padded rows have no gradient)
            G = torch.nn.functional.pad(G, (0, 0, 0, rows - G.size(0)))
        assert G.size(0) == rows, "mul_t: G has more rows than A"
        G = G.contiguous()
        h = G.size(1)
        handle = self._transposed(h)
        out = pim_ops._new_out((total_cols, h), self.dtype, G.device)
        pim_ops._lib.spmm_run_group(handle, [G.data_ptr()], out.data_ptr(), pim_ops._stream_of(out))
        return out[:self.raw.size(1)] if total_cols != self.raw.size(1) else out

    # -- the product with values given per call (pygim_amd/attention.py) -----------------------------------
    def mul_values(self, value: torch.Tensor, B: torch.Tensor, heads: int = 1):
        """``out[r] = sum_e value[e, head] * B[col[e]]`` on the raw tensor's structure, in its CSR entry order: value [nnz] or
        [nnz, heads], float32 / float64 like B (B may also be bfloat16 / float16, value then float32 or B's dtype: float32 sums, one rounding
        of the result).  ``mul`` multiplies by the values the group was created with; this is the product for
        values that change between calls (no group is created or used).  Differentiable in value and B."""
        from ..attention import EdgeGraph, spmm_values

        return spmm_values(EdgeGraph.of(self), value, B, heads)

    # -- mean / max / min over a row's stored entries (pygim_amd/reduce.py) --------------------------------------
    def mul_reduce(self, B: torch.Tensor, reduce: str):
        """``torch_sparse.matmul(self.raw, B, reduce)`` for ``"mean"``, ``"max"`` or ``"min"`` on the raw tensor's structure, weighted
        by its stored values (cast to B's dtype) when it has them and by ones otherwise.  A reduction other than the sum cannot be
        compiled into a group: none is created or used.  Differentiable in B (float32 / float64; ``"mean"`` also takes bfloat16 / float16 B)."""
        from ..reduce import matmul_reduce

        return matmul_reduce(self, B, reduce)

    def mul_multi_reduce(self, B: torch.Tensor, reduces=("mean", "min", "max", "std"), eps: float = 1e-5):
        """several statistics of every row's neighbourhood (``"sum"``, ``"mean"``, ``"min"``, ``"max"``, ``"var"``, ``"std"``) of B on
        the raw tensor's structure with unit weights, concatenated as ``[rows, len(reduces) * h]`` from one gather
        (``pygim_amd.reduce.spmm_multi_reduce``).  No group is created or used.  Differentiable in B (float32 / float64 / bfloat16 / float16)."""
        from ..reduce import matmul_multi_reduce

        return matmul_multi_reduce(self, B, reduces, eps)

    def mul_softmax(self, B: torch.Tensor, t=1.0):
        """softmax aggregation of B per row and feature on the raw tensor's structure with unit weights,
        ``out[r, f] = sum_e softmax_e(t[f] * B[col[e], f]) * B[col[e], f]`` (``pygim_amd.reduce.spmm_softmax``: PyG's ``aggr="softmax"``),
        from one gather.  t: a float, a 0-d tensor or ``[h]``.  No group is created or used.  Differentiable in B and t
        (float32 / float64 / bfloat16 / float16)."""
        from ..reduce import matmul_softmax

        return matmul_softmax(self, B, t)

    def mul_edge(self, B: torch.Tensor, E: torch.Tensor, reduce="sum", act=None, eps=0.0, t=1.0):
        """aggregation of messages with a feature-wide edge feature on the raw tensor's structure with unit weights,
        ``out[r, f] = REDUCE_e (act(B[col[e], f] + E[e, f]) + eps)`` (``pygim_amd.reduce.spmm_edge``: GINEConv, GENConv with ``edge_dim``),
        from one gather; E [nnz, h] in the stored (row-major CSR) order of the entries.  reduce: sum, mean, max, min or softmax (with the
        temperature t).  No group is created or used.  Differentiable in B, E and t."""
        from ..reduce import matmul_edge

        return matmul_edge(self, B, E, reduce, act, eps, t)

    # -- partitioning -----------------------------------------------------------
    def col_split(self, nparts=4):
        assert nparts > 0
        if nparts != len(self.parts):
            assert len(self.parts) == 1
            step = (self.raw.size(1) + nparts - 1) // nparts
            cuts = [(i * step, (i + 1) * step) for i in range(nparts - 1)] + [((nparts - 1) * step, None)]
            self.parts = [self.raw[:, a:b] if b is not None else self.raw[:, a:] for a, b in cuts]
            self.csr, self.coo = [], []
        return self.parts

    def row_split(self, nparts=4):
        # not implemented in the reference either (spmm.py:124-125); the multi-GPU row split
        # lives in pygim_amd.dist
        assert False

    # -- per-part arrays ----------------------------------------------------------
    def build_csr(self):
        self.csr = []
        for item in self.parts:
            rowptr, col, _ = item.csr()
            self.csr.append(CSRPart(rowptr.int().contiguous(), col.int().contiguous(),
                                    part_values(item, self.dtype).contiguous(), item.sizes()))

    def _coalesced(self, item, shape):
        row, col, _ = item.coo()
        return torch.sparse_coo_tensor(torch.stack([row, col], dim=0), part_values(item, self.dtype),
                                       shape).coalesce()

    def build_coo(self):
        self.coo = [self._coalesced(item, item.sizes()) for item in self.parts]

    def _coo_arrays(self):
        self.row_indices = [c.indices()[0].int().contiguous() for c in self.coo]
        self.col_indices = [c.indices()[1].int().contiguous() for c in self.coo]
        self.values = [c.values() for c in self.coo]
        return [c.size(0) for c in self.coo], [c.size(1) for c in self.coo]

    # -- quantise -> aggregate -> dequantise in one device call (pygim_amd/quantize.py) ---------------
    def mul_quantized(self, x: torch.Tensor, post=None):
        """``dequantize(self.mul(quantize(x)))`` with models/quantize.py's arithmetic, on device.
        x: float32 CUDA tensor [ncols, hidden_size].  Returns (out float32 [nrows, hidden_size], scale).
        ``post = (col_mul, col_add, relu)``: per-column epilogue ``out = col_mul * out + col_add`` (then ReLU) applied in
        the sweep's last store (a GCN layer's bias + eval-mode BatchNorm + ReLU folded into one affine map)."""
        from .. import _lib

        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(1) == self.hidden_size
        x = x.contiguous()
        out = torch.empty((self.raw.size(0), self.hidden_size), dtype=torch.float32, device=x.device)
        scale = torch.empty((), dtype=torch.float32, device=x.device)
        mul_p = add_p = 0
        relu = False
        if post is not None:
            col_mul, col_add, relu = post
            col_mul = col_mul.to(x.device, torch.float32).contiguous()
            col_add = col_add.to(x.device, torch.float32).contiguous()
            assert col_mul.numel() == self.hidden_size and col_add.numel() == self.hidden_size
            mul_p, add_p = col_mul.data_ptr(), col_add.data_ptr()
        _lib.quant_spmm_run(self.sp_info_ptr, x.data_ptr(), x.size(1), out.data_ptr(), scale.data_ptr(),
                            torch.cuda.current_stream(x.device).cuda_stream, mul_p, add_p, relu)
        return out, scale
