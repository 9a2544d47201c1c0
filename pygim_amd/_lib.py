"""ctypes binding of the C-ABI HIP library (include/pygim_hip.h).

The library is built in-tree (``pygim_amd/libpygim_hip.so``, see csrc/Makefile or
``__graft_entry__.build``).  There is no fallback: if it is missing, importing the
ops fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYGIM_HIP_LIB", os.path.join(_HERE, "libpygim_hip.so"))

# symbols include/pygim_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "pygim_init_ranks", "pygim_init_units", "pygim_release", "pygim_is_initialized", "pygim_last_error",
    "pygim_device_info", "pygim_group_create", "pygim_group_free", "pygim_spmm_run_group",
    "pygim_grande_run_group", "pygim_spmv_run_group", "pygim_block_run", "pygim_group_timers",
    "pygim_group_info", "pygim_set_tunable", "pygim_group_kernel_ms", "pygim_quant_spmm_run",
    "pygim_quant_absmax", "pygim_quantize", "pygim_dequantize", "pygim_spmm_run_group_x", "pygim_block_run_x",
    "pygim_group_kernel_events", "pygim_group_plan", "pygim_spmm_run_dequant",
    "pygim_quant_spmm_run_post", "pygim_generation", "pygim_group_lds_plan", "pygim_group_lds_code", "pygim_group_lds_geometry", "pygim_group_lds_note",
    "pygim_group_lds_tiles", "pygim_group_lds_runs", "pygim_group_serial", "pygim_group_host_windows",
    "pygim_group_create_transposed", "pygim_sddmm",
    "pygim_spmm_values", "pygim_spmm_values_workspace", "pygim_edge_softmax", "pygim_edge_softmax_workspace", "pygim_edge_softmax_backward",
    "pygim_gat_aggregate", "pygim_gat_aggregate_workspace", "pygim_sparse_attention", "pygim_sparse_attention_workspace",
    "pygim_gatv2_aggregate", "pygim_gatv2_aggregate_workspace", "pygim_gatv2_backward", "pygim_gatv2_backward_workspace",
    "pygim_spmm_reduce", "pygim_spmm_reduce_workspace", "pygim_spmm_reduce_backward", "pygim_gather_launch_shape",
    "pygim_spmm_multi_reduce", "pygim_spmm_multi_reduce_workspace",
    "pygim_spmm_softmax", "pygim_spmm_softmax_workspace", "pygim_spmm_softmax_backward", "pygim_spmm_softmax_backward_workspace",
    "pygim_gat_aggregate_dropout", "pygim_sparse_attention_dropout", "pygim_gatv2_aggregate_dropout", "pygim_gatv2_backward_dropout",
    "pygim_attention_dropout_mask", "pygim_attention_dropout_host",
    "pygim_gat_aggregate_edge", "pygim_sparse_attention_bias",
    "pygim_spmm_edge", "pygim_spmm_edge_workspace", "pygim_spmm_edge_softmax", "pygim_spmm_edge_softmax_workspace",
    "pygim_spmm_edge_backward", "pygim_spmm_edge_backward_workspace",
]

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_UNSORTED = 0, 1, 2, 3, 4
INT8, INT16, INT32, INT64, FLT32, DBL64 = range(6)
FLT16, BF16 = 6, 7   # 16-bit features: sddmm, spmm_values, gat_aggregate, sparse_attention, gatv2_* and spmm_reduce mean only (include/pygim_hip.h)
CSR, COO = 0, 1
REDUCE_MEAN, REDUCE_MAX, REDUCE_MIN = 1, 2, 3
REDUCE_SUM, REDUCE_SOFTMAX = 4, 5   # pygim_spmm_edge (SUM) and pygim_spmm_edge_backward (both)
ACT_NONE, ACT_RELU = 0, 1           # the activation inside the message of pygim_spmm_edge*
STAT_SUM, STAT_MEAN, STAT_MIN, STAT_MAX, STAT_VAR, STAT_STD = range(6)   # pygim_spmm_multi_reduce
# pygim_gather_launch_shape: the kinds, the names of out[0..7] and the bits of "flags"
(SHAPE_SPMM_VALUES, SHAPE_SPMM_REDUCE, SHAPE_GAT_AGGREGATE, SHAPE_SPARSE_ATTENTION, SHAPE_GATV2_AGGREGATE, SHAPE_GATV2_BACKWARD, SHAPE_SDDMM,
 SHAPE_EDGE_SOFTMAX, SHAPE_SPMM_REDUCE_BACKWARD, SHAPE_SPMM_MULTI_REDUCE, SHAPE_SPMM_SOFTMAX, SHAPE_SPMM_SOFTMAX_BACKWARD, SHAPE_SPMM_EDGE,
 SHAPE_SPMM_EDGE_BACKWARD) = range(14)
SHAPE_FIELDS = ("vec", "pieces", "LH", "L", "per", "chunks", "launches", "flags")
SHAPE_PART_PIECE, SHAPE_PART_CHUNK, SHAPE_PART_HEADS, SHAPE_SCALAR_SIZE, SHAPE_SCALAR_ALIGN = 1, 2, 4, 8, 16
GATHER_MAX_H = 65535 * 128   # the widest row of spmm_values, spmm_reduce, spmm_multi_reduce, spmm_softmax, gat_aggregate and spmm_reduce_backward


class PygimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pygim_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the .so is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build the HIP extension first "
                f"(`make -C pygim_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`). "
                f"This backend has no CPU fallback.")
        # torch ships its own libamdhip64; load it FIRST so that this library binds to the same
        # HIP runtime (device pointers, streams and events are shared with torch tensors)
        import torch  # noqa: F401

        L = ctypes.CDLL(LIB_PATH)
        c_i64, c_int, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
        p_i64 = ctypes.POINTER(ctypes.c_int64)
        L.pygim_last_error.restype = ctypes.c_char_p
        L.pygim_init_ranks.argtypes = [c_i64, p_i64]
        L.pygim_init_units.argtypes = [c_i64, p_i64, p_i64]
        L.pygim_device_info.argtypes = [ctypes.c_char_p, c_int, ctypes.POINTER(c_int), p_i64]
        L.pygim_group_create.argtypes = [c_int, c_int, c_int, vp, vp, vp, p_i64, p_i64, p_i64, p_i64, p_i64, c_i64,
                                         p_i64]
        L.pygim_group_create_transposed.argtypes = list(L.pygim_group_create.argtypes)
        L.pygim_sddmm.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, c_i64, vp, vp]
        L.pygim_spmm_values.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, c_i64, vp, c_i64, vp, c_i64, vp]
        L.pygim_spmm_values_workspace.argtypes = [c_int, c_i64, c_i64, c_i64, c_i64]
        L.pygim_spmm_values_workspace.restype = c_i64
        L.pygim_edge_softmax.argtypes = [c_int, c_i64, vp, c_i64, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_edge_softmax_backward.argtypes = [c_int, c_i64, vp, c_i64, vp, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_edge_softmax_workspace.argtypes = [c_int, c_i64, c_i64, c_i64]
        L.pygim_edge_softmax_workspace.restype = c_i64
        L.pygim_gat_aggregate.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, vp, c_i64, ctypes.c_double, vp, c_i64, c_i64, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_gat_aggregate_workspace.argtypes = [c_int, c_i64, c_i64, c_i64, c_i64]
        L.pygim_gat_aggregate_workspace.restype = c_i64
        L.pygim_sparse_attention.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, c_i64, c_i64, ctypes.c_double, vp, c_i64, vp, vp,
                                             c_i64, vp]
        L.pygim_sparse_attention_workspace.argtypes = [c_int, c_i64, c_i64, c_i64, c_i64]
        L.pygim_sparse_attention_workspace.restype = c_i64
        L.pygim_gatv2_aggregate.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, c_i64, ctypes.c_double, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_gatv2_aggregate_workspace.argtypes = [c_int, c_i64, c_i64, c_i64, c_i64]
        L.pygim_gatv2_aggregate_workspace.restype = c_i64
        L.pygim_gatv2_backward.argtypes = [c_int, c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, c_i64, ctypes.c_double, vp, c_i64, vp, vp, vp,
                                           c_i64, vp, vp, c_i64, vp]
        L.pygim_gatv2_backward_workspace.argtypes = [c_int, c_i64, c_i64, c_i64, c_i64]
        L.pygim_gatv2_backward_workspace.restype = c_i64
        # attention dropout: the base signature, then (entry_ids,) p, seed
        c_dbl, c_u64 = ctypes.c_double, ctypes.c_uint64
        L.pygim_gat_aggregate_dropout.argtypes = list(L.pygim_gat_aggregate.argtypes) + [c_dbl, c_u64]
        L.pygim_sparse_attention_dropout.argtypes = list(L.pygim_sparse_attention.argtypes) + [c_dbl, c_u64]
        L.pygim_gatv2_aggregate_dropout.argtypes = list(L.pygim_gatv2_aggregate.argtypes) + [c_dbl, c_u64]
        L.pygim_gatv2_backward_dropout.argtypes = list(L.pygim_gatv2_backward.argtypes) + [vp, c_dbl, c_u64]
        L.pygim_attention_dropout_mask.argtypes = [c_int, c_i64, c_i64, vp, c_dbl, c_u64, vp, vp]
        L.pygim_attention_dropout_host.argtypes = [c_i64, c_i64, c_i64, c_dbl, c_u64, vp]
        # edge terms: the base signature, then the term [nnz, heads], p, seed
        L.pygim_gat_aggregate_edge.argtypes = list(L.pygim_gat_aggregate.argtypes) + [vp, c_dbl, c_u64]
        L.pygim_sparse_attention_bias.argtypes = list(L.pygim_sparse_attention.argtypes) + [vp, c_dbl, c_u64]
        L.pygim_spmm_reduce.argtypes = [c_int, c_int, c_i64, vp, vp, c_i64, vp, vp, c_i64, c_i64, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_spmm_reduce_workspace.argtypes = [c_int, c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_reduce_workspace.restype = c_i64
        L.pygim_spmm_reduce_backward.argtypes = [c_int, c_i64, vp, vp, vp, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp]
        L.pygim_gather_launch_shape.argtypes = [c_int, c_int, c_i64, c_i64, c_int, p_i64]
        p_int = ctypes.POINTER(c_int)
        L.pygim_spmm_multi_reduce_workspace.argtypes = [c_int, p_int, c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_multi_reduce_workspace.restype = c_i64
        L.pygim_spmm_multi_reduce.argtypes = [c_int, p_int, c_int, ctypes.c_double, c_i64, vp, vp, c_i64, vp, c_i64, c_i64, vp, c_i64, vp, vp, vp, c_i64, vp]
        L.pygim_spmm_softmax_workspace.argtypes = [c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_softmax_workspace.restype = c_i64
        L.pygim_spmm_softmax.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_spmm_softmax_backward_workspace.argtypes = [c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_softmax_backward_workspace.restype = c_i64
        L.pygim_spmm_softmax_backward.argtypes = [c_int, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, vp, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_spmm_edge_workspace.argtypes = [c_int, c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_edge_workspace.restype = c_i64
        L.pygim_spmm_edge.argtypes = [c_int, c_int, c_int, ctypes.c_double, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, c_i64, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_spmm_edge_softmax_workspace.argtypes = [c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_edge_softmax_workspace.restype = c_i64
        L.pygim_spmm_edge_softmax.argtypes = [c_int, c_int, ctypes.c_double, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, vp, vp, c_i64, vp]
        L.pygim_spmm_edge_backward_workspace.argtypes = [c_int, c_int, c_i64, c_i64, c_i64]
        L.pygim_spmm_edge_backward_workspace.restype = c_i64
        L.pygim_spmm_edge_backward.argtypes = [c_int, c_int, c_int, ctypes.c_double, c_i64, vp, vp, c_i64, vp, c_i64, vp, c_i64, vp, c_i64, vp, vp, vp, c_i64,
                                               vp, c_i64, vp, c_i64, vp, vp]
        L.pygim_group_free.argtypes = [c_i64]
        L.pygim_group_serial.argtypes = [c_i64, p_i64]
        L.pygim_spmm_run_group.argtypes = [c_i64, vp, vp, vp]
        L.pygim_spmm_run_group_x.argtypes = [c_i64, vp, vp, c_int, vp]
        L.pygim_grande_run_group.argtypes = [c_i64, vp, p_i64, vp, vp]
        L.pygim_spmv_run_group.argtypes = [c_i64, vp, vp, vp]
        L.pygim_block_run.argtypes = [c_i64, c_int, vp, c_i64, vp, c_i64, c_i64, c_int, vp]
        L.pygim_block_run_x.argtypes = [c_i64, c_int, vp, c_i64, vp, c_i64, c_i64, c_int, c_int, vp]
        L.pygim_group_timers.argtypes = [c_i64, ctypes.POINTER(ctypes.c_double)]
        L.pygim_group_info.argtypes = [c_i64, p_i64]
        L.pygim_group_kernel_ms.argtypes = [c_i64, ctypes.POINTER(ctypes.c_double), p_i64, c_int]
        L.pygim_group_kernel_events.argtypes = [c_i64, c_int]
        L.pygim_group_plan.argtypes = [c_i64, p_i64]
        L.pygim_group_lds_plan.argtypes = [c_i64, p_i64]
        L.pygim_group_lds_code.argtypes = [c_i64, p_i64]
        L.pygim_group_lds_geometry.argtypes = [c_i64, p_i64]
        L.pygim_group_lds_note.argtypes = [c_i64, ctypes.c_char_p, c_i64]
        L.pygim_group_lds_tiles.argtypes = [c_i64, p_i64]
        L.pygim_group_lds_runs.argtypes = [c_i64, p_i64]
        L.pygim_group_host_windows.argtypes = [c_i64, p_i64, p_i64]
        L.pygim_generation.restype = c_i64
        L.pygim_quant_spmm_run.argtypes = [c_i64, vp, c_i64, vp, vp, vp]
        L.pygim_quant_spmm_run_post.argtypes = [c_i64, vp, c_i64, vp, vp, vp, vp, c_int, vp]
        L.pygim_quant_absmax.argtypes = [vp, c_i64, c_i64, c_i64, vp, vp]
        L.pygim_quantize.argtypes = [c_int, vp, c_i64, c_i64, c_i64, vp, vp, vp, vp]
        L.pygim_dequantize.argtypes = [c_int, vp, c_i64, vp, vp, vp]
        L.pygim_spmm_run_dequant.argtypes = [c_i64, vp, c_i64, vp, vp, vp]
        L.pygim_set_tunable.argtypes = [ctypes.c_char_p, c_i64]
        L.pygim_set_tunable.restype = c_i64
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise PygimError(rc, lib().pygim_last_error().decode())


def i64_array(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[ctypes.c_void_p(int(p) if p else None) for p in ptrs])


def _env_tunables():
    """PYGIM_TUNE="name=value,name=value": kernel tunables for a whole run without touching the driver scripts (A/B runs)"""
    for kv in filter(None, os.environ.get("PYGIM_TUNE", "").split(",")):
        name, _, value = kv.partition("=")
        if set_tunable(name.strip(), int(value)) == -1:
            raise ValueError(f"PYGIM_TUNE: unknown tunable {name!r}")


def init_ranks(nr_ranks, want_units=False):
    out = (ctypes.c_int64 * max(int(nr_ranks), 1))()
    check(lib().pygim_init_ranks(int(nr_ranks), out))
    _env_tunables()
    return list(out)[: int(nr_ranks)] if want_units else None


def init_units(nr_units):
    n = max((int(nr_units) + 7) // 8, 1)
    out = (ctypes.c_int64 * n)()
    ranks = ctypes.c_int64(0)
    check(lib().pygim_init_units(int(nr_units), out, ctypes.byref(ranks)))
    return list(out)[: ranks.value]


def release():
    check(lib().pygim_release())


def is_initialized():
    return bool(lib().pygim_is_initialized())


def device_info():
    name = ctypes.create_string_buffer(256)
    cu = ctypes.c_int(0)
    mem = ctypes.c_int64(0)
    check(lib().pygim_device_info(name, 256, ctypes.byref(cu), ctypes.byref(mem)))
    return name.value.decode(), cu.value, mem.value


def group_create(fmt, dtype, idx0_ptrs, col_ptrs, val_ptrs, nrows, ncols, nnz, n_dense, dense_cols, h):
    n = len(col_ptrs)
    handle = ctypes.c_int64(0)
    vals = None if val_ptrs is None else ptr_array(val_ptrs)
    check(lib().pygim_group_create(fmt, dtype, n, ptr_array(idx0_ptrs), ptr_array(col_ptrs), vals, i64_array(nrows),
                                   i64_array(ncols), i64_array(nnz), i64_array(n_dense), i64_array(dense_cols),
                                   int(h), ctypes.byref(handle)))
    return handle.value


def group_create_transposed(fmt, dtype, idx0_ptrs, col_ptrs, val_ptrs, nrows, ncols, nnz, n_dense, dense_cols, h):
    """the group of A^T for the arguments that describe A (include/pygim_hip.h): one CSR part of sum(ncols) x nrows[0]"""
    n = len(col_ptrs)
    handle = ctypes.c_int64(0)
    vals = None if val_ptrs is None else ptr_array(val_ptrs)
    check(lib().pygim_group_create_transposed(fmt, dtype, n, ptr_array(idx0_ptrs), ptr_array(col_ptrs), vals, i64_array(nrows),
                                              i64_array(ncols), i64_array(nnz), i64_array(n_dense), i64_array(dense_cols),
                                              int(h), ctypes.byref(handle)))
    return handle.value


def sddmm(dtype, nrows, rowptr_ptr, col_ptr, nnz, g_ptr, ldg, x_ptr, ldx, h, out_ptr, stream=0):
    """out[e] = G[row(e)] . X[col[e]] for every stored entry of a CSR (device pointers; FLT32 / DBL64, or FLT16 / BF16 G and X with a float32 out)"""
    check(lib().pygim_sddmm(int(dtype), int(nrows), ctypes.c_void_p(rowptr_ptr or None), ctypes.c_void_p(col_ptr or None), int(nnz),
                            ctypes.c_void_p(g_ptr or None), int(ldg), ctypes.c_void_p(x_ptr or None), int(ldx), int(h),
                            ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)))


def _vp(p):
    return ctypes.c_void_p(p or None)


def spmm_values_workspace(dtype, nrows, nnz, h, heads):
    """bytes of scratch spmm_values needs for this shape (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_values_workspace(int(dtype), int(nrows), int(nnz), int(h), int(heads)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_values_workspace arguments")
    return n


def spmm_values(dtype, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, heads, x_ptr, ldx, h, out_ptr, ldo, ws_ptr, ws_bytes, stream=0):
    """out[r, f] = sum_e values[e, head of f] * X[col[e], f] over the entries of row r (device pointers; FLT32 / DBL64, or FLT16 / BF16 X and out with
    float32 values)"""
    check(lib().pygim_spmm_values(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(val_ptr), int(heads), _vp(x_ptr),
                                  int(ldx), int(h), _vp(out_ptr), int(ldo), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def edge_softmax_workspace(dtype, nrows, nnz, heads):
    """bytes of scratch edge_softmax / edge_softmax_backward need for this shape"""
    n = int(lib().pygim_edge_softmax_workspace(int(dtype), int(nrows), int(nnz), int(heads)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad edge_softmax_workspace arguments")
    return n


def edge_softmax(dtype, nrows, rowptr_ptr, nnz, scores_ptr, heads, out_ptr, ws_ptr, ws_bytes, stream=0):
    """softmax of scores [nnz, heads] over the stored entries of every row, per head"""
    check(lib().pygim_edge_softmax(int(dtype), int(nrows), _vp(rowptr_ptr), int(nnz), _vp(scores_ptr), int(heads), _vp(out_ptr),
                                   _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def edge_softmax_backward(dtype, nrows, rowptr_ptr, nnz, p_ptr, dp_ptr, heads, out_ptr, ws_ptr, ws_bytes, stream=0):
    """out = P * (dP - sum_row P * dP): the gradient of edge_softmax with respect to the scores"""
    check(lib().pygim_edge_softmax_backward(int(dtype), int(nrows), _vp(rowptr_ptr), int(nnz), _vp(p_ptr), _vp(dp_ptr), int(heads),
                                            _vp(out_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def gat_aggregate_workspace(dtype, nrows, nnz, h, heads):
    """bytes of scratch gat_aggregate needs for this shape (a function of the numbers alone)"""
    n = int(lib().pygim_gat_aggregate_workspace(int(dtype), int(nrows), int(nnz), int(h), int(heads)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad gat_aggregate_workspace arguments")
    return n


def gat_aggregate(dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr, ldo, lse_ptr, ws_ptr,
                  ws_bytes, stream=0):
    """out[r, f] = sum_e softmax_e(leaky_relu(a_dst[r, k] + a_src[col[e], k])) * X[col[e], f] over the entries of row r, k the head of f, in
    one pass; lse_ptr (0: not wanted) receives max + log(sum exp) per row and head (device pointers; FLT32 / DBL64, or FLT16 / BF16 X and out
    with float32 a_dst, a_src and lse)"""
    check(lib().pygim_gat_aggregate(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(a_dst_ptr), _vp(a_src_ptr), int(heads),
                                    float(negative_slope), _vp(x_ptr), int(ldx), int(h), _vp(out_ptr), int(ldo), _vp(lse_ptr), _vp(ws_ptr),
                                    int(ws_bytes), _vp(stream)))


def sparse_attention_workspace(dtype, nrows, nnz, h, heads):
    """bytes of scratch sparse_attention needs for this shape (a function of the numbers alone; heads wider than 256 are rejected)"""
    n = int(lib().pygim_sparse_attention_workspace(int(dtype), int(nrows), int(nnz), int(h), int(heads)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad sparse_attention_workspace arguments")
    return n


def sparse_attention(dtype, nrows, rowptr_ptr, col_ptr, nnz, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, h, heads, scale, out_ptr, ldo, lse_ptr, ws_ptr,
                     ws_bytes, stream=0):
    """out[r, f] = sum_e softmax_e(scale * Q[r, head k] . K[col[e], head k]) * V[col[e], f] over the entries of row r, k the head of f, in one
    pass; lse_ptr (0: not wanted) receives max + log(sum exp) per row and head (device pointers; FLT32 / DBL64, or FLT16 / BF16 Q, K, V and
    out with float32 lse; h / heads <= 256)"""
    check(lib().pygim_sparse_attention(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(q_ptr), int(ldq), _vp(k_ptr), int(ldk),
                                       _vp(v_ptr), int(ldv), int(h), int(heads), float(scale), _vp(out_ptr), int(ldo), _vp(lse_ptr), _vp(ws_ptr),
                                       int(ws_bytes), _vp(stream)))


def gatv2_aggregate_workspace(dtype, nrows, nnz, h, heads):
    """bytes of scratch gatv2_aggregate needs for this shape (a function of the numbers alone; heads wider than 256 are rejected)"""
    n = int(lib().pygim_gatv2_aggregate_workspace(int(dtype), int(nrows), int(nnz), int(h), int(heads)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad gatv2_aggregate_workspace arguments")
    return n


def gatv2_aggregate(dtype, nrows, rowptr_ptr, col_ptr, nnz, xd_ptr, ld_dst, xs_ptr, ld_src, att_ptr, h, heads, negative_slope, out_ptr, ldo, lse_ptr,
                    ws_ptr, ws_bytes, stream=0):
    """out[r, f] = sum_e softmax_e(sum_{f' in head k} att[f'] * leaky_relu(x_dst[r, f'] + x_src[col[e], f'])) * x_src[col[e], f] over the entries
    of row r, k the head of f, in one pass; lse_ptr (0: not wanted) receives max + log(sum exp) per row and head (device pointers; FLT32 /
    DBL64, or FLT16 / BF16 x_dst, x_src and out with float32 att and lse; h / heads <= 256)"""
    check(lib().pygim_gatv2_aggregate(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(xd_ptr), int(ld_dst), _vp(xs_ptr),
                                      int(ld_src), _vp(att_ptr), int(h), int(heads), float(negative_slope), _vp(out_ptr), int(ldo), _vp(lse_ptr),
                                      _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def gatv2_backward_workspace(dtype, nrows, nnz, h, heads):
    """bytes of scratch gatv2_backward needs for this shape, either direction (a function of the numbers alone)"""
    n = int(lib().pygim_gatv2_backward_workspace(int(dtype), int(nrows), int(nnz), int(h), int(heads)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad gatv2_backward_workspace arguments")
    return n


def gatv2_backward(dtype, transposed, nrows, rowptr_ptr, col_ptr, nnz, own_ptr, ld_own, oth_ptr, ld_oth, att_ptr, h, heads, negative_slope, g_ptr, ldg,
                   lse_ptr, delta_ptr, d_own_ptr, ldd, datt_ptr, ws_ptr, ws_bytes, stream=0):
    """one direction of the backward of gatv2_aggregate on the CSR it is given: transposed = 0 (the CSR of A, own = x_dst, oth = x_src) stores
    dx_dst into d_own and, when datt_ptr is not 0, datt [h]; transposed = 1 (the CSR of A^T, own = x_src, oth = x_dst, datt_ptr 0) stores
    dx_src.  G, lse and delta [rows of A, heads] belong to the rows of A (device pointers; types as for gatv2_aggregate)"""
    check(lib().pygim_gatv2_backward(int(dtype), int(transposed), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(own_ptr), int(ld_own),
                                     _vp(oth_ptr), int(ld_oth), _vp(att_ptr), int(h), int(heads), float(negative_slope), _vp(g_ptr), int(ldg),
                                     _vp(lse_ptr), _vp(delta_ptr), _vp(d_own_ptr), int(ldd), _vp(datt_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


# ---- attention dropout (include/pygim_hip.h): the base calls with a rate p in [0, 1) and a 64-bit seed; p = 0 is the base call.  The
# base entry points' *_workspace functions serve them.
def _seed(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def gat_aggregate_dropout(dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr, ldo, lse_ptr,
                          ws_ptr, ws_bytes, stream, p, seed):
    """gat_aggregate with the probabilities dropped at rate p by the mask of (seed, entry, head) after the softmax"""
    check(lib().pygim_gat_aggregate_dropout(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(a_dst_ptr), _vp(a_src_ptr),
                                            int(heads), float(negative_slope), _vp(x_ptr), int(ldx), int(h), _vp(out_ptr), int(ldo), _vp(lse_ptr),
                                            _vp(ws_ptr), int(ws_bytes), _vp(stream), float(p), _seed(seed)))


def sparse_attention_dropout(dtype, nrows, rowptr_ptr, col_ptr, nnz, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, h, heads, scale, out_ptr, ldo, lse_ptr,
                             ws_ptr, ws_bytes, stream, p, seed):
    """sparse_attention with the probabilities dropped at rate p by the mask of (seed, entry, head) after the softmax"""
    check(lib().pygim_sparse_attention_dropout(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(q_ptr), int(ldq), _vp(k_ptr),
                                               int(ldk), _vp(v_ptr), int(ldv), int(h), int(heads), float(scale), _vp(out_ptr), int(ldo),
                                               _vp(lse_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream), float(p), _seed(seed)))


def gatv2_aggregate_dropout(dtype, nrows, rowptr_ptr, col_ptr, nnz, xd_ptr, ld_dst, xs_ptr, ld_src, att_ptr, h, heads, negative_slope, out_ptr, ldo,
                            lse_ptr, ws_ptr, ws_bytes, stream, p, seed):
    """gatv2_aggregate with the probabilities dropped at rate p by the mask of (seed, entry, head) after the softmax"""
    check(lib().pygim_gatv2_aggregate_dropout(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(xd_ptr), int(ld_dst),
                                              _vp(xs_ptr), int(ld_src), _vp(att_ptr), int(h), int(heads), float(negative_slope), _vp(out_ptr),
                                              int(ldo), _vp(lse_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream), float(p), _seed(seed)))


def gatv2_backward_dropout(dtype, transposed, nrows, rowptr_ptr, col_ptr, nnz, own_ptr, ld_own, oth_ptr, ld_oth, att_ptr, h, heads, negative_slope,
                           g_ptr, ldg, lse_ptr, delta_ptr, d_own_ptr, ldd, datt_ptr, ws_ptr, ws_bytes, stream, entry_ids_ptr, p, seed):
    """gatv2_backward of a forward that ran with dropout (p, seed); entry_ids_ptr: int32 [nnz], the index in A of every entry of the CSR
    that is walked (the perm of the transposed CSR), 0 for the CSR of A itself"""
    check(lib().pygim_gatv2_backward_dropout(int(dtype), int(transposed), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(own_ptr),
                                             int(ld_own), _vp(oth_ptr), int(ld_oth), _vp(att_ptr), int(h), int(heads), float(negative_slope),
                                             _vp(g_ptr), int(ldg), _vp(lse_ptr), _vp(delta_ptr), _vp(d_own_ptr), int(ldd), _vp(datt_ptr),
                                             _vp(ws_ptr), int(ws_bytes), _vp(stream), _vp(entry_ids_ptr), float(p), _seed(seed)))


def attention_dropout_mask(dtype, nnz, heads, entry_ids_ptr, p, seed, mask_ptr, stream=0):
    """mask [nnz, heads] (FLT32 / DBL64, device) = 1 / (1 - p) where entry (entry_ids[i], or i when entry_ids_ptr is 0) and head are kept, else 0"""
    check(lib().pygim_attention_dropout_mask(int(dtype), int(nnz), int(heads), _vp(entry_ids_ptr), float(p), _seed(seed), _vp(mask_ptr), _vp(stream)))


def attention_dropout_host(nnz, heads, e0, p, seed):
    """the keep mask of entries e0 .. e0 + nnz - 1 as a numpy uint8 [nnz, heads], computed on the host by the kernels' own function (no device)"""
    import numpy as np

    keep = np.empty((int(nnz), int(heads)), dtype=np.uint8)
    check(lib().pygim_attention_dropout_host(int(nnz), int(heads), int(e0), float(p), _seed(seed), keep.ctypes.data if keep.size else None))
    return keep


# ---- edge terms (include/pygim_hip.h): the *_dropout calls with one scalar per (stored entry, head) inside the score; the term is
# [nnz, heads] in the compute type, in the stored order of A.  The base entry points' *_workspace functions serve them.
def gat_aggregate_edge(dtype, nrows, rowptr_ptr, col_ptr, nnz, a_dst_ptr, a_src_ptr, heads, negative_slope, x_ptr, ldx, h, out_ptr, ldo, lse_ptr,
                       ws_ptr, ws_bytes, stream, a_edge_ptr, p=0.0, seed=0):
    """gat_aggregate with the score leaky_relu(a_dst[row] + a_src[col] + a_edge[entry]); p > 0: with attention dropout (p, seed)"""
    check(lib().pygim_gat_aggregate_edge(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(a_dst_ptr), _vp(a_src_ptr),
                                         int(heads), float(negative_slope), _vp(x_ptr), int(ldx), int(h), _vp(out_ptr), int(ldo), _vp(lse_ptr),
                                         _vp(ws_ptr), int(ws_bytes), _vp(stream), _vp(a_edge_ptr), float(p), _seed(seed)))


def sparse_attention_bias(dtype, nrows, rowptr_ptr, col_ptr, nnz, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, h, heads, scale, out_ptr, ldo, lse_ptr,
                          ws_ptr, ws_bytes, stream, bias_ptr, p=0.0, seed=0):
    """sparse_attention with the score scale * Q[row] . K[col] + bias[entry]; p > 0: with attention dropout (p, seed)"""
    check(lib().pygim_sparse_attention_bias(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(q_ptr), int(ldq), _vp(k_ptr),
                                            int(ldk), _vp(v_ptr), int(ldv), int(h), int(heads), float(scale), _vp(out_ptr), int(ldo),
                                            _vp(lse_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream), _vp(bias_ptr), float(p), _seed(seed)))


def spmm_reduce_workspace(dtype, op, nrows, nnz, h):
    """bytes of scratch spmm_reduce needs for this type, reduction and shape (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_reduce_workspace(int(dtype), int(op), int(nrows), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_reduce_workspace arguments")
    return n


def spmm_reduce(dtype, op, nrows, rowptr_ptr, col_ptr, nnz, val_ptr, x_ptr, ldx, h, out_ptr, ldo, arg_ptr, ws_ptr, ws_bytes, stream=0):
    """out[r, f] = mean / max / min over the entries e of row r of values[e] * X[col[e], f] (REDUCE_*; val_ptr 0: unit weights;
    arg_ptr: int32 [nrows, h] for the winning entry of max / min, or 0; FLT16 / BF16 X and out with float32 values: REDUCE_MEAN only)"""
    check(lib().pygim_spmm_reduce(int(dtype), int(op), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(val_ptr), _vp(x_ptr), int(ldx),
                                  int(h), _vp(out_ptr), int(ldo), _vp(arg_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def spmm_reduce_backward(dtype, ncols, rowptr_t_ptr, rows_t_ptr, perm_ptr, nnz, val_ptr, g_ptr, ldg, arg_ptr, h, dx_ptr, ldd, stream=0):
    """dX[c] = sum over the entries of row c of A^T of (arg[r] == e ? values[e] * G[r] : 0): the gradient of max / min (FLT32 / DBL64)"""
    check(lib().pygim_spmm_reduce_backward(int(dtype), int(ncols), _vp(rowptr_t_ptr), _vp(rows_t_ptr), _vp(perm_ptr), int(nnz), _vp(val_ptr),
                                           _vp(g_ptr), int(ldg), _vp(arg_ptr), int(h), _vp(dx_ptr), int(ldd), _vp(stream)))


def _stat_array(stats):
    stats = [int(s) for s in stats]
    return (ctypes.c_int * max(len(stats), 1))(*stats), len(stats)


def spmm_multi_reduce_workspace(dtype, stats, nrows, nnz, h):
    """bytes of scratch spmm_multi_reduce needs for this type, list of statistics (STAT_*) and shape (a function of the numbers alone)"""
    arr, k = _stat_array(stats)
    n = int(lib().pygim_spmm_multi_reduce_workspace(int(dtype), arr, k, int(nrows), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_multi_reduce_workspace arguments")
    return n


def spmm_multi_reduce(dtype, stats, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, h, out_ptr, ldo, arg_max_ptr, arg_min_ptr, ws_ptr, ws_bytes, stream=0):
    """out[r, j * h + f] = statistic stats[j] (STAT_*: sum, mean, min, max, var, std = sqrt(var + eps)) over the entries e of row r of
    X[col[e], f], all in one gather; arg_max_ptr / arg_min_ptr: int32 [nrows, h] for the winning entries, or 0 (FLT32, DBL64, FLT16, BF16)"""
    arr, k = _stat_array(stats)
    check(lib().pygim_spmm_multi_reduce(int(dtype), arr, k, float(eps), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(x_ptr), int(ldx), int(h),
                                        _vp(out_ptr), int(ldo), _vp(arg_max_ptr), _vp(arg_min_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def spmm_softmax_workspace(dtype, nrows, nnz, h):
    """bytes of scratch spmm_softmax needs for this type and shape (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_softmax_workspace(int(dtype), int(nrows), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_softmax_workspace arguments")
    return n


def spmm_softmax(dtype, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, t_ptr, h, out_ptr, ldo, lse_ptr, ws_ptr, ws_bytes, stream=0):
    """out[r, f] = sum over the entries e of row r of softmax_e(t[f] * X[col[e], f]) * X[col[e], f], in one gather; t_ptr: [h] in the compute
    type; lse_ptr: [nrows, h] in the compute type for the log-sum-exp, or 0 (FLT32, DBL64, FLT16, BF16)"""
    check(lib().pygim_spmm_softmax(int(dtype), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(x_ptr), int(ldx), _vp(t_ptr), int(h),
                                   _vp(out_ptr), int(ldo), _vp(lse_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def spmm_softmax_backward_workspace(dtype, ncols, nnz, h):
    """bytes of scratch spmm_softmax_backward needs for this type and shape (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_softmax_backward_workspace(int(dtype), int(ncols), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_softmax_backward_workspace arguments")
    return n


def spmm_softmax_backward(dtype, ncols, rowptr_t_ptr, rows_t_ptr, nnz, x_ptr, ldx, t_ptr, h, g_ptr, ldg, out_ptr, ldo, lse_ptr, dx_ptr, ldd, dt_ptr,
                          ws_ptr, ws_bytes, stream=0):
    """the gradient of spmm_softmax in one gather on the CSR of A^T: dX [ncols, h] and, when dt_ptr is not 0, dT [ncols, h] in the compute
    type, whose column sum is the gradient of t; out_ptr / lse_ptr: what the forward stored"""
    check(lib().pygim_spmm_softmax_backward(int(dtype), int(ncols), _vp(rowptr_t_ptr), _vp(rows_t_ptr), int(nnz), _vp(x_ptr), int(ldx), _vp(t_ptr), int(h),
                                            _vp(g_ptr), int(ldg), _vp(out_ptr), int(ldo), _vp(lse_ptr), _vp(dx_ptr), int(ldd), _vp(dt_ptr), _vp(ws_ptr),
                                            int(ws_bytes), _vp(stream)))


def spmm_edge_workspace(dtype, op, nrows, nnz, h):
    """bytes of scratch spmm_edge needs for this type, fold (REDUCE_SUM / _MEAN / _MAX / _MIN) and shape (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_edge_workspace(int(dtype), int(op), int(nrows), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_edge_workspace arguments")
    return n


def spmm_edge(dtype, op, act, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, h, out_ptr, ldo, arg_ptr, ws_ptr, ws_bytes, stream=0):
    """out[r, f] = sum / mean / max / min over the entries e of row r of act(X[col[e], f] + E[e, f]) + eps (REDUCE_*, ACT_*), in one gather with
    E [nnz, h] read as a stream; arg_ptr: int32 [nrows, h] for the winning entry of max / min, or 0"""
    check(lib().pygim_spmm_edge(int(dtype), int(op), int(act), float(eps), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(x_ptr), int(ldx),
                                _vp(e_ptr), int(lde), int(h), _vp(out_ptr), int(ldo), _vp(arg_ptr), _vp(ws_ptr), int(ws_bytes), _vp(stream)))


def spmm_edge_softmax_workspace(dtype, nrows, nnz, h):
    """bytes of scratch spmm_edge_softmax needs for this type and shape (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_edge_softmax_workspace(int(dtype), int(nrows), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_edge_softmax_workspace arguments")
    return n


def spmm_edge_softmax(dtype, act, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, t_ptr, h, out_ptr, ldo, lse_ptr, ws_ptr, ws_bytes, stream=0):
    """spmm_softmax of the messages act(X[col[e], f] + E[e, f]) + eps; t_ptr: [h] and lse_ptr: [nrows, h] or 0, in the compute type"""
    check(lib().pygim_spmm_edge_softmax(int(dtype), int(act), float(eps), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(x_ptr), int(ldx),
                                        _vp(e_ptr), int(lde), _vp(t_ptr), int(h), _vp(out_ptr), int(ldo), _vp(lse_ptr), _vp(ws_ptr), int(ws_bytes),
                                        _vp(stream)))


def spmm_edge_backward_workspace(dtype, op, nrows, nnz, h):
    """the rows of dT_part: the runs of 512 entries (a function of the numbers alone)"""
    n = int(lib().pygim_spmm_edge_backward_workspace(int(dtype), int(op), int(nrows), int(nnz), int(h)))
    if n < 0:
        raise PygimError(ERR_INVALID, "bad spmm_edge_backward_workspace arguments")
    return n


def spmm_edge_backward(dtype, op, act, eps, nrows, rowptr_ptr, col_ptr, nnz, x_ptr, ldx, e_ptr, lde, g_ptr, ldg, arg_ptr, t_ptr, out_ptr, ldo, lse_ptr, h,
                       de_ptr, ldde, dt_part_ptr, stream=0):
    """dE [nnz, h] of spmm_edge (REDUCE_SUM / _MEAN / _MAX / _MIN, with arg_ptr for max / min) or spmm_edge_softmax (REDUCE_SOFTMAX, with
    t_ptr, out_ptr, lse_ptr; dt_part_ptr: [runs, h] in the compute type, whose column sum is the gradient of t, or 0), in entry order"""
    check(lib().pygim_spmm_edge_backward(int(dtype), int(op), int(act), float(eps), int(nrows), _vp(rowptr_ptr), _vp(col_ptr), int(nnz), _vp(x_ptr),
                                         int(ldx), _vp(e_ptr), int(lde), _vp(g_ptr), int(ldg), _vp(arg_ptr), _vp(t_ptr), _vp(out_ptr), int(ldo),
                                         _vp(lse_ptr), int(h), _vp(de_ptr), int(ldde), _vp(dt_part_ptr), _vp(stream)))


def gather_launch_shape(kind, dtype, h, heads=1, aligned=True):
    """the kernel instantiation and lane layout the entry point `kind` (SHAPE_*) launches for these numbers, as a dict over SHAPE_FIELDS
    (include/pygim_hip.h); no device is needed.  PygimError for numbers the entry point rejects"""
    out = (ctypes.c_int64 * 8)()
    if lib().pygim_gather_launch_shape(int(kind), int(dtype), int(h), int(heads), 1 if aligned else 0, out) != 0:
        raise PygimError(ERR_INVALID, f"no launch shape for kind {kind}, type {dtype}, h {h}, heads {heads}")
    return dict(zip(SHAPE_FIELDS, [int(v) for v in out]))


def group_free(handle):
    check(lib().pygim_group_free(int(handle)))


def spmm_run_group(handle, b_ptrs, out_ptr, stream=0, x_unchanged=False):
    """``x_unchanged``: the dense parts hold exactly what the most recent product on the same pointers held
    (include/pygim_hip.h, "Threading"): its slice-major copy is reused instead of being made again."""
    check(lib().pygim_spmm_run_group_x(int(handle), ptr_array(b_ptrs), ctypes.c_void_p(out_ptr),
                                       1 if x_unchanged else 0, ctypes.c_void_p(stream or None)))


def grande_run_group(handle, b_ptrs, lds, out_ptr, stream=0):
    check(lib().pygim_grande_run_group(int(handle), ptr_array(b_ptrs), i64_array(lds), ctypes.c_void_p(out_ptr),
                                       ctypes.c_void_p(stream or None)))


def spmv_run_group(handle, b_ptrs, out_ptr, stream=0):
    check(lib().pygim_spmv_run_group(int(handle), ptr_array(b_ptrs), ctypes.c_void_p(out_ptr),
                                     ctypes.c_void_p(stream or None)))


def block_run(handle, part, x_ptr, ldx, c_ptr, ldc, width, accumulate=False, stream=0, x_unchanged=False):
    check(lib().pygim_block_run_x(int(handle), int(part), ctypes.c_void_p(x_ptr), int(ldx), ctypes.c_void_p(c_ptr),
                                  int(ldc), int(width), 1 if accumulate else 0, 1 if x_unchanged else 0,
                                  ctypes.c_void_p(stream or None)))


def group_timers(handle):
    out = (ctypes.c_double * 5)()
    check(lib().pygim_group_timers(int(handle), out))
    return list(out)


def group_kernel_events(handle, on=True):
    check(lib().pygim_group_kernel_events(int(handle), 1 if on else 0))


def group_plan(handle):
    out = (ctypes.c_int64 * 8)()
    check(lib().pygim_group_plan(int(handle), out))
    keys = ["n_panels", "panel_cols", "n_items", "col16", "n_coop_items", "n_segment_tasks", "merged", "has_extra"]
    return dict(zip(keys, [int(v) for v in out]))


def group_lds_plan(handle):
    out = (ctypes.c_int64 * 4)()
    check(lib().pygim_group_lds_plan(int(handle), out))
    return dict(zip(["tiles", "chunk_fills", "tokens", "nnz"], [int(v) for v in out]))


def group_lds_code(handle):
    out = (ctypes.c_int64 * 4)()
    check(lib().pygim_group_lds_code(int(handle), out))
    return dict(zip(["code_bytes", "paired_entries", "active", "device_generated"], [int(v) for v in out[:4]]))


def group_lds_tiles(handle):
    """which rows share a tile: similarity order (label propagation) or consecutive rows"""
    out = (ctypes.c_int64 * 4)()
    check(lib().pygim_group_lds_tiles(int(handle), out))
    return dict(zip(["similarity", "labels", "largest_label_rows", "sweep_locality"], [int(v) for v in out[:4]]))


def group_lds_runs(handle):
    """products (or blocks) the LDS-staged kernels served for this group so far"""
    out = ctypes.c_int64(0)
    check(lib().pygim_group_lds_runs(int(handle), ctypes.byref(out)))
    return int(out.value)


def group_host_windows(handle):
    """feature windows the last run with host operands moved as a pipeline (1 = upload, product, download one after the other)"""
    return group_host_call(handle)["windows"]


def group_host_call(handle):
    """... and whether their products stored straight into the caller's page-locked result (``direct``)"""
    w, d = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().pygim_group_host_windows(int(handle), ctypes.byref(w), ctypes.byref(d)))
    return {"windows": int(w.value), "direct": int(d.value)}


def group_lds_geometry(handle):
    out = (ctypes.c_int64 * 10)()
    check(lib().pygim_group_lds_geometry(int(handle), out))
    return dict(zip(["waves", "acc_per_wave", "chunk_cols", "buffers", "group", "x_sets", "shared_entries", "col_splits", "xcd_slices", "touch_share"],
                    [int(v) for v in out]))


def group_lds_note(handle):
    """which form of the product the group got (code stream / token kernels / sweep) and why"""
    buf = ctypes.create_string_buffer(1024)
    check(lib().pygim_group_lds_note(int(handle), buf, 1024))
    return buf.value.decode()


def generation():
    """count of pygim_release calls: handles of an earlier generation are dead"""
    return int(lib().pygim_generation())


def group_serial(handle):
    """creation serial of a live group (never reused, unlike the address that is the handle); PygimError for a dead handle"""
    out = ctypes.c_int64(0)
    check(lib().pygim_group_serial(int(handle), ctypes.byref(out)))
    return int(out.value)


def group_info(handle):
    out = (ctypes.c_int64 * 8)()
    check(lib().pygim_group_info(int(handle), out))
    keys = ["total_rows", "total_cols", "h", "n_parts", "n_long_rows", "all_ones", "n_panels", "n_items"]
    return dict(zip(keys, list(out)))


def set_tunable(name, value):
    return int(lib().pygim_set_tunable(name.encode(), int(value)))


def group_kernel_ms(handle, reset=True):
    """(sum of milliseconds, launches) of the dominant kernel since the last reset
    (needs set_tunable('kernel_events', 1))."""
    ms = ctypes.c_double(0)
    n = ctypes.c_int64(0)
    check(lib().pygim_group_kernel_ms(int(handle), ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0))
    return ms.value, n.value


def quant_absmax(x_ptr, ldx, rows, width, bits_ptr, stream=0):
    check(lib().pygim_quant_absmax(ctypes.c_void_p(x_ptr or None), int(ldx), int(rows), int(width), ctypes.c_void_p(bits_ptr),
                                   ctypes.c_void_p(stream or None)))


def quantize(dtype, x_ptr, ldx, rows, width, bits_ptr, xq_ptr, scale_ptr=0, stream=0):
    check(lib().pygim_quantize(int(dtype), ctypes.c_void_p(x_ptr or None), int(ldx), int(rows), int(width),
                               ctypes.c_void_p(bits_ptr), ctypes.c_void_p(xq_ptr or None), ctypes.c_void_p(scale_ptr or None),
                               ctypes.c_void_p(stream or None)))


def dequantize(dtype, q_ptr, n, bits_ptr, out_ptr, stream=0):
    check(lib().pygim_dequantize(int(dtype), ctypes.c_void_p(q_ptr or None), int(n), ctypes.c_void_p(bits_ptr),
                                 ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)))


def spmm_run_dequant(handle, xq_ptr, ldx, out_ptr, bits_ptr, stream=0):
    check(lib().pygim_spmm_run_dequant(int(handle), ctypes.c_void_p(xq_ptr), int(ldx), ctypes.c_void_p(out_ptr),
                                       ctypes.c_void_p(bits_ptr), ctypes.c_void_p(stream or None)))


def quant_spmm_run(handle, x_ptr, ldx, out_ptr, scale_ptr=0, stream=0, col_mul_ptr=0, col_add_ptr=0, relu=False):
    """quantise -> aggregate -> dequantise; with ``col_mul_ptr`` / ``col_add_ptr`` (device float[h]) the per-column
    epilogue out = col_mul * out + col_add (then ReLU) runs in the sweep's last store"""
    check(lib().pygim_quant_spmm_run_post(int(handle), ctypes.c_void_p(x_ptr), int(ldx), ctypes.c_void_p(out_ptr),
                                          ctypes.c_void_p(scale_ptr or None), ctypes.c_void_p(col_mul_ptr or None),
                                          ctypes.c_void_p(col_add_ptr or None), 1 if relu else 0,
                                          ctypes.c_void_p(stream or None)))
