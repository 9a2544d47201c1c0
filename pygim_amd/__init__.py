"""MI355X-native GNN aggregation backend with PyGim's ``backend_pim`` surface.

Layout:
  csrc/            hand-written HIP kernels (gfx950) + the C ABI (include/pygim_hip.h)
  _lib.py          ctypes binding of that ABI (fails loudly when the .so is missing)
  pim_ops.py       ``torch.ops.pim_ops`` registration (the reference's custom-op names)
  backend_pim/     ``prepare_pim_*`` / ``SparseTensorCOO.mul`` wrappers (reference surface)
  sparse_tensor.py stand-in for torch_sparse.SparseTensor when that package is absent
  synth.py         seeded synthetic graphs in the shapes BASELINE.json names
  dist.py          sp_parts / ds_parts across the GPUs of one node (torch.distributed/RCCL)
  autograd.py      gradients of ``mul``: A^T . G through a transposed group, the edge values' SDDMM (``sddmm``)
  attention.py     products and softmax with per-call edge values (``EdgeGraph``, ``spmm_values``, ``edge_softmax``, the fused ``gat_aggregate``, ``sparse_attention`` and ``gatv2_aggregate``)
  reduce.py        aggregation with a reduction other than the sum (``spmm_reduce``: mean / max / min, with gradients; ``spmm_multi_reduce``: several statistics in one gather; ``spmm_softmax``: softmax aggregation per feature in one gather; ``spmm_edge``: messages with a feature-wide edge feature)
"""
__version__ = "0.1.0"

from .attention import EdgeGraph, dropout_mask, edge_softmax, gat_aggregate, gatv2_aggregate, sparse_attention, spmm_values  # noqa: E402,F401
from .autograd import sddmm  # noqa: E402,F401
from .reduce import matmul_edge, matmul_softmax, spmm_edge, spmm_multi_reduce, spmm_reduce, spmm_softmax  # noqa: E402,F401
