"""GPU parity of the shared touches of the 8-wave code-stream kernels (k_lds_code8_*, tunable lds_touch_share).

The workgroups that an XCD runs side by side on ONE code stream (lds_xcd_slices = 2 / 4) share its touches: wave w of the workgroup at
slice position w % sx pulls the stream's lines into the L2, its partners' touches ask for one dword.  A touch is a prefetch and nothing
else, so C must not change by a bit: equal to the oracle's stored-order loop and to the run with lds_touch_share = 0, for every
arrangement -- two slices (pairs), three (no XCD mapping, every wave touches), four (pairs or all four on one XCD), the integer stream,
the dequantising stores and the wide register map of DBL64.

The graph: uniform random CSR, 4 000 x 4 000, ~48 entries per row -- three row tiles of the 8 x 228 geometry (not a multiple of an XCD
group: the last group of workgroups has tiles missing), 32 chunks of 128 columns (the ring of five wraps six times), streams of tens of
KiB (dozens of touches each)."""
import numpy as np
import pytest
import torch

import oracle
from conftest import random_csr
from pygim_amd import _lib

pytestmark = pytest.mark.gpu
N, AVG = 4000, 48
ARRANGEMENTS = [(share, sx) for share in (0, 1) for sx in (1, 2, 4)]   # share = 0 first: the run the others are compared with


@pytest.fixture(scope="module", autouse=True)
def backend():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.init_ranks(1)
    old = _lib.set_tunable("lds_mode", 1)   # the LDS-staged plan whenever one can be made (as the small code-stream tests force it)
    yield
    _lib.set_tunable("lds_mode", old)
    _lib.release()


@pytest.fixture(scope="module")
def graph():
    rng = np.random.default_rng(20240607)
    rowptr, col = random_csr(rng, N, N, AVG, empty_frac=0.0)
    rp, ci = torch.from_numpy(rowptr.astype(np.int32)).cuda(), torch.from_numpy(col.astype(np.int32)).cuda()
    return rng, rowptr, col, rp, ci


def create(graph, code, h, round_tiles=0):
    """round_tiles = 0: tiles of the geometry's full height (three of 1 824 rows; long streams), not the many light ones that fill one round of workgroups"""
    _, _, col, rp, ci = graph
    old = _lib.set_tunable("lds_round_tiles", round_tiles)
    try:
        hd = _lib.group_create(_lib.CSR, code, [rp.data_ptr()], [ci.data_ptr()], None, [N], [N], [len(col)], [1], [h], h)
    finally:
        _lib.set_tunable("lds_round_tiles", old)
    assert _lib.group_lds_plan(hd)["tiles"] > 0 and _lib.group_lds_code(hd)["active"] == 1, _lib.group_lds_note(hd)
    assert _lib.group_lds_geometry(hd)["waves"] == 8
    return hd


def every_arrangement(hd, run, nslices, shareable=True):
    """run() under lds_touch_share x lds_xcd_slices; the geometry report must name the arrangement the launch takes"""
    old = _lib.set_tunable("lds_touch_share", 0), _lib.set_tunable("lds_xcd_slices", 0)
    outs = {}
    try:
        for share, sx in ARRANGEMENTS:
            _lib.set_tunable("lds_touch_share", share)
            _lib.set_tunable("lds_xcd_slices", sx)
            geo = _lib.group_lds_geometry(hd)
            sx_eff = sx if (nslices in (2, 4, 8) and sx <= nslices and nslices % sx == 0) else 1
            assert geo["xcd_slices"] == sx_eff and geo["touch_share"] == (1 if (share and sx_eff > 1 and shareable) else 0), (share, sx, geo)
            outs[(share, sx)] = run()
    finally:
        _lib.set_tunable("lds_touch_share", old[0])
        _lib.set_tunable("lds_xcd_slices", old[1])
    return outs


def plain_product(graph, code, x, nslices, tiles=None, round_tiles=0):
    _, rowptr, col, _, _ = graph
    h = x.shape[1]
    want = oracle.spmm_csr(rowptr, col, None, x)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    hd = create(graph, code, h, round_tiles)
    try:
        if tiles is not None:
            assert _lib.group_lds_plan(hd)["tiles"] == tiles, _lib.group_lds_plan(hd)
        if tiles is not None and nslices == 4:
            assert _lib.group_lds_geometry(hd)["chunk_cols"] * 32 >= N > _lib.group_lds_geometry(hd)["chunk_cols"] * 31, _lib.group_lds_geometry(hd)

        def run():
            out = torch.full((N, h), 77, dtype=xd.dtype, device="cuda")
            _lib.spmm_run_group(hd, [xd.data_ptr()], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.cpu().numpy()

        outs = every_arrangement(hd, run, nslices)
    finally:
        _lib.group_free(hd)
    for key, out in outs.items():
        assert out.tobytes() == want.tobytes(), (code, h, key, "against the oracle")
        assert out.tobytes() == outs[(0, key[1])].tobytes(), (code, h, key, "against lds_touch_share = 0")


@pytest.mark.parametrize("h", [128, 192, 256])
def test_flt32_is_bit_identical_under_every_arrangement(graph, h):
    x = (graph[0].random((N, h), dtype=np.float32) * 2 - 1).astype(np.float32)   # U(-1, 1): sums round at every step
    plain_product(graph, _lib.FLT32, x, nslices=h // 64, tiles=3)


def test_flt32_light_tiles_of_one_round(graph):
    """the default tile height: 64 tiles x 4 slices = one workgroup per compute unit, short streams (a few touches each)"""
    x = (graph[0].random((N, 256), dtype=np.float32) * 2 - 1).astype(np.float32)
    plain_product(graph, _lib.FLT32, x, nslices=4, round_tiles=1)


def test_int32_is_bit_identical_under_every_arrangement(graph):
    x = graph[0].integers(-2**31, 2**31 - 1, size=(N, 256), dtype=np.int64).astype(np.int32)   # sums wrap
    plain_product(graph, _lib.INT32, x, nslices=4)


@pytest.mark.parametrize("h,nslices", [(64, 1), (128, 2)])
def test_dbl64_wide_register_map(graph, h, nslices):
    """register pairs: 2 x 5 pairs of x registers end at v25, the touch register is free here too; one slice per XCD at h = 64 (every wave
    touches), pairs at h = 128 when lds_xcd_slices asks for them"""
    x = graph[0].random((N, h)) * 2 - 1
    plain_product(graph, _lib.DBL64, x, nslices=nslices)


@pytest.mark.parametrize("code,dt", [("INT8", np.int8), ("INT32", np.int32), ("FLT32", np.float32)])
def test_dequantising_store_is_bit_identical_under_every_arrangement(graph, code, dt):
    """quantise -> aggregate -> dequantise in one call (k_lds_code8_i8_deq: two slices of 128 features; k_lds_code8_i32_deq and k_lds_code8_f32_deq: four)"""
    rng, rowptr, col, _, _ = graph
    h = 256
    xf = rng.standard_normal((N, h)).astype(np.float32)
    s_ref, xq = oracle.symmetric_quantize(xf, dt)
    want = oracle.symmetric_dequantize(oracle.spmm_csr(rowptr, col, None, xq), 1.0, s_ref)
    xd = torch.from_numpy(xf).cuda()
    hd = create(graph, getattr(_lib, code), h)
    try:
        def run():
            out = torch.full((N, h), float("nan"), dtype=torch.float32, device="cuda")
            scale = torch.empty(1, dtype=torch.float32, device="cuda")
            _lib.quant_spmm_run(hd, xd.data_ptr(), h, out.data_ptr(), scale.data_ptr())
            torch.cuda.synchronize()
            assert np.float32(scale.item()) == s_ref
            return out.cpu().numpy()

        outs = every_arrangement(hd, run, nslices=2 if dt == np.int8 else 4)
    finally:
        _lib.group_free(hd)
    for key, out in outs.items():
        assert out.tobytes() == want.tobytes(), (code, key, "against the oracle")
        assert out.tobytes() == outs[(0, key[1])].tobytes(), (code, key, "against lds_touch_share = 0")
