"""CPU: what one call of a group product does is a set of pure functions (pygim_amd/csrc/run_plan.hpp: run_windows, place_runs, plan_host_pipeline,
plan_products) -- asked here without a device.

tests/native/run_plan_main.cpp puts them behind a command line.  The shapes the documents quote must plan as a hand derivation gives; the window count must
be what tests/test_parity_gpu.py predicts from its own restatement of the rule (and then reads back from the device); the product plan of a small grid is
asserted copy by copy.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

_SRC = os.path.join(ROOT, "tests", "native", "run_plan_main.cpp")
_BIN = os.path.join(ROOT, "tests", "native", "run_plan")
_CSRC = os.path.join(ROOT, "pygim_amd", "csrc")
ALIAS = 0x7F0000000000   # the page-locked result as the kernels see it: on a 256-byte boundary
REDDIT = dict(es=4, is_float=1, h=256, total_rows=232965, ncols=[232965], dense=[256], out_pinned=1, out_alias=ALIAS, stage_out=0x20000000)


@pytest.fixture(scope="module")
def plan():
    deps = [_SRC, os.path.join(_CSRC, "run_plan.hpp")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(_BIN) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", _SRC, "-o", _BIN])   # plain g++: the header needs no device compiler

    def ask(cases):
        lines = [_line(**c) for c in cases]
        out = subprocess.run([_BIN, "-"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [_parsed(ln) for ln in out]

    return ask


def _line(**fields):
    def text(v):
        if isinstance(v, dict):
            return ",".join(f"{k}:{int(x)}" for k, x in v.items())
        if isinstance(v, (list, tuple)):
            return ",".join(str(int(x)) for x in v)
        return str(int(v))

    return " ".join(f"{k}={text(v)}" for k, v in fields.items())


def _parsed(line):
    got = {k: (v.strip('"') if v.startswith('"') else int(v)) for k, v in re.findall(r'(\w+)=("[^"]*"|\S+)', line)}
    rows = lambda s: [tuple(int(x) for x in item.split(":")) for item in s.split("|")] if s else []
    if got["refusal"]:
        return got
    got["geometry"] = rows(got["geometry"])     # (rows, ld, width) per window
    got["products"] = rows(got["products"])     # (part, in_place, base, ldx, ccol, width, accumulate, copy0, copy1)
    got["copies"] = rows(got["copies"])         # (dst_off, window, src_off, width, rows)
    host = []
    for item in got["host"].split("|") if got["host"] else []:
        head, *pieces = item.split("/")
        acol, w, pitch, dev_off, xcat_ld = (int(x) for x in head.split(":"))
        host.append(dict(acol=acol, w=w, pitch=pitch, dev_off=dev_off, xcat_ld=xcat_ld, pieces=[tuple(int(x) for x in p.split(":")) for p in pieces]))   # (acol, w, pitch, dev_off)
    got["host"] = host
    return got


def _cut(p):
    return [(q["acol"], q["w"]) for q in p["host"]]


def test_self_check_of_the_harness(plan):
    # every plan of a sweep over element sizes, widths, splits, strides, both conventions, the tunables and random writes_once tables (the run that is also
    # made under ASan + UBSan): windows disjoint, in order, covering [0, h), at most 16; offsets and copies inside the sizes asked for; every column of C
    # written once per part, added to from the second part on; a direct plan has only writes_once windows
    out = subprocess.run([_BIN], capture_output=True, text=True, check=True).stdout
    assert "all within the invariants" in out
    counts = [int(x) for x in re.findall(r"(\d+) ", out)]
    assert all(c > 0 for c in counts), out


def test_the_reddit_shaped_host_call_is_two_windows_of_128_features(plan):
    # FLT32, h = 256: 1024 bytes of a row / 512 per window = 2 windows, each two whole 256-byte slices; X and C are 238.6 MB each; nothing forced
    auto, four, pageable, small_x, small_c = plan([
        REDDIT,
        dict(REDDIT, host_windows=4),
        dict(REDDIT, out_pinned=0, out_alias=0),
        dict(REDDIT, ncols=[32767]),         # X: 32 767 x 1024 bytes, 1 KB short of 32 MB
        dict(REDDIT, total_rows=32767)])     # C likewise
    assert _cut(auto) == [(0, 128), (128, 128)] and auto["direct"] == 0 and auto["need_pinned"] == 1 and auto["need_alias"] == 0
    assert [(q["pitch"], q["dev_off"], q["pieces"]) for q in auto["host"]] == [(256, 0, []), (256, 512, [])]   # (windows of the one matrix in stage_in, at its stride)
    assert auto["stage_in_bytes"] == (232965 * 1024 + 255) // 256 * 256 and auto["host_xcat_bytes"] == 0
    assert _cut(four) == [(0, 64), (64, 64), (128, 64), (192, 64)] and four["need_pinned"] == 0
    assert pageable["windows"] == 0 and small_x["windows"] == 0 and small_c["windows"] == 0
    assert (small_x["need_pinned"], small_c["need_pinned"]) == (0, 0)   # (not asked where the sizes already say no)
    (exact,) = plan([dict(REDDIT, ncols=[32768], total_rows=32768)])   # exactly 32 MB both ways
    assert exact["windows"] == 2


def test_a_width_that_is_no_multiple_of_the_slice(plan):
    # h = 200 of 4-byte elements: S = 4 slices of 64; host_windows = 3 -> min(3, 4) windows of S / n + (k < S % n) = 2, 1, 1 slices, the last cut at h
    small = dict(es=4, h=200, total_rows=700, ncols=[700], dense=[200])
    three, many, one = plan([dict(small, host_windows=3), dict(small, host_windows=9), dict(small, host_windows=1)])
    assert _cut(three) == [(0, 128), (128, 64), (192, 8)]
    assert _cut(many) == [(0, 64), (64, 64), (128, 64), (192, 8)]   # no more windows than slices
    assert one["windows"] == 0


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_the_window_count_test_parity_gpu_predicts(plan, es):
    # tests/test_parity_gpu.py test_host_operands_as_a_pipeline_of_feature_windows: its shapes, its formula
    n = 700
    cases, want = [], []
    for h, ncols in ((256, [n]), (200, [n]), (320, [250, 1, 449])):
        slices = (h * es + 255) // 256
        for ds_parts in (1, 3):
            chunk = -(-h // ds_parts)
            widths = [min(chunk, h - a) for a in range(0, h, chunk)]   # torch.chunk
            for hw in (1, 2, 3, 4):
                cases.append(dict(es=es, is_float=es >= 4, h=h, total_rows=n, ncols=ncols, dense=widths, has_merged=len(ncols) > 1, host_windows=hw, once_default=0))
                if hw == 1:
                    want.append(1)
                elif ds_parts == 1:
                    want.append(min(hw, slices))
                elif all(wk * es >= 512 for wk in widths):
                    want.append(len(widths))
                else:
                    target, cur, count = -(-h // hw), 0, 0
                    for i, wk in enumerate(widths):
                        cur += wk
                        if cur >= target or i + 1 == len(widths):
                            count, cur = count + 1, 0
                    want.append(count)
    got = [max(p["windows"], 1) for p in plan(cases)]
    assert got == want


@pytest.mark.parametrize("es", [1, 4, 8])
def test_grandes_per_unit_windows_are_gathered(plan, es):
    # tests/test_parity_gpu.py test_grande_windows_with_host_operands_...: eight windows of `pad` columns each (ld = pad > width for most)
    n, units, mul = 900, 8, 8 // es
    cases = []
    for h in (256, 100):
        widths = [h // units + (1 if u < h % units else 0) for u in range(units)]
        pad = (widths[0] + mul - 1) // mul * mul
        for hw in (1, 2, 3):
            cases.append(dict(es=es, is_float=es >= 4, h=h, total_rows=n, ncols=[n], dense=widths, ld=[pad] * units, per_part=1, host_windows=hw, once_default=0))
    for c, p in zip(cases, plan(cases)):
        if c["host_windows"] == 1:
            assert p["windows"] == 0
            continue
        h = c["h"]
        assert 2 <= p["windows"] <= units
        ldc = p["host"][0]["xcat_ld"]
        assert (ldc * es) % 16 == 0 and h <= ldc < h + 16 and p["host_xcat_bytes"] == n * ldc * es
        pieces = [pc for q in p["host"] for pc in q["pieces"]]
        assert len(pieces) == units and [pc[1] for pc in pieces] == c["dense"]
        col = 0
        for acol, w, pitch, dev_off in pieces:   # the pieces' destination columns tile [0, h)
            assert acol == col and pitch == c["ld"][0] and dev_off % 256 == 0
            col += w
        assert col == h
        assert [q["acol"] for q in p["host"]] == [q["pieces"][0][0] for q in p["host"]] and sum(q["w"] for q in p["host"]) == h


def test_direct_mode(plan):
    forced = dict(REDDIT, host_windows=2, host_direct=2)
    always, one_window_not, off_boundary, full_width_not, adaptive, adaptive_slow, never = plan([
        forced,
        dict(forced, once={128: 0}),             # a window's product is not the one-pass kernel's: the second attempt, the copies, the same windows
        dict(forced, out_alias=ALIAS + 64),
        dict(forced, once={256: 0}),             # decided on the full width first
        dict(forced, host_direct=1),
        dict(forced, host_direct=1, copies_slow=1),
        dict(forced, host_direct=0, copies_slow=1)])
    assert always["direct"] == 1 and always["need_alias"] == 1 and _cut(always) == [(0, 128), (128, 128)]
    assert one_window_not["direct"] == 0 and one_window_not["host"] == always["host"]
    assert off_boundary["direct"] == 0 and full_width_not["direct"] == 0
    assert (adaptive["direct"], adaptive["need_alias"]) == (0, 0) and (adaptive_slow["direct"], adaptive_slow["need_alias"]) == (1, 1)
    assert (never["direct"], never["need_alias"]) == (0, 0)
    # the caller's own blocks as windows (INT8, 512 bytes of a row and more): the second starts at column 520, off a 16-byte boundary; at 528 it does not
    blocks = dict(es=1, total_rows=700, ncols=[700], out_pinned=1, out_alias=ALIAS, host_windows=2, host_direct=2)
    off16, on16 = plan([dict(blocks, h=1040, dense=[520, 520]), dict(blocks, h=1040, dense=[528, 512])])
    assert _cut(off16) == [(0, 520), (520, 520)] and off16["direct"] == 0
    assert _cut(on16) == [(0, 528), (528, 512)] and on16["direct"] == 1


def test_float_products_keep_the_serial_calls_bits(plan):
    # left to itself (host_windows = 0) a float product is pipelined only where every window's product is the LDS-staged kernel's
    dbl = dict(REDDIT, es=8)   # 2048 bytes of a row: four windows of 64
    f_gated, f_forced, f_fine, i_never, d_gated, d_fine = plan([
        dict(REDDIT, once={128: 0}),
        dict(REDDIT, once={128: 0}, host_windows=2),
        REDDIT,
        dict(REDDIT, is_float=0, once_default=0),
        dict(dbl, once={64: 0}),
        dbl])
    assert f_gated["windows"] == 0 and d_gated["windows"] == 0
    assert _cut(f_forced) == _cut(f_fine) == _cut(i_never) == [(0, 128), (128, 128)]
    assert _cut(d_fine) == [(0, 64), (64, 64), (128, 64), (192, 64)]


def test_a_window_stride_below_its_width_is_refused_in_the_per_part_convention(plan):
    (p,) = plan([dict(es=4, h=100, total_rows=300, ncols=[300], dense=[60, 40], ld=[60, 39], per_part=1)])
    assert p["refusal"] == "window stride smaller than its width"


BASE = 0x40000000
PARTS = dict(es=4, h=100, total_rows=300, ncols=[120, 180], dense=[40, 33, 27])


@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
def test_products_of_windows_that_sit_side_by_side_are_taken_in_place(plan, merge, fuse):
    # three views of one row-major matrix of 300 x 100, both sparse parts read their row range of it
    views = dict(PARTS, ld=[100] * 3, addr=[BASE, BASE + 160, BASE + 292], has_merged=1, merge_parts=merge, fuse_windows=fuse)
    (p,) = plan([views])
    assert p["copies"] == [] and p["xcat_bytes"] == 0
    second = BASE + 120 * 100 * 4   # the second part's rows
    if merge:
        assert p["products"] == [(-1, 1, BASE, 100, 0, 100, 0, 0, 0)]
    elif fuse:
        assert p["products"] == [(0, 1, BASE, 100, 0, 100, 0, 0, 0), (1, 1, second, 100, 0, 100, 1, 0, 0)]
    else:
        assert p["products"] == [(i, 1, b + off, 100, ccol, w, i, 0, 0) for i, b in ((0, BASE), (1, second)) for off, ccol, w in ((0, 0, 40), (160, 40, 33), (292, 73, 27))]


@pytest.mark.parametrize("per_part", [0, 1])
def test_products_of_windows_with_gaps_go_through_xcat(plan, per_part):
    # ld = width + 3.  Shared convention: three windows of 300 rows, part 1 reads from row 120 on.  Per-part: six windows, windows 3..5 hold part 1's 180 rows.
    lds = [43, 36, 30]
    gaps = dict(PARTS, ld=lds * (2 if per_part else 1), per_part=per_part, has_merged=1)
    merged, fused, single, narrow = plan([gaps, dict(gaps, merge_parts=0), dict(gaps, merge_parts=0, fuse_windows=0), dict(gaps, es=1)])
    dst = [0, 160, 292]
    src1 = [0, 0, 0] if per_part else [120 * ld * 4 for ld in lds]   # per-part windows start at their own row 0
    win1 = [3, 4, 5] if per_part else [0, 1, 2]
    part0 = [(dst[j], j, 0, PARTS["dense"][j], 120) for j in range(3)]
    # merged: ONE product; the second part's windows start at row ncols[0] = 120 of xcat (row stride 100 elements = 400 bytes, already a multiple of 16)
    assert merged["products"] == [(-1, 0, 0, 100, 0, 100, 0, 0, 6)] and merged["xcat_bytes"] == 300 * 400
    assert merged["copies"] == part0 + [(120 * 400 + dst[j], win1[j], src1[j], PARTS["dense"][j], 180) for j in range(3)]
    # fused: a product per part, each laying its windows at row 0 of xcat, the second adding to C
    assert fused["products"] == [(0, 0, 0, 100, 0, 100, 0, 0, 3), (1, 0, 0, 100, 0, 100, 1, 3, 6)] and fused["xcat_bytes"] == 180 * 400
    assert fused["copies"] == part0 + [(dst[j], win1[j], src1[j], PARTS["dense"][j], 180) for j in range(3)]
    # a product per window: nothing is laid anywhere
    assert single["copies"] == [] and single["xcat_bytes"] == 0 and [q[0:2] + q[3:7] for q in single["products"]] == [
        (i, 1, lds[j], (0, 40, 73)[j], PARTS["dense"][j], i) for i in (0, 1) for j in range(3)]
    # INT8: 100 bytes of a row are rounded up to 112
    assert narrow["products"][0][3] == 112 and narrow["xcat_bytes"] == 300 * 112 and narrow["copies"][3][0] == 120 * 112


def test_the_rules_are_host_only_and_the_layout_is_written_once():
    header = open(os.path.join(_CSRC, "run_plan.hpp")).read()
    for word in ("hip", "g_tune", "g_ctx", "Group *", "Part &"):
        assert word not in header, word
    rounding = "+ 15) & ~(size_t)15) /"
    assert header.count(rounding) == 1
    runtime = "".join(open(os.path.join(_CSRC, f)).read() for f in ("rt_launch.inc", "rt_run.inc", "rt_plans.inc", "rt_state.inc", "pygim_hip.hip"))
    assert rounding not in runtime
    assert "struct HostWindow" not in runtime and "struct HostPiece" not in runtime
