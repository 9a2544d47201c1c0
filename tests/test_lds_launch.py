"""CPU: how a product runs on an LDS-staged plan is a set of pure functions (pygim_amd/csrc/lds_launch.hpp: lds_staged, lds_xcd_layout, lds_takes,
lds_plan_launch) -- asked here without a device.

tests/native/lds_launch_main.cpp puts them behind a command line.  The XCD layout must be what the library reported on an MI355X for every case of
tests/golden/lds_form_record.json that has a plan (the record holds every input of the rule: tiles, chunk fills, chunk columns, waves, the code
stream's read groups and register sets, code or not, the half-split, element type, width and columns; lds_xcd_layout's text is unchanged since the
record's commit, it only moved), and the launches of the shapes the documents quote must be what a hand derivation gives.
"""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

_SRC = os.path.join(ROOT, "tests", "native", "lds_launch_main.cpp")
_BIN = os.path.join(ROOT, "tests", "native", "lds_launch")
_CSRC = os.path.join(ROOT, "pygim_amd", "csrc")
_RECORD = os.path.join(ROOT, "tests", "golden", "lds_form_record.json")
DTYPES = {"INT8": (0, 1), "INT16": (1, 2), "INT32": (2, 4), "INT64": (3, 8), "FLT32": (4, 4), "DBL64": (5, 8)}   # code, bytes


@pytest.fixture(scope="module")
def rules():
    deps = [_SRC] + [os.path.join(_CSRC, h) for h in ("lds_launch.hpp", "lds_form.hpp", "lds_plan.hpp")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(_BIN) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", _SRC, "-o", _BIN])   # plain g++: the header needs no device compiler

    def ask(lines):
        out = subprocess.run([_BIN, "-"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: (v.strip('"') if v.startswith('"') else int(v)) for k, v in re.findall(r'(\w+)=("[^"]*"|\S+)', ln)} for ln in out]

    return ask


def _line(**fields):
    return " ".join(f"{k}={int(v)}" for k, v in fields.items())


def _code8(dtype, w, ntiles, nrows, ncols, slots, **more):
    """an 8-wave code-stream plan on a ring of 128-column chunks (what the chooser gives the wide 4-byte products), C aligned and as wide as the product"""
    return _line(dtype=DTYPES[dtype][0], w=w, ldc=w, c_aligned16=1, c_addr=4096, has_plan=1, is_code=1, nw=8, batch=8, kc=128, ntiles=ntiles, nrows=nrows, ncols=ncols,
                 slots=slots, **more)


def test_self_check_of_the_harness(rules):
    # the quoted shapes, then every plan of the chooser on a grid through the launch rules (the run that is also made under ASan + UBSan): what lds_takes
    # accepts lds_plan_launch launches, the scratch layout's two uses agree, no launch is empty
    out = subprocess.run([_BIN], capture_output=True, text=True, check=True).stdout
    assert "all within the invariants" in out and "none refused" in out


def test_the_layout_is_what_the_library_reported_on_the_device(rules):
    rec = json.load(open(_RECORD))
    cases = [c for c in rec["cases"] if c["parent"]["plan"]["tiles"] > 0]
    assert len(cases) >= 35
    lines = []
    for c in cases:
        par, geo = c["parent"], c["parent"]["geometry"]
        code, es = DTYPES[c["dtype"]]
        knobs = {k: v for k, v in c["tunables"].items() if k in ("lds_xcd_slices", "lds_touch_share", "lds_code")}
        lines.append(_line(dtype=code, w=c["h"], ldc=c["h"], has_plan=1, is_code=par["code"]["active"], nw=geo["waves"], kc=geo["chunk_cols"],
                           row_bytes=512 if es == 8 else 256, col_splits=geo["col_splits"], half=par["half_H"], ntiles=par["plan"]["tiles"],
                           slots=par["plan"]["chunk_fills"], code_gsize=geo["group"], code_nsets=geo["x_sets"], nrows=c["nrows"], ncols=c["ncols"], **knobs))
    for c, got in zip(cases, rules(lines)):
        assert (got["xcd_sx"], got["touch_share"]) == (c["parent"]["geometry"]["xcd_slices"], c["parent"]["geometry"]["touch_share"]), c["name"]


def test_the_reddit_shaped_product_is_two_whole_rounds_of_workgroups(rules):
    # FLT32, h = 256: 4 slices of 64 features; 128 tiles that stream every one of their 1 821 chunks -> two slices per XCD, groups of 8 / 4 * 2 = 4 XCDs,
    # 8 * ceil(128 / 4) * 2 workgroups
    (f,) = rules([_code8("FLT32", 256, 128, 232965, 232965, 128 * 1821)])
    assert (f["takes"], f["refusal"], f["nslices"], f["eps"], f["xcd_sx"], f["xcd_group"], f["touch_share"]) == (1, "", 4, 64, 2, 4, 1)
    assert f["grid"] == 8 * -(-128 // 4) * 2 == 512 == 2 * 256 and f["block"] == 512
    assert (f["reduce"], f["tail"], f["scratch_bytes"]) == (0, 0, 0)


def test_a_row_share_parks_its_tail_sums_exactly_behind_its_partial_sums(rules):
    # 1/8 row share, INT32, h = 256: 16 row tiles x 4 column ranges hold 29 184 of 29 384 rows and fill a quarter of their chunks (5 008 of 64 x 313) -> all four
    # slices on one XCD, groups of 8, 8 * ceil(64 / 8) * 4 workgroups.  Partial sums: 4 ranges x 29 184 rows x 256 features x 4 bytes; the parked block starts there
    share = dict(col_splits=4, rows=29184, tail_tables=1, tail_nseg=200)
    f, odd = rules([_code8("INT32", 256, 64, 29384, 40000, 5008, **share),
                    _code8("INT32", 256, 64, 29384, 40000, 5008, **share).replace("c_aligned16=1", "c_aligned16=0")])
    assert (f["takes"], f["refusal"], f["xcd_sx"], f["xcd_group"], f["grid"]) == (1, "", 4, 8, 256)
    assert f["split_bytes"] == 4 * 29184 * 256 * 4 == 119537664 and f["split_bytes"] % 256 == 0
    assert f["scratch_bytes"] == f["split_bytes"] + f["park_bytes"] and f["park_bytes"] >= 200 * 4 * 64 * 4
    assert (f["to_scratch"], f["accumulate"], f["ldc_bytes"], f["tail"], f["ntail"], f["lds_rows"]) == (1, 0, 1024, 1, 200, 29184)
    assert (f["reduce"], f["reduce_total"]) == (4, 29184 * 64)        # k_lds_reduce_v4: four features a thread
    assert (odd["reduce"], odd["reduce_total"]) == (6, 29184 * 256)   # C off a 16-byte boundary: k_lds_reduce


def test_the_staged_copy_of_the_narrowest_the_widest_and_the_half_split(rules):
    int8, dbl, half = rules([
        _line(dtype=0, w=256, ldc=256, c_addr=4096, has_plan=1, is_code=1, nw=8, kc=128, ntiles=2, nrows=2500, ncols=30000, slots=470),
        _line(dtype=5, w=64, ldc=64, c_addr=4096, has_plan=1, is_code=1, nw=8, kc=64, row_bytes=512, ntiles=9, nrows=8192, ncols=4096, slots=576),
        _line(dtype=2, w=32, ldc=32, c_addr=4096, has_plan=1, is_code=1, nw=8, kc=128, half=10112, col_splits=8, ntiles=88, nrows=20000, ncols=20000, slots=869),
    ])
    # INT8: widened to 16 bits, 2 slices of 128 elements, kind 3, on the INT8 stores of the INT16 stream
    assert (int8["nslices"], int8["eps"], int8["row_bytes"], int8["kind"], int8["takes"], int8["refusal"], int8["shell"], int8["el"]) == (2, 128, 256, 3, 1, "", 5, 0)
    # DBL64: one 512-byte slice, one slice per XCD
    assert (dbl["nslices"], dbl["eps"], dbl["row_bytes"], dbl["slice_stride"], dbl["kind"], dbl["xcd_sx"], dbl["takes"], dbl["refusal"]) == (1, 64, 512, 4096 * 512, 1, 1, 1, "")
    # half-split: one slice, H padded rows, kind 5, the store adds the halves
    assert (half["nslices"], half["rows_pad"], half["kind"], half["half_split"], half["xcd_sx"], half["takes"], half["refusal"]) == (1, 10112, 5, 1, 1, 1, "")


def test_the_rules_are_host_only_and_the_runtime_keeps_no_slice_arithmetic():
    header = open(os.path.join(_CSRC, "lds_launch.hpp")).read()
    for word in ("hip", "g_tune", "g_ctx"):
        assert word not in header, word
    runtime = "".join(open(os.path.join(_CSRC, f)).read() for f in ("rt_launch.inc", "rt_run.inc", "pygim_hip.hip"))
    for spelled in ("256 / sizeof", "? 512 : 256", "uint64_t lds_rows_pad("):
        assert spelled not in runtime, spelled
    assert "want_lds" not in runtime and header.count("inline uint64_t lds_rows_pad(") == 1
