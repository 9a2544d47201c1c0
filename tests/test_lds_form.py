"""CPU: which LDS-staged form a part gets is a pure function (pygim_amd/csrc/lds_form.hpp lds_choose_form) -- asked here without a device.

tests/native/lds_form_main.cpp puts the chooser behind a command line.  It must say what the library said on an MI355X for every case of
tests/golden/lds_form_record.json (written by scripts/exp_lds_form.py: the answers of the commit BEFORE the chooser existed, read through
group_lds_geometry / _plan / _code / _note), and what the documents quote for the two shapes they quote.
"""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

_SRC = os.path.join(ROOT, "tests", "native", "lds_form_main.cpp")
_BIN = os.path.join(ROOT, "tests", "native", "lds_form")
_CSRC = os.path.join(ROOT, "pygim_amd", "csrc")
_RECORD = os.path.join(ROOT, "tests", "golden", "lds_form_record.json")
DTYPES = {"INT8": (0, 1), "INT16": (1, 2), "INT32": (2, 4), "INT64": (3, 8), "FLT32": (4, 4), "DBL64": (5, 8)}   # code, bytes


@pytest.fixture(scope="module")
def chooser():
    deps = [_SRC, os.path.join(_CSRC, "lds_form.hpp"), os.path.join(_CSRC, "lds_plan.hpp")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(_BIN) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", _SRC, "-o", _BIN])   # plain g++: the header needs no device compiler

    def ask(lines):
        out = subprocess.run([_BIN, "-"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: (v.strip('"') if v.startswith('"') else float(v) if "." in v or "e" in v else int(v)) for k, v in re.findall(r'(\w+)=("[^"]*"|\S+)', ln)} for ln in out]

    return ask


def _line(dtype, nrows, ncols, nnz, h, cus=256, valued=False, allow_code=True, **knobs):
    code, es = DTYPES[dtype]
    fields = dict(dtype=code, val_es=es, nrows=nrows, ncols=ncols, nnz=nnz, h_hint=h, cu_count=cus, valued=int(valued), allow_code=int(allow_code), **knobs)
    return " ".join(f"{k}={v}" for k, v in fields.items())


def test_self_check_of_the_harness(chooser):
    # the quoted shapes and a sweep of 12 M inputs against the chooser's invariants (the run that is also made under ASan + UBSan)
    assert "all within the invariants" in subprocess.run([_BIN], capture_output=True, text=True, check=True).stdout


def test_a_share_that_all_but_fits_one_workgroup_per_cu_leaves_its_last_rows_to_the_tail(chooser):
    # 256 CUs, INT32, h = 256 (4 slices): 16 full tiles x 4 slices x 4 ranges = 256 workgroups hold 29 184 of the 29 384 rows;
    # without the tail all rows need 17 tiles: 17 x 4 x 3 = 204 workgroups
    tail, whole = chooser([_line("INT32", 29384, 40000, 1100000, 256), _line("INT32", 29384, 40000, 1100000, 256, lds_row_tail=0)])
    assert (tail["plan"], tail["col_splits"], tail["rows_lds"], tail["covered_rows"]) == (1, 4, 29184, 29184)
    assert (whole["plan"], whole["col_splits"], whole["rows_lds"], whole["covered_rows"]) == (1, 3, 29384, 0)


def test_the_reddit_shaped_product_is_two_whole_rounds_of_workgroups(chooser):
    (f,) = chooser([_line("FLT32", 232965, 232965, 114615892, 256)])
    assert (f["plan"], f["code"], f["waves"], f["acc_per_wave"], f["buffers"], f["chunk_cols"], f["boundary"], f["col_splits"]) == (1, 1, 8, 228, 5, 128, 1, 1)
    assert f["rows_per_tile"] == 1821 and -(-232965 // 1821) == 128 and 128 * 4 == 2 * 256


def test_the_chooser_says_what_the_library_said_on_the_device(chooser):
    rec = json.load(open(_RECORD))
    cases = rec["cases"]
    assert len(cases) >= 40

    def line(c, allow_code):
        return _line(c["dtype"], c["nrows"], c["ncols"], c["nnz"], c["h"], rec["cu_count"], c["valued"], allow_code, **c["tunables"])

    first = chooser([line(c, True) for c in cases])
    second = chooser([line(c, False) for c in cases])
    for c, f1, f2 in zip(cases, first, second):
        # build_lds_plan's ladder, whose failures are injected in the builder: a code stream that cannot be generated (1) or placed (2)
        # takes the token form of the same product; a schedule that cannot be built (4) leaves the sweep
        fail = c["tunables"].get("lds_fail", 0)
        f = f2 if f1["plan"] and f1["code"] and fail & 3 else f1
        plan = f["plan"] and not fail & 4
        want, geo = c["parent"], c["parent"]["geometry"]
        assert plan == (want["plan"]["tiles"] > 0), c["name"]
        if not plan:
            continue
        got = (f["waves"], f["acc_per_wave"], f["chunk_cols"], f["buffers"], f["col_splits"], f["code"], f["covered_rows"], f["half_H"])
        assert got == (geo["waves"], geo["acc_per_wave"], geo["chunk_cols"], geo["buffers"], geo["col_splits"], want["code"]["active"], want["covered_rows"],
                       want["half_H"]), c["name"]
        # the device generator wrote the stream exactly where the chooser allows it and the generator covers the plan (the note says when not)
        assert want["code"]["device_generated"] == (f["device_codegen"] and "written by the host encoder" not in want["note"]), c["name"]


def test_the_chooser_is_host_only_and_the_builder_says_things_once():
    header = open(os.path.join(_CSRC, "lds_form.hpp")).read()
    for word in ("hip", "g_tune", "g_ctx", "t_plan_dtype"):
        assert word not in header, word
    builder = open(os.path.join(_CSRC, "rt_plans.inc")).read()
    for once in ("LDS_CODE_ADD_F64", "p.lds_code_piece =", "p.lds_nbuf =", "p.lds_ka ="):
        assert builder.count(once) <= 1 and (header + builder).count(once) >= 1, once
