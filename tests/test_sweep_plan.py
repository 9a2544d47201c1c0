"""CPU: what the plan of the L2 sweep holds is a set of pure functions (pygim_amd/csrc/sweep_plan.hpp: sweep_panel_count, sweep_heavy_rows,
sweep_locality_rank, sweep_items, plan_long_rows), and so are creation's argument checks (group_args.hpp) -- asked here without a device.

tests/native/sweep_plan_main.cpp puts them behind a command line.  Every plan is compared, element for element, with tests/sweep_plan_ref.py, a numpy
restatement written from the rules; the panel counts the documents quote must come out as a hand derivation gives; every refusal of a group's creation
comes by text and code, and of two defects the one the library has always reported.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_plan_ref as ref
from conftest import ROOT

_SRC = os.path.join(ROOT, "tests", "native", "sweep_plan_main.cpp")
_BIN = os.path.join(ROOT, "tests", "native", "sweep_plan")
_CSRC = os.path.join(ROOT, "pygim_amd", "csrc")
LISTS = ("base_tasks", "heavy", "segment_tasks", "rows", "beg", "lens", "panel_off", "panel_coop", "panel_long128", "panel_nnz")
INVALID, UNSORTED = 1, 4   # include/pygim_hip.h


@pytest.fixture(scope="module")
def ask():
    deps = [_SRC, os.path.join(_CSRC, "sweep_plan.hpp"), os.path.join(_CSRC, "group_args.hpp")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(_BIN) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", _SRC, "-o", _BIN])   # plain g++: the headers need no device compiler

    def run(lines):
        out = subprocess.run([_BIN, "-"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        got = []
        for ln in out:
            d = {k: v.strip('"') for k, v in re.findall(r'(\w+)=("[^"]*"|\S+)', ln)}
            got.append({k: ([int(x) for x in v.split(",")] if v else []) if k in LISTS else (v if k == "text" else int(v)) for k, v in d.items()})
        return got

    return run


def _line(**fields):
    return " ".join(f"{k}={','.join(str(int(x)) for x in v) if isinstance(v, (list, tuple, np.ndarray)) else int(v)}" for k, v in fields.items())


def csr(rng, nrows, ncols, lengths):
    """rows of the given lengths, columns drawn without repeats and stored in order"""
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    col = np.concatenate([np.sort(rng.choice(ncols, size=n, replace=False)) for n in lengths] + [np.empty(0, dtype=np.int64)])
    return rowptr.astype(np.int64), col.astype(np.int64)


def check(ask, cases):
    """every case (rowptr, col, ncols, settings) planned by the header equals the reference's plan; returns the header's plans"""
    got = ask([_line(nrows=len(rp) - 1, ncols=nc, rowptr=rp, col=ci, **kw) for rp, ci, nc, kw in cases])
    for g, (rp, ci, nc, kw) in zip(got, cases):
        want = ref.plan(rp, ci, nc, **kw)
        for key, value in want.items():
            assert g[key] == value, (key, kw)
    return got


def test_self_check_of_the_harness(ask):
    # random small matrices and knob settings (the run that is also made under ASan + UBSan): every non-heavy row's entries covered exactly once by its
    # items across panels, FIRST and LAST once each, panel_off monotone and ending at n_items, the cooperative prefix and the four length classes true
    # prefixes, panel_nnz adding up to nnz minus the heavy rows' entries
    out = subprocess.run([_BIN], capture_output=True, text=True, check=True).stdout
    assert "all within the invariants" in out
    counts = [int(x) for x in re.findall(r"(\d+) ", out)]
    assert len(counts) == 14 and all(c > 0 for c in counts), out


def test_panel_counts_by_hand(ask):
    rng = np.random.default_rng(1)
    rp, ci = csr(rng, 40, 300, [5] * 40)
    # 128 * 40 bytes: 40 columns a panel, ceil(300 / 40) = 8 panels of ceil(300 / 8) = 38 columns
    eight, = check(ask, [(rp, ci, 300, dict(panel_mode=1, panel_bytes=128 * 40))])
    assert (eight["n_panels"], eight["panel_cols"], eight["ask_sorted"]) == (8, 38, 1)
    # the SpMV budget: h_hint = 4 of 8-byte elements caps a panel at (131072 - 64) / 32 = 4094 columns whatever panel_bytes says
    rp, ci = csr(rng, 30, 9000, [4] * 30)
    big = dict(panel_mode=1, panel_bytes=128 * 100000, es=8)
    four, one, five, no_lds, no_vec = check(ask, [(rp, ci, 9000, dict(big, h_hint=4)), (rp, ci, 9000, dict(big, h_hint=1)), (rp, ci, 9000, dict(big, h_hint=5)),
                                                  (rp, ci, 9000, dict(big, h_hint=4, vec_lds=0)), (rp, ci, 9000, dict(big, h_hint=4, vec_kernel=0))])
    assert (four["n_panels"], four["panel_cols"]) == (3, 3000)          # ceil(9000 / 4094) = 3
    assert (one["n_panels"], one["panel_cols"]) == (1, 9000)            # (131072 - 64) / 8 = 16376 columns
    assert five["n_panels"] == no_lds["n_panels"] == no_vec["n_panels"] == 1
    # ... and by 65536 columns (16-bit panel-local ids) for a narrow type
    rp, ci = csr(rng, 20, 70000, [3] * 20)
    narrow, = check(ask, [(rp, ci, 70000, dict(big, es=1, h_hint=1))])
    assert (narrow["n_panels"], narrow["panel_cols"], narrow["col16"]) == (2, 35000, 1)


def test_panel_mode_and_the_pays_rule(ask):
    rng = np.random.default_rng(2)
    rp, ci = csr(rng, 50, 400, [16] * 50)   # 16 entries a row: 4 panels hold 4 a (row, panel), 2 panels 8
    four = dict(panel_bytes=128 * 100)
    auto_pays, auto_exactly, auto_not, forced, never = check(ask, [
        (rp, ci, 400, dict(four, panel_mode=0, panel_min_seg=3)), (rp, ci, 400, dict(four, panel_mode=0, panel_min_seg=4)),
        (rp, ci, 400, dict(four, panel_mode=0, panel_min_seg=5)), (rp, ci, 400, dict(four, panel_mode=1, panel_min_seg=5)),
        (rp, ci, 400, dict(four, panel_mode=2))])
    assert [p["n_panels"] for p in (auto_pays, auto_exactly, auto_not, forced)] == [4, 4, 1, 4]
    assert (auto_not["plan"], auto_not["ask_sorted"], auto_not["n_items"]) == (1, 0, 50)   # ONE panel, never no plan -- and nothing to ask the device
    assert never["plan"] == 0
    # an empty part has no plan either
    nothing, = check(ask, [(np.zeros(6, dtype=np.int64), np.empty(0, dtype=np.int64), 10, dict(panel_mode=1))])
    assert nothing["plan"] == 0


def test_unsorted_columns_force_one_panel(ask):
    rng = np.random.default_rng(3)
    rp, ci = csr(rng, 60, 500, [7] * 60)
    swapped = ci.copy()
    swapped[[rp[20], rp[20] + 1]] = swapped[[rp[20] + 1, rp[20]]]
    kw = dict(panel_mode=1, panel_bytes=128 * 100)
    sorted_, unsorted = check(ask, [(rp, ci, 500, kw), (rp, swapped, 500, kw)])
    assert (sorted_["n_panels"], unsorted["want_npan"], unsorted["unsorted"], unsorted["n_panels"], unsorted["panel_cols"]) == (5, 5, 1, 1, 500)
    assert unsorted["rows"] == list(range(60)) and unsorted["beg"] == rp[:-1].tolist()   # the rows as they are


def test_items_of_the_length_classes_the_cooperative_prefix_and_empty_rows(ask):
    rng = np.random.default_rng(4)
    # lengths exactly 32, 64, 128, 256 and one more each, exactly the cooperative cap (100) and one more, short rows and empty ones between them
    lengths = [3, 0, 32, 33, 64, 65, 0, 128, 129, 256, 257, 100, 101, 1, 0, 9, 2, 300]
    rp, ci = csr(rng, len(lengths), 400, lengths)
    kw = dict(panel_mode=1, panel_bytes=128 * 400, panel_coop=100)
    one, adding, capped = check(ask, [(rp, ci, 400, kw), (rp, ci, 400, dict(kw, is_extra=1)), (rp, ci, 400, dict(kw, panel_coop=10))])
    assert one["panel_long128"] == [2, 4, 8, 10] and one["panel_coop"] == [6] and one["n_items"] == 18   # 300, 257 | 256, 129 | 128, 101, 100, 65 | 64, 33; above 100: six
    assert one["rows"][:8] == [17, 10, 9, 8, 7, 12, 11, 5] and one["rows"][-3:] == [1, 6, 14]             # 101 is cooperative, 100 is not; the empty rows last, in order
    assert [x >> 30 for x in one["lens"]] == [3] * 18                                                    # one panel: every item is its row's first and last
    assert adding["n_items"] == 15 and set(adding["rows"]) == set(range(18)) - {1, 6, 14}                # a part that only adds has no items of empty rows
    assert capped["panel_coop"] == [8]                                                                   # panel_coop below 64 counts as 64: 65 and longer
    # several panels, a count that does not divide ncols: 400 columns in 3 panels of 134
    three, three_adding = check(ask, [(rp, ci, 400, dict(kw, panel_bytes=128 * 150)), (rp, ci, 400, dict(kw, panel_bytes=128 * 150, is_extra=1))])
    assert (three["n_panels"], three["panel_cols"]) == (3, 134)
    assert [r for r in three["rows"][:three["panel_off"][1]] if lengths[r] == 0] == [1, 6, 14]           # empty rows: items of panel 0 alone
    assert sorted(three["rows"]).count(1) == 1 and 1 not in three_adding["rows"]


def test_a_row_whose_entries_all_lie_in_the_last_panel(ask):
    rp = np.array([0, 4, 7, 9])
    ci = np.array([1, 50, 120, 290, 210, 250, 299, 5, 110])   # row 1: columns 210, 250, 299 -- panel 2 of three panels of 100
    last, = check(ask, [(rp, ci, 300, dict(panel_mode=1, panel_bytes=128 * 100))])
    assert last["n_panels"] == 3 and last["rows"] == [0, 2, 0, 2, 1, 0]
    assert last["lens"] == [2 | ref.FIRST, 1 | ref.FIRST, 1, 1 | ref.LAST, 3 | ref.FIRST | ref.LAST, 1 | ref.LAST]
    assert last["beg"] == [0, 7, 2, 8, 4, 3]


def test_heavy_rows_leave_for_the_segment_kernels(ask):
    rng = np.random.default_rng(5)
    # long_row_threshold = 64 (its floor): a row is heavy from 1025 entries in ONE panel.  2100 columns in 2 panels of 1050
    lengths = [4] * 12
    rp, ci = csr(rng, 12, 2100, lengths)
    rows = [ci[rp[r]:rp[r + 1]] for r in range(12)]
    rows[2] = np.arange(0, 1024)                                   # exactly 16 * 64 in panel 0: stays
    rows[5] = np.arange(0, 1025)                                   # one more: heavy
    rows[7] = np.concatenate([np.arange(10, 20), np.arange(1050, 2080)])   # 10 in panel 0, 1030 in panel 1: heavy in one panel only
    rows[9] = np.concatenate([np.arange(0, 1000), np.arange(1050, 2050)])  # 2000 entries, 1000 a panel: not heavy
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    ci = np.concatenate(rows)
    kw = dict(panel_mode=1, panel_bytes=128 * 1050, long_row_threshold=10, long_segment=100, panel_coop=64)
    two, one, low_segment = check(ask, [(rp, ci, 2100, kw), (rp, ci, 2100, dict(kw, panel_bytes=128 * 2100)), (rp, ci, 2100, dict(kw, long_segment=1))])
    assert (two["n_panels"], two["base_thresh"], two["seg"], two["heavy"]) == (2, 64, 64, [5, 7])
    assert len(two["segment_tasks"]) // 3 == 17 + 17 and 5 not in two["rows"] and 7 not in two["rows"]   # ceil(1025 / 64) + ceil(1040 / 64) tasks of 64 entries
    assert two["rows"].count(9) == 2 and two["rows"].count(2) == 1
    assert one["heavy"] == [5, 7, 9]                               # in ONE panel row 9's 2000 entries are too many as well
    assert low_segment["seg"] == 64                                # long_segment has the same floor
    assert two["panel_nnz"] == [sum(len(rows[r][rows[r] < 1050]) for r in range(12) if r not in (5, 7)), sum(len(rows[r][rows[r] >= 1050]) for r in range(12) if r not in (5, 7))]
    # the plan of the row-per-wave kernels cuts rows above the threshold itself
    assert [two["base_tasks"][i] for i in range(0, len(two["base_tasks"]), 3)] == [2] * 16 + [5] * 17 + [7] * 17 + [9] * 32


def test_locality_blocks_behind_the_cooperative_prefix(ask):
    rng = np.random.default_rng(6)
    n = 2300   # more than 2048 rows: two locality blocks
    lengths = rng.integers(0, 9, size=n)
    lengths[[5, 2100, 900]] = [200, 180, 160]   # some 90 entries a panel, cooperative items (cap 64): a prefix whatever their block
    rp, ci = csr(rng, n, 600, lengths)
    order = rng.permutation(n)
    kw = dict(panel_mode=1, panel_bytes=128 * 300, panel_coop=64)
    by_id, by_label, none, off, spmv, adding, adding_with_order = check(ask, [
        (rp, ci, 600, dict(kw, sim_kind=1)), (rp, ci, 600, dict(kw, sim_kind=2, sim_order=order)), (rp, ci, 600, dict(kw, sim_kind=0)),
        (rp, ci, 600, dict(kw, sim_kind=1, panel_locality=0)), (rp, ci, 600, dict(kw, sim_kind=1, h_hint=4)),
        (rp, ci, 600, dict(kw, sim_kind=1, is_extra=1)), (rp, ci, 600, dict(kw, sim_kind=2, sim_order=order, is_extra=1))])
    assert [p["locality"] for p in (by_id, by_label, none, off, spmv, adding, adding_with_order)] == [1, 1, 0, 0, 0, 0, 1]
    assert [p["want_sim"] for p in (none, off, spmv, adding)] == [1, 0, 0, 0]
    assert by_id["n_panels"] == 2 and by_id["panel_coop"] == by_label["panel_coop"] == [3, 3]
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    for p, rk in ((by_id, np.arange(n)), (by_label, rank)):
        for q in range(2):
            behind = p["rows"][p["panel_off"][q] + p["panel_coop"][q]:p["panel_off"][q + 1]]
            blocks = [int(rk[r]) >> 11 for r in behind]
            assert blocks == sorted(blocks) and set(blocks) == {0, 1}
    assert sorted(by_id["rows"]) == sorted(none["rows"]) and by_id["rows"] != none["rows"]


def _args(**kw):
    base = dict(kind="args", format=0, es=4, n_parts=2, h_size=12, nrows=[5, 5], ncols=[7, 9], nnz=[3, 2], n_dense=[2, 1], dense=[4, 8, 12])
    base.update(kw)
    return " ".join(f"{k}={','.join(str(x) for x in v) if isinstance(v, list) else v}" for k, v in base.items())


REFUSALS = [   # in the order the library makes them: the call, then inside a part (the second part here: the parts before it are checked first)
    (dict(format=2), "format must be CSR(0) or COO(1)"),
    (dict(es=0), "unknown dtype"),
    (dict(n_parts=0), "null argument or n_parts <= 0"),
    (dict(h_size=0), "h_size must be positive"),
    (dict(nrows=[5, 6]), "all sparse parts must have the same number of rows"),
    (dict(nnz=[3, 1 << 32]), "part sizes must fit 32-bit indices (the reference's uint32 matrices)"),
    (dict(n_dense=[2, 0], dense=[4, 8]), "n_dense must be positive"),
    (dict(n_dense=[2, 2], dense=[4, 8, -1, 13]), "negative dense width"),
    (dict(dense=[4, 8, 11]), "dense widths of a part must add up to h_size"),
    (dict(null_idx=[0, 1]), "null index array"),
    (dict(null_col=[0, 1]), "null colind"),
]


def test_creation_refuses_each_defect_by_text_and_the_earlier_of_two(ask):
    fine, *alone = ask([_args()] + [_args(**kw) for kw, _ in REFUSALS])
    assert (fine["code"], fine["text"]) == (0, "")
    assert [(g["code"], g["text"]) for g in alone] == [(INVALID, text) for _, text in REFUSALS]
    pairs = [(i, j) for i in range(len(REFUSALS)) for j in range(i + 1, len(REFUSALS)) if not set(REFUSALS[i][0]) & set(REFUSALS[j][0])]
    both = ask([_args(**REFUSALS[i][0], **REFUSALS[j][0]) for i, j in pairs])
    assert [g["text"] for g in both] == [REFUSALS[i][1] for i, _ in pairs]
    # part by part: the LAST check of part 0 comes before the FIRST of part 1
    parts, null_table, null_out, more = ask([_args(null_col=[1, 0], nrows=[5, 6]), _args(null_table=1), _args(null_out=1), _args(nrows=[-1, -1])])
    assert parts["text"] == "null colind" and null_table["text"] == null_out["text"] == "null argument or n_parts <= 0"
    assert more["text"] == "part sizes must fit 32-bit indices (the reference's uint32 matrices)"
    # an index array may be null where nothing is read through it: a COO part without entries (a CSR part always has its row pointers)
    coo, csr_, coo_col = ask([_args(format=1, nnz=[3, 0], null_idx=[0, 1]), _args(nnz=[3, 0], null_idx=[0, 1]), _args(format=1, nnz=[3, 0], null_col=[0, 1])])
    assert (coo["code"], csr_["text"], coo_col["code"]) == (0, "null index array", 0)


def test_the_validation_flags_map_to_the_error(ask):
    fine, csr_order, coo_order, coo_range, both_csr, both_coo = ask([f"kind=flags format={f} f0={a} f1={b}" for f, a, b in ((0, 0, 0), (0, 1, 0), (1, 3, 0), (1, 0, 1), (0, 1, 1), (1, 1, 2))])
    assert fine["code"] == 0
    assert (csr_order["code"], csr_order["text"]) == (INVALID, "rowptr is not a non-decreasing prefix array ending at nnz")
    assert (coo_order["code"], coo_order["text"]) == (UNSORTED, "COO row indices are not sorted (pass a coalesced tensor)")
    for g in (coo_range, both_csr, both_coo):   # out of range comes first
        assert (g["code"], g["text"]) == (INVALID, "index out of range in a sparse part")


def test_the_rules_are_host_only_and_written_once():
    for name in ("sweep_plan.hpp", "group_args.hpp"):
        header = open(os.path.join(_CSRC, name)).read()
        for word in ("hip", "g_tune", "g_ctx", "Group *", "Part &", "Part *"):
            assert word not in header.replace("pygim_hip.h", ""), (name, word)
    runtime = {f: open(os.path.join(_CSRC, f)).read() for f in ("rt_launch.inc", "rt_run.inc", "rt_plans.inc", "rt_state.inc", "pygim_hip.hip")}
    everything = "".join(runtime.values())
    assert "panel_min_seg)" in runtime["rt_launch.inc"] and "(double)g_tune.panel_min_seg" not in everything   # the pays-rule: panels_pay alone
    assert everything.count("panels_pay(") == 1
    for text in [t for _, t in REFUSALS[4:]] + ["index out of range in a sparse part", "COO row indices are not sorted"]:
        assert text not in everything, text   # creation's refusals: group_args.hpp alone
    knobs = ("panel_bytes", "panel_min_seg", "panel_coop", "panel_locality", "panel_col16", "long_row_threshold", "long_segment")
    plans = runtime["rt_plans.inc"]
    body = plans[plans.index("int build_plans("):plans.index("return allow_lds ?")]
    assert "g_tune" not in body and body.count("\n") < 70
    for k in knobs:
        assert plans.count("g_tune." + k) == 0 and plans.count("PYGIM_KNOB(" + k + ")") == 1, k
