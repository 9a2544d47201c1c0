"""Planning the sweep's panels and items in pure functions (pygim_amd/csrc/sweep_plan.hpp), leaving build_plans to do what needs the device, and making
creation's argument checks once (group_args.hpp) must change no bit, no plan and cost no time: this build against the parent commit's libpygim_hip.so,
both loaded in one process (ParentBuild of exp_walker_refactor.py), each creating the same groups from the same arrays.  JSON lines.
  --section bits: the shapes of the sweep's guards in tests/test_parity_gpu.py, every element type -- the panel sweep with cooperative items and heavy rows
    (300 x 900, rows of 9000 / 2049 / 700 / 65 entries, panel_mode = 1, 3 panels, panel_coop = 64, unit weights and values, h = 32 and 96), long rows beside
    the sweep (long_row_threshold = 64), the automatic rule and panel_mode = 2, columns stored out of order, a COO group, two column blocks with their merged
    matrix, items in locality order (panel_locality = 2 on a square part, 5 panels), the LDS-staged SpMV kernel's panels (2600 x 2600 in 3 panels, h = 1 and 4, vec_lds 1 and 0) and
    the SpMV entry point.  One line per group with "equal": the bytes of the result, group_plan, group_info and group_lds_note.  The last line counts the
    groups and the unequal ones; exit status 1 if any.
  --section time: creation (group_timers' creation entry, ms) of a Reddit-shaped group, a products-shaped uniform group and a 4096 x 4096 group under
    panel_mode = 1 (8 panels), parent and this build alternating, --rounds rounds after one discarded round.  This build passes when each of its medians lies
    inside [min, max] of the parent's own repeats, or below.
    python scripts/exp_sweep_plan.py --parent-lib PATH [--section bits|time|all] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from exp_lds_form import TORCH, random_csr  # noqa: E402
from exp_run_plan import features, split_columns, with_tunables  # noqa: E402
from pygim_amd import _lib, pim_ops, synth  # noqa: E402

TYPES = ("INT8", "INT16", "INT32", "INT64", "FLT32", "DBL64")


def with_long_rows(rp, ci, ncols, long_rows, seed):
    """the CSR with some rows replaced by rows of the given lengths (columns sorted, duplicates allowed), as host arrays"""
    rng = np.random.default_rng(seed)
    rp, ci = rp.cpu().numpy(), ci.cpu().numpy()
    rows = [ci[rp[r]:rp[r + 1]] for r in range(len(rp) - 1)]
    for r, k in long_rows:
        rows[r] = np.sort(rng.integers(0, ncols, size=k)).astype(np.int32)
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32), np.ascontiguousarray(np.concatenate(rows), dtype=np.int32)


def observed(hd, out):
    torch.cuda.synchronize()
    return {"bytes": out.cpu().contiguous().view(torch.uint8).numpy().tobytes(), "plan": _lib.group_plan(hd), "info": _lib.group_info(hd), "note": _lib.group_lds_note(hd)}


def one_group(code, dt, fmt, parts, n, ncols, h, vals=None, spmv=False):
    """create, one product from host operands, what it left behind, free"""
    x = features(sum(ncols), 1 if spmv else h, dt, 3)
    hd = _lib.group_create(fmt, code, [p[0].ctypes.data for p in parts], [p[1].ctypes.data for p in parts], None if vals is None else [v.ctypes.data for v in vals],
                           [n] * len(parts), ncols, [len(p[1]) for p in parts], [h if spmv else 1] * len(parts), ([1] * h if spmv else [h]) * len(parts), h)
    out = torch.full((n, h), 77, dtype=dt)
    if spmv:
        xs = [x.clone() for _ in range(h)]
        _lib.spmv_run_group(hd, [t.data_ptr() for t in xs], out.data_ptr())
    else:
        _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr())
    got = observed(hd, out)
    _lib.group_free(hd)
    return got


def sweep_cases(dtname, dev):
    """(name, tunables, function that creates and runs the group with the library that is current -> observed)"""
    dt, code = TORCH[dtname], getattr(_lib, dtname)
    rp0, ci0 = random_csr(300, 900, 30, 21, dev)
    rp, ci = with_long_rows(rp0, ci0, 900, [(0, 9000), (7, 65), (100, 700), (299, 2049)], 22)
    vals = features(len(ci), 1, dt, 6).numpy().reshape(-1).copy()
    coop = {"lds_mode": 0, "panel_mode": 1, "panel_bytes": 128 * 300, "panel_coop": 64}
    for h in (32, 96):
        for v in (None, [vals]):
            yield f"cooperative items {dtname} h={h} valued={v is not None}", coop, lambda h=h, v=v: one_group(code, dt, _lib.CSR, [(rp, ci)], 300, [900], h, v)
    yield f"heavy rows {dtname}", dict(coop, long_row_threshold=64, long_segment=64), lambda: one_group(code, dt, _lib.CSR, [(rp, ci)], 300, [900], 64)
    yield f"automatic rule {dtname}", {"lds_mode": 2, "panel_bytes": 128 * 300}, lambda: one_group(code, dt, _lib.CSR, [(rp, ci)], 300, [900], 64)
    yield f"no sweep {dtname}", {"lds_mode": 2, "panel_mode": 2}, lambda: one_group(code, dt, _lib.CSR, [(rp, ci)], 300, [900], 64)
    shuffled = ci.copy()
    rng = np.random.default_rng(23)
    for r in range(300):
        rng.shuffle(shuffled[rp[r]:rp[r + 1]])
    yield f"unsorted columns {dtname}", coop, lambda: one_group(code, dt, _lib.CSR, [(rp, shuffled)], 300, [900], 64)
    rows_of = np.repeat(np.arange(300, dtype=np.int32), np.diff(rp))
    yield f"COO {dtname}", coop, lambda: one_group(code, dt, _lib.COO, [(rows_of, ci)], 300, [900], 64)
    blocks = split_columns(torch.from_numpy(rp), torch.from_numpy(ci), [0, 400, 900])
    for merge in (1, 0):
        yield f"two column blocks {dtname} merge_parts={merge}", dict(coop, merge_parts=merge), lambda: one_group(code, dt, _lib.CSR, blocks, 300, [400, 500], 64)
    sq = tuple(a.cpu().numpy() for a in random_csr(5000, 5000, 12, 24, dev))
    for loc in (2, 0):
        yield f"locality order {dtname} panel_locality={loc}", {"lds_mode": 2, "panel_mode": 1, "panel_bytes": 128 * 1024, "panel_locality": loc}, lambda: one_group(code, dt, _lib.CSR, [sq], 5000, [5000], 64)
    n = 2600
    rv = with_long_rows(*random_csr(n, n, 160, 25, dev), n, [(7, 3000), (n - 2, 900)], 26)
    for w in (1, 4):
        for lds_on in (1, 0):
            yield f"SpMV panels {dtname} h={w} vec_lds={lds_on}", {"panel_bytes": 128 * 900, "vec_lds": lds_on}, lambda w=w: one_group(code, dt, _lib.CSR, [rv], n, [n], w)
    yield f"SpMV entry point {dtname}", {"panel_bytes": 128 * 900}, lambda: one_group(code, dt, _lib.CSR, [rv], n, [n], 2, spmv=True)


def bits_section(parent, dev, line):
    groups = unequal = 0
    for dtname in TYPES:
        for name, tunables, run in sweep_cases(dtname, dev):
            mine = with_tunables(tunables, run)
            with parent:
                theirs = with_tunables(tunables, run)
            differ = sorted(k for k in theirs if mine.get(k) != theirs[k])
            groups += 1
            unequal += bool(differ)
            line(section="bits", group=name, equal=not differ, differ=differ, plan=theirs["plan"], n_long_rows=theirs["info"]["n_long_rows"], note=theirs["note"])
    line(section="bits", groups=groups, unequal=unequal)
    return unequal


def time_section(parent, dev, line, rounds):
    shapes = []
    for name, shape, tunables in (("reddit-shaped, FLT32 h=256", "reddit", {}), ("products-shaped uniform, FLT32 h=100", "ogbn-products", {})):
        n, nnz, d_max = synth.SHAPES[shape]
        rp, ci = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
        shapes.append((name, rp, ci, n, 256 if shape == "reddit" else 100, tunables))
    rp, ci = random_csr(4096, 4096, 120, 5, dev)
    shapes.append(("4096 x 4096, FLT32 h=64, panel_mode=1 (8 panels)", rp, ci, 4096, 64, {"panel_mode": 1, "panel_bytes": 128 * 512, "lds_mode": 0}))
    bad = []
    for name, rp, ci, n, h, tunables in shapes:

        def create_ms():
            hd = _lib.group_create(_lib.CSR, _lib.FLT32, [rp.data_ptr()], [ci.data_ptr()], None, [n], [n], [ci.numel()], [1], [h], h)
            got = _lib.group_timers(hd)[4], _lib.group_plan(hd), _lib.group_lds_note(hd)
            _lib.group_free(hd)
            return got

        series, what = {"parent": [], "new": []}, {}
        for rnd in range(rounds + 1):
            for who in ("parent", "new"):
                if who == "parent":
                    with parent:
                        ms, *what[who] = with_tunables(tunables, create_ms)
                else:
                    ms, *what[who] = with_tunables(tunables, create_ms)
                if rnd:   # (the first round of each build is discarded: first touches of the allocator and of the code objects)
                    series[who].append(round(ms, 4))
        p, q = series["parent"], series["new"]
        ok = statistics.median(q) <= max(p) and what["new"] == what["parent"]
        line(section="time", group=name, nnz=int(ci.numel()), parent_ms=p, new_ms=q, parent_min=min(p), parent_max=max(p), parent_median=statistics.median(p),
             new_median=statistics.median(q), below_parent_min=statistics.median(q) < min(p), plan=what["new"][0], note=what["new"][1], same_plan=what["new"] == what["parent"],
             inside_parent_spread_or_below=ok)
        if not ok:
            bad.append(name)
    line(section="time", rounds=rounds, not_passing=bad)
    return len(bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libpygim_hip.so")
    ap.add_argument("--section", default="all", choices=["all", "bits", "time"])
    ap.add_argument("--out", default=None, help="write the lines here as well (profiles/exp_sweep_plan.txt)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pim_ops.load("spmm")
    torch.ops.pim_ops.dpu_init_ranks(1)
    from exp_walker_refactor import ParentBuild

    parent = ParentBuild(args.parent_lib)
    sink = open(args.out, "w") if args.out else None

    def line(**kw):
        text = json.dumps(kw)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    bad = 0
    if args.section in ("all", "bits"):
        bad += bits_section(parent, dev, line)
    if args.section in ("all", "time"):
        bad += time_section(parent, dev, line, args.rounds)
    with parent:
        _lib.release()
    torch.ops.pim_ops.dpu_release()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
