"""Planning a call's windows and products in pure functions (pygim_amd/csrc/run_plan.hpp) and leaving run_group_common to do what the plan says must change
no bit, no path and cost no time: this build against the parent commit's libpygim_hip.so, both loaded in one process (ParentBuild of
exp_walker_refactor.py), each running the same calls on the same tensors.  JSON lines.
  --section bits: the cases of the three host-operand tests and of the product-plan test --
    tests/test_parity_gpu.py test_host_operands_as_a_pipeline_of_feature_windows (h = 256 / 200 / 320, one sparse part and three, ds_parts 1 and 3,
    host_windows 1..4, a pageable and a page-locked result, every element type), test_grande_windows_with_host_operands_are_gathered_into_pipeline_windows
    (eight per-unit windows, h = 256 and 100, host_windows 1..3), tests/test_lds_gpu.py test_host_windows_store_straight_into_the_page_locked_result (host_direct 2 and 0,
    unit weights and values), and test_device_windows_with_gaps_and_side_by_side_under_every_product_plan (device windows apart, with gaps and side by side under
    merge_parts x fuse_windows).  One line per group with "equal": for every call the bytes of the result, group_host_call (windows and direct),
    the count of group_lds_runs and which of group_timers' entries are non-zero.  The last line counts the calls and the unequal ones; exit status 1 if any.
  --section time: parent and this build alternating, --rounds rounds after one discarded round, every window of calls ending in a synchronise: the
    host-dominated device-pointer call (4096 x 4096, ~120 entries a row, FLT32, h = 64, lds_mode = 1 in both), the Reddit-shaped device product at h = 256, the
    Reddit-shaped host call (CPU features, a page-locked result, automatic windows) and grande's host call of eight windows of 32 features.  This build passes
    when each of its medians lies inside [min, max] of the parent's own repeats, or below.
    python scripts/exp_run_plan.py --parent-lib PATH [--section bits|time|all] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from exp_lds_form import TORCH, random_csr  # noqa: E402
from pygim_amd import _lib, pim_ops, synth  # noqa: E402

TYPES = ("INT8", "INT16", "INT32", "INT64", "FLT32", "DBL64")


def features(rows, h, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    if dt.is_floating_point:
        return (torch.rand(rows, h, dtype=torch.float64, generator=gen) * 2 - 1).to(dt)
    return torch.randint(-3, 4, (rows, h), generator=gen).to(dt)


def observed(hd, out, runs_before, host):
    """what a call left behind: the result's bytes and the path it took"""
    torch.cuda.synchronize()
    got = {"bytes": out.cpu().contiguous().view(torch.uint8).numpy().tobytes(), "lds_runs": _lib.group_lds_runs(hd) - runs_before}
    if host:
        got["host_call"] = _lib.group_host_call(hd)
        got["timers"] = [t != 0 for t in _lib.group_timers(hd)]
    return got


def split_columns(rp, ci, bounds):
    """the column blocks of a CSR with local column ids, as host arrays"""
    rp, ci = rp.cpu().numpy(), ci.cpu().numpy()
    rows_of = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        keep = (ci >= lo) & (ci < hi)
        prp = np.concatenate([[0], np.cumsum(np.bincount(rows_of[keep], minlength=len(rp) - 1))]).astype(np.int32)
        parts.append((prp, np.ascontiguousarray(ci[keep] - lo, dtype=np.int32)))
    return parts


def create(code, parts, n, ncols, n_dense, widths, h, vals=None):
    return _lib.group_create(_lib.CSR, code, [p[0].ctypes.data for p in parts], [p[1].ctypes.data for p in parts], None if vals is None else [v.ctypes.data for v in vals],
                             [n] * len(parts), ncols, [len(p[1]) for p in parts], [n_dense] * len(parts), widths * len(parts), h)


def with_tunables(settings, fn):
    old = {k: _lib.set_tunable(k, v) for k, v in settings.items()}
    try:
        return fn()
    finally:
        for k, v in old.items():
            _lib.set_tunable(k, v)


def host_window_cases(dtname, dev):
    """(name, function that runs every call of the group with the library that is current -> {call: observed})"""
    dt, code = TORCH[dtname], getattr(_lib, dtname)
    n = 700
    for h, bounds in ((256, [0, n]), (200, [0, n]), (320, [0, 250, 251, n])):
        rp, ci = random_csr(n, n, 11, 40 + h, dev)
        parts = split_columns(rp, ci, bounds)
        x = features(n, h, dt, 3)
        for ds_parts in (1, 3):
            xs = [t.contiguous() for t in torch.chunk(x, ds_parts, 1)]

            def run(parts=parts, xs=xs, h=h, bounds=bounds):
                hd = create(code, parts, n, list(np.diff(bounds)), len(xs), [t.shape[1] for t in xs], h)
                got = {}
                for hw in (1, 2, 3, 4):
                    for pinned in (False, True):
                        out = torch.full((n, h), 77, dtype=dt, pin_memory=pinned)
                        runs = _lib.group_lds_runs(hd)
                        with_tunables({"host_windows": hw}, lambda: _lib.spmm_run_group(hd, [t.data_ptr() for t in xs], out.data_ptr()))
                        got[f"host_windows={hw} pinned={pinned}"] = observed(hd, out, runs, True)
                _lib.group_free(hd)
                return got

            yield f"host windows {dtname} h={h} sparse_parts={len(parts)} ds_parts={ds_parts}", run


def grande_cases(dtname, dev):
    dt, code = TORCH[dtname], getattr(_lib, dtname)
    es = torch.empty(0, dtype=dt).element_size()
    n, units, mul = 900, 8, 8 // es
    for h in (256, 100):
        rp, ci = random_csr(n, n, 12, 50 + h, dev)
        parts = split_columns(rp, ci, [0, n])
        x = features(n, h, dt, 4)
        widths = [h // units + (1 if u < h % units else 0) for u in range(units)]
        pad = (widths[0] + mul - 1) // mul * mul
        xp = torch.nn.functional.pad(x, (0, pad))
        wins = [xp[:, a:a + pad].contiguous() for a in np.cumsum([0] + widths[:-1])]

        def run(parts=parts, wins=wins, widths=widths, pad=pad, h=h):
            hd = create(code, parts, n, [n], units, widths, h)
            got = {}
            for hw in (1, 2, 3):
                for pinned in (False, True):
                    out = torch.full((n, h), 77, dtype=dt, pin_memory=pinned)
                    runs = _lib.group_lds_runs(hd)
                    with_tunables({"host_windows": hw}, lambda: _lib.grande_run_group(hd, [w.data_ptr() for w in wins], [pad] * units, out.data_ptr()))
                    got[f"host_windows={hw} pinned={pinned}"] = observed(hd, out, runs, True)
            _lib.group_free(hd)
            return got

        yield f"grande host windows {dtname} h={h}", run


def direct_cases(dtname, dev):
    dt, code = TORCH[dtname], getattr(_lib, dtname)
    es = torch.empty(0, dtype=dt).element_size()
    n, ncols = 2100, 1900
    h = 1024 // es if es < 8 else 192
    rp, ci = random_csr(n, ncols, 14, 60, dev)
    parts = split_columns(rp, ci, [0, ncols])
    x = features(ncols, h, dt, 5)
    vals = features(len(parts[0][1]), 1, dt, 6).numpy().reshape(-1).copy()
    for valued in (False, True):

        def run(valued=valued):
            hd = create(code, parts, n, [ncols], 1, [h], h, [vals] if valued else None)
            got = {}
            for hw in ((2, 3) if es == 8 else (2, 4)):
                for direct, pinned in ((2, True), (0, True), (2, False), (1, True)):
                    out = torch.full((n, h), 77, dtype=dt, pin_memory=pinned)
                    runs = _lib.group_lds_runs(hd)
                    with_tunables({"host_windows": hw, "host_direct": direct}, lambda: _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr()))
                    got[f"host_windows={hw} host_direct={direct} pinned={pinned}"] = observed(hd, out, runs, True)
            _lib.group_free(hd)
            return got

        yield f"direct stores {dtname} valued={valued}", lambda run=run: with_tunables({"lds_mode": 1}, run)   # (the test's fixture: every group gets the LDS-staged plan)


def product_plan_cases(dtname, dev):
    dt, code = TORCH[dtname], getattr(_lib, dtname)
    n, h, bounds, widths = 300, 100, [0, 120, 300], [40, 33, 27]
    rp, ci = random_csr(n, n, 10, 70, dev)
    parts = split_columns(rp, ci, bounds)
    xd = features(n, h, dt, 7).to(dev)
    starts = [0, 40, 73]
    blocks = [xd[:, a:a + w].contiguous() for a, w in zip(starts, widths)]
    padded, views = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for a, w in zip(starts, widths):
            buf = torch.full((hi - lo, w + 3), 99, dtype=dt, device=dev)
            buf[:, :w] = xd[lo:hi, a:a + w]
            padded.append(buf)
            views.append(xd.data_ptr() + (lo * h + a) * xd.element_size())

    def run():
        st = torch.cuda.current_stream().cuda_stream
        hd = create(code, parts, n, [120, 180], 3, widths, h)
        calls = {"spmm blocks": lambda o: _lib.spmm_run_group(hd, [b.data_ptr() for b in blocks], o, st),
                 "grande gaps": lambda o: _lib.grande_run_group(hd, [b.data_ptr() for b in padded], [w + 3 for w in widths] * 2, o, st),
                 "grande views": lambda o: _lib.grande_run_group(hd, views, [h] * 6, o, st)}
        got = {}
        for merge in (1, 0):
            for fuse in (1, 0):
                for name, call in calls.items():
                    out = torch.full((n, h), 77, dtype=dt, device=dev)
                    runs = _lib.group_lds_runs(hd)
                    with_tunables({"merge_parts": merge, "fuse_windows": fuse}, lambda: call(out.data_ptr()))
                    got[f"{name} merge_parts={merge} fuse_windows={fuse}"] = observed(hd, out, runs, False)
        _lib.group_free(hd)
        return got

    yield f"product plan {dtname}", run


def bits_section(parent, dev, line):
    todo = []
    for dtname in TYPES:
        todo += list(host_window_cases(dtname, dev))
        if dtname in ("INT8", "INT32", "FLT32", "DBL64"):
            todo += list(grande_cases(dtname, dev))
        todo += list(direct_cases(dtname, dev))
        if dtname in ("INT32", "FLT32"):
            todo += list(product_plan_cases(dtname, dev))
    calls = unequal = 0
    for name, run in todo:
        mine = run()
        with parent:
            theirs = run()
        differ = sorted(k for k in set(mine) | set(theirs) if mine.get(k) != theirs.get(k))
        calls += len(theirs)
        unequal += len(differ)
        seen = sorted({(v["host_call"]["windows"], v["host_call"]["direct"]) for v in theirs.values() if "host_call" in v})
        line(section="bits", group=name, calls=len(theirs), equal=not differ, differ=differ, windows_and_direct_seen=seen, lds_runs=sum(v["lds_runs"] for v in theirs.values()))
    line(section="bits", groups=len(todo), calls=calls, unequal=unequal)
    return unequal


def time_section(parent, dev, line, rounds, iters):
    st = torch.cuda.current_stream().cuda_stream
    n, nnz, d_max = synth.SHAPES["reddit"]
    rp2, ci2 = random_csr(4096, 4096, 120, 5, dev)
    rp, ci = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    x_host = synth.features(n, 256, torch.float32, seed=3, kind="uniform")
    units = [x_host[:, a:a + 32].contiguous() for a in range(0, 256, 32)]
    out_host = torch.empty((n, 256), dtype=torch.float32, pin_memory=True)
    x_dev, out_dev = x_host.to(dev), torch.empty((n, 256), dtype=torch.float32, device=dev)
    x_small, out_small = x_dev[:4096, :64].contiguous(), torch.empty((4096, 64), dtype=torch.float32, device=dev)
    shapes = [   # name, CSR, rows, dense split, calls per window, the call, lds_mode
        ("device pointers, 4096 x 4096 FLT32 h=64 (the host side of the call dominates)", rp2, ci2, 4096, [64], iters * 20,
         lambda hd: _lib.spmm_run_group(hd, [x_small.data_ptr()], out_small.data_ptr(), st), 1),
        ("device pointers, reddit FLT32 h=256", rp, ci, n, [256], iters, lambda hd: _lib.spmm_run_group(hd, [x_dev.data_ptr()], out_dev.data_ptr(), st), 0),
        ("host call, reddit FLT32 h=256, page-locked result, automatic windows", rp, ci, n, [256], max(2, iters // 4),
         lambda hd: _lib.spmm_run_group(hd, [x_host.data_ptr()], out_host.data_ptr(), st), 0),
        ("grande host call, reddit FLT32 h=256, eight windows of 32", rp, ci, n, [32] * 8, max(2, iters // 4),
         lambda hd: _lib.grande_run_group(hd, [u.data_ptr() for u in units], [32] * 8, out_host.data_ptr(), st), 0),
    ]
    bad = []
    for name, srp, sci, nr, widths, k, call, lds_mode in shapes:
        h = sum(widths)

        def make():
            return with_tunables({"lds_mode": lds_mode}, lambda: _lib.group_create(_lib.CSR, _lib.FLT32, [srp.data_ptr()], [sci.data_ptr()], None, [nr], [nr], [sci.numel()],
                                                                                   [len(widths)], widths, h))

        with parent:
            hds = {"parent": make()}
        hds["new"] = make()

        def window(hd):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                call(hd)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / k

        series, path = {"parent": [], "new": []}, {}
        for rnd in range(rounds + 1):
            for who in ("parent", "new"):
                if who == "parent":
                    with parent:
                        ms = with_tunables({"lds_mode": lds_mode}, lambda: window(hds[who]))
                else:
                    ms = with_tunables({"lds_mode": lds_mode}, lambda: window(hds[who]))
                if rnd:   # (the first round of each build is discarded: first touches of the allocator and of the code objects)
                    series[who].append(round(ms, 5))
        with parent:
            path["parent"] = (_lib.group_host_call(hds["parent"]) if "host call" in name else None, _lib.group_lds_runs(hds["parent"]))
            _lib.group_free(hds["parent"])
        path["new"] = (_lib.group_host_call(hds["new"]) if "host call" in name else None, _lib.group_lds_runs(hds["new"]))
        _lib.group_free(hds["new"])
        p, q = series["parent"], series["new"]
        ok = statistics.median(q) <= max(p) and path["new"] == path["parent"]
        line(section="time", call=name, calls_per_window=k, parent_ms=p, new_ms=q, parent_min=min(p), parent_max=max(p), parent_median=statistics.median(p),
             new_median=statistics.median(q), below_parent_min=statistics.median(q) < min(p), host_call=path["new"][0], lds_runs=path["new"][1], same_path=path["new"] == path["parent"],
             inside_parent_spread_or_below=ok)
        if not ok:
            bad.append(name)
    line(section="time", rounds=rounds, iters=iters, not_passing=bad)
    return len(bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libpygim_hip.so")
    ap.add_argument("--section", default="all", choices=["all", "bits", "time"])
    ap.add_argument("--out", default=None, help="write the lines here as well (profiles/exp_run_plan.txt)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
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
        bad += time_section(parent, dev, line, args.rounds, args.iters)
    with parent:
        _lib.release()
    torch.ops.pim_ops.dpu_release()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
