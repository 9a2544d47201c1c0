"""Splitting build_lds_plan_form into a pure chooser (pygim_amd/csrc/lds_form.hpp lds_choose_form) and a short builder must change no
decision and cost no time: this build against the parent commit's libpygim_hip.so, both loaded in one process (ParentBuild of
exp_walker_refactor.py), each creating the same groups.
  --section forms: for every case of cases() -- a random CSR of at most ~1.2 M entries, an element type, a product width and a few
    tunables set in BOTH libraries -- the group is created by each library and group_lds_geometry, group_lds_plan, group_lds_code and
    group_lds_note are compared.  One line per case with "equal"; the last line counts the cases and the unequal ones, exit status 1 if
    any.  --record PATH writes the cases, the device's compute units and the PARENT's answers (what tests/test_lds_form.py pins the
    chooser to on a CPU); the rows a plan's tiles cover and the H of a half-split plan are read out of the note's text.
  --section time: group creation (group_timers()[4], the wall clock and the laps PYGIM_PLAN_TIMING=1 prints) and the headline
    product (the Reddit-shaped graph, FLT32, h = 256) of the parent and of this build, alternating, --rounds rounds after one
    discarded round.  The new build passes when each of its medians lies inside [min, max] of the parent's own repeats, or below.
  --section restatement (no device, no parent): where pygim_amd/autotune.py lds_form -- the partition chooser's restatement of the
    rules -- and lds_choose_form (through tests/native/lds_form_main.cpp, built on demand) part: FLT32, unit weights, default tunables,
    256 compute units, row shares 1/1 ... 1/16 of the Reddit-shaped graph at h = 16, 32, 64, 128, 256.  One line per grid point with
    both answers and the fields that differ; nothing is fixed here, and the exit status is 0 either way.
    python scripts/exp_lds_form.py --parent-lib PATH [--section forms|time|all] [--record PATH] [--out PATH]
    python scripts/exp_lds_form.py --section restatement [--out PATH]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pygim_amd import _lib, pim_ops, synth  # noqa: E402

TORCH = {"INT8": torch.int8, "INT16": torch.int16, "INT32": torch.int32, "INT64": torch.int64, "FLT32": torch.float32, "DBL64": torch.float64}
SHARE = dict(nrows=16 * 1824 + 200, ncols=40000, deg=42)      # a 1/8 row share's shape: 29 384 rows, ~1.1 M entries


def case(name, dtype, h, nrows, ncols, deg, valued=False, **tunables):
    return dict(name=name, dtype=dtype, h=h, nrows=nrows, ncols=ncols, deg=deg, valued=valued, tunables=tunables)


def cases():
    out = []
    for h in (256, 200, 128):
        out.append(case(f"share INT32 h={h}", "INT32", h, **SHARE))
        for f32 in (0, 1, 2):
            out.append(case(f"share FLT32 h={h} lds_col_split_f32={f32}", "FLT32", h, **SHARE, lds_col_split_f32=f32))
    for dt in ("INT32", "FLT32"):
        out.append(case(f"share {dt} h=256 lds_row_tail=0", dt, 256, **SHARE, lds_row_tail=0))
    for s in (1, 3):
        out.append(case(f"share INT32 h=256 lds_col_split={s}", "INT32", 256, **SHARE, lds_col_split=s))
    out.append(case("share INT32 h=256 lds_fill_tiles=0", "INT32", 256, **SHARE, lds_fill_tiles=0))
    out.append(case("share INT32 h=256 lds_row_tail=0 lds_fill_tiles=0", "INT32", 256, **SHARE, lds_row_tail=0, lds_fill_tiles=0))
    for dt in ("INT8", "INT16"):
        out.append(case(f"2500 x 30000 {dt} h=256", dt, 256, 2500, 30000, 150))
    wide = dict(nrows=8192, ncols=4096, deg=140)   # (a one-slice product gets 256 light tiles: ~1 M entries keep them above the reuse rule)
    for dt in ("FLT32", "INT32", "INT16"):
        out.append(case(f"valued {dt} h=128", dt, 128, **wide, valued=True))
    out.append(case("valued DBL64 h=64", "DBL64", 64, **wide, valued=True))
    for dt in ("DBL64", "INT64"):
        out.append(case(f"unit {dt} h=64", dt, 64, **wide))
    for half in (1, 0):
        out.append(case(f"narrow INT32 h=32 lds_half_split={half}", "INT32", 32, 20000, 20000, 50, lds_half_split=half))
        out.append(case(f"narrow FLT32 h=16 lds_half_split={half}", "FLT32", 16, 20000, 20000, 64, lds_half_split=half))
    out.append(case("narrow INT32 h=32 ncols=400 (fewer than four chunks)", "INT32", 32, 20000, 400, 50))
    out.append(case("below the reuse threshold", "INT32", 256, 29384, 40000, 3))
    for mode in (1, 2):
        out.append(case(f"below the reuse threshold lds_mode={mode}", "INT32", 256, 29384, 40000, 3, lds_mode=mode))
    out.append(case("token form: lds_code=0", "INT32", 256, **SHARE, lds_code=0))
    out.append(case("token form: lds_waves=8 lds_mode=1", "FLT32", 256, **SHARE, lds_waves=8, lds_mode=1))
    out.append(case("lds_code_waves=16", "FLT32", 256, **SHARE, lds_code_waves=16))
    for nbuf in (2, 3, 4):
        out.append(case(f"lds_code_nbuf={nbuf}", "FLT32", 256, **SHARE, lds_code_nbuf=nbuf))
    out.append(case("lds_code_boundary=2", "FLT32", 256, **SHARE, lds_code_boundary=2))
    for fail in (1, 2, 4):
        out.append(case(f"lds_fail={fail}", "FLT32", 128, 4096, 4096, 120, lds_fail=fail))
    for cg in (0, 2):
        out.append(case(f"lds_codegen={cg}", "INT32", 256, **SHARE, lds_codegen=cg))
    out.append(case("square, 1.2 M entries, lds_tile_order=1", "FLT32", 256, 16 * 1824, 16 * 1824, 44, lds_tile_order=1))
    return out


def random_csr(nrows, ncols, deg, seed, dev):
    """tests/conftest.py random_csr (Poisson degrees, a tenth of the rows empty, columns sorted inside a row, duplicates allowed), sorted on the device"""
    rng = np.random.default_rng(seed)
    d = rng.poisson(deg, size=nrows).astype(np.int64)
    d[rng.random(nrows) < 0.1] = 0
    rowptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(d, out=rowptr[1:])
    col = torch.from_numpy(rng.integers(0, ncols, size=int(rowptr[-1]), dtype=np.int64)).to(dev)
    row = torch.repeat_interleave(torch.arange(nrows, device=dev), torch.from_numpy(d).to(dev))
    col = (torch.sort(row * ncols + col).values % ncols).to(torch.int32)
    return torch.from_numpy(rowptr.astype(np.int32)).to(dev), col


def answers(c, rp, ci, vals):
    """create the group with the library that is current and read what it decided"""
    old = {k: _lib.set_tunable(k, v) for k, v in c["tunables"].items()}
    try:
        hd = _lib.group_create(_lib.CSR, getattr(_lib, c["dtype"]), [rp.data_ptr()], [ci.data_ptr()], None if vals is None else [vals.data_ptr()],
                               [c["nrows"]], [c["ncols"]], [ci.numel()], [1], [c["h"]], c["h"])
        got = dict(geometry=_lib.group_lds_geometry(hd), plan=_lib.group_lds_plan(hd), code=_lib.group_lds_code(hd), note=_lib.group_lds_note(hd))
        _lib.group_free(hd)
    finally:
        for k, v in old.items():
            _lib.set_tunable(k, v)
    m = re.search(r"hold the first (\d+) of", got["note"])
    got["covered_rows"] = int(m.group(1)) if m else 0          # 0: the tiles cover every row
    m = re.search(r"two column ranges of (\d+) columns", got["note"])
    got["half_H"] = int(m.group(1)) if m else 0
    return got


def forms_section(parent, dev, line, record):
    unequal, rec = 0, []
    for i, c in enumerate(cases()):
        rp, ci = random_csr(c["nrows"], c["ncols"], c["deg"], 100 + i, dev)
        vals = None
        if c["valued"]:
            gen = torch.Generator(device=dev).manual_seed(i)
            vals = (torch.randint(-3, 4, (ci.numel(),), device=dev, generator=gen)).to(TORCH[c["dtype"]])
        mine = answers(c, rp, ci, vals)
        with parent:
            theirs = answers(c, rp, ci, vals)
        torch.cuda.synchronize()
        eq = mine == theirs
        unequal += not eq
        line(section="forms", case=c["name"], nnz=ci.numel(), equal=eq, tiles=theirs["plan"]["tiles"], waves=theirs["geometry"]["waves"],
             col_splits=theirs["geometry"]["col_splits"], code=theirs["code"]["active"], device_generated=theirs["code"]["device_generated"],
             **({} if eq else dict(new=mine, parent=theirs)))
        rec.append(dict(c, nnz=ci.numel(), parent=theirs))
    line(section="forms", cases=len(rec), unequal=unequal)
    if record:
        with open(record, "w") as f:
            json.dump(dict(device=_lib.device_info()[0], cu_count=_lib.device_info()[1], cases=rec), f, indent=1)
            f.write("\n")
    return unequal


class Stderr:
    """what the library prints to standard error inside the block (the PYGIM_PLAN_TIMING laps)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def time_section(parent, dev, line, rounds, iters):
    n, nnz, d_max = synth.SHAPES["reddit"]
    rp, ci = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    h = 256
    x = synth.features(n, h, torch.float32, seed=3, device=dev, kind="uniform")
    out = torch.empty((n, h), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def one():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with Stderr() as err:
            hd = _lib.group_create(_lib.CSR, _lib.FLT32, [rp.data_ptr()], [ci.data_ptr()], None, [n], [n], [nnz], [1], [h], h)
        wall = (time.perf_counter() - t0) * 1e3
        laps = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^\[pygim plan\] (.+?)\s+([0-9.]+) ms$", err.text, re.M)}
        note = _lib.group_lds_note(hd)
        for _ in range(3):
            _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr(), st)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr(), st)
        ev[1].record()
        torch.cuda.synchronize()
        rec = dict(create_ms=round(_lib.group_timers(hd)[4], 2), create_wall_ms=round(wall, 2), product_ms=round(ev[0].elapsed_time(ev[1]) / iters, 4), laps=laps, note=note)
        _lib.group_free(hd)
        return rec

    series = {"parent": [], "new": []}
    for rnd in range(rounds + 1):
        for who in ("parent", "new"):
            if who == "parent":
                with parent:
                    rec = one()
            else:
                rec = one()
            if rnd:   # (the first round of each build is discarded: first touches of the allocator and of the code objects)
                series[who].append(rec)
            line(section="time", build=who, round=rnd, discarded=rnd == 0, **rec)
    bad = []
    for key in ("create_ms", "create_wall_ms", "product_ms"):
        p, q = [r[key] for r in series["parent"]], [r[key] for r in series["new"]]
        ok = statistics.median(q) <= max(p)
        line(section="time", figure=key, parent=p, new=q, parent_min=min(p), parent_max=max(p), new_median=statistics.median(q), inside_parent_spread_or_below=ok)
        if not ok:
            bad.append(key)
    if series["parent"][0]["note"] != series["new"][0]["note"]:
        bad.append("note")
    line(section="time", rounds=rounds, iters=iters, not_passing=bad)
    return len(bad)


def restatement_section(line):
    import subprocess

    from pygim_amd import autotune

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(root, "tests", "native", "lds_form_main.cpp"), os.path.join(root, "tests", "native", "lds_form")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(root, "pygim_amd", "csrc", "lds_form.hpp"))):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", exe])
    n, nnz, _ = synth.SHAPES["reddit"]
    grid = [(k, h, -(-n // k), nnz // k) for k in range(1, 17) for h in (16, 32, 64, 128, 256)]
    asked = "\n".join(f"dtype=4 val_es=4 nrows={nr} ncols={n} nnz={z} h_hint={h} cu_count=256" for _, h, nr, z in grid) + "\n"
    told = subprocess.run([exe, "-"], input=asked, capture_output=True, text=True, check=True).stdout.splitlines()
    differ = 0
    for (k, h, nr, z), ln in zip(grid, told):
        f = {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)(?= |$)", ln)}
        rpt = f["rows_per_tile"] or f["waves"] * f["acc_per_wave"]
        lib = dict(sweep=not f["plan"], split=f["col_splits"], tail_rows=nr - f["rows_lds"], half=bool(f["half_H"]), tiles=-(-f["rows_lds"] // rpt)) if f["plan"] else dict(sweep=True)
        sweep, split, _, tail_rows, half, tiles = autotune.lds_form(nr, n, z, h, 4)
        py = dict(sweep=False, split=split, tail_rows=tail_rows, half=half, tiles=tiles) if not sweep else dict(sweep=True)
        diff = sorted(a for a in set(lib) | set(py) if lib.get(a) != py.get(a))
        differ += bool(diff)
        line(section="restatement", share=f"1/{k}", h=h, nrows=nr, nnz=z, library=lib, autotune=py, differ=diff)
    line(section="restatement", points=len(grid), differing=differ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libpygim_hip.so")
    ap.add_argument("--section", default="all", choices=["all", "forms", "time", "restatement"])
    ap.add_argument("--record", default=None, help="write the cases and the parent's answers here (tests/golden/lds_form_record.json)")
    ap.add_argument("--out", default=None, help="write the lines here as well (profiles/exp_lds_form.txt)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.section == "restatement":
        with open(args.out, "w") if args.out else open(os.devnull, "w") as sink:
            def say(**kw):
                print(json.dumps(kw), flush=True)
                sink.write(json.dumps(kw) + "\n")
            restatement_section(say)
        return
    if not args.parent_lib:
        ap.error("--parent-lib is needed for the forms and time sections")
    os.environ["PYGIM_PLAN_TIMING"] = "1"   # (both libraries read it at their first plan)
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
    if args.section in ("all", "forms"):
        err = Stderr()   # (the laps of forty small groups are of no interest -- unless one of them fails)
        try:
            with err:
                bad += forms_section(parent, dev, line, args.record)
        except Exception:
            sys.stderr.write(err.text[-4000:])
            raise
    if args.section in ("all", "time"):
        bad += time_section(parent, dev, line, args.rounds, args.iters)
    with parent:
        _lib.release()
    torch.ops.pim_ops.dpu_release()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
