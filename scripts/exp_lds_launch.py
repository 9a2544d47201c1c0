"""Splitting launch_lds into a pure launch plan (pygim_amd/csrc/lds_launch.hpp lds_plan_launch), one staging step (lds_stage_x) and a short
launcher must change no bit and cost no time: this build against the parent commit's libpygim_hip.so, both loaded in one process
(ParentBuild of exp_walker_refactor.py), each running the same products on the same tensors.
  --section bits: for every case of exp_lds_form.cases() -- a random CSR of at most ~1.2 M entries, an element type, a product width and a
    few tunables set in BOTH libraries -- each library creates the group and runs: spmm_run_group at the group's width; block_run windows
    (one slice of a wider X, a one-slice X of its own that is taken in place, an odd width from an odd column, and one that adds into C);
    the same product twice under spmm_run_group_x(x_unchanged = 1); for INT8, INT16, INT32 and FLT32 quant_spmm_run and
    spmm_run_dequant.  One line per case with "equal": the bytes of every output (or the text of the error, where a call is refused),
    group_lds_geometry, and the count of group_lds_runs -- the same path was taken.  The last line counts the cases and the unequal
    ones; exit status 1 if any.
  --section time: two products, parent and this build alternating, --rounds rounds after one discarded round, every window of --iters
    calls ending in a synchronise: the headline product (the Reddit-shaped graph, FLT32, h = 256) and one where the host side of the
    launch dominates (4096 x 4096, ~120 entries a row, FLT32, h = 64, under lds_mode = 1 in both libraries since its light tiles lie below the reuse rule, X taken in place: the line reports the device memory this build's first product takes -- none -- and what the same
    product takes under lds_direct_x = 0, the staged copy; a probe only -- an allocation served from memory the runtime already holds reads 0).  The new build passes when each of its medians
    lies inside [min, max] of the parent's own repeats, or below.
    python scripts/exp_lds_launch.py --parent-lib PATH [--section bits|time|all] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from exp_lds_form import TORCH, cases, random_csr  # noqa: E402
from pygim_amd import _lib, pim_ops, synth  # noqa: E402

QUANT = ("INT8", "INT16", "INT32", "FLT32")


def operand(rows, h, dtype, seed, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    if dtype.is_floating_point:
        return (torch.rand(rows, h, dtype=torch.float32, device=dev, generator=gen) * 2 - 1).to(dtype)
    return torch.randint(-3, 4, (rows, h), device=dev, generator=gen).to(dtype)


def attempt(fn, *outs):
    """the bytes the call wrote, or the text of its refusal"""
    try:
        fn()
    except _lib.PygimError as e:
        return "error: " + str(e)
    torch.cuda.synchronize()
    return [o.clone() for o in outs]


def products(c, rp, ci, vals, x, xf, st):
    """create the group with the library that is current, run every product, read the path it took"""
    dt, h, n, m = TORCH[c["dtype"]], c["h"], c["nrows"], c["ncols"]
    dev = x.device
    old = {k: _lib.set_tunable(k, v) for k, v in c["tunables"].items()}
    got = {}
    try:
        hd = _lib.group_create(_lib.CSR, getattr(_lib, c["dtype"]), [rp.data_ptr()], [ci.data_ptr()], None if vals is None else [vals.data_ptr()],
                               [n], [m], [ci.numel()], [1], [h], h)
        es = x.element_size()
        eps = 128 if es <= 2 else 64            # elements of one slice of the staged copy
        out = torch.zeros((n, h), dtype=dt, device=dev)
        got["run_group"] = attempt(lambda: _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr(), st), out)
        if eps <= h:
            o1 = torch.zeros((n, h), dtype=dt, device=dev)
            got["window of one slice"] = attempt(lambda: _lib.block_run(hd, 0, x.data_ptr(), h, o1.data_ptr(), h, eps, False, st), o1)
            x1, o2 = x[:, :eps].contiguous(), torch.zeros((n, eps), dtype=dt, device=dev)
            got["one-slice X in place"] = attempt(lambda: _lib.block_run(hd, 0, x1.data_ptr(), eps, o2.data_ptr(), eps, eps, False, st), o2)
        wodd = min(h - 1, 37) | 1
        if 0 < wodd < h:
            o3 = torch.zeros((n, h), dtype=dt, device=dev)
            got["odd window"] = attempt(lambda: _lib.block_run(hd, 0, x.data_ptr() + es, h, o3.data_ptr() + es, h, wodd, False, st), o3)
        o4 = operand(n, h, dt, 11, dev)
        got["accumulating window"] = attempt(lambda: _lib.block_run(hd, 0, x.data_ptr(), h, o4.data_ptr(), h, h, True, st), o4)
        o5, o6 = torch.zeros((n, h), dtype=dt, device=dev), torch.zeros((n, h), dtype=dt, device=dev)
        got["x_unchanged first"] = attempt(lambda: _lib.spmm_run_group(hd, [x.data_ptr()], o5.data_ptr(), st, x_unchanged=True), o5)
        got["x_unchanged again"] = attempt(lambda: _lib.spmm_run_group(hd, [x.data_ptr()], o6.data_ptr(), st, x_unchanged=True), o6)
        if c["dtype"] in QUANT:
            of, scale = torch.zeros((n, h), dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
            got["quant_spmm_run"] = attempt(lambda: _lib.quant_spmm_run(hd, xf.data_ptr(), h, of.data_ptr(), scale.data_ptr(), st), of, scale)
            bits, xq, od = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((m, h), dtype=dt, device=dev), torch.zeros((n, h), dtype=torch.float32, device=dev)

            def dequant():
                _lib.quant_absmax(xf.data_ptr(), h, m, h, bits.data_ptr(), st)
                _lib.quantize(getattr(_lib, c["dtype"]), xf.data_ptr(), h, m, h, bits.data_ptr(), xq.data_ptr(), 0, st)
                _lib.spmm_run_dequant(hd, xq.data_ptr(), h, od.data_ptr(), bits.data_ptr(), st)

            got["spmm_run_dequant"] = attempt(dequant, od, xq)
        got["geometry"] = _lib.group_lds_geometry(hd)
        got["lds_runs"] = _lib.group_lds_runs(hd)
        _lib.group_free(hd)
    finally:
        for k, v in old.items():
            _lib.set_tunable(k, v)
    return got


def same(a, b):
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))
    return type(a) is type(b) and a == b


def bits_section(parent, dev, line):
    st = torch.cuda.current_stream().cuda_stream
    unequal = 0
    todo = cases()
    for i, c in enumerate(todo):
        rp, ci = random_csr(c["nrows"], c["ncols"], c["deg"], 100 + i, dev)
        vals = None
        if c["valued"]:
            vals = torch.randint(-3, 4, (ci.numel(),), device=dev, generator=torch.Generator(device=dev).manual_seed(i)).to(TORCH[c["dtype"]])
        x = operand(c["ncols"], c["h"], TORCH[c["dtype"]], 7, dev)
        xf = operand(c["ncols"], c["h"], torch.float32, 8, dev)
        mine = products(c, rp, ci, vals, x, xf, st)
        with parent:
            theirs = products(c, rp, ci, vals, x, xf, st)
        differ = sorted(k for k in set(mine) | set(theirs) if k not in mine or k not in theirs or not same(mine[k], theirs[k]))
        errors = {k: v for k, v in theirs.items() if isinstance(v, str)}
        unequal += bool(differ)
        line(section="bits", case=c["name"], nnz=ci.numel(), calls=len(theirs) - 2, equal=not differ, differ=differ, lds_runs=theirs["lds_runs"], new_lds_runs=mine["lds_runs"],
             xcd_slices=theirs["geometry"]["xcd_slices"], refused=errors)
    line(section="bits", cases=len(todo), unequal=unequal)
    return unequal


def time_section(parent, dev, line, rounds, iters):
    st = torch.cuda.current_stream().cuda_stream
    n, nnz, d_max = synth.SHAPES["reddit"]
    shapes = []
    rp2, ci2 = random_csr(4096, 4096, 120, 5, dev)
    shapes.append(("4096 x 4096 FLT32 h=64, X in place", rp2, ci2, 4096, 4096, 64, iters * 20))   # (first: no staged copy exists yet, so making one shows)
    rp, ci = synth.make_csr(n, nnz, d_max, seed=0, device=dev)
    shapes.append(("reddit FLT32 h=256", rp, ci, n, n, 256, iters))
    bad = []
    for name, rp, ci, nr, nc, h, k in shapes:
        x = synth.features(nc, h, torch.float32, seed=3, device=dev, kind="uniform")
        out = torch.empty((nr, h), dtype=torch.float32, device=dev)
        hds = {}

        def create():
            # (the small product's 256 light tiles lie below the reuse rule: lds_mode = 1 gives it the LDS-staged plan in both libraries, for its whole life)
            if "in place" in name:
                _lib.set_tunable("lds_mode", 1)
            return _lib.group_create(_lib.CSR, _lib.FLT32, [rp.data_ptr()], [ci.data_ptr()], None, [nr], [nc], [ci.numel()], [1], [h], h)

        with parent:
            hds["parent"] = create()
        hds["new"] = create()

        def taken(hd):
            """device memory the library takes for one product (a staged copy of X is an allocation of its own)"""
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr(), st)
            torch.cuda.synchronize()
            return free0 - torch.cuda.mem_get_info()[0]

        in_place = None
        if "in place" in name:
            # this build's first product takes X in place: no allocation; the same product under lds_direct_x = 0 then makes the staged copy
            first = taken(hds["new"])
            old = _lib.set_tunable("lds_direct_x", 0)
            copied = taken(hds["new"])
            _lib.set_tunable("lds_direct_x", old)
            in_place = dict(first_product_bytes=first, lds_direct_x_0_bytes=copied, x_in_place=first == 0 and copied > 0)

        def window(hd):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                _lib.spmm_run_group(hd, [x.data_ptr()], out.data_ptr(), st)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / k

        series = {"parent": [], "new": []}
        for rnd in range(rounds + 1):
            for who in ("parent", "new"):
                if who == "parent":
                    with parent:
                        ms = window(hds[who])
                else:
                    ms = window(hds[who])
                if rnd:   # (the first round of each build is discarded: first touches of the allocator and of the code objects)
                    series[who].append(round(ms, 5))
        with parent:
            runs_parent = _lib.group_lds_runs(hds["parent"])
            _lib.group_free(hds["parent"])
            _lib.set_tunable("lds_mode", 0)
        runs_new = _lib.group_lds_runs(hds["new"])
        _lib.group_free(hds["new"])
        _lib.set_tunable("lds_mode", 0)
        p, q = series["parent"], series["new"]
        extra = 2 if in_place else 0
        ok = statistics.median(q) <= max(p) and runs_new == runs_parent + extra and runs_new == (rounds + 1) * k + extra
        line(section="time", product=name, **(in_place or {}), calls_per_window=k, parent_ms=p, new_ms=q, parent_min=min(p), parent_max=max(p), parent_median=statistics.median(p),
             new_median=statistics.median(q), lds_runs=runs_new, inside_parent_spread_or_below=ok)
        if not ok:
            bad.append(name)
    line(section="time", rounds=rounds, iters=iters, not_passing=bad)
    return len(bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libpygim_hip.so")
    ap.add_argument("--section", default="all", choices=["all", "bits", "time"])
    ap.add_argument("--out", default=None, help="write the lines here as well (profiles/exp_lds_launch.txt)")
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
