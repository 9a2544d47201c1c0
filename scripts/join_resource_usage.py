"""Join two resource_usage.txt files (`make -C pygim_amd/csrc asm` on two commits) by kernel name:
    python scripts/join_resource_usage.py OLD NEW [--prefix k_row_gather,k_gat_,...] [--added k_softmax_] > profiles/NAME.txt
One line per kernel whose unqualified name starts with one of the prefixes: VGPRs, SGPRs, scratch bytes per lane and waves per SIMD,
old and new.  Exits 1 when the two sides do not hold the same kernels, when scratch grows or when waves per SIMD drop anywhere.
--added: prefixes of kernels that exist on the new side alone (a new family): they are listed after the joined ones with their own
numbers, must not use scratch, and do not count as a difference of the kernel sets.  --prefix "" joins every kernel."""
import argparse
import re
import sys

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "waves"))


def parse(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def short(mangled):
    """_ZN5pygim12k_gat_gatherI... -> k_gat_gather"""
    m = re.match(r"_ZN5pygim(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--prefix", default="k_row_gather,k_gat_,k_multi_,k_sa_,k_gatv2_")
    ap.add_argument("--added", default="")
    args = ap.parse_args()
    pre = tuple(args.prefix.split(","))
    add = tuple(a for a in args.added.split(",") if a)
    old, new = ({k: v for k, v in parse(p).items() if short(k).startswith(pre)} for p in (args.old, args.new))
    added = {k: new.pop(k) for k in sorted(new) if add and short(k).startswith(add) and k not in old}
    bad = []
    if set(old) != set(new):
        bad.append(f"kernel sets differ: only old {sorted(set(old) - set(new))}, only new {sorted(set(new) - set(old))}")
    rows = sorted(set(old) & set(new), key=lambda k: (short(k), k))
    print("# vgpr sgpr scratch waves/SIMD: old | new | kernel (mangled)")
    for k in rows:
        o, n = old[k], new[k]
        mark = ""
        if n["scratch"] > o["scratch"]:
            mark += "  SCRATCH GROWS"
        if n["waves"] < o["waves"]:
            mark += "  WAVES DROP"
        if mark:
            bad.append(k + mark)
        print(f"{o['vgpr']:4d} {o['sgpr']:4d} {o['scratch']:4d} {o['waves']:2d} | {n['vgpr']:4d} {n['sgpr']:4d} {n['scratch']:4d} {n['waves']:2d} | {k}{mark}")
    up = sum(new[k]["waves"] > old[k]["waves"] for k in rows)
    print(f"# {len(rows)} kernels; waves per SIMD higher in {up}, lower in {sum(new[k]['waves'] < old[k]['waves'] for k in rows)}; "
          f"scratch above 0: old {sum(old[k]['scratch'] > 0 for k in rows)}, new {sum(new[k]['scratch'] > 0 for k in rows)}")
    if added:
        print("# new kernels: vgpr sgpr scratch waves/SIMD | kernel (mangled)")
        for k, n in sorted(added.items(), key=lambda kv: (short(kv[0]), kv[0])):
            mark = "  USES SCRATCH" if n["scratch"] > 0 else ""
            if mark:
                bad.append(k + mark)
            print(f"{n['vgpr']:4d} {n['sgpr']:4d} {n['scratch']:4d} {n['waves']:2d} | {k}{mark}")
        print(f"# {len(added)} new kernels; scratch above 0: {sum(n['scratch'] > 0 for n in added.values())}")
    for b in bad:
        print("FAIL:", b, file=sys.stderr)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
