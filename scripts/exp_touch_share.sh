#!/bin/bash
# Shared touches of the 8-wave code-stream kernels (lds_touch_share) under 2 / 4 slices per XCD: the bench workload, INT16 h = 256, the
# one-GPU GCN config's dequantising aggregation, and one counters-only pass per arrangement.  Writes $OUT (default results/touch_share/).
# Every step runs under its own time limit and the script stops at the first step that fails.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
out=${OUT:-$R/results/touch_share}
mkdir -p $out
cd $R
declare -A ARR=( [sx1]="lds_xcd_slices=1,lds_touch_share=0" [sx2_share0]="lds_xcd_slices=2,lds_touch_share=0" [sx2_share1]="lds_xcd_slices=2,lds_touch_share=1"
                 [sx4_share0]="lds_xcd_slices=4,lds_touch_share=0" [sx4_share1]="lds_xcd_slices=4,lds_touch_share=1" )
for i in 1 2 3; do
  for tag in sx2_share0 sx2_share1 sx4_share1 sx4_share0; do
    PYGIM_TUNE=${ARR[$tag]} timeout -k 10 200 python3 bench.py --gpus 1 --steps 20 --warmup 5 > $out/bench_${tag}_$i.json 2> $out/bench_${tag}_$i.err || exit $?
  done
done
for i in 1 2 3 4 5; do
  for tag in sx1 sx2_share0 sx2_share1; do
    timeout -k 10 200 python3 scripts/exp_code_geo.py --dtype i16 --h 256 --reps 31 --tune ${ARR[$tag]} 0:0:0:0:0 2>&1 | grep -v amdgpu.ids > $out/i16_${tag}_$i.txt || exit $?
  done
done
for i in 1 2 3; do
  for tag in sx2_share0 sx2_share1; do
    PYGIM_TUNE=${ARR[$tag]} timeout -k 10 300 python3 scripts/exp_cfg_one.py c4 2>&1 | grep -v amdgpu.ids > $out/gcn_${tag}_$i.txt || exit $?
  done
done
# counters on their own: no tracing beside --pmc
for tag in sx2_share0 sx2_share1 sx4_share1; do
  timeout -k 10 300 rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCC_REQ_sum --output-format csv -d $out/pmc_$tag -- python3 scripts/exp_code_geo.py --reps 2 --tune ${ARR[$tag]} 0:0:0:0:0 > $out/pmc_$tag.log 2>&1 || exit $?
done
python3 - "$out" <<'PY' | tee $out/summary.txt
import collections, csv, glob, json, os, sys
out = sys.argv[1]
for f in sorted(glob.glob(out + "/bench_*.json")):
    d = json.loads(open(f).read().strip().splitlines()[-1])
    g = d["roofline"]["on_chip"]["geometry"]
    print(os.path.basename(f), d["ms_per_step_median"], d["roofline"]["kernel_ms"], "xcd_slices", g["xcd_slices"], "touch_share", g["touch_share"])
for f in sorted(glob.glob(out + "/i16_*.txt")):
    print(os.path.basename(f), open(f).read().strip().splitlines()[-1][:75])
for f in sorted(glob.glob(out + "/gcn_*.txt")):
    d = json.loads(open(f).read().strip().splitlines()[0])
    print(os.path.basename(f), d["ms_per_forward"], d["roofline"]["kernel_ms"])
for d in sorted(glob.glob(out + "/pmc_*/")):
    agg = collections.defaultdict(lambda: [0.0, 0])
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_lds_code8_f32" in row["Kernel_Name"]:
                a = agg[row["Counter_Name"]]; a[0] += float(row["Counter_Value"]); a[1] += 1
    print(os.path.basename(d.rstrip("/")), " ".join(f"{k} = {v[0] / max(v[1], 1):.0f} (mean of {v[1]} dispatches)" for k, v in sorted(agg.items())))
PY
