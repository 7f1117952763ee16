#!/bin/bash
# Interleaved A/B of two builds of the library on one box:  tools/ab_lib.sh VARIANT_LIB [PAIRS] [extra bench.py args]
# A = the product library, B = VARIANT_LIB (through FVQA_LIB). One C2 bench line per arm per pair (--full: with the roofline passes)
# -> $OUT/ab_*.json, OUT defaults to bench_out/ab
v=$1; n=${2:-3}; shift; shift
out=${OUT:-bench_out/ab}
mkdir -p $out
for i in $(seq 1 $n); do
  python bench.py --steps 20 --warmup 5 --full --no_cpu_baseline --no_other_configs "$@" > $out/ab_A$i.json 2> $out/ab_A$i.err || exit 1
  FVQA_LIB=$v python bench.py --steps 20 --warmup 5 --full --no_cpu_baseline --no_other_configs "$@" > $out/ab_B$i.json 2> $out/ab_B$i.err || exit 1
done
python - <<PY
import json, glob
for f in sorted(glob.glob("$out/ab_[AB]*.json")):
    d = json.loads([l for l in open(f) if l.startswith("{")][-1])
    sh = {k: round(v["avg_launch_us"], 1) for k, v in d["roofline"].get("per_instantiation", {}).items()}
    print(f[-8:-5], "%.3f ms  loss %s" % (d["ms_per_step"], d.get("loss", d.get("final_loss", ""))), sh)
PY
