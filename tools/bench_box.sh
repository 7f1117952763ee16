#!/bin/bash
# One default bench line (C2 + --full: roofline passes and other-config legs, no CPU baseline) tagged with the box it ran on:
#   tools/bench_box.sh TAG -> $OUT/box_TAG.json (the line) + box_TAG.txt (GPU unique id); OUT defaults to bench_out/box.
#   Run it once per box to be compared.
t=${1:-x}; out=${OUT:-bench_out/box}; mkdir -p $out
(hostname; rocm-smi --showuniqueid 2>/dev/null | grep -i "unique id") > $out/box_$t.txt
python bench.py --steps 20 --warmup 5 --full --no_cpu_baseline > $out/box_$t.json 2> $out/box_$t.err
python - <<PY
import json
d=json.loads([l for l in open("$out/box_$t.json") if l.startswith("{")][-1])
print("$t", open("$out/box_$t.txt").read().split()[-1], "%.1f samples/s %.3f ms step %.4f gemm %.4f" % (d["value"], d["ms_per_step"], d["step_roofline"]["frac"], d["roofline"]["frac"]),
      {k: round(v["samples_per_s"], 1) for k, v in d.get("other_configs", {}).items()}, d.get("invalid", ""))
PY
