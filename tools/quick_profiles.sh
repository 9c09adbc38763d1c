#!/bin/bash
# other single-GPU shapes through bench.py (config 2, config 4's per-rank shape, config 5's per-rank shape): ms per step and top kernels
# usage: bash tools/quick_profiles.sh c2 c4 c5; lines under $OUT_DIR/qp (default out/qp)
O=${OUT_DIR:-out}/qp; mkdir -p $O
for p in "$@"; do
  timeout -k 10 300 python bench.py --full --profile $p --no-cpu-baseline --no-host-path --steps 20 > $O/$p.json 2> $O/$p.err || { tail -3 $O/$p.err; continue; }
  python - <<P
import json
d=json.load(open("$O/$p.json"))
print("$p", "ms_per_step", d["ms_per_step"], "value %.3g" % d["value"], "kernel_sum", d["gpu_kernel_ms_per_step_total"], "launches", d["launches_per_step"])
print("   "+" ".join("%s=%.3f" % (k.split("/")[1] if k.startswith("collapse") else k, v) for k, v in list(d["kernel_ms_per_step"].items())[:14]))
P
done
