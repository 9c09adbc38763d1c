#!/bin/bash
# quick GPU check used during kernel work: window-path tests, then a short default bench (config 3) with the per-kernel table
# usage: bash tools/quick_gpu.sh <tag> [pytest targets...]; logs and the bench line under $OUT_DIR/<tag> (default out/<tag>)
tag=${1:-q}; shift
O=${OUT_DIR:-out}/$tag; mkdir -p $O
targets=${@:-tests/test_gpu_window.py}
timeout -k 10 900 python -m pytest $targets -x -q > $O/pytest.log 2>&1; rc=$?
tail -5 $O/pytest.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full --no-cpu-baseline --no-host-path --steps 10 > $O/bench.json 2> $O/bench.err || { tail -5 $O/bench.err; exit 1; }
python - <<P
import json
d=json.load(open("$O/bench.json"))
print("ms_per_step", d["ms_per_step"], "value", d["value"], "kernel_sum", d["gpu_kernel_ms_per_step_total"], "launches", d["launches_per_step"])
print(" ".join("%s=%.2f" % (k.split("/")[1] if k.startswith("collapse") else k, v) for k, v in list(d["kernel_ms_per_step"].items())[:22]))
P
