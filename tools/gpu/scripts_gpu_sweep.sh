#!/bin/bash
# tuning sweep of the range-scan launch geometry (prints one line per point; files under $BENCH_OUT, default bench_out/)
out=${BENCH_OUT:-bench_out}
mkdir -p $out
for sb in 1280 2048 2560 4096; do for it in 2048 4096 8192; do for tq in 32 64 128; do
timeout -k 10 120 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --scan-blocks $sb --scan-items $it --tile-q $tq > $out/sweep.json 2>> $out/bench_err.log
python - "$sb" "$it" "$tq" "$out/sweep.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[4]))
print("blocks", sys.argv[1], "items", sys.argv[2], "tile_q", sys.argv[3], "scan_ms %.4f step_ms %.4f" % (d["kernel_ms"]["nn_scan"], d["ms_per_step"]))
PY
done; done; done
