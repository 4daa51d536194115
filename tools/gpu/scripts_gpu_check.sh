#!/bin/bash
# standard GPU check: parity tests, then a short bench; prints the kernel split (files under $BENCH_OUT, default bench_out/)
out=${BENCH_OUT:-bench_out}
mkdir -p $out
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $out/pytest_gpu.log 2>&1
tail -4 $out/pytest_gpu.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline "$@" > $out/bench_tmp.json 2>> $out/bench_err.log
python - "$out/bench_tmp.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print("edges/s %.4g  ms/step %.4f  kernels %s  hbm_frac %.3f" % (d["value"], d["ms_per_step"], {k: round(v, 4) for k, v in d["kernel_ms"].items()}, d["roofline"]["frac"]))
PY
