#!/bin/bash
# Kernel and VP-engine GPU tests, then the bench line with its roofline and precision modes (--full).  Logs go to $OUT (default gpu_logs/); the first
# failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT="${OUT:-gpu_logs}"; mkdir -p "$OUT"
timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { echo "build failed: $OUT/build.log"; exit 1; }
timeout -k 10 900 python -m pytest tests/test_gpu_kernels.py tests/test_gpu_vp_engine.py -m gpu -q --tb=short > "$OUT/t_vp.log" 2>&1; rc=$?
grep -n -i "fault\|Error\|passed\|failed\|^E  " "$OUT/t_vp.log" | head -30
[ $rc -eq 0 ] || { echo "pytest rc=$rc: stopping"; exit $rc; }
timeout -k 10 600 python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline | grep '^{"metric"' | cut -c1-1200 || { rc=$?; echo "bench rc=$rc"; exit $rc; }
