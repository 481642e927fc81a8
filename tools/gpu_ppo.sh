#!/bin/bash
# PPO / environment GPU tests, then the bench's PPO leg (`secondary`, a --full leg).  Logs go to $OUT (default gpu_logs/); the first failing step ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT="${OUT:-gpu_logs}"; mkdir -p "$OUT"
timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { echo "build failed: $OUT/build.log"; exit 1; }
timeout -k 10 900 python -m pytest tests/test_gpu_ppo.py tests/test_gpu_ppo_cli.py tests/test_gpu_env.py -m gpu -q --tb=short > "$OUT/t_ppo.log" 2>&1; rc=$?
grep -n -i "fault\|Error\|passed\|failed\|^E  \|warn" "$OUT/t_ppo.log" | head -30
[ $rc -eq 0 ] || { echo "pytest rc=$rc: stopping"; exit $rc; }
timeout -k 10 600 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline | grep '^{"metric"' | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(json.dumps(d['secondary'])[:700])" || { rc=$?; echo "bench rc=$rc"; exit $rc; }
