#!/bin/bash
# bench.py --full three times: the dp_form legs of the PPO cycle (host enqueue per cycle under graph replay) run to run.  Logs go to $OUT (default
# gpu_logs/); the first failing run ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT="${OUT:-gpu_logs}"; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { echo "build failed: $OUT/build.log"; exit 1; }
for i in 1 2 3; do
  timeout -k 10 900 python bench.py --full | grep '^{"metric"' | python -c "
import json,sys
j=json.loads(sys.stdin.readline()); s=j['secondary']
print('vp', j['ms_per_step'], [(m['dtype'], m['ms_per_step']) for m in j['precision_modes']], 'ppo', s['ms_per_cycle'], s['host_enqueue_ms_per_cycle'])
print({k:(v.get('ms_per_cycle'), v.get('host_enqueue_ms_per_cycle'), v.get('update_graph_replays')) for k,v in s['dp_form'].items() if isinstance(v,dict) and 'ms_per_cycle' in v})"
  rc=$?
  [ $rc -eq 0 ] || { echo "bench run $i rc=$rc: stopping"; exit $rc; }
done
