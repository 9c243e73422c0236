#!/bin/bash
# configs[0] process model: job processes per task (graph, block features, merge features), twice each.
set -o pipefail
TAG=${1:-r6z}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG; mkdir -p $O
i=0
for rep in 0 1; do
  for j in 1,1,1 2,1,1 4,1,1 2,2,2 4,2,2; do
    timeout -k 10 400 python bench.py --full --config 0 --steps 3 --warmup 1 --no-cpu-baseline --c0-jobs $j > $O/bench_c0_$i.json 2> $O/bench_c0_$i.err || { echo "C0 FAILED"; tail -5 $O/bench_c0_$i.err; exit 1; }
    python -c "
import json; d=json.load(open('$O/bench_c0_$i.json')); s=d['process_split_last_step']
print('$j', d['value'], d['ms_per_step'], {k: round(v, 3) for k, v in d['stage_s'].items()}, {k: (v.get('start_s_max'), v.get('body_s_max'), v.get('exit_s_max')) for k, v in s.items() if isinstance(v, dict) and 'body_s_max' in v})"
    i=$((i+1))
  done
done
