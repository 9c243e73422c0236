#!/bin/bash
# configs[0] process model: readahead pool size (CTG_IO_READAHEAD 8 default / 16) and the ROI decode pool
# (CTG_IO_THREADS 16 default / 32), twice each.
set -o pipefail
TAG=${1:-r6y}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG; mkdir -p $O
i=0
for rep in 0 1; do
  for v in "CTG_IO_READAHEAD=8" "CTG_IO_READAHEAD=16" "CTG_IO_READAHEAD=16 CTG_IO_THREADS=32"; do
    env $v timeout -k 10 400 python bench.py --full --config 0 --steps 3 --warmup 1 --no-cpu-baseline > $O/bench_c0_$i.json 2> $O/bench_c0_$i.err || { echo "C0 FAILED"; tail -5 $O/bench_c0_$i.err; exit 1; }
    python -c "
import json; d=json.load(open('$O/bench_c0_$i.json')); s=d['process_split_last_step']
print('$v', d['value'], d['ms_per_step'], 'threads', d['thread_mode']['value'], 'cpu_layout', d['process_mode_cpu_layout']['value'], {k: round(v, 3) for k, v in d['stage_s'].items()}, {k: (v.get('body_s_max'), v.get('exit_s_max')) for k, v in s.items() if isinstance(v, dict) and 'body_s_max' in v})"
    i=$((i+1))
  done
done
