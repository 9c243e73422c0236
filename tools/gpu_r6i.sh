#!/bin/bash
# configs[0] under the process model: page-locked arenas as hipHostRegister-ed transparent-huge-page memory (default)
# against hipHostMalloc (CTG_HOST_ALLOC=hip); GPU suite first (this tree's product build).
set -o pipefail
TAG=${1:-r6i}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG; mkdir -p $O
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1
rc=$?; echo "PYTEST rc=$rc"; tail -n 1 $O/pytest_gpu.log; grep -E "FAILED|Error" $O/pytest_gpu.log | head -20; [ $rc -eq 0 ] || exit 1
for v in default hip default; do
  if [ $v = hip ]; then export CTG_HOST_ALLOC=hip; else unset CTG_HOST_ALLOC; fi
  timeout -k 10 900 python bench.py --full --config 0 --no-cpu-baseline > $O/bench_c0_$v.json 2> $O/bench_c0_$v.err || { echo "C0 $v FAILED"; tail -5 $O/bench_c0_$v.err; exit 1; }
  python -c "
import json; d=json.load(open('$O/bench_c0_$v.json'))
print('C0 $v', d['value'], d['ms_per_step'], 'threads', d['thread_mode']['value'], 'stages', d['stage_s'])
print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk in ('start_s_max', 'body_s_max', 'exit_s_max')} for k, v in d['process_split_last_step'].items() if k.startswith('_') and 'profile' not in k}))"
done
