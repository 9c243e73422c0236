#!/bin/bash
# bench.py --gpus N self-launch rehearsals on one GPU (gloo, every rank on device 0): configs[2] at N=2, configs[1]
# at N=4; configs[0] under the process model with the gzip statistics companion and its CPU baseline; the job
# process exit cost on this tree (tools/exit_cost.py).
set -o pipefail
TAG=${1:-r6g}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG; mkdir -p $O
timeout -k 10 400 python bench.py --gpus 2 --backend gloo --device 0 --config 2 --steps 5 --warmup 1 --no-cpu-baseline \
  > $O/bench_n2_gloo_c2.json 2> $O/bench_n2_gloo_c2.err || { echo "N2 c2 FAILED"; tail -5 $O/bench_n2_gloo_c2.err; exit 1; }
grep '^{' $O/bench_n2_gloo_c2.json | cut -c1-300
timeout -k 10 300 python bench.py --gpus 4 --backend gloo --device 0 --config 1 --steps 5 --warmup 1 --no-cpu-baseline \
  > $O/bench_n4_gloo_c1.json 2> $O/bench_n4_gloo_c1.err || { echo "N4 c1 FAILED"; tail -5 $O/bench_n4_gloo_c1.err; exit 1; }
grep '^{' $O/bench_n4_gloo_c1.json | cut -c1-300
timeout -k 10 900 python bench.py --full --config 0 > $O/bench_c0.json 2> $O/bench_c0.err || { echo "C0 FAILED"; tail -5 $O/bench_c0.err; exit 1; }
python -c "
import json; d=json.load(open('$O/bench_c0.json'))
print('C0', d['value'], d['ms_per_step'], 'threads', d['thread_mode']['value'], 'cpu', d['cpu_baseline']['value'], d['config']['output_bytes'])
print(json.dumps(d['process_split_last_step']))"
timeout -k 10 300 python tools/exit_cost.py > $O/exit_cost.jsonl 2> $O/exit_cost.err || { echo "EXIT COST FAILED"; tail -5 $O/exit_cost.err; exit 1; }
cat $O/exit_cost.jsonl
