#!/bin/bash
# Closing check of the committed tree: GPU suite, smoke, the default line and the configs[0] line with its
# cpu_baseline (in-body and process start-to-exit rates).
set -o pipefail
TAG=${1:-final2}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG; mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 400 --timeout-method thread > $O/pytest_gpu.log 2>&1; rc=$?
echo "PYTEST rc=$rc"; tail -1 $O/pytest_gpu.log; grep FAILED $O/pytest_gpu.log | head; [ $rc -eq 0 ] || exit 1
timeout -k 10 200 python -c 'import __graft_entry__ as g; g.smoke()' > $O/smoke.log 2>&1 && echo SMOKE_OK || exit 1
timeout -k 10 300 python bench.py --full > $O/bench.json 2> $O/bench.err && echo BENCH_OK && python -c "import json; d=json.load(open('$O/bench.json')); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'])" || exit 1
timeout -k 10 500 python bench.py --full --config 0 --steps 3 --warmup 1 > $O/bench_c0.json 2> $O/bench_c0.err || { echo "C0 FAILED"; exit 1; }
python -c "import json; d=json.load(open('$O/bench_c0.json')); print('C0', d['value'], d['ms_per_step'], d['cpu_baseline']['value'], d['cpu_baseline']['with_process_start_exit'], d['thread_mode']['value'])"
