#!/bin/bash
# Probe A/B: wave-aggregated fill counter (variants/libctg_agg.so) and the overflow probe inlined
# (variants/libctg_inl.so) against the product build; parity subset on each variant first.
set -o pipefail
TAG=${1:-r6h}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG; mkdir -p $O
for v in agg inl; do
  CTG_LIB=variants/libctg_$v.so timeout -k 10 600 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py -m gpu -x -v \
    --timeout 300 --timeout-method thread -k "golden or narrow or configs4 or configs1 or fresh or heavy" > $O/pytest_$v.log 2>&1
  rc=$?; echo "$v PYTEST rc=$rc"; tail -n 1 $O/pytest_$v.log; [ $rc -eq 0 ] || exit 1
done
bash tools/gpu_ab_sets.sh $TAG/ab "2 4 1" - CTG_LIB=variants/libctg_agg.so CTG_LIB=variants/libctg_inl.so - CTG_LIB=variants/libctg_agg.so CTG_LIB=variants/libctg_inl.so
O=gpurun_out/$TAG
timeout -k 10 900 python bench.py --full --config 0 --no-cpu-baseline > $O/bench_c0.json 2> $O/bench_c0.err || { echo "C0 FAILED"; tail -5 $O/bench_c0.err; exit 1; }
python -c "
import json; d=json.load(open('$O/bench_c0.json'))
print('C0', d['value'], d['ms_per_step'], 'threads', d['thread_mode']['value'], d['config']['output_bytes'])
print(json.dumps(d['process_split_last_step']))"
