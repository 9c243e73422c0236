#!/bin/bash
# Round 6, first GPU call: the bounds-checked parity run (CTG_DIAG build, one
# fresh process, tests/test_gpu_parity.py -- small cases), the whole GPU suite
# on the product build, bench.py --gpus 2 launching its own ranks (gloo, both
# on device 0), --gpus 2 over RCCL on a one-GPU box (must refuse, rc != 0),
# and the default bench line.
#   tools/gpu.sh bash tools/gpu_r6a.sh TAG
set -o pipefail
TAG=${1:-r6a}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out/$TAG
mkdir -p $O
git_sha=$(cat .tree_sha 2>/dev/null || echo unknown); echo "$git_sha" > $O/TREE
CTG_LIB=variants/libctg_diag.so CTG_BOUNDS_CHECK=1 timeout -k 10 600 \
  python -u -m pytest tests/test_gpu_parity.py -m gpu -x -v --timeout 120 --timeout-method thread > $O/pytest_bounds.log 2>&1
rc=$?; echo "BOUNDS rc=$rc"; tail -3 $O/pytest_bounds.log; grep -E "FAILED|bounds check" $O/pytest_bounds.log | head; [ $rc -eq 0 ] || exit 1
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1
rc=$?; echo "PYTEST rc=$rc"; tail -3 $O/pytest_gpu.log; grep -E "FAILED|Error" $O/pytest_gpu.log | head -20; [ $rc -eq 0 ] || exit 1
timeout -k 10 300 python bench.py --gpus 2 --backend gloo --device 0 --config 1 --steps 5 --warmup 1 --no-cpu-baseline \
  > $O/bench_n2_gloo_c1.json 2> $O/bench_n2_gloo_c1.err
rc=$?; echo "N2 gloo rc=$rc"; cat $O/bench_n2_gloo_c1.json | cut -c1-400; [ $rc -eq 0 ] || { tail -20 $O/bench_n2_gloo_c1.err; exit 1; }
timeout -k 10 120 python bench.py --gpus 2 --config 1 --steps 5 > $O/bench_n2_nccl.json 2> $O/bench_n2_nccl.err
echo "N2 nccl on one device rc=$? (expect 2): $(cat $O/bench_n2_nccl.err | tail -1)"
timeout -k 10 300 python bench.py --full > $O/bench.json 2> $O/bench.err || { tail -5 $O/bench.err; exit 1; }
cut -c1-600 $O/bench.json
