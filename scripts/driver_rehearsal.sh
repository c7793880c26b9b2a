#!/bin/bash
# The round-end driver sequence on the GPU box, from the tree as it travels (built here first with
# `python -c "import __graft_entry__ as e; e.build()"`): pytest -m gpu, smoke(), bench.py --gpus 1,
# then a rocprofv3 kernel-trace --stats run of the same bench command.  Each GPU step has its own
# time limit and the script stops at the first failure.  Outputs under $OUT/final_*.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${OUT:-out}"; mkdir -p "$OUT"; export TMPDIR=/tmp
stop() { echo "STOP $1 (exit $2)"; exit "$2"; }
timeout -k 10 1200 python -u -m pytest tests -x -q -m gpu --timeout 600 --timeout-method thread --durations=12 \
    > $OUT/final_pytest_gpu.log 2>&1 || { tail -30 $OUT/final_pytest_gpu.log; stop pytest $?; }
tail -16 $OUT/final_pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as e; e.smoke()" > $OUT/final_smoke.log 2>&1 || stop smoke $?
tail -1 $OUT/final_smoke.log
timeout -k 10 400 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/final_bench.log 2>&1 || stop bench $?
tail -1 $OUT/final_bench.log | cut -c1-300
rm -rf $OUT/final_prof
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/final_prof -o run --output-format csv -- \
    python3 bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > $OUT/final_prof.log 2>&1 || stop prof $?
grep path_kernel $OUT/final_prof/run_kernel_stats.csv | cut -c1-200
echo REHEARSAL_DONE
