#!/bin/bash
# One gpurun call: parity tests, smoke, benches, optional rocprof kernel trace.
# Every step is bounded by `timeout -k`; nothing here reads stdin.
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-results}; export OUT  # every output of this script (and of the scripts it calls) goes here
mkdir -p "$OUT"
exec </dev/null
if [ -z "$SKIP_TESTS" ]; then
timeout -k 5 ${TEST_TIMEOUT:-500} python -X faulthandler -m pytest tests -m gpu -x -q ${PYTEST_ARGS} > $OUT/pytest_gpu.log 2>&1
echo "pytest rc=$?"; tail -15 $OUT/pytest_gpu.log
timeout -k 5 200 python __graft_entry__.py --smoke > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -3 $OUT/smoke.log
fi
if [ -n "$BENCH_SMALL" ]; then
timeout -k 5 300 python bench.py --full --bytes 10000000 --vocab 1024 --steps 2 --warmup 1 > $OUT/bench_small.log 2>&1; echo "bench_small rc=$?"; tail -2 $OUT/bench_small.log
fi
if [ -n "$BENCH_FULL" ]; then
timeout -k 5 600 python bench.py --full ${BENCH_ARGS} > $OUT/bench_full.log 2>&1; echo "bench_full rc=$?"; tail -2 $OUT/bench_full.log
fi
if [ -n "$BENCH_RECOUNT" ]; then
timeout -k 5 600 python bench.py --full --mode 0 --steps 1 --warmup 1 > $OUT/bench_recount.log 2>&1; echo "bench_recount rc=$?"; tail -2 $OUT/bench_recount.log
fi
if [ -n "$PROF" ]; then
rm -rf $OUT/prof
timeout -k 5 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run -- python bench.py --full --steps 1 --warmup 0 --cpu-iters 0 ${PROF_ARGS} > $OUT/prof_bench.log 2>&1
echo "prof rc=$?"; tail -2 $OUT/prof_bench.log
ls -la $OUT/prof
fi
