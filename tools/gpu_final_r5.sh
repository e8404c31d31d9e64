#!/bin/bash
# Round-5 evidence, one gpurun call per PART (1: GPU suite + the PMC passes; 2: the bench line, phases, the 3.9 GB run).
# Every step is bounded by `timeout -k`; outputs under $OUT/r5_*; nothing reads stdin.
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-results}; export OUT  # every output of this script (and of the scripts it calls) goes here
mkdir -p "$OUT"
exec </dev/null
export TAG=r5
case "$1" in
1)
  timeout -k 5 600 python -X faulthandler -m pytest tests -m gpu -q > $OUT/r5_final_pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -3 $OUT/r5_final_pytest_gpu.log | cut -c1-200
  bash tools/gpu_pmc.sh regex1g 2>&1 | tail -6 | cut -c1-400
  SKIP_KT=1 bash tools/gpu_pmc.sh basic1g 2>&1 | tail -4 | cut -c1-400
  SKIP_KT=1 bash tools/gpu_pmc.sh encode 2>&1 | tail -4 | cut -c1-400
  ;;
2)
  cp $OUT/r5_regex1g_pmc.json $OUT/r5_basic1g_pmc.json $OUT/r5_encode_pmc.json profiles/ 2>/dev/null
  timeout -k 5 900 python bench.py --full > $OUT/r5_final_bench.json 2> $OUT/r5_final_bench.err; echo "bench rc=$?"; cut -c1-700 $OUT/r5_final_bench.json; tail -2 $OUT/r5_final_bench.err | cut -c1-300
  ITER_NPY=$OUT/r5_final_regex1g_iter_us.npy timeout -k 5 300 python tools/iter_profile.py regex1g > $OUT/r5_final_regex1g_iter_profile.json 2> $OUT/r5_iter.err; echo "iter rc=$?"
  rm -rf $OUT/r5_prof; timeout -k 5 400 rocprofv3 --kernel-trace --stats -d $OUT/r5_prof -o run -- python tools/train_n.py regex1g 31744 > $OUT/r5_prof.log 2>&1; echo "prof rc=$?"
  db=$(ls $OUT/r5_prof/*/*.db $OUT/r5_prof/*.db 2>/dev/null | head -1)
  [ -n "$db" ] && python tools/rocpd_stats.py $db > $OUT/r5_final_regex1g_kernel_stats_one_train.csv && python tools/rocpd_phases.py $db 0 123 261 453 746 1301 2483 3529 1073741824 > $OUT/r5_final_regex1g_phases_by_step.json
  rm -rf $OUT/r5_prof
  ;;
3)
  timeout -k 5 900 python bench.py --full --bytes 3900000000 --steps 2 --warmup 1 --cpu-iters 0 --secondary none > $OUT/r5_big_3p9gb_bench.json 2> $OUT/r5_big.err; echo "big rc=$?"; cut -c1-900 $OUT/r5_big_3p9gb_bench.json; tail -2 $OUT/r5_big.err | cut -c1-300
  ;;
esac
