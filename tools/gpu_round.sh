#!/bin/bash
# One GPU-box visit: parity tests, bench line, rocprofv3 kernel stats.  Usage: tools/gpu_round.sh <tag> [workload]   (output under $OUT, default out/)
TAG=${1:-r1}
WL=${2:-x3d_m}
R=$PWD
OUT=$(realpath -m ${OUT:-out})
mkdir -p $OUT
PV_RUN_SLOW=1 python -m pytest tests -m gpu -x -q --durations=40 > $OUT/${TAG}_pytest.log 2>&1
tail -5 $OUT/${TAG}_pytest.log
PV_BENCH_VERBOSE=1 python bench.py --full --workload $WL --steps 20 --warmup 5 > $OUT/${TAG}_bench_${WL}.json 2> $OUT/${TAG}_bench_${WL}.err
cat $OUT/${TAG}_bench_${WL}.json; tail -30 $OUT/${TAG}_bench_${WL}.err
cd /tmp; export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_${WL} -o ${WL} -- python $R/bench.py --full --workload $WL --steps 5 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_rocprof_${WL}.log 2>&1
tail -3 $OUT/${TAG}_rocprof_${WL}.log
find $OUT/prof_${TAG}_${WL} -name '*stats*' | head
