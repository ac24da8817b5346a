#!/bin/bash
# bench lines (+ per-op table) for a list of workloads.  Usage: tools/gpu_bench.sh <tag> wl1 wl2 ...   (output under $OUT, default out/)
TAG=$1; shift
OUT=${OUT:-out}
mkdir -p $OUT
for WL in "$@"; do
  PV_BENCH_VERBOSE=2 python bench.py --full --workload $WL --steps 10 --warmup 3 > $OUT/${TAG}_bench_${WL}.json 2> $OUT/${TAG}_bench_${WL}.err
  cat $OUT/${TAG}_bench_${WL}.json; grep -v amdgpu.ids $OUT/${TAG}_bench_${WL}.err | grep -v "^  op" | tail -32
done
