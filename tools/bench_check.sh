#!/bin/bash
# the driver's bench commands, literally (N = 1) and the self-launching N = 2 rehearsal on one shared GPU (gloo: never a reported number)
export OUT_ROOT=${OUT_ROOT:-out}      # where this script writes its logs and summaries
mkdir -p $OUT_ROOT/bench
timeout 600 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT_ROOT/bench/n1.out 2> $OUT_ROOT/bench/n1.err; echo "n1 rc=$?"; cat $OUT_ROOT/bench/n1.err | grep -v amdgpu.ids | tail -20; cut -c1-3000 $OUT_ROOT/bench/n1.out
HAR_BENCH_SHARE_GPU=1 HAR_BENCH_BACKEND=gloo timeout 600 python3 bench.py --full --gpus 2 --steps 3 --warmup 1 --no-cpu-baseline > $OUT_ROOT/bench/n2_rehearsal.out 2> $OUT_ROOT/bench/n2_rehearsal.err; echo "n2 rc=$?"; tail -5 $OUT_ROOT/bench/n2_rehearsal.err; cut -c1-600 $OUT_ROOT/bench/n2_rehearsal.out
