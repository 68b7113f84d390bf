#!/bin/bash
# Round measurement on the GPU box (one gpurun call): the GPU suite, the driver's literal bench command, rocprofv3 passes of the same workload
# (kernel trace + stats, SQ counters, FETCH / WRITE in separate --pmc runs), the other workloads, the N = 2 rehearsal.  Outputs under $OUT_ROOT/.
export OUT_ROOT=${OUT_ROOT:-out}      # where this script writes its logs and summaries
TAG=${1:-r02}
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT_ROOT/bench $OUT_ROOT/prof
timeout 900 python3 -m pytest tests -m gpu -q 2>&1 | tail -3 > $OUT_ROOT/pytest_gpu.log; cat $OUT_ROOT/pytest_gpu.log
timeout 600 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT_ROOT/bench/${TAG}_n1.json 2> $OUT_ROOT/bench/${TAG}_n1.err; echo "bench rc=$?"; cut -c1-400 $OUT_ROOT/bench/${TAG}_n1.json
bash tools/gpu_profile.sh ${TAG} kt sq mem -- --workload instanced1m
for wl in flat1m cornell materials1m; do timeout 300 python3 bench.py --full --workload $wl --steps 5 --warmup 2 --no-cpu-baseline > $OUT_ROOT/bench/${TAG}_$wl.json 2> $OUT_ROOT/bench/${TAG}_$wl.err; cut -c1-200 $OUT_ROOT/bench/${TAG}_$wl.json; done
HAR_BENCH_SHARE_GPU=1 HAR_BENCH_BACKEND=gloo timeout 300 python3 bench.py --full --gpus 2 --steps 3 --warmup 1 --no-cpu-baseline > $OUT_ROOT/bench/${TAG}_n2_rehearsal.json 2> $OUT_ROOT/bench/${TAG}_n2_rehearsal.err; echo "n2 rehearsal rc=$?"
timeout -k 5 240 rocprofv3 --kernel-trace --stats -d /tmp/prof_${TAG}_prb -o r -- python3 tools/prb_breakdown.py instanced1m textured > $OUT_ROOT/prof/${TAG}_prb_bench.log 2>&1
python3 tools/rocpd_summary.py $(find /tmp/prof_${TAG}_prb -name '*.db') --json $OUT_ROOT/prof/${TAG}_prb_kt.json > $OUT_ROOT/prof/${TAG}_prb_kt.txt 2>&1
ls $OUT_ROOT/prof | grep ${TAG}
