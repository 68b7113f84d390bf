export OUT_ROOT=${OUT_ROOT:-out}      # where this script writes its logs and summaries
cd ${GRAFT_REPO_ROOT:-.}
export TMPDIR=/tmp
mkdir -p $OUT_ROOT/r03 $OUT_ROOT/prof
timeout 300 python -m pytest tests -m gpu -q > $OUT_ROOT/r03/gpu_suite6.log 2>&1; tail -2 $OUT_ROOT/r03/gpu_suite6.log
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT_ROOT/r03/bench_final4.json 2> $OUT_ROOT/r03/bench_final4.err; tail -1 $OUT_ROOT/r03/bench_final4.err
bash tools/gpu_profile.sh r03_instanced1m kt mem sq -- --workload instanced1m
head -6 $OUT_ROOT/prof/r03_instanced1m_kt.txt
python - <<'PY'
import json, os
d = json.loads(open(os.environ["OUT_ROOT"] + "/r03/bench_final4.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"].get("profile_check"), (d.get("prb_adjoint") or {}).get("value"), (d.get("secondary") or {}).get("value"), (d.get("cpu_baseline") or {}).get("value"))
PY
