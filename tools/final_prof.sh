export OUT_ROOT=${OUT_ROOT:-out}      # where this script writes its logs and summaries
cd ${GRAFT_REPO_ROOT:-.}
export TMPDIR=/tmp
mkdir -p $OUT_ROOT/r03 $OUT_ROOT/prof
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT_ROOT/r03/bench_final.json 2> $OUT_ROOT/r03/bench_final.err
tail -3 $OUT_ROOT/r03/bench_final.err
bash tools/gpu_profile.sh r03_instanced1m kt mem sq -- --workload instanced1m
# PRB step (record tape, default build)
cat > /tmp/prb_only.py <<'PY'
import sys, torch
sys.path.insert(0, ".")
import mitsuba3_amd as mi
mi.set_variant("hip_ad_rgb")
d = mi.instanced_spheres_scene(width=512, height=512, spp=256, textured=True)
d["integrator"] = {"type": "prb", "max_depth": 8, "rr_depth": 5, "emitter_gradients": True}
scene = mi.load_dict(d); integ = scene.integrator()
g = torch.full((512, 512, 3), 1.0 / (512 * 512 * 3), device="cuda")
for _ in range(3):
    mi.render_backward_distributed(scene, g, integ, seed=1, spp=256)
torch.cuda.synchronize()
PY
D=/tmp/prof_prb_final; rm -rf $D
rocprofv3 --kernel-trace --stats -d $D -o r -- python /tmp/prb_only.py > $OUT_ROOT/prof/r03_prb_final_kt.log 2>&1
python tools/rocpd_summary.py $(find $D -name '*.db') > $OUT_ROOT/prof/r03_prb_final_kt.txt 2>&1
head -16 $OUT_ROOT/prof/r03_prb_final_kt.txt
head -12 $OUT_ROOT/prof/r03_instanced1m_kt.txt
python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > $OUT_ROOT/r03/bench_final2.json 2> $OUT_ROOT/r03/bench_final2.err
python -c "
import json
for f in ('$OUT_ROOT/r03/bench_final.json','$OUT_ROOT/r03/bench_final2.json'):
    d=json.load(open(f)); print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["profile_check"], (d.get("prb_adjoint") or {}).get("value"), (d.get("secondary") or {}).get("value"), (d.get("cpu_baseline") or {}).get("value"))
"
