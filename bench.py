#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hip_ad_rgb hot path (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one complete forward `path` render of the workload (all W*H*spp lanes:
raygen -> [trace, shade, resolve]* -> splat -> film reduce -> develop), scene and BVH
already resident in HBM.  value = W*H*spp / seconds / 1e6 (Mpaths/s), whole job over all
ranks.  The image is fixed and sharded by pixel rows => "strong" scaling (BASELINE.json:
"1M-tri scene 512^2 x 256 spp, 1/2/4/8 GPU"); the row bands are rebalanced by measured
per-rank time over the first three frames.  rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line; everything else the
benchmark measures runs only with --full (its fields are null otherwise):
  prb_adjoint   the PRB adjoint (RBIntegrator.render_backward: weight pass + primal pass +
                adjoint replay) timed the same way on the TEXTURED variant of the scene (bitmap
                albedo: texel gradient atomics) with emitter gradients on;
  secondary     the flattened 1M-triangle scene (instanced1m only);
  roofline      per-kernel HIP-event breakdown over extra profiled frames, roofline of the
                dominant kernel, committed PMC summaries;
  cpu_baseline  the CPU oracle on the same scene;
  loop          (c4_loop / vertex_loop) kernel share, GPU-busy trace, params.update() cost, plain
                primal + backward step.
--dump-outputs DIR writes what the last timed step returned to its caller as DIR/<name>.npy
(float32; the forward image, or the loop's image, loss and updated parameter), right after the
timed steps.  An array above its share of 64 MB is written as a fixed, seeded sample of its
elements.  Inputs are fixed (seed 0 scenes and sampler seeds), so two builds can be compared
output for output.

Process layout.  Started without a torch.distributed environment, this file is a LAUNCHER:
  --gpus 1 : runs the measurement in one child process (`--worker`); a child killed by a
             signal BEFORE its PyTorch-only preflight passed (a bad box: nothing of this repository
             has run yet) is re-run after a pause (at most twice); a crash after the preflight is the
             product's and is reported, not retried (--retry-on-signal overrides).  The line reports
             "attempts" and, when > 1, says so in `metric`;
  --gpus N : starts N ranks through `python -m torch.distributed.run` (RCCL), one per GPU.
Under torch.distributed.run (RANK / WORLD_SIZE set, the driver's way for N > 1) it is a rank.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
T0 = time.perf_counter()


def log(msg):
    """phase log on stderr (rank 0): a run that dies mid-way says where"""
    if int(os.environ.get("RANK", "0")) == 0:
        sys.stderr.write("[bench %7.2fs] %s\n" % (time.perf_counter() - T0, msg)); sys.stderr.flush()


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="instanced1m", choices=["instanced1m", "flat1m", "cornell", "materials1m", "c4_loop", "vertex_loop"])
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=0, help="wavefront chunk size in lanes (0 = library default)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prb", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--retry-on-signal", action="store_true", help="re-run a worker killed by a signal even when it died after the preflight (off: such a crash is reported, not retried)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary forward workload (flat1m: the 64 MB-BVH variant of the scene)")
    ap.add_argument("--full", action="store_true", help="also run the measurements beyond the headline figure: PRB adjoint, secondary workload, "
                    "per-kernel breakdown and roofline, CPU baseline, loop details (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--worker", action="store_true", help="(internal) this process measures; see the module docstring")
    return ap.parse_args(argv)


def shading_geometry_bytes(scene):
    """unique bytes of the geometry a shading launch gathers from (96-byte shading triangles): L2 / Infinity-Cache resident, counted once per launch"""
    try:
        return 96 * int(sum(int(m["F"].shape[0]) for m in scene.meshes))
    except Exception:
        return 0


def algorithmic_bytes(kernel, stats, accel, launches, overlapped=False, shading_bytes=0):
    """Algorithmic HBM bytes of one frame's launches of a kernel class -- SURVEY.md section 8(d)'s per-unit figures with this implementation's record sizes
    (DESIGN.md section 2), scene data cache-resident and counted ONCE PER LAUNCH:
      trace_closest  56 B per ray (32 B ray in + 24 B hit out) + the accel's unique bytes per launch
      resolve        33 B per shadow ray + the accel per launch
      shade          32-B hit record per vertex in; 72-B path state in for every vertex past the first of its path (the first launch rebuilds the state from the
                     lane index: `k_shade<..., FIRST>`) and 72 B out for every SURVIVOR (= the vertices of the next bounce: vertices - paths over the frame);
                     one 48-B NEE item per shadow ray; the shading triangles once per launch.
                     Round 5 charged 72 B out for EVERY vertex and 112 B of gathers per vertex as HBM bytes: 73 GB per frame = 8.3 TB/s, above the peak;
                     the PMC counters say 41.4 GB (profiles/r05_traffic_instanced1m.json), this model 41.8 GB.
      raygen, splat  32 B ray + 16 B result written per path; 16 B per path read + the film."""
    v, p, sr = stats["vertices"], stats["paths"], stats["shadow_rays"]
    if kernel == "trace_closest":
        if overlapped:
            return stats["closest_rays"] * 56 + sr * 33 + 2 * accel["bytes"] * launches
        return stats["closest_rays"] * 56 + accel["bytes"] * launches
    if kernel == "resolve":
        return sr * 33 + accel["bytes"] * launches
    if kernel == "shade":
        return v * 32 + max(v - p, 0) * (72 + 72) + sr * 48 + shading_bytes * launches
    if kernel == "raygen":
        return p * (32 + 16)
    return p * 16


DUMP_BYTES = 64 << 20


def dump_outputs(directory, arrays):
    """arrays: {name: tensor or array} -> directory/<name>.npy in float32 (float64 stays float64).  Every array gets an equal share of
    DUMP_BYTES; a larger one is written as a sample of its flattened elements at fixed indices (seed 0, sorted), the same from run to run"""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    share = DUMP_BYTES // max(1, len(arrays))
    for name, a in arrays.items():
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        cap = share // a.itemsize
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(directory, name + ".npy"), a)
    log("outputs written to %s: %s" % (directory, ", ".join(sorted(arrays))))


# --------------------------------------------------------------------------------------------- launcher

def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launcher(args):
    import subprocess
    passthrough = [a for a in sys.argv[1:] if a != "--worker"]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.gpus > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), os.path.abspath(__file__)] + passthrough
        return subprocess.call(cmd, env=env)
    cmd = [sys.executable, os.path.abspath(__file__)] + passthrough + ["--worker"]
    # A child killed by a signal (SIGABRT after "Memory access fault by GPU", SIGSEGV, ...) is re-run ONLY when it died before this repository's
    # library did anything: the worker first runs a PyTorch-only preflight (host-to-device copy + reduction) and records in a stage file that it
    # passed.  Twice in round 2 a freshly leased box faulted inside the HIP runtime's first copy of every process started on it; such a box
    # fails the preflight, which is not evidence about the product, and gets two more chances after a pause.  A crash AFTER the preflight is
    # the product's: it is reported as it is (return code, stderr), never retried -- unless --retry-on-signal asks for the round-2 behaviour.
    import tempfile
    pauses = (10.0, 30.0)
    stage_file = tempfile.NamedTemporaryFile(prefix="har_bench_stage_", delete=False).name
    env["HAR_BENCH_STAGE_FILE"] = stage_file
    for attempt in range(1, len(pauses) + 2):
        env["HAR_BENCH_ATTEMPT"] = str(attempt)
        open(stage_file, "w").close()
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
        out = p.stdout.decode(errors="replace")
        crashed = p.returncode < 0 or p.returncode in (134, 139)
        try:
            stage = open(stage_file).read()
        except OSError:
            stage = ""
        retry = crashed and attempt <= len(pauses) and ("preflight_ok" not in stage or args.retry_on_signal)
        if not retry:
            if crashed and "preflight_ok" in stage:
                sys.stderr.write("[bench] the worker was killed (return code %d) AFTER the PyTorch-only preflight passed: a fault of this repository's "
                                 "code path, not retried (use --retry-on-signal to override)\n" % p.returncode)
            sys.stdout.write(out); sys.stdout.flush()
            try:
                os.unlink(stage_file)
            except OSError:
                pass
            return p.returncode
        sys.stderr.write("[bench] WARNING attempt %d ended with return code %d (killed by a signal / aborted) %s; waiting %.0f s, then measuring again "
                         "with the runtime's copies on shader blits instead of the SDMA engines (HSA_ENABLE_SDMA=0)\n"
                         % (attempt, p.returncode, "before the preflight passed" if "preflight_ok" not in stage else "after the preflight (--retry-on-signal)", pauses[attempt - 1]))
        sys.stderr.flush()
        # both bad-box episodes of round 2 faulted inside the runtime's first host-to-device copy: take the other copy path on the retry.
        # The timed region holds no copies (everything is resident), so the reported numbers do not depend on it; "copy_path" in the line says so.
        env["HSA_ENABLE_SDMA"] = "0"
        time.sleep(pauses[attempt - 1])


# --------------------------------------------------------------------------------------------- measurement

def build_scene(mi, args, integrator_type):
    textured = integrator_type == "prb"
    if args.workload == "cornell":
        d = mi.textured_cornell_box(res=args.res, tex_res=256, spp=args.spp, max_depth=args.max_depth) if textured else mi.cornell_box()
        d["sensor"]["film"]["width"] = args.res; d["sensor"]["film"]["height"] = args.res
        d["sensor"]["sampler"]["sample_count"] = args.spp
    else:
        d = mi.instanced_spheres_scene(width=args.res, height=args.res, spp=args.spp, grid=10, n_u=100, n_v=50,
                                       flatten=(args.workload in ("flat1m", "materials1m")), max_depth=args.max_depth,
                                       materials=(args.workload == "materials1m"), textured=textured)
    d["integrator"] = {"type": integrator_type, "max_depth": args.max_depth, "rr_depth": 5, "chunk_lanes": args.chunk}
    if integrator_type == "prb":
        d["integrator"]["emitter_gradients"] = True       # every differentiable scene parameter of the path: albedo texels, constant albedos, emitter radiance
    return mi.load_dict(d)


def load_profile(kind, workload):
    """committed rocprofv3 PMC summaries (tools/gpu_profile.sh, copied to profiles/): newest round first"""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_%s.json" % (kind, workload))), reverse=True):
        try:
            with open(path) as f:
                return json.load(f), os.path.basename(path)
        except Exception:
            continue
    return None, None


# kernels of a HIP-event class of har_integrator_timing: the closest-hit class holds the per-lane kernel (whole wavefront or the packets' left-overs) AND the
# wave-shared camera-ray descent of bounce 0 (k_trace_packet) -- one family, one set of rays
CLASS_KERNELS = {"trace_closest": ("k_trace_closest", "k_trace_packet")}


def class_kernels(cls):
    return CLASS_KERNELS.get(cls, ("k_" + cls,))


def kernel_record(profile, kernel):
    """the class's kernels of a committed PMC summary merged into one record (counter sums, dispatches, total_ms)"""
    out = None
    for name, rec in (profile or {}).items():
        if any(k in name for k in class_kernels(kernel)) and "counters" in rec:
            if out is None:
                out = {"counters": {}, "total_ms": 0.0, "calls": 0}
            out["total_ms"] += float(rec.get("total_ms", 0.0)); out["calls"] += int(rec.get("calls", 0))
            for cname, c in rec["counters"].items():
                acc = out["counters"].setdefault(cname, {"sum": 0.0, "dispatches": 0})
                acc["sum"] += float(c["sum"]); acc["dispatches"] += int(c["dispatches"])
    return out


def profile_matches_run(profile, timing):
    """True when the committed PMC summary was taken from a build with this run's launch sequence: for every kernel class of the frame the
    profile holds a `k_<class>` kernel whose dispatches per frame (frames = its raygen dispatches) equal this run's launches per frame
    (HIP-event classes of har_integrator_timing).  Otherwise a string that says what differs -- the caller then quotes no counter figure."""
    if not profile:
        return "no committed profile for this workload"
    def disp(kernel):
        n = 0
        for name, rec in profile.items():
            if any(k in name for k in class_kernels(kernel)):
                c = rec.get("counters", {})
                n += int(next(iter(c.values()))["dispatches"]) if c else int(rec.get("calls", 0))
        return n
    frames = disp("raygen")
    if frames == 0:
        return "the profile holds no k_raygen dispatch"
    for cls in ("raygen", "trace_closest", "shade", "resolve", "splat"):
        want = int(timing[cls][1])
        got = disp(cls)
        if got != want * frames:
            return "stale profile: k_%s has %d dispatches in %d profiled frame(s), this run launches it %d time(s) per frame" % (cls, got, frames, want)
    return True


def optimisation_loop(args, mi, torch, timed, sync_barrier, world, rank):
    """BASELINE config 4 as it is used: the inverse-rendering LOOP (src/python/python/util.py:344-528 mi.render + SceneParameters.update):
        c4_loop     render(prb, 256^2 x 256 spp, Cornell box, 256^2 albedo bitmap) -> mean(img^2) -> backward -> Adam step -> params.update()
        vertex_loop the same loop over the vertex positions of a 1 000 000-triangle smooth-shaded mesh in the Cornell box (shape gradients; positions stay on the GPU:
                    vertex records, regenerated normals, shading triangles and the BLAS refit are kernels -- har_scene_update_vertices_device)
    one step = all of that; value = steps / s; `outside_kernels` = the share of a step's wall time in which none of the library's kernels runs
    (HIP events of every launch of the profiled steps, har_integrator_set_profiling), i.e. host work + torch's own small kernels."""
    import numpy as np
    if world != 1:
        raise SystemExit("bench.py --workload %s is a single-GPU measurement" % args.workload)
    res = args.res if args.res != 512 else 256          # config 4's film (BASELINE.json: Cornell resolution); --res overrides
    spp = args.spp
    if args.workload == "c4_loop":
        d = mi.textured_cornell_box(res=res, tex_res=256, spp=spp, max_depth=args.max_depth)
        key = "white.reflectance.data"
        what = "Cornell box %dx%dx%dspp prb max_depth=%d, 256x256x3 albedo bitmap on the white walls" % (res, res, spp, args.max_depth)
    else:
        d = mi.cornell_box(); d["sensor"]["film"]["width"] = res; d["sensor"]["film"]["height"] = res
        d["sensor"]["sampler"]["sample_count"] = spp
        d["integrator"] = {"type": "prb", "max_depth": args.max_depth, "rr_depth": 5}
        from mitsuba3_amd.scenes import bumpy_sphere
        n_u = int(os.environ.get("HAR_BENCH_VERTEX_LOOP_NU", "1000"))          # 1000 x 500 quads = 1 000 000 triangles, 501 501 vertices, smooth-shaded (vertex normals:
        P, N, UV, F = bumpy_sphere(n_u=n_u, n_v=n_u // 2, radius=0.35)         # every update regenerates them, Mesh::compute_normals); round 5 measured 102 400 flat-shaded ones
        d.pop("small-box"); d.pop("large-box")
        d["blob"] = {"type": "mesh", "positions": P + np.array([0.0, -0.45, 0.0], np.float32), "normals": N, "faces": F, "bsdf": {"type": "ref", "id": "white"}}
        key = "blob.positions"
        what = "Cornell box + a %d-triangle mesh, %dx%dx%dspp prb max_depth=%d, gradients w.r.t. its %d vertex positions" % (F.shape[0], res, res, spp, args.max_depth, P.shape[0])
    log("optimisation loop: building the scene")
    scene = mi.load_dict(d)
    integ = scene.integrator()
    params = mi.traverse(scene)
    params[key] = params[key].clone().requires_grad_(True)
    params.update()
    opt = torch.optim.Adam([params[key]], lr=(0.01 if args.workload == "c4_loop" else 1e-4))
    it = [0]
    last = {}              # the latest step's image and loss: --dump-outputs

    def step():
        opt.zero_grad(set_to_none=True)
        img = mi.render(scene, params, spp=spp, seed=it[0])
        loss = (img ** 2).mean()
        loss.backward()
        opt.step()
        params.update()
        it[0] += 1
        last["image"] = img; last["loss"] = loss

    log("first step (workspace allocation, code object load)")
    step(); sync_barrier()
    log("loop: %d warmup + %d timed steps" % (args.warmup, args.steps))
    dt = timed(step, args.steps, args.warmup)
    ms = dt / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"image": last["image"], "loss": last["loss"], "parameter": params[key]})
    last.clear()
    out = {"metric": "optimisation steps/s: render -> loss -> backward -> Adam -> params.update() (BASELINE config 4 loop)" if args.workload == "c4_loop"
                     else "optimisation steps/s over vertex positions (device accel refit per step)",
           "value": round(args.steps / dt, 3), "unit": "steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": what, "parameter": key, "parameter_values": int(params[key].numel()), "optimizer": "torch.optim.Adam"}, "loop": None}
    if not args.full:
        print(json.dumps(out)); sys.stdout.flush()
        log("done")
        return
    # kernel time of the library per step: HIP events around every launch (forward render = 1 frame, backward = 1 frame)
    integ.set_profiling(True)
    n_prof = max(2, min(args.steps, 5))
    for _ in range(n_prof):
        step()
    sync_barrier()
    timing = integ.timing(); integ.set_profiling(False)
    frames = max(1, int(timing["frames"][0]))
    kernel_ms = float(timing["total"][0]) * frames / n_prof            # timing() averages per frame; a step holds frames / n_prof of them
    # host-only cost of the step's non-render parts, measured alone: params.update() and the optimiser step with the GPU idle
    # GPU-side account of a step from the kernel intervals themselves (torch.profiler = roctracer: every kernel of the process, the library's included): the UNION of the
    # intervals is the time some kernel runs -- frames too large for the shadow-ray overlap run as two half-jobs on two streams (har_render), so the SUM of the launch
    # durations above is not a time.  idle = span - union (no kernel at all); outside = span - union of the library's kernels and the runtime's fills / copies
    # (what is left is torch's loss / optimiser kernels and the gaps)
    busy = None
    try:
        from torch.profiler import profile, ProfilerActivity
        n_trace = 5
        sync_barrier()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n_trace):
                step()
            sync_barrier()
        evs = sorted(((e.time_range.start, e.time_range.end, e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and e.time_range.end > e.time_range.start))

        def union(items):
            tot = 0.0; cs = ce = None
            for a, b, _ in items:
                if cs is None:
                    cs, ce = a, b
                elif a > ce:
                    tot += ce - cs; cs, ce = a, b
                else:
                    ce = max(ce, b)
            return tot + ((ce - cs) if cs is not None else 0.0)
        if evs:
            span = evs[-1][1] - evs[0][0]
            lib = [e for e in evs if "har::" in e[2] or e[2].startswith("Memset") or e[2].startswith("Memcpy") or "rocclr" in e[2]]
            busy = {"steps": n_trace, "span_ms_per_step": round(span / n_trace / 1e3, 3), "gpu_idle_ms_per_step": round((span - union(evs)) / n_trace / 1e3, 3),
                    "outside_library_kernels_ms_per_step": round((span - union(lib)) / n_trace / 1e3, 3),
                    "other_kernels_ms_per_step": round(sum(b - a for a, b, nme in evs if not ("har::" in nme or nme.startswith("Memset") or nme.startswith("Memcpy") or "rocclr" in nme)) / n_trace / 1e3, 3),
                    "source": "torch.profiler kernel intervals of %d back-to-back steps (union, not sum)" % n_trace}
    except Exception as ex:        # no profiler in this build: the field stays empty
        busy = {"error": str(ex)[:200]}
    # (a) nothing changed since the last update(): the "same tensor, same version" early-out; (b) the parameter WAS written (what an optimiser step leaves behind:
    # a new version counter) -- the in-loop cost: device-to-device pushes / the device-resident vertex update with its refit, enqueue + execution
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20):
        params.update()
    torch.cuda.synchronize(); update_nochange_ms = (time.perf_counter() - t0) / 20 * 1e3
    for _ in range(3):                  # untimed: the first written update after the rendered steps pays one-off costs of the runtime (measured: ~2 ms per preceding step)
        with torch.no_grad():
            params[key].add_(0)
        params.update()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20):
        with torch.no_grad():
            params[key].add_(0)
        params.update()
    t1 = time.perf_counter(); torch.cuda.synchronize()
    update_host_ms = (t1 - t0) / 20 * 1e3; update_ms = (time.perf_counter() - t0) / 20 * 1e3
    # plain PRB step of the same scene without the loop around it (render_backward with a fixed adjoint): what the loop adds
    grad_in = torch.full((res, res, 3), 1.0 / (res * res * 3), device="cuda")
    saved = integ.shape_gradients
    if args.workload == "vertex_loop":
        integ.shape_gradients = [key]

    def plain():
        integ.render(scene, seed=1, spp=spp, evaluate=False)
        integ.render_backward(scene, None, grad_in, seed=2, spp=spp)

    plain(); sync_barrier()
    dt_plain = timed(plain, max(2, min(args.steps, 5)), 1)
    integ.shape_gradients = saved
    plain_ms = dt_plain / max(2, min(args.steps, 5)) * 1e3
    out.update({
           # frames too large for the shadow-ray overlap run as two half-jobs on two streams (har_render): their kernels overlap in time, the sum of the
           # launch durations is then no longer a time and `outside_kernels` is left out -- profiles/rNN_kernel_trace_stats_vertex_loop.txt holds the step's
           # GPU-idle time from the union of the kernel intervals of a rocprofv3 trace (tools/rocpd_summary.py --busy)
           "loop": {"library_kernel_ms_per_step": round(kernel_ms, 3),
                    "outside_kernels_ms_per_step": (busy["outside_library_kernels_ms_per_step"] if busy and "outside_library_kernels_ms_per_step" in busy else (round(ms - kernel_ms, 3) if kernel_ms <= ms else None)),
                    "outside_kernels_share": (round(busy["outside_library_kernels_ms_per_step"] / ms, 4) if busy and "outside_library_kernels_ms_per_step" in busy else (round((ms - kernel_ms) / ms, 4) if kernel_ms <= ms else None)), "loop_minus_plain_ms": round(ms - plain_ms, 3), "gpu_busy": busy, "params_update_ms": round(update_ms, 4), "params_update_host_enqueue_ms": round(update_host_ms, 4), "params_update_no_change_ms": round(update_nochange_ms, 4),
                    "plain_primal_plus_backward_ms": round(plain_ms, 3), "loop_over_plain": round(ms / plain_ms, 3),
                    "mpaths_per_s_primal_plus_adjoint": round(res * res * spp / (ms / 1e3) / 1e6, 2),
                    "kernel_ms_per_frame": {k: round(v[0], 3) for k, v in timing.items() if k != "frames"}, "frames_per_step": frames / n_prof}})
    if args.workload == "vertex_loop":
        try:
            out["loop"]["accel"] = dict(scene.refit_info(), device_resident_updates=bool(getattr(scene, "_stale_meshes", None)), accel=scene.accel_info())
        except Exception as e:          # a rebuild was advised by the last step: no handle right now
            out["loop"]["accel"] = {"note": str(e)[:200], "rebuilds": getattr(scene, "accel_rebuilds", 0)}
    print(json.dumps(out)); sys.stdout.flush()
    log("done")


def forward_breakdown(args, scene, integ, accel, fwd, sync_barrier, world, value, ms_per_step):
    """--full: per-kernel HIP events over a few extra frames right after the timed region, and the roofline of the dominant kernel.
    Returns (roofline, stats), the counters read after the profiled frames"""
    prof_frames = max(2, min(args.steps, 5))
    integ.set_profiling(True)
    for _ in range(prof_frames):
        fwd()
    sync_barrier()
    timing = integ.timing()            # per-kernel HIP-event durations, average per frame over the profiled frames of this rank
    integ.set_profiling(False)
    stats = integ.stats()
    log("forward done: %.1f Mpaths/s (%d timed frames, then %d profiled frames for the kernel breakdown)" % (value, args.steps, prof_frames))

    # roofline of the dominant kernel, algorithmic bytes per SURVEY.md 8(d):
    #   trace_closest: 56 B/ray (32 B ray in + 24 B hit out) + unique accel bytes once per launch
    #   resolve: 33 B/shadow ray + accel ; shade: state in/out + hit + gathers ; raygen/splat: 152 + 16 B/path
    kern_ms = {k: v[0] for k, v in timing.items() if k != "frames"}
    frames_profiled = int(timing["frames"][0])
    dominant = max(("trace_closest", "shade", "resolve", "splat", "raygen"), key=lambda k: kern_ms[k])
    launches = max(timing[dominant][1], 1)
    # jobs of at most 2^25 lanes per rank (N > 1) run bounce b's shadow rays on a second stream NEXT TO bounce b + 1's closest-hit rays (har_capi.hip overlap_applies):
    # the interval the trace class times then holds both traversal kernels, so its bytes are the bytes of both
    overlapped = stats["shadow_rays"] > 0 and kern_ms["resolve"] < 0.05 * kern_ms["trace_closest"]
    alg_bytes = algorithmic_bytes(dominant, stats, accel, launches, overlapped=overlapped, shading_bytes=shading_geometry_bytes(scene))
    achieved = alg_bytes / 1e9 / (kern_ms[dominant] / 1e3) if kern_ms[dominant] > 0 else 0.0
    # HBM traffic from the committed PMC passes (separate FETCH_SIZE / WRITE_SIZE runs of this command, tools/gpu_profile.sh ... mem):
    # bytes = (FETCH_SIZE x 2 [gfx950 correction, MI355X_MICROARCH.md "HBM"] + WRITE_SIZE) KiB x 1024; per launch for the dominant kernel,
    # summed over all kernels of a frame for `frame_traffic`.  Only valid for the launch shape it was collected at (N = 1, 512^2 x 256).
    traffic = frame_traffic = traffic_src = None
    bound_actual = None
    profile_check = None
    if args.res == 512 and args.spp == 256 and world == 1 and not args.chunk:
        prof, traffic_src = load_profile("traffic", args.workload)
        rec = kernel_record(prof, dominant)
        # a committed profile is only quoted when it describes THIS build's launch sequence: same kernels, same launches per frame
        profile_check = profile_matches_run(prof, timing)
        if profile_check is not True:
            rec = None
        if rec and "FETCH_SIZE" in rec["counters"] and "WRITE_SIZE" in rec["counters"]:
            f, w = rec["counters"]["FETCH_SIZE"], rec["counters"]["WRITE_SIZE"]
            traffic = round((2.0 * f["sum"] / f["dispatches"] + w["sum"] / w["dispatches"]) * 1024.0)
            # whole frame: every kernel's FETCH x 2 + WRITE of the profiled run, divided by the frames that run rendered (= raygen dispatches)
            rg = kernel_record(prof, "raygen")
            frames_prof = max(1, int(rg["counters"]["FETCH_SIZE"]["dispatches"])) if rg else 1
            tot = 0.0
            for r in prof.values():
                c = r.get("counters", {})
                if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                    tot += (2.0 * c["FETCH_SIZE"]["sum"] + c["WRITE_SIZE"]["sum"]) * 1024.0
            tot /= frames_prof
            frame_traffic = {"bytes_per_frame": round(tot), "GBs": round(tot / 1e9 / (ms_per_step / 1e3), 1),
                             "frac_of_peak": round(tot / 1e9 / (ms_per_step / 1e3) / HBM_PEAK_GBS, 4), "source": "profiles/" + traffic_src}
        sq, sq_src = load_profile("sq", args.workload)
        rec = kernel_record(sq, dominant) if profile_matches_run(sq, timing) is True else None
        if rec and "SQ_INSTS_VALU" in rec["counters"] and rec.get("total_ms"):
            c = rec["counters"]
            rays = stats["closest_rays"] if dominant == "trace_closest" else stats["shadow_rays"] if dominant == "resolve" else stats["vertices"]
            frames_sq = max(1, int(c["SQ_INSTS_VALU"]["dispatches"]) // max(launches, 1))
            # what the kernel is really bound by: wave64 VALU instructions issued (SQ_INSTS_VALU) x ~2.7 cycles per instruction (tools/ubench/valu_ubench,
            # the fma / mul / add rate; conversions and min3 / max3 are slower) over the SIMD cycles of its launches (1024 SIMDs x 2.4 GHz x duration)
            bound_actual = {"kind": "valu_issue",
                            "valu_insts_per_64_rays": round(c["SQ_INSTS_VALU"]["sum"] / frames_sq / max(rays / 64.0, 1.0), 1),
                            "valu_issue_frac_of_simd_cycles": round(c["SQ_INSTS_VALU"]["sum"] * 2.7 / (1024 * rec["total_ms"] * 1e-3 * 2.4e9), 3),
                            "source": "profiles/" + sq_src}
    # `bound`: what the committed counters say the dominant kernel is limited by ("valu_issue" for the traversal kernels); achieved / peak / frac stay the
    # HBM figures the contract asks for (algorithmic bytes per launch over the measured launch duration against the 8 TB/s peak), repeated as `hbm_frac`
    roofline = {"bound": (bound_actual["kind"] if bound_actual else "hbm"), "hbm_frac": round(achieved / HBM_PEAK_GBS, 5),
                "valu_issue_frac": (bound_actual["valu_issue_frac_of_simd_cycles"] if bound_actual else None), "kernel": dominant + ("+resolve (concurrent on two streams)" if dominant == "trace_closest" and overlapped else ""), "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": ("profiles/" + traffic_src) if traffic is not None else None,
                "algorithmic_bytes_per_launch": round(alg_bytes / launches),
                "avg_launch_ms": round(kern_ms[dominant] / launches, 4), "launches": launches, "frames_averaged": frames_profiled,
                "kernel_ms": {k: round(v, 3) for k, v in kern_ms.items()},
                "bound_actual": bound_actual, "frame_traffic": frame_traffic,
                "profile_check": ("ok: the committed profile's kernels and launches per frame equal this run's" if profile_check is True else profile_check)}
    return roofline, stats


def further_measurements(args, mi, torch, np, scene, timed, sync_barrier, world, rank, n_paths):
    """--full: the PRB adjoint, the secondary forward workload and the CPU baseline.  Returns (prb, secondary, cpu)"""
    # ---------------- PRB adjoint ----------------
    prb = None
    scene_p = None
    if not args.no_prb:
        log("PRB adjoint: building the textured scene")
        scene_p = build_scene(mi, args, "prb")
        integ_p = scene_p.integrator()
        grad_in = torch.full((args.res, args.res, 3), 1.0 / (args.res * args.res * 3), device="cuda")

        def bwd():
            return mi.render_backward_distributed(scene_p, grad_in, integ_p, seed=1, spp=args.spp)

        p_steps = max(1, min(args.steps, 5))
        log("PRB adjoint: 1 warmup + %d timed steps" % p_steps)
        dtp = timed(bwd, p_steps, 1)
        pst = integ_p.stats()
        prb = {"metric": "Mpaths/s prb adjoint (weight pass + primal + adjoint replay)",
               "value": round(n_paths / (dtp / p_steps) / 1e6, 2), "ms_per_step": round(dtp / p_steps * 1e3, 2), "steps": p_steps,
               "workload": "%s + 256x256 bitmap albedo on the `white` BSDF (walls + spheres), emitter_gradients=True" % args.workload,
               "gradient_targets": {"texels": int(sum(int(np.prod(t.shape)) for t in scene_p.textures)), "constant_albedos": len(scene_p.bsdfs), "emitters": len(scene_p.emitters)},
               "stats": {k: int(v) for k, v in pst.items()},
               "stats_note": "counters of the adjoint replay: its ray queries are served by the replay cache (shadow_rays = 0 traced); the primal pass of the same step traces the rays"}
        log("PRB adjoint done: %.1f Mpaths/s" % prb["value"])

    # ---------------- secondary forward workload: the FLATTENED 1M-triangle scene (64 MB BVH instead of 0.65 MB: SURVEY.md 8(d)'s BVH-size stress) ----------------
    secondary = None
    if args.workload == "instanced1m" and not args.no_secondary and world == 1:
        import copy
        a2 = copy.copy(args); a2.workload = "flat1m"
        log("secondary workload flat1m: building the scene + BVH")
        scene2 = build_scene(mi, a2, "path")
        integ2 = scene2.integrator()

        def fwd2():
            return mi.render_distributed(scene2, integ2, seed=0, spp=args.spp)

        fwd2(); sync_barrier()
        s_steps = max(1, min(args.steps, 5))
        dt2 = timed(fwd2, s_steps, 1)
        integ2.set_profiling(True)
        for _ in range(2):
            fwd2()
        sync_barrier()
        t2 = integ2.timing(); integ2.set_profiling(False)
        st2 = integ2.stats(); acc2 = scene2.accel_info()
        l2 = max(t2["trace_closest"][1], 1)
        ach2 = (st2["closest_rays"] * 56 + acc2["bytes"] * l2) / 1e9 / (t2["trace_closest"][0] / 1e3)
        secondary = {"workload": "flat1m %dx%dx%dspp (flattened: unique triangles, %.0f MB BVH)" % (args.res, args.res, args.spp, acc2["bytes"] / 1e6),
                     "value": round(n_paths / (dt2 / s_steps) / 1e6, 2), "unit": "Mpaths/s", "ms_per_step": round(dt2 / s_steps * 1e3, 2), "steps": s_steps,
                     "accel": acc2, "kernel_ms": {k: round(v[0], 3) for k, v in t2.items() if k != "frames"},
                     "trace_closest_achieved_GBs": round(ach2, 2), "trace_closest_frac_of_hbm_peak": round(ach2 / HBM_PEAK_GBS, 5),
                     "stats": {k: int(v) for k, v in st2.items()}}
        log("secondary done: %.1f Mpaths/s" % secondary["value"])
        del scene2, integ2

    # ---------------- CPU baseline (oracle = CPU restatement of llvm_ad_rgb; rank 0, N = 1 only) ----------------
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import oracle as O
        # threads = the cores this container may really use (affinity mask capped by its cgroup CPU quota: the GPU boxes show 256 logical CPUs behind a quota of
        # 16, and 256 threads run at HALF the rate of 16 there -- profiles/r03_cpu_scaling.txt); `cores` in the line is this count
        cores = max(1, int(O.lib().orc_default_threads()))
        log("CPU baseline: oracle on %d host threads of %d logical CPUs (forward)" % (cores, os.cpu_count() or 1))
        if args.workload in ("instanced1m", "flat1m"):      # the oracle's own lowering of the scene description (independent of the product's host code)
            sd_o, sensor = O.benchmark_spheres_scene(args.res, args.res, flatten=(args.workload == "flat1m"))
            osc = O.OracleScene(sd_o)
        else:
            osc, sensor = O.scene_from_product(scene)
        t0 = time.perf_counter()
        _, st = osc.render_path(sensor, seed=0, spp=1, max_depth=args.max_depth, threads=cores)
        probe = time.perf_counter() - t0
        budget = args.cpu_seconds * (0.6 if scene_p is not None else 1.0)
        spp_cpu = int(max(1, min(64, budget / max(probe, 1e-3))))
        t0 = time.perf_counter()
        _, st = osc.render_path(sensor, seed=0, spp=spp_cpu, max_depth=args.max_depth, threads=cores)
        el = time.perf_counter() - t0
        cpu = {"value": round(st.paths / el / 1e6, 4), "unit": "Mpaths/s", "cores": cores, "logical_cpus": os.cpu_count() or 1, "kind": "port",
               "note": "the oracle is a slow, readable restatement written as a CHECKER (%.0f us x thread per path in this run); it is NOT llvm_ad_rgb -- an Embree-backed llvm_ad_rgb on these cores would be one to two orders of magnitude faster; the ratio value / cpu_baseline.value bounds nothing" % (el * cores / max(st.paths, 1) * 1e6),
               "sample": "%dx%dx%d spp of the same scene/seed (%.1f s); CPU restatement of llvm_ad_rgb (reference not installable)"
                         % (args.res, args.res, spp_cpu, el)}
        if scene_p is not None:
            log("CPU baseline: oracle PRB backward")
            if args.workload in ("instanced1m", "flat1m"):
                sd_p, sensorp = O.benchmark_spheres_scene(args.res, args.res, flatten=(args.workload == "flat1m"), textured=True)
                oscp = O.OracleScene(sd_p)
            else:
                oscp, sensorp = O.scene_from_product(scene_p)
            g = np.full((args.res, args.res, 3), 1.0 / (args.res * args.res * 3), np.float32)
            t0 = time.perf_counter()
            oscp.render_prb_backward(sensorp, g, seed=1, spp=1, max_depth=args.max_depth, threads=cores)
            probe = time.perf_counter() - t0
            spp_p = int(max(1, min(32, args.cpu_seconds * 0.4 / max(probe, 1e-3))))
            t0 = time.perf_counter()
            oscp.render_prb_backward(sensorp, g, seed=1, spp=spp_p, max_depth=args.max_depth, threads=cores)
            elp = time.perf_counter() - t0
            cpu["prb_adjoint"] = {"value": round(args.res * args.res * spp_p / elp / 1e6, 4), "unit": "Mpaths/s",
                                  "sample": "%dx%dx%d spp of the textured scene (%.1f s), render_prb_backward of the oracle" % (args.res, args.res, spp_p, elp)}
    return prb, secondary, cpu


def worker(args):
    import faulthandler
    faulthandler.enable()                      # a GPU fault ends in abort(): say which Python line was running
    log("importing torch")
    import numpy as np
    import torch
    import torch.distributed as dist
    import mitsuba3_amd as mi

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the process group has %d rank(s); start it as `python bench.py --gpus N` (self-launching) "
                         "or under torch.distributed.run with --nproc-per-node N" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hip_ad_rgb path has no CPU fallback")
    # HAR_BENCH_SHARE_GPU=1 + HAR_BENCH_BACKEND=gloo: rehearsal of the N-rank code path on a box with fewer GPUs than ranks
    # (ranks share devices, the film reduce goes through gloo); never used for reported numbers
    device_index = local_rank % torch.cuda.device_count() if os.environ.get("HAR_BENCH_SHARE_GPU") else local_rank
    if os.environ.get("HAR_BENCH_SHARE_GPU") and world > 1:
        # ranks that SHARE a GPU are time-sliced process by process: the per-rank auxiliary stream of the shadow-ray overlap then only adds queue switches
        # (measured: PRB 636 -> 271 Mpaths/s with two ranks on one GPU; on a GPU of its own a rank gains 3-6 %, profiles/r03_ab_shadow_overlap.txt)
        os.environ.setdefault("HAR_OVERLAP", "0")
    torch.cuda.set_device(device_index)
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("HAR_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend=backend)
        assert dist.get_world_size() == args.gpus
    log("device %s, %d rank(s)" % (torch.cuda.get_device_name(device_index), world))
    # preflight WITHOUT this repository's library: a pageable host-to-device copy and a reduction through PyTorch.  Twice in ~70 leases of this
    # round a box faulted ("Memory access fault by GPU") inside the HIP runtime's own copy of the first upload, for every process started on it,
    # with builds that run clean everywhere else; if that happens here the traceback points at this line, not at
    # libhip_ad_rgb.so, and the launcher's retry / the reader can tell the two apart
    pre = torch.ones(1 << 22, dtype=torch.float32).to("cuda")
    if float(pre.sum().item()) != float(1 << 22):
        raise SystemExit("bench.py: the GPU preflight (torch copy + sum) returned a wrong value -- this box's GPU is not usable")
    del pre
    torch.cuda.synchronize()
    log("preflight ok (torch H2D copy + reduction, before libhip_ad_rgb.so is loaded)")
    if os.environ.get("HAR_BENCH_STAGE_FILE"):
        try:
            with open(os.environ["HAR_BENCH_STAGE_FILE"], "w") as f:
                f.write("preflight_ok\n")
        except OSError:
            pass
    mi.set_variant("hip_ad_rgb")

    def sync_barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, warmup, on_start=None):
        # N > 1: the row-band balancer adapts (and synchronises) over its first frames; with fewer warm-up frames than that, run the rest untimed here so
        # that no adaptation frame -- with its event synchronisation and all-gather -- lands inside the timed region
        settle = 0
        if world > 1:
            from mitsuba3_amd.distributed import BandBalancer
            settle = max(0, BandBalancer.ADAPT_FRAMES - warmup)
        for _ in range(warmup + settle):
            fn()
        sync_barrier()
        if on_start:
            on_start()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync_barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    if args.workload in ("c4_loop", "vertex_loop"):
        return optimisation_loop(args, mi, torch, timed, sync_barrier, world, rank)

    n_paths = args.res * args.res * args.spp

    # ---------------- forward `path` ----------------
    log("building the %s scene + BVH" % args.workload)
    scene = build_scene(mi, args, "path")
    integ = scene.integrator()
    accel = scene.accel_info()

    # HAR_BENCH_GROUP=k (single process, A/B only): the frame goes through the single-call multi-GPU entry of the C ABI (har_multi_render, mi.DeviceGroup) with k
    # replicas on device 0 -- k = 1 measures what the entry adds to har_render (nothing: same launches), k > 1 rehearses the bands + the reduce on one GPU
    group = mi.DeviceGroup(scene, devices=[0] * int(os.environ["HAR_BENCH_GROUP"])) if os.environ.get("HAR_BENCH_GROUP") and world == 1 else None

    last = [None]          # what the latest frame returned to its caller (the developed image on rank 0): --dump-outputs

    def fwd():
        if group is not None:
            last[0] = group.render(seed=0, spp=args.spp)
        else:
            last[0] = mi.render_distributed(scene, integ, seed=0, spp=args.spp)
        return last[0]

    log("first forward frame (workspace allocation, code object load)")
    fwd(); sync_barrier()
    log("forward: %d warmup + %d timed frames" % (args.warmup, args.steps))
    # HIP events on the launch stream, one per kernel launch, over the TIMED frames only (har_integrator_set_profiling restarts the statistics;
    # every frame records into its own event set, see include/hip_ad_rgb.h)
    # `value` comes from frames rendered WITHOUT the per-launch events; the per-kernel breakdown (HIP events on the launch stream, one per kernel launch,
    # har_integrator_set_profiling) is taken over a few extra frames right after the timed region (--full)
    dt = timed(fwd, args.steps, args.warmup)
    ms_per_step = dt / args.steps * 1e3
    value = n_paths / (dt / args.steps) / 1e6
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"image": last[0]})
    last[0] = None
    roofline = prb = secondary = cpu = None
    if args.full:
        roofline, stats = forward_breakdown(args, scene, integ, accel, fwd, sync_barrier, world, value, ms_per_step)
        prb, secondary, cpu = further_measurements(args, mi, torch, np, scene, timed, sync_barrier, world, rank, n_paths)
    else:
        stats = integ.stats()
        log("forward done: %.1f Mpaths/s (%d timed frames)" % (value, args.steps))

    if rank == 0:
        out = {
            "metric": "Mpaths/s forward (PRB-adjoint in `prb_adjoint`), 1M-tri scene 512^2x256spp" if args.workload != "cornell" else "Mpaths/s forward path, Cornell box",
            "value": round(value, 2), "unit": "Mpaths/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s %dx%dx%dspp max_depth=%d rr_depth=5 seed=0" % (args.workload, args.res, args.res, args.spp, args.max_depth),
                       "triangles_effective": 100 * 10000 + 12 if args.workload != "cornell" else 36,
                       "accel": accel, "parallelism": "pixel-row tiles x%d, one RCCL film reduce" % world,
                       "ranks": world, "collective_backend": ("rccl (torch.distributed nccl)" if backend == "nccl" else backend),
                       # row bands of equal measured cost (mitsuba3_amd/distributed.py BandBalancer; adapts over the first 3 frames, then frozen)
                       "row_bands": next(iter(getattr(integ, "_band_balancers", {}).values())).bounds if world > 1 and getattr(integ, "_band_balancers", None) else None},
            "prb_adjoint": prb, "secondary": secondary, "roofline": roofline, "cpu_baseline": cpu,
            "stats": {k: int(v) for k, v in stats.items()},
            "attempts": int(os.environ.get("HAR_BENCH_ATTEMPT", "1")),
            "copy_path": "shader blits (HSA_ENABLE_SDMA=0, retry)" if os.environ.get("HSA_ENABLE_SDMA") == "0" else "runtime default",
        }
        if out["attempts"] > 1:
            out["metric"] = "WARNING measured on attempt %d (earlier worker(s) died before the GPU preflight passed) -- " % out["attempts"] + out["metric"]
        print(json.dumps(out)); sys.stdout.flush()
    if world > 1:
        dist.destroy_process_group()
    log("done")


if __name__ == "__main__":
    _args = parse()
    if _args.worker or "RANK" in os.environ:
        worker(_args)
    else:
        sys.exit(launcher(_args))
