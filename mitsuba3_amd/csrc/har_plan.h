/*
 * har_plan.h -- what run_chunk (har_capi.hip) decides BEFORE its first launch, as plain data: the integrator's settings, the kind of replay
 * cache a pass uses, and plan_chunk, which derives every per-chunk decision from the switch table, the settings, a few facts about the scene
 * and the job.  HIP-free, integers and flags only, so that the decisions are tested on the host (tests/test_switches_cpu.py).
 * Scenes with a `blendbsdf` record (HAR_SCENE_BLEND): no first-vertex regeneration and no material queues (one widest shading kernel per flavour, launch_shade), and
 * every backward pass takes the re-shading replay with the in-place commit -- the state tape or the lane-indexed cache, never the record tape (backward_range, har_capi.hip:
 * as with har_integrator_set_grad_bsdf_params, max_depth <= HAR_REPLAY_CACHE_BOUNCES = 12 and the replay cache on) -- because that commit deposits the nested records' gradients.
 * Scenes with a `mask` record (HAR_SCENE_MASK) are planned the same way, with their own widest set.  In `path` the validity of a camera sample is decided along the
 * path there (a null lobe does not make it valid, path.cpp:307-308): ChunkPlan::valid_shade -- the per-lane flags start at 0 and the shading kernel stores 1 from the vertex
 * at which a non-null lobe was sampled, instead of k_alpha_flags; run_chunk then clears the radiance of the lanes that stayed invalid (path.cpp:341-345).
 * Scenes with a `normalmap` record (HAR_SCENE_NORMALMAP) take the same route with a set of their own (forward, prb primal and the in-place adjoint commit).
 */
#pragma once
#include "../../include/hip_ad_rgb.h"
#include "har_path.h"
#include "har_switches.h"

namespace har {

/* What a bounce's ReplayCache / TapeArrays are used for; ReplayCache::mode carries the value into the kernels (har_kernels.h) */
enum CacheMode : int {
    CACHE_NONE = 0,
    CACHE_WRITE = 1, CACHE_READ = 2,      /* lane-indexed replay cache: the primal pass records the ray-query results, the adjoint pass reads them */
    TAPE_WRITE = 3, TAPE_READ = 4,        /* state tape: the primal pass keeps its wavefronts, the adjoint pass re-shades them in slot order */
    RECORD_WRITE = 5, RECORD_READ = 6     /* record tape: the primal pass writes one adjoint record per vertex, the adjoint pass is k_commit */
};
static_assert(CACHE_NONE == 0 && CACHE_WRITE == 1 && CACHE_READ == 2 && TAPE_WRITE == 3 && TAPE_READ == 4 && RECORD_WRITE == 5 && RECORD_READ == 6,
              "the kernels compare ReplayCache::mode with these numbers");

/* The settings of an integrator (as opposed to its workspace, caches, events and the user buffers of a single call).  The twin of two-stream mode
 * gets them as ONE value (dual_split), so a new setting reaches it without a list to extend. */
struct Settings {
    int type = HAR_INTEGRATOR_PATH;
    /* lanes per wavefront chunk (multiple of 2048).  Every chunk pays ~3.4 ms of kernel tails (26 launches that each wait for their slowest wave), so
     * chunks are as large as HBM comfortably allows: 2^26 lanes = 15.6 GB of forward workspace, 32 GB with the adjoint items and the replay cache
     * (measured on the 1M-triangle scene, 67 M lanes: 16 M-lane chunks 708, 32 M 758, one 64 M chunk 783 Mpaths/s) */
    uint32_t max_depth = 0, rr_depth = 5, chunk = 1u << 26;
    uint32_t samples_per_pass = 0xffffffffu;
    bool hide_emitters = false;           /* Integrator property (integrator.cpp:29) */
    bool material_queues = false;         /* har_integrator_set_material_queues */
    int packet_tracing = -1;              /* har_integrator_set_packet_tracing: -1 automatic, 0 off, 1 every first closest-hit launch */
    int top_seed = -1, top_seed_env = -1; /* har_integrator_set_top_seed: -1 the scene's choice (Accel::top_seed), 0 off, 1 on; HAR_TOP_SEED as read when the integrator was created (it wins) */
    bool use_cache = true;                /* har_integrator_set_replay_cache */
    bool profiling = false;
    float *grad_emitters = nullptr;       /* user buffer (DEVICE, emitter_count x 3) of har_integrator_set_grad_emitters, or null */
    float *grad_bsdf_params = nullptr;    /* user buffer (DEVICE, bsdf_count x 15) of har_integrator_set_grad_bsdf_params, or null */
    bool grad_light_texels = false;       /* har_integrator_set_grad_light_texels: the texels of bitmap `radiance` textures of area lights are differentiated (into their entries of grad_textures) */
    bool grad_envmap = false;             /* har_integrator_set_grad_envmap: the texels of the environment map are differentiated (into the image's entry of grad_textures, without the map's `scale`) */
    float *alpha_film = nullptr;         /* user buffer (DEVICE, H x W x 4: channel 3 accumulates w * alpha) of har_integrator_set_alpha_film, or null */
    /* har_integrator_set_batch_sensors: the child cameras of a batch sensor (DEVICE table, a block of its own) -- batch.n != 0: the `sensor` of the render calls is the
     * batch sensor's wide film and the camera rays come from the table (k_raygen_batch) */
    DBatch batch{ nullptr, 0u, 0u };
};

#define HAR_OVERLAP_MAX_LANES (1u << 25)
#ifndef HAR_LATE_OVERLAP_DEFAULT          /* first bounce whose shadow rays run next to the following bounce's closest-hit rays in jobs above HAR_OVERLAP_MAX_LANES (run_chunk) */
#define HAR_LATE_OVERLAP_DEFAULT(rr_depth) 0xffffffffu
#endif
constexpr uint32_t PLAN_MAX_TRAVERSAL_BLOCKS = 2048;      /* HAR_MAX_TRAVERSAL_BLOCKS (har_kernels.h; har_capi.hip asserts the two agree) */

struct SceneFacts {
    uint32_t stack_need;      /* HostScene::stack_need() + HAR_STACK_MARGIN */
    uint32_t lds_stack;       /* HAR_LDS_STACK_SMALL: deeper scenes run the traversal kernels with the HBM spill */
    uint32_t mat_classes;     /* bit mask of the material classes of the scene's BSDF records */
    uint32_t bsdf_types;      /* DScene::bsdf_types */
    int32_t env_emitter;      /* DScene::env_emitter */
};

struct ChunkJob {
    int mode;                 /* MODE_PATH / MODE_PRB_PRIMAL / MODE_PRB_ADJOINT */
    CacheMode cache_mode;
    uint32_t n, spp, lane_base;
    uint32_t nb;              /* bounce_limit */
    bool rays;                /* caller-supplied rays instead of the sensor */
    bool valid_lane;          /* ... whose masks are asked for */
    bool pass_rng;            /* PassState::rng: sampler states kept from pass to pass */
    uint32_t projection;      /* DSensor::projection (2 = thin lens) */
    /* state of the integrator that is no setting */
    bool forward_mode, shape_on, adjoint_image /* adj */, alpha_lane;
};

struct ChunkPlan {
    bool mq_on;               /* "material queues on": the switch, or the integrator's setting */
    bool first_regen, use_mq;
    bool overlap, late_on;    /* WANTED: run_chunk clears them when the stream, the events or the second item set cannot be created */
    uint32_t late_from;
    bool inline_commit, spill, shape, fwd;
    bool packet;              /* bounce 0 (when it traces at all) */
    bool alpha_flags; float alpha_miss;
    bool valid_shade;         /* mask scenes, `path`: the validity flags are written by the shading kernels (run_chunk hands them to launch_shade) */
    uint32_t grid, tgrid, shade_flags;
};

/* shadow-ray overlap (HarIntegratorImpl::aux_stream) for a job of n lanes?  `path` and the primal passes of `prb`, at most HAR_OVERLAP_MAX_LANES lanes -- the share
 * of a rank when several GPUs split a frame, where a launch is short and its tail (the chip waiting for the launch's longest rays) is a sizeable part of it:
 * measured on the middle bands of the headline frame (tools/band_bench.py, profiles/r03_ab_shadow_overlap.txt), one stream without / with overlap | two streams
 * without / with: 2 M lanes 5.46 / 4.67 | 5.11 / 4.60 ms, 4 M 8.56 / 7.64 | 8.09 / 7.68, 8 M 13.89 / 13.03 | 13.47 / 13.16, 16 M 24.58 / 23.76 | 24.42 / 24.36,
 * 33 M 42.50 / 41.90, 67 M 77.07 / 77.30; with the asynchronous join (second item set + `result2`) and 64-ray fetches 2 M 4.11, 8 M 12.60, 16 M 23.66, 33 M 42.06, 67 M still
 * neutral (78.05 / 78.37).  A single large wavefront keeps one stream and sequential launches (its kernels are timed one by one for the bench
 * line).  Not with the HBM stack spill (both traversal kernels would share it) nor with hide_emitters.  HAR_OVERLAP = 0 / 1 forces it off / on (A/B). */
inline bool overlap_applies(const Switches &W, const SceneFacts &F, bool hide_emitters, uint64_t n) {
    if (W.force_stack_spill || F.stack_need > F.lds_stack || hide_emitters) return false;
    return W.overlap < 0 ? n <= HAR_OVERLAP_MAX_LANES : W.overlap != 0;
}

inline ChunkPlan plan_chunk(const Switches &W, const Settings &I, const SceneFacts &F, const ChunkJob &J) {
    ChunkPlan P{};
    const int mode = J.mode;
    const bool tape_r = J.cache_mode == TAPE_READ, rec_w = J.cache_mode == RECORD_WRITE;
    P.mq_on = W.material_queues < 0 ? I.material_queues : W.material_queues != 0;      /* -1: the integrator's setting; 0 / 1 force (A/B) */
    /* FIRST VERTEX: the state of a path at bounce 0 is a function of its lane index -- the ray generation kernel stores only the rays (32 of 72 B per lane) and the first
     * shading launch rebuilds the state instead of reading it (k_raygen<.., LITE>, k_shade<.., FIRST>; ShadeParams::sensor).  Plain forward renders and the recording pass of prb, of one pass, whose
     * bounce-0 wavefront nobody else reads (no alpha / validity flags, no material queues, no tape); the passes of a multi-pass forward render resume their samplers from the pass state in both kernels.  HAR_FIRST_VERTEX=0 switches it off (A/B) */
    P.first_regen = W.first_vertex && ((mode == MODE_PATH && J.cache_mode == CACHE_NONE) || (mode == MODE_PRB_PRIMAL && rec_w && J.adjoint_image && !J.forward_mode && !J.pass_rng)) && !J.rays && !J.valid_lane && !(I.alpha_film && J.alpha_lane) && !I.batch.n && J.projection != 2u /* thin lens: k_raygen_lens stores the full state, as k_raygen_batch does */ &&
                    !P.mq_on && !(F.bsdf_types & HAR_SCENE_WIDE_ROUTE) /* scenes with a `blendbsdf` / `mask` / `normalmap` record or a `mesh_attribute` texture run one widest shading kernel per flavour (launch_shade): no FIRST instantiation */;
    P.fwd = mode == MODE_PRB_ADJOINT && J.forward_mode;
    P.shade_flags = ((mode != MODE_PATH && I.grad_emitters) ? HAR_SHADE_EMITTER_GRADS : 0u)      /* (the primal pass of a backward step too: it traces the shadow rays of samples that only carry a radiance gradient, shade_lane) */ | (I.hide_emitters ? HAR_SHADE_HIDE_EMITTERS : 0u) |
                    (P.fwd ? HAR_SHADE_FORWARD_MODE : 0u) | ((mode == MODE_PRB_ADJOINT && I.grad_bsdf_params && !P.fwd) ? HAR_SHADE_EXTRA_GRADS : 0u) |
                    /* both passes of a backward step: the primal pass traces the shadow rays whose visibility the adjoint pass reads (shade_lane: lt_item) */
                    ((mode != MODE_PATH && I.grad_light_texels && !J.forward_mode && (F.bsdf_types & HAR_SCENE_TEXLIGHT)) ? HAR_SHADE_LIGHT_TEXELS : 0u) |
                    /* ... likewise for the texels of the environment map (the kernels that carry its code: HAR_SCENE_ENVMAP; env_emitter: the scene has an environment) */
                    ((mode != MODE_PATH && I.grad_envmap && !J.forward_mode && (F.bsdf_types & HAR_SCENE_ENVMAP) && F.env_emitter >= 0) ? HAR_SHADE_ENV_TEXELS : 0u);
    /* grid: a multiple of 8 so that block b serves shard b % 8; enough blocks to cover the chunk once */
    P.grid = std::max<uint32_t>(SWITCH_SHARDS, std::min<uint32_t>(((J.n + 255) / 256 + SWITCH_SHARDS - 1) / SWITCH_SHARDS * SWITCH_SHARDS, 4096u));
    /* persistent traversal kernels: enough blocks to fill the chip (<= 8 blocks/CU), never more than the work; HAR_TRACE_GRID (A/B): blocks of a persistent launch */
    P.tgrid = std::min<uint32_t>(P.grid, W.trace_grid ? std::min<uint32_t>(W.trace_grid, PLAN_MAX_TRAVERSAL_BLOCKS) : PLAN_MAX_TRAVERSAL_BLOCKS);
    /* scenes whose depth-first stack bound fits the LDS entries run the kernels without the HBM spill path */
    P.spill = W.force_stack_spill || F.stack_need > F.lds_stack;
    P.shape = mode == MODE_PRB_ADJOINT && J.shape_on;
    /* adjoint replay of a cached bounce: `shade` commits the vertex adjoint itself (the shadow-ray result is in the cache), no items, no resolve launch */
    P.inline_commit = W.adjoint_inline && mode == MODE_PRB_ADJOINT && !P.shape && !J.forward_mode;      /* forward mode commits in the resolve kernels (own instantiation) */
    /* per-material shading queues: scenes with more than one BSDF model, `path` and the primal pass of `prb` (the adjoint kernels keep the generic code:
     * their in-place commit is bound by memory traffic, not by the model code).  HAR_MATERIAL_QUEUES=0: the generic kernel with its block-local sort (A/B) */
    P.use_mq = P.mq_on && mode != MODE_PRB_ADJOINT && J.cache_mode != RECORD_WRITE && __builtin_popcount(F.mat_classes) >= 2 && !(F.bsdf_types & (HAR_SCENE_ENVMAP | HAR_SCENE_WIDE_ROUTE));
    P.overlap = mode != MODE_PRB_ADJOINT && !J.rays && overlap_applies(W, F, I.hide_emitters, J.n);
    /* LATE OVERLAP (jobs too large for the full overlap above): from bounce `late_from` on, bounce b's shadow rays run on the second stream NEXT TO bounce b + 1's
     * closest-hit rays, and bounce b + 1's shading waits for them -- so both kernels keep writing the one `result` array (no second item set, no result2, no final add:
     * what made the full overlap neutral on a 67 M-lane frame).  The idea was that the launches past the Russian-roulette depth (0.4 - 1 ms each for a few per cent of the
     * frame's rays) would hide each other's tails; measured +0.7 % at best on the headline frame and -0.7 ... +0.4 % elsewhere (profiles/r05_ab_late_overlap.txt): two
     * persistent launches share the same issue slots, there was no idle tail to fill.  DEFAULT OFF; HAR_LATE_OVERLAP=<first bounce> switches it on (A/B) */
    const bool late_ok = !P.overlap && mode != MODE_PRB_ADJOINT && !J.rays && W.late_overlap != -1 && overlap_applies(W, F, I.hide_emitters, 0);      /* n = 0: every condition of the full overlap but the job's size */
    P.late_from = W.late_overlap >= 0 ? (uint32_t) W.late_overlap : (uint32_t) HAR_LATE_OVERLAP_DEFAULT(I.rr_depth);
    P.late_on = late_ok && P.late_from < J.nb;
    /* camera rays at >= 64 samples per pixel: a wave is one pixel, its 64 rays walk the BVH together (k_trace_packet); what that kernel gives up on
     * -- incoherent packets -- goes to the per-lane kernel through a list.  Same hit records either way.  HAR_PACKET=0 / 1 forces it off / on (A/B). */
    const int packet_mode = W.packet >= 0 ? W.packet : I.packet_tracing;
    P.packet = !tape_r && (packet_mode < 0 ? (!J.rays && J.spp >= 64 && J.spp % 64 == 0 && J.lane_base % 64 == 0) : packet_mode != 0);
    /* `rgba` films: is the camera sample valid?  (path.cpp:114-115,307-308; prb.py:332) */
    P.alpha_flags = ((I.alpha_film && J.alpha_lane) || J.valid_lane) && mode != MODE_PRB_ADJOINT;
    P.alpha_miss = (mode == MODE_PATH && F.env_emitter >= 0 && !I.hide_emitters) ? 1.f : 0.f;
    /* a scene with a mask record, `path`, no visible environment (with one every sample is valid from the start): the flags come out of shading, asked for or not -- the
     * radiance of an invalid sample is dropped.  prb keeps depth != 0 (prb.py:332: null interactions count), i.e. k_alpha_flags */
    /* ... and a scene with a `thindielectric` record likewise: its transmission lobe is a null lobe (thindielectric.cpp:126), whichever record sampled it */
    P.valid_shade = mode == MODE_PATH && (F.bsdf_types & (HAR_SCENE_MASK | HAR_SCENE_THIN)) != 0u && P.alpha_miss == 0.f;
    if (P.valid_shade) P.alpha_flags = false;
    return P;
}

}
