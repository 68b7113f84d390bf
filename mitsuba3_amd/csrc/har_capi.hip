/*
 * har_capi.hip -- the render half of the C ABI declared in include/hip_ad_rgb.h: the integrator handle and the render calls.
 * (Device memory and profiling events: har_device_mem.hip; scenes and the ray / sampler / BSDF / sensor / film queries: har_scene_api.hip.)
 *
 * Host-side driver of the wavefront integrators: SamplingIntegrator::render
 * (src/render/integrator.cpp:151-396, JIT branch) and RBIntegrator.render_backward
 * (src/python/python/ad/integrators/common.py:625-783) re-expressed as an
 * asynchronous sequence of HIP kernel launches on the caller's stream.
 */
#include "har_impl.h"
#include "har_aov_launch.h"

static_assert(SWITCH_SHARDS == HAR_SHARDS && PLAN_MAX_TRAVERSAL_BLOCKS == HAR_MAX_TRAVERSAL_BLOCKS, "har_switches.h / har_plan.h carry copies of two constants of har_kernels.h");

namespace {

uint32_t log2_exact(uint32_t v) { for (uint32_t k = 0; k < 32; ++k) if ((1u << k) == v) return k; return 0xffffffffu; }

static inline uint32_t *cnt_alive(HarIntegratorImpl *I, uint32_t b) { return I->counters + (size_t) b * HAR_SHARDS * HAR_COUNTER_STRIDE; }
static inline uint32_t *cnt_items(HarIntegratorImpl *I, uint32_t b) { return I->counters + (size_t) (HAR_MAX_BOUNCE_SLOTS + b) * HAR_SHARDS * HAR_COUNTER_STRIDE; }
/* work cursors of the persistent traversal kernels (one per bounce and shard) */
static inline uint32_t *cur_trace(HarIntegratorImpl *I, uint32_t b) { return I->counters + (size_t) (2 * HAR_MAX_BOUNCE_SLOTS + b) * HAR_SHARDS * HAR_COUNTER_STRIDE; }
static inline uint32_t *cur_resolve(HarIntegratorImpl *I, uint32_t b) { return I->counters + (size_t) (3 * HAR_MAX_BOUNCE_SLOTS + b) * HAR_SHARDS * HAR_COUNTER_STRIDE; }

/* the acceleration structure as this integrator's closest-hit launches see it: Accel::top_seed is the scene's choice (build_tlas) unless the integrator's `top_seed`
 * property or HAR_TOP_SEED (as read when the integrator was created) forces it.  On needs a two-level scene with top-level geometry. */
static Accel seeded_accel(const HarIntegratorImpl *I, const Accel &scene_accel) {
    Accel A = scene_accel;
    const int mode = I->set.top_seed_env >= 0 ? I->set.top_seed_env : I->set.top_seed;
    if (mode == 0) A.top_last &= ~HAR_TOP_SEED_BIT;
    else if (mode == 1 && A.has_tlas && A.top_root != HAR_NO_NODE && A.top_count >= 1u) A.top_last |= HAR_TOP_SEED_BIT;
    return A;
}
static SceneFacts scene_facts(const HarSceneImpl *S) {
    return SceneFacts{ S->hs.stack_need() + HAR_STACK_MARGIN, HAR_LDS_STACK_SMALL, S->mat_classes, S->ds.bsdf_types, S->ds.env_emitter };
}
/* shadow-ray overlap for a job of n lanes of this scene and integrator?  (har_plan.h) */
static bool overlap_applies(const HarSceneImpl *S, const HarIntegratorImpl *I, uint64_t n) { return overlap_applies(switches(), scene_facts(S), I->set.hide_emitters, n); }

/* rays of har_integrator_sample: SoA arrays of n_total rays, the chunk covers [first, first + n) */
struct RaySource { const float *o, *d, *maxt; const uint64_t *state; const uint8_t *active; uint32_t n_total, first; };

/* texel gradients of a launch through the band queues (TexelQueues): clear the queues' counters before the launch that fills them ... */
static int texel_queues_begin(HarIntegratorImpl *I, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(I->tq.count, 0, (size_t) (HAR_SHARDS * I->tq.nq + 1) * HAR_COUNTER_STRIDE * sizeof(uint32_t), s));
    return 0;
}
/* ... and add the bands to the textures' gradient buffers behind it.  HAR_TQ_BPQ: blocks per queue (A/B) */
static void texel_queues_accumulate(HarIntegratorImpl *I, uint32_t n, hipStream_t s) {
    const uint32_t bpq = switches().tq_bpq;
    launch_texel_accumulate(s, I->tq, I->d_grad_tex, bpq ? bpq : (n > (1u << 22) ? 4u : 1u), I->tq_lds);
}

/* the whole adjoint pass of the record tape: L / dL into bounce 0's slot order, then one streaming commit per bounce (+ the texel queues' accumulation) */
static int commit_pass(HarSceneImpl *S, HarIntegratorImpl *I, uint32_t nb, uint32_t n, uint32_t cgrid, float *grad_refl, hipStream_t s) {
    for (uint32_t b = 0; b < nb; ++b) {
        const size_t off = (size_t) b * I->ws_lanes;
        const TapeArrays tp{ I->tape_next + off, I->tape_la[b & 1], I->tape_lb[b & 1], I->tape_la[(b & 1) ^ 1], I->tape_lb[(b & 1) ^ 1],
                             I->tape_rec[0] + off, I->tape_rec[1] + off, I->tape_rec[2] + off, I->tape_rec[3] + off };
        const bool queued = I->tq.nq != 0;
        if (queued && texel_queues_begin(I, s)) return 1;
        launch_commit(s, cgrid, S->ds, I->shard_cap, cnt_alive(I, b), tp, I->tape_vis + off, grad_refl, I->d_grad_tex, queued ? &I->tq : nullptr,
                      b == 0 ? I->result : nullptr, b == 0 ? I->dL : nullptr);
        prof_mark(I, s, CLS_SHADE);
        if (queued) { texel_queues_accumulate(I, n, s); prof_mark(I, s, CLS_OTHER); }
    }
    launch_accumulate_stats(s, I->counters, nb, I->totals, n);
    prof_mark(I, s, CLS_OTHER);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Integrator::skip_area_emitters (integrator.cpp:96-124) for the camera rays: continuation rays are gathered into a list, traced, and
 * their hits replace the lanes' hits until no lane sits on an area emitter any more.  Scratch: the other wavefront buffer holds the two
 * lists, the (still unused) item arrays the re-traced hits.  One host round trip per round -- `hide_emitters` is not a hot path. */
static int skip_area_emitters(HarSceneImpl *S, HarIntegratorImpl *I, uint32_t grid, uint32_t tgrid, uint2 *spill, const WaveState &st_in, const WaveState &st_out,
                              float4 *h0, uint2 *h1, hipStream_t s) {
    const size_t cs = (size_t) HAR_SHARDS * HAR_COUNTER_STRIDE;
    uint32_t *cnt[2] = { I->skip_counters, I->skip_counters + 2 * cs }, *cursor[2] = { I->skip_counters + cs, I->skip_counters + 3 * cs };
    float4 *lo[2] = { st_out.a0, st_out.a2 }, *ld[2] = { st_out.a1, st_out.a3 };
    if (!I->hit_scratch && ws_alloc(I, &I->hit_scratch, (size_t) 2 * I->ws_lanes)) return 1;       /* re-traced hits: records in the layout of h0 / h1 */
    float4 *sh0 = I->hit_scratch; uint2 *sh1 = HAR_HIT_INTERLEAVED ? reinterpret_cast<uint2 *>(I->hit_scratch + 1) : reinterpret_cast<uint2 *>(I->hit_scratch + I->ws_lanes);
    HIP_TRY(hipMemsetAsync(I->skip_counters, 0, 4 * cs * sizeof(uint32_t), s));
    launch_skip_emitters(s, grid, S->ds, 1, I->shard_cap, cnt_alive(I, 0), st_in.a0, st_in.a1, nullptr, nullptr, h0, h1, lo[0], ld[0], cnt[0]);
    for (int round = 0, a = 0; round < 256; ++round, a ^= 1) {
        uint32_t host[HAR_SHARDS * HAR_COUNTER_STRIDE];
        HIP_TRY(hipMemcpyAsync(host, cnt[a], sizeof(host), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        uint32_t total = 0; for (int k = 0; k < HAR_SHARDS; ++k) total += host[k * HAR_COUNTER_STRIDE];
        if (total == 0) break;
        WaveState list{ lo[a], ld[a], nullptr, nullptr, nullptr };
        launch_trace_closest(s, tgrid, spill, S->ds.accel, cnt[a], cursor[a], I->shard_cap, list, sh0, sh1, I->status);
        HIP_TRY(hipMemsetAsync(cnt[a ^ 1], 0, cs * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(cursor[a ^ 1], 0, cs * sizeof(uint32_t), s));
        launch_skip_emitters(s, grid, S->ds, 0, I->shard_cap, cnt[a], lo[a], ld[a], sh0, sh1, h0, h1, lo[a ^ 1], ld[a ^ 1], cnt[a ^ 1]);
    }
    prof_mark(I, s, CLS_OTHER);
    return 0;
}

/* one chunk: raygen + bounce loop.  `mode` selects path / prb primal / prb adjoint kernels; `rays` != nullptr: the wavefront starts from
 * caller-supplied rays (SamplingIntegrator::sample) instead of the sensor; `valid_lane` != nullptr receives the samples' masks.  Everything that is
 * decided per chunk is decided by plan_chunk (har_plan.h) before the first launch. */
int run_chunk(HarSceneImpl *S, HarIntegratorImpl *I, const DSensor &C, int mode, uint32_t seed, uint32_t spp, uint32_t log_spp,
              uint32_t lane_base, uint32_t n, float *grad_refl, hipStream_t s, CacheMode cache_mode = CACHE_NONE, const PassState &ps = PassState{ nullptr, nullptr, 0 },
              const RaySource *rays = nullptr, float *valid_lane = nullptr) {
    const uint32_t nb = bounce_limit(I);
    const size_t used = (size_t) std::min<uint32_t>(nb + 2, HAR_MAX_BOUNCE_SLOTS) * HAR_SHARDS * HAR_COUNTER_STRIDE * sizeof(uint32_t);
    /* replay tape (the primal pass records, the adjoint pass replays; TapeArrays in har_kernels.h) */
    const bool tape_w = cache_mode == TAPE_WRITE, tape_r = cache_mode == TAPE_READ, tape = tape_w || tape_r;
    /* record tape (the primal pass shades with the adjoint flavour and writes one record per vertex, the adjoint pass is k_commit) */
    const bool rec_w = cache_mode == RECORD_WRITE, rec_r = cache_mode == RECORD_READ;
    if (tape && (I->ws_tape != 1 || nb > I->tape_bounces || rays)) return fail("internal: tape mode without a tape workspace");
    if ((rec_w || rec_r) && (I->ws_tape != 2 || nb > I->tape_bounces || rays)) return fail("internal: record-tape mode without its workspace");
    const ChunkJob job{ mode, cache_mode, n, spp, lane_base, nb, rays != nullptr, valid_lane != nullptr, ps.rng != nullptr, C.projection,
                        I->forward_mode, I->shape_on, I->adj != nullptr, I->alpha_lane != nullptr };
    const ChunkPlan plan = plan_chunk(switches(), I->set, scene_facts(S), job);
    /* a scene with a `normalmap` record has the forward, the prb-primal and the in-place adjoint shading kernels (launch_shade): every other flavour is refused here, where
     * every shading launch starts, instead of running a bounce that shades nothing */
    if ((S->ds.bsdf_types & HAR_SCENE_NORMALMAP) && (rec_w || rec_r || (mode == MODE_PRB_ADJOINT && !(plan.inline_commit && (cache_mode == CACHE_READ || cache_mode == TAPE_READ)))))
        return fail("normalmap: a scene with a `normalmap` record has no item-writing adjoint or record-tape shading kernel (its gradients take the in-place commit of the replay cache)");
    if ((S->ds.bsdf_types & HAR_SCENE_BUMPMAP) && (rec_w || rec_r || (mode == MODE_PRB_ADJOINT && !(plan.inline_commit && (cache_mode == CACHE_READ || cache_mode == TAPE_READ)))))
        return fail("bumpmap: a scene with a `bumpmap` record has no item-writing adjoint or record-tape shading kernel (its gradients take the in-place commit of the replay cache)");
    if ((S->ds.bsdf_types & HAR_SCENE_ALPHAMAP) && (rec_w || rec_r || (mode == MODE_PRB_ADJOINT && !(plan.inline_commit && (cache_mode == CACHE_READ || cache_mode == TAPE_READ)))))
        return fail("roughness map: a scene with a bitmap `alpha` has no item-writing adjoint or record-tape shading kernel (its gradients take the in-place commit of the replay cache)");
    /* (a pane among plain models -- the lean set -- has the item-writing adjoint that forward mode reads) */
    const bool thin_lean_fwd = (S->ds.bsdf_types & HAR_SCENE_WIDE_ROUTE) == HAR_SCENE_THIN && I->forward_mode && !rec_w && !rec_r;
    if (plan.mq_on && (S->ds.bsdf_types & HAR_SCENE_THIN))
        return fail("thindielectric: `material_queues` cannot serve a scene with a `thindielectric` record (the model has no material class of its own; its scenes run one shading kernel per flavour)");
    if ((S->ds.bsdf_types & HAR_SCENE_THIN) && !thin_lean_fwd && (rec_w || rec_r || (mode == MODE_PRB_ADJOINT && !(plan.inline_commit && (cache_mode == CACHE_READ || cache_mode == TAPE_READ)))))
        return fail("thindielectric: a scene with a `thindielectric` record has no item-writing adjoint or record-tape shading kernel (its gradients take the in-place commit of the replay cache)");
    const uint32_t grid = plan.grid, tgrid = plan.tgrid;
    if (rec_r) return commit_pass(S, I, nb, n, grid, grad_refl, s);
    if (!tape_r) HIP_TRY(hipMemsetAsync(cnt_alive(I, 0), 0, used, s));      /* the replay reads the primal pass's wavefront sizes */
    HIP_TRY(hipMemsetAsync(cnt_items(I, 0), 0, used, s));
    HIP_TRY(hipMemsetAsync(cur_trace(I, 0), 0, used, s));
    HIP_TRY(hipMemsetAsync(cur_resolve(I, 0), 0, used, s));
    const bool first_regen = plan.first_regen;
    if (tape_r) launch_tape_begin(s, C, seed, spp, log_spp, lane_base, n, I->shard_cap, I->result, I->adj, I->tape_la[0], I->tape_lb[0]);
    else if (rays) launch_raygen_rays(s, seed, lane_base, n, rays->n_total, rays->first, rays->o, rays->d, rays->maxt, rays->state, rays->active, I->shard_cap, I->st[0], I->result, cnt_alive(I, 0));
    /* forward mode: k_raygen<ADJOINT> takes `adj == nullptr` as "zero dL" -- a workspace that served render_backward before still holds that call's adjoint
     * image in I->adj (possibly of a smaller film), which must not be gathered here */
    /* the adjoint image goes to the adjoint raygen (dL per lane; not in forward mode: dL accumulates there) and to the primal raygen of the record tape (dL for its emission terms) */
    else launch_raygen(mode, s, C, seed, spp, log_spp, lane_base, n, I->shard_cap, tape_w ? I->tape_st[0] : I->st[0], I->result, cnt_alive(I, 0),
                       (I->forward_mode || (mode == MODE_PRB_PRIMAL && !rec_w)) ? nullptr : I->adj, I->dL, ps, first_regen, I->set.batch.n ? &I->set.batch : nullptr);
    prof_mark(I, s, CLS_RAYGEN);
    const bool fwd = plan.fwd;
    ShadeParams P{ seed, I->set.max_depth, I->set.rr_depth, plan.shade_flags };
    /* generic shading kernels: material-sort window in tiles of 256 paths (k_shade; HAR_SORT_WINDOW=1 is the round-3 kernel, A/B) */
    P.sort_window = switches().sort_window;
    /* `path` in a scene with a mask record: the validity flags start at 0 (the miss value: no visible environment here) and come out of shading */
    float *valid_dst = nullptr;
    if (plan.valid_shade) {
        if (!valid_lane && !I->alpha_lane && ws_alloc(I, &I->alpha_lane, I->ws_lanes)) return 1;
        valid_dst = valid_lane ? valid_lane : I->alpha_lane;
        HIP_TRY(hipMemsetAsync(valid_dst, 0, (size_t) n * sizeof(float), s));
    }
    ShadeParams P0 = P;           /* bounce 0 with first_regen */
    if (first_regen) { P0.flags |= HAR_SHADE_FIRST_VERTEX; P0.spp = spp; P0.log_spp = log_spp; P0.sensor = C; P0.resume = (ps.rng && ps.pass) ? 1u : 0u; }
    uint2 *spill = plan.spill ? I->stack_spill : nullptr;
    const bool shape = plan.shape, inline_commit = plan.inline_commit, use_mq = plan.use_mq;
    const ShapeTargets targets{ I->d_pos_offset, I->grad_pos, I->pos_verts, I->d_inst_slot, I->grad_inst, I->inst_count, I->grad_nrm };
    if (use_mq && !I->mq_idx && (ws_alloc(I, &I->mq_idx, (size_t) HAR_MAT_CLASSES * I->ws_lanes) || ws_alloc(I, &I->mq_count, (size_t) HAR_MAT_CLASSES * HAR_SHARDS * HAR_COUNTER_STRIDE))) return 1;
    const MaterialQueues mq{ I->mq_idx, I->mq_count, I->ws_lanes, S->mat_miss_class };
    /* the plan WANTS the overlaps; without the second stream, its events or the second item set the chunk runs on one stream (an optimisation, not a requirement) */
    bool overlap = plan.overlap, late_on = plan.late_on, late_pending = false;
    const uint32_t late_from = plan.late_from;
    if ((overlap || late_on) && !I->aux_stream) {
        if (hipStreamCreateWithFlags(&I->aux_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&I->ev_shaded, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&I->ev_resolved, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&I->ev_resolved2, hipEventDisableTiming) != hipSuccess) { I->aux_stream = nullptr; overlap = false; late_on = false; }
    }
    if (overlap && !I->result2 && (ws_alloc(I, &I->items2.s0, I->ws_lanes) || ws_alloc(I, &I->items2.s1, I->ws_lanes) || ws_alloc(I, &I->items2.s2, I->ws_lanes) || ws_alloc(I, &I->result2, I->ws_lanes))) {
        I->result2 = nullptr; overlap = false; (void) hipGetLastError();      /* no room for the second item set: one stream (an optimisation, not a requirement) */
    }
    if (overlap) HIP_TRY(hipMemsetAsync(I->result2, 0, (size_t) n * sizeof(float4), s));
    /* `path` on one stream adds an emitter sample as path.cpp:279 does, with one rounding (HAR_SHADE_FUSED_NEE): k_resolve reads the throughput from the bounce's input
     * wavefront, which stands until the NEXT bounce is shaded (the ping-pong pair) -- later than every resolve launch below but the overlapped one, whose shadow rays
     * run next to that shading launch and whose sums reach `result` in another order anyway (result2).  Not bounce 0 of FIRST VERTEX (no stored state; the throughput is 1).
     * Only for caller-supplied rays (Integrator::sample), whose per-lane radiance the caller sees and can hold against the reference bit by bit; a film is a sum of
     * atomics in no fixed order, and there the extra 16-byte read per unoccluded shadow ray cost 1.5 % of the headline frame (1125 against 1142 Mpaths/s on an MI355X) */
    const bool fused_nee = mode == MODE_PATH && rays && !overlap;
    if (fused_nee) P.flags |= HAR_SHADE_FUSED_NEE;
    hipEvent_t ev_res[2] = { I->ev_resolved, I->ev_resolved2 };
    bool resolve_pending[2] = { false, false };
    int cur = 0; uint32_t b = 0;
    for (; b < nb; ++b) {
        /* PRB replay cache: the primal pass of render_backward records this bounce's ray-query results per lane, the adjoint pass reads them */
        ReplayCache rc{ nullptr, nullptr, nullptr, CACHE_NONE };
        if (tape || rec_w) rc = ReplayCache{ nullptr, nullptr, I->tape_vis + (size_t) b * I->ws_lanes, cache_mode };
        else if (cache_mode && b < I->cache_bounces)
            rc = ReplayCache{ I->rc_h0 + (size_t) b * I->ws_lanes, I->rc_h1 + (size_t) b * I->ws_lanes, I->rc_vis + (size_t) b * I->ws_lanes, cache_mode };
        const bool cached = rc.mode == CACHE_READ || rc.mode == TAPE_READ;             /* adjoint replay of a cached / taped bounce */
        /* the wavefront buffers of this bounce: the ping-pong pair, or the tape's per-bounce buffers (path state in / out, hit records) */
        const WaveState st_in = tape ? I->tape_st[b] : I->st[cur], st_out = tape ? I->tape_st[b + 1] : I->st[cur ^ 1];
        float4 *const h0 = tape ? I->tape_h0 + (size_t) 2 * I->ws_lanes * b : I->h0;
        uint2 *const h1 = tape ? (HAR_HIT_INTERLEAVED ? reinterpret_cast<uint2 *>(h0 + 1) : reinterpret_cast<uint2 *>(h0 + I->ws_lanes)) : I->h1;
        const size_t toff = (size_t) b * I->ws_lanes;
        const TapeArrays tp{ (tape || rec_w) ? I->tape_next + toff : nullptr, I->tape_la[b & 1], I->tape_lb[b & 1], I->tape_la[(b & 1) ^ 1], I->tape_lb[(b & 1) ^ 1],
                             rec_w ? I->tape_rec[0] + toff : nullptr, rec_w ? I->tape_rec[1] + toff : nullptr, rec_w ? I->tape_rec[2] + toff : nullptr, rec_w ? I->tape_rec[3] + toff : nullptr };
        if (!cached) {
            if (b == 0 && plan.packet) {
                const size_t cs = (size_t) HAR_SHARDS * HAR_COUNTER_STRIDE;
                const PacketList pl{ I->pk_list, I->pk_counters, I->pk_counters + cs, cnt_alive(I, b), I->shard_cap / 64u + 1u };
                HIP_TRY(hipMemsetAsync(I->pk_counters, 0, 2 * cs * sizeof(uint32_t), s));
                launch_trace_packet(s, tgrid, S->ds.accel, cnt_alive(I, b), cur_trace(I, b), I->shard_cap, st_in, h0, h1, pl, switches().packet_budget);
                prof_mark(I, s, CLS_TRACE);             /* two launches of the closest-hit class: the packets, then the rays of the packets that gave up */
                launch_trace_closest(s, tgrid, spill, S->ds.accel, pl.count, pl.cursor, I->shard_cap, st_in, h0, h1, I->status, &pl);
            } else
            launch_trace_closest(s, tgrid, spill, seeded_accel(I, S->ds.accel), cnt_alive(I, b), cur_trace(I, b), I->shard_cap, st_in, h0, h1, I->status);
            prof_mark(I, s, CLS_TRACE);
            if (I->stagger_record && b == 0) { HIP_TRY(hipEventRecord(I->ev_stagger, s)); I->stagger_record = false; }
        }
        if (I->set.hide_emitters && b == 0 && !cached && skip_area_emitters(S, I, grid, tgrid, spill, st_in, st_out, h0, h1, s)) return 1;
        if (plan.alpha_flags && b == 0) launch_alpha_flags(s, grid, I->shard_cap, cnt_alive(I, 0), st_in, h0, lane_base, plan.alpha_miss, valid_lane ? valid_lane : I->alpha_lane);
        /* vertex-position gradients of the PREVIOUS bounce's vertices: its items are still in place, `result` holds its L, and this bounce's ray
         * queries give the (detached) next interaction of every continued path */
        if (shape && b > 0) {
            launch_shape_adjoint(s, grid, S->ds, cnt_items(I, b - 1), I->shard_cap, I->items, I->geo, I->result, I->dL, 1, st_in, h0, h1, rc, targets);
            prof_mark(I, s, CLS_OTHER);
        }
        /* bounce b - 2's shadow rays used the item set this bounce's shading is about to fill */
        if (resolve_pending[b & 1]) { HIP_TRY(hipStreamWaitEvent(s, ev_res[b & 1], 0)); resolve_pending[b & 1] = false; }
        /* late overlap: bounce b - 1's shadow rays ran next to this bounce's closest-hit rays; shading touches `result` and refills the item set they read */
        if (late_pending) { HIP_TRY(hipStreamWaitEvent(s, I->ev_resolved, 0)); late_pending = false; prof_mark(I, s, CLS_RESOLVE); }
        const ItemArrays &items_b = (overlap && (b & 1)) ? I->items2 : I->items;
        const bool queued = inline_commit && cached && I->tq.nq != 0;                 /* texel gradients of this bounce go through the band queues */
        if (queued && texel_queues_begin(I, s)) return 1;
        if (use_mq) {
            /* classify the bounce's hits, then one specialised launch per material class of the scene; the launches append their survivors / items to the
             * same compacted queues (slot reservation is per block, so the order of the classes does not matter to any path) */
            HIP_TRY(hipMemsetAsync(I->mq_count, 0, (size_t) HAR_MAT_CLASSES * HAR_SHARDS * HAR_COUNTER_STRIDE * sizeof(uint32_t), s));
            launch_classify(s, grid, S->ds, I->shard_cap, cnt_alive(I, b), h0, h1, mq);
            for (uint32_t c = 0; c < HAR_MAT_CLASSES; ++c)
                if (S->mat_classes & (1u << c))
                    launch_shade(mode, s, grid, S->ds, P, lane_base, I->shard_cap, cnt_alive(I, b), st_in, h0, h1, st_out, cnt_alive(I, b + 1),
                                 items_b, cnt_items(I, b), I->result, rc, ps.rng, I->dL, grad_refl, nullptr, nullptr, nullptr, nullptr, &mq, c, tape ? &tp : nullptr);
        } else
        launch_shade(mode, s, grid, S->ds, (b == 0 && first_regen) ? P0 : P, lane_base, I->shard_cap, cnt_alive(I, b), st_in, h0, h1, st_out, cnt_alive(I, b + 1),
                     items_b, cnt_items(I, b), I->result, rc, ps.rng, I->dL, grad_refl, shape ? &I->geo : nullptr, inline_commit && cached ? I->d_grad_tex : nullptr,
                     queued ? &I->tq : nullptr, valid_dst ? valid_dst /* `path`, mask scene: launch_shade hands the flags to the kernel in this slot */ : (inline_commit && cached) ? I->set.grad_bsdf_params : nullptr, nullptr, 0, (tape || rec_w) ? &tp : nullptr);
        prof_mark(I, s, CLS_SHADE);
        const float4 *const beta = (fused_nee && !(b == 0 && first_regen)) ? st_in.a2 : nullptr;
        if (queued) { texel_queues_accumulate(I, n, s); prof_mark(I, s, CLS_OTHER); }
        if (overlap) {
            HIP_TRY(hipEventRecord(I->ev_shaded, s));
            HIP_TRY(hipStreamWaitEvent(I->aux_stream, I->ev_shaded, 0));
            launch_resolve(mode, I->aux_stream, tgrid, spill, S->ds, cnt_items(I, b), cur_resolve(I, b), I->shard_cap, items_b, I->result2, I->dL, grad_refl, I->d_grad_tex, I->status, rc, nullptr, 0);
            HIP_TRY(hipEventRecord(ev_res[b & 1], I->aux_stream));
            resolve_pending[b & 1] = true;
        } else if (late_on && b >= late_from && b + 1 < nb) {
            HIP_TRY(hipEventRecord(I->ev_shaded, s));
            HIP_TRY(hipStreamWaitEvent(I->aux_stream, I->ev_shaded, 0));
            launch_resolve(mode, I->aux_stream, tgrid, spill, S->ds, cnt_items(I, b), cur_resolve(I, b), I->shard_cap, I->items, I->result, I->dL, grad_refl, I->d_grad_tex, I->status, rc, nullptr, 0, nullptr, beta);
            HIP_TRY(hipEventRecord(I->ev_resolved, I->aux_stream));
            late_pending = true;
        } else if (!(inline_commit && cached)) {
            /* adjoint items of a cached bounce (the path vertex-position gradients take): texel gradients through the band queues, as in the in-place commit */
            const bool item_queued = mode == MODE_PRB_ADJOINT && rc.mode == CACHE_READ && !fwd && I->tq.nq != 0;
            if (item_queued && texel_queues_begin(I, s)) return 1;
            launch_resolve(mode, s, rc.mode == CACHE_READ ? grid : tgrid, spill, S->ds, cnt_items(I, b), cur_resolve(I, b), I->shard_cap, I->items, I->result, I->dL, grad_refl, I->d_grad_tex, I->status, rc,
                           shape ? I->geo.vis : nullptr, fwd ? 1 : 0, item_queued ? &I->tq : nullptr, beta);
            if (item_queued) texel_queues_accumulate(I, n, s);
        }
        prof_mark(I, s, CLS_RESOLVE);
        cur ^= 1;
        if (b >= 15 && (b & 7) == 7) {           /* deep paths are rare: poll so that max_depth = -1 terminates */
            uint32_t alive[HAR_SHARDS * HAR_COUNTER_STRIDE];
            HIP_TRY(hipMemcpyAsync(alive, cnt_alive(I, b + 1), sizeof(alive), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            uint32_t total = 0; for (int k = 0; k < HAR_SHARDS; ++k) total += alive[k * HAR_COUNTER_STRIDE];
            if (total == 0) { ++b; break; }
        }
    }
    for (int k = 0; k < 2; ++k) if (resolve_pending[k]) HIP_TRY(hipStreamWaitEvent(s, ev_res[k], 0));
    if (late_pending) { HIP_TRY(hipStreamWaitEvent(s, I->ev_resolved, 0)); late_pending = false; prof_mark(I, s, CLS_RESOLVE); }
    if (overlap) launch_add(s, reinterpret_cast<const float *>(I->result2), reinterpret_cast<float *>(I->result), 4u * n);      /* the shadow rays' share of the radiance */
    if (valid_dst) launch_drop_invalid(s, n, valid_dst, I->result);
    if (shape && b > 0) {            /* the last bounce: no path continues */
        launch_shape_adjoint(s, grid, S->ds, cnt_items(I, b - 1), I->shard_cap, I->items, I->geo, I->result, I->dL, 0, I->st[cur], I->h0, I->h1, ReplayCache{ nullptr, nullptr, nullptr, CACHE_NONE }, targets);
        prof_mark(I, s, CLS_OTHER);
    }
    if (mode != MODE_PRB_PRIMAL) {
        launch_accumulate_stats(s, I->counters, std::min(b + 1, nb), I->totals, n);
        prof_mark(I, s, CLS_OTHER);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* pixels of the sample grid of render(): the crop window, plus the filter border with Film::sample_border (integrator.cpp:162-165) */
int sample_grid(const HarSensor *sensor, uint32_t &w, uint32_t &h) {
    DSensor C; std::string e;
    if (!sensor) return fail("null sensor");
    if (!lower_sensor(*sensor, C, e)) return fail(e);
    w = C.samp_w; h = C.samp_h;
    return 0;
}

/* SamplingIntegrator::render, integrator.cpp:173-183,276-294 + Sampler::set_samples_per_wavefront, sampler.cpp:88-96 */
int pass_layout(const HarIntegratorImpl *I, uint32_t crop_w, uint32_t crop_h, uint32_t spp, uint32_t &spp_per_pass, uint32_t &n_passes) {
    if (spp == 0) return fail("spp must be > 0");
    spp_per_pass = I->set.samples_per_pass == 0xffffffffu ? spp : std::min(I->set.samples_per_pass, spp);
    if (spp_per_pass == 0 || spp % spp_per_pass != 0) return fail("sample_count (" + std::to_string(spp) + ") must be a multiple of spp_per_pass (" + std::to_string(spp_per_pass) + ").");
    n_passes = spp / spp_per_pass;
    const uint64_t limit = 0xffffffffull;
    uint64_t wavefront = (uint64_t) crop_w * crop_h * spp_per_pass;
    if (wavefront > limit) {
        spp_per_pass /= (uint32_t) ((wavefront + limit - 1) / limit);
        if (spp_per_pass == 0) return fail("the film alone exceeds the wavefront size limit of 2^32 - 1 lanes");
        n_passes = spp / spp_per_pass;
        /* the reference then calls sampler->set_samples_per_wavefront(spp_per_pass), which throws unless it divides the sample count */
        if (spp % spp_per_pass != 0) return fail("sample_count should be a multiple of samples_per_wavefront! (" + std::to_string(spp) + " samples in passes of " + std::to_string(spp_per_pass) + "; set samples_per_pass)");
    }
    return 0;
}

int check_common(HarSceneImpl *S, HarIntegratorImpl *I, const HarSensor *sensor, uint32_t spp, uint64_t &lb, uint64_t &le, DSensor &C, uint32_t &log_spp) {
    if (!S || !I || !sensor) return fail("null scene / integrator / sensor");
    std::string e;
    if (!lower_sensor(*sensor, C, e)) return fail(e);
    if (C.rfilter != 0 && 2 * (uint32_t) ceilf(C.radius - .5f) + 1 > HAR_MAX_FILTER_TAPS) return fail("reconstruction filter radius too large (max 9 taps)");
    if (spp == 0) return fail("spp must be > 0");
    if (I->set.batch.n) {        /* batch.cpp:114-119; a crop window / sample border on the batch film is refused (the reference would divide the crop window between the children) */
        if (C.crop_x || C.crop_y || C.crop_w != sensor->film_width || C.crop_h != sensor->film_height || C.border)
            return fail("batch sensor: a crop window or sample_border on the batch film is not implemented by hip_ad_rgb");
        if (C.crop_w % I->set.batch.n) return fail("BatchSensor: the horizontal resolution (currently " + std::to_string(C.crop_w) + ") must be divisible by the number of child sensors (" + std::to_string(I->set.batch.n) + ")!");
    }
    uint64_t total = (uint64_t) C.samp_w * C.samp_h * spp;
    /* 2^32 wavefront limit of JIT variants (integrator.cpp:276-294, common.py:358-363) */
    if (total > 0xffffffffull) return fail("the rendering task exceeds 2^32 - 1 Monte Carlo samples; render in several passes");
    if (lb == 0 && le == 0) le = total;
    if (lb > le || le > total) return fail("invalid lane range");
    log_spp = log2_exact(spp);
    return 0;
}

} // namespace

extern "C" {

int har_integrator_create(int type, int32_t max_depth, int32_t rr_depth, uint32_t chunk_lanes, HarIntegrator *out) {
    if (!out) return fail("null argument");
    if (type != HAR_INTEGRATOR_PATH && type != HAR_INTEGRATOR_PRB) return fail("unknown integrator type");
    /* MonteCarloIntegrator ctor, src/render/integrator.cpp:539-550 */
    if (max_depth < 0 && max_depth != -1) return fail("\"max_depth\" must be set to -1 (infinite) or a value >= 0");
    if (rr_depth <= 0) return fail("\"rr_depth\" must be set to a value greater than zero!");
    HarIntegratorImpl *I = new HarIntegratorImpl();
    I->set.type = type; I->set.max_depth = (uint32_t) max_depth; I->set.rr_depth = (uint32_t) rr_depth;
    if (chunk_lanes) I->set.chunk = std::max<uint32_t>(2048u, (chunk_lanes + 2047u) / 2048u * 2048u);
    if (const char *e = getenv("HAR_TOP_SEED")) I->set.top_seed_env = atoi(e) != 0 ? 1 : 0;      /* per integrator, not cached: one process can hold both kinds */
    *out = I;
    return 0;
}
int har_integrator_destroy(HarIntegrator I) {
    if (!I) return 0;
    (void) hipDeviceSynchronize();
    I->free_ws();
    if (I->aov.status || I->aov.h0 || I->aov.val) {
        (void) hipDeviceSynchronize();
        dev_free(I->aov.h0, true); dev_free(I->aov.h1, true); dev_free(I->aov.val, true); dev_free(I->aov.status, true);
    }
    if (I->batch_cams || I->aov_rays) { (void) hipDeviceSynchronize(); dev_free(I->batch_cams, true); dev_free(I->aov_rays, true); }
    prof_destroy(I);
    if (I->twin) { I->twin->free_ws(); prof_destroy(I->twin); }
    if (I->ev_fork) (void) hipEventDestroy(I->ev_fork);
    if (I->ev_join) (void) hipEventDestroy(I->ev_join);
    if (I->ev_stagger) (void) hipEventDestroy(I->ev_stagger);
    if (I->side_stream) (void) hipStreamDestroy(I->side_stream);
    for (HarIntegratorImpl *J : { I->twin, I })
        if (J) {
            if (J->ptr_ring) (void) hipHostFree(J->ptr_ring);
            for (int k = 0; k < 8; ++k) if (J->ptr_ring_ev[k]) (void) hipEventDestroy(J->ptr_ring_ev[k]);
            if (J->ev_shaded) (void) hipEventDestroy(J->ev_shaded);
            if (J->ev_resolved) (void) hipEventDestroy(J->ev_resolved);
            if (J->ev_resolved2) (void) hipEventDestroy(J->ev_resolved2);
            if (J->aux_stream) (void) hipStreamDestroy(J->aux_stream);
        }
    if (I->twin) delete I->twin;
    delete I;
    return 0;
}

static int render_range(HarScene S, HarIntegrator I, const HarSensor *sensor, uint32_t seed, uint32_t spp, uint64_t lb, uint64_t le, float *film, void *stream) {
    DSensor C; uint32_t log_spp;
    if (!S || !I || !sensor) return fail("null scene / integrator / sensor");
    /* multi-pass layout; `path` only: the Python AD integrators render one wavefront or refuse (common.py:358-363) */
    uint32_t spp_pass = spp, n_passes = 1, grid_w = 0, grid_h = 0;
    if (sample_grid(sensor, grid_w, grid_h)) return 1;
    if (I->set.type == HAR_INTEGRATOR_PATH && pass_layout(I, grid_w, grid_h, spp, spp_pass, n_passes)) return 1;
    if (check_common(S, I, sensor, spp_pass, lb, le, C, log_spp)) return 1;
    if (!film) return fail("null film");
    hipStream_t s = (hipStream_t) stream;
    uint32_t chunk = (uint32_t) std::min<uint64_t>(I->set.chunk, (std::max<uint64_t>(le - lb, 2048) + 2047) / 2048 * 2048);
    if (ensure_workspace(I, chunk, false)) return 1;
    const bool multi = n_passes > 1;
    if (multi) {
        if (I->pass_rng_cap < le - lb && I->set.max_depth != 0) { if (ws_alloc(I, &I->pass_rng, (size_t) (le - lb))) return 1; I->pass_rng_cap = (size_t) (le - lb); }
        if (I->pass_jitter_cap < chunk) { if (ws_alloc(I, &I->pass_jitter, chunk)) return 1; I->pass_jitter_cap = chunk; }
    }
    HIP_TRY(hipMemsetAsync(I->totals, 0, 4 * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(I->status, 0, sizeof(int), s));
    I->last_stream = s;
    if (prof_begin(I, s)) return 1;
    const int mode = I->set.type == HAR_INTEGRATOR_PATH ? MODE_PATH : MODE_PRB_PRIMAL;
    for (uint32_t pass = 0; pass < n_passes; ++pass) {
        if (I->set.max_depth == 0) {      /* path.cpp:102-103: nothing but the weight channel */
            for (uint64_t base = lb; base < le; base += chunk) {
                uint32_t n = (uint32_t) std::min<uint64_t>(chunk, le - base);
                if (multi) launch_pass_jitter(s, seed, (uint32_t) base, n, pass, I->pass_jitter);
                launch_splat(s, C, seed, spp_pass, log_spp, (uint32_t) base, n, nullptr, 1, film, multi ? I->pass_jitter : nullptr);
            }
            continue;
        }
        for (uint64_t base = lb; base < le; base += chunk) {
            uint32_t n = (uint32_t) std::min<uint64_t>(chunk, le - base);
            const PassState ps{ multi ? I->pass_rng + (base - lb) : nullptr, multi ? I->pass_jitter : nullptr, pass };
            if (run_chunk(S, I, C, mode, seed, spp_pass, log_spp, (uint32_t) base, n, nullptr, s, CACHE_NONE, ps)) return 1;
            if (mode == MODE_PRB_PRIMAL) { launch_accumulate_stats(s, I->counters, bounce_limit(I), I->totals, n); prof_mark(I, s, CLS_OTHER); }
            launch_splat(s, C, seed, spp_pass, log_spp, (uint32_t) base, n, I->result, 0, film, ps.jitter);
            if (I->set.alpha_film && I->alpha_lane) launch_splat(s, C, seed, spp_pass, log_spp, (uint32_t) base, n, nullptr, 1, I->set.alpha_film, ps.jitter, I->alpha_lane);
            prof_mark(I, s, CLS_SPLAT);
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* The table of texture gradient (tangent) buffers is a HOST array of the caller that only lives for the call, while the kernels read it from the device.  It is
 * staged through a ring of eight PINNED slots, so that the copy is asynchronous and the call returns without waiting for the stream (round 4 synchronised the
 * stream here, once per optimisation step: the GPU then idled while the host enqueued the whole adjoint pass).  A slot is reused only after the copy that read it
 * has run (its event); the device table itself is rewritten in stream order. */
static int upload_pointer_table(HarIntegratorImpl *I, const void *const *host, size_t n, hipStream_t s) {
    if (I->ptr_ring_cap < n) {
        (void) hipDeviceSynchronize();
        if (I->ptr_ring) (void) hipHostFree(I->ptr_ring);
        I->ptr_ring = nullptr; I->ptr_ring_cap = 0;
        HIP_TRY(hipHostMalloc((void **) &I->ptr_ring, 8 * n * sizeof(void *), hipHostMallocDefault));
        I->ptr_ring_cap = n;
        for (int k = 0; k < 8; ++k) { if (!I->ptr_ring_ev[k]) HIP_TRY(hipEventCreateWithFlags(&I->ptr_ring_ev[k], hipEventDisableTiming)); I->ptr_ring_used[k] = false; }
    }
    const uint32_t k = I->ptr_ring_next; I->ptr_ring_next = (k + 1u) & 7u;
    if (I->ptr_ring_used[k]) HIP_TRY(hipEventSynchronize(I->ptr_ring_ev[k]));
    void **slot = I->ptr_ring + (size_t) k * I->ptr_ring_cap;
    std::memcpy(slot, host, n * sizeof(void *));
    HIP_TRY(hipMemcpyAsync(I->d_grad_tex, slot, n * sizeof(void *), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(I->ptr_ring_ev[k], s)); I->ptr_ring_used[k] = true;
    return 0;
}

static int backward_range(HarScene S, HarIntegrator I, const HarSensor *sensor, const float *grad_in, const float *weight_film, uint32_t seed,
                          uint32_t spp, uint64_t lb, uint64_t le, float *grad_reflectance, float *const *grad_textures, void *stream);

/* two-stream driver (see HarIntegratorImpl::twin): returns the split point, or `le` when the job runs on one stream */
static uint64_t dual_split(HarIntegrator I, uint64_t lb, uint64_t le, hipStream_t s) {
    /* measured on MI355X (1M-triangle scene): 2 M lanes 5.84 -> 5.40 ms, 8 M 13.6 -> 13.0, 16 M 24.0 -> 23.5, 32 M +-0, 67 M 85.4 -> 86.5 ms: the two
     * launch sequences run in lock-step, so only part of the tails is hidden -- worth it for the small jobs a rank sees when N GPUs share a
     * frame, not for a single large wavefront.  HAR_STREAMS = 1 / 2 forces one / two streams. */
    const int forced = switches().streams;
    I->twin_used = false;
    if (forced == 1 || le - lb < HAR_DUAL_MIN_LANES || (forced != 2 && le - lb > HAR_DUAL_MAX_LANES)) return le;
    if (!I->twin) {
        if (hipStreamCreateWithFlags(&I->side_stream, hipStreamNonBlocking) != hipSuccess) return le;
        if (hipEventCreateWithFlags(&I->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&I->ev_join, hipEventDisableTiming) != hipSuccess) return le;
        I->twin = new HarIntegratorImpl();
    }
    HarIntegratorImpl *T = I->twin;
    if (T->set.use_cache != I->set.use_cache) { (void) hipDeviceSynchronize(); T->free_ws(); }      /* the replay cache is part of the workspace */
    T->set = I->set;
    if (hipEventRecord(I->ev_fork, s) != hipSuccess || hipStreamWaitEvent(I->side_stream, I->ev_fork, 0) != hipSuccess) return le;
    I->twin_used = true;
    /* HAR_DUAL_FRAC (percent, default 50): the share of the first half -- an uneven cut de-synchronises the two launch sequences (A/B) */
    const uint64_t frac = switches().dual_frac;
    return lb + ((le - lb) * frac / 100 + 2047) / 2048 * 2048;
}
static int dual_join(HarIntegrator I, hipStream_t s) {
    HIP_TRY(hipEventRecord(I->ev_join, I->side_stream));
    HIP_TRY(hipStreamWaitEvent(s, I->ev_join, 0));
    return 0;
}

/* film window (har_integrator_set_film_window): the rows the lanes [lb, le) can splat into -- their pixel rows in the sample grid, moved by the sample border, widened by
 * the reconstruction filter's footprint (film_footprint, har_path.h) -- must lie inside the window; the kernels then get the address row 0 WOULD have */
static int apply_film_window(HarIntegrator I, const HarSensor *sensor, uint32_t spp, uint64_t lb, uint64_t le, float *&film, uint32_t channels = 4) {
    if (!I->film_rows) return 0;
    DSensor C; std::string e;
    if (!lower_sensor(*sensor, C, e)) return fail(e);
    uint32_t spp_pass = spp, n_passes = 1;
    if (I->set.type == HAR_INTEGRATOR_PATH && pass_layout(I, C.samp_w, C.samp_h, spp, spp_pass, n_passes)) return 1;
    const uint64_t per_row = (uint64_t) C.samp_w * spp_pass;
    if (lb == 0 && le == 0) le = per_row * C.samp_h;
    if (le <= lb || per_row == 0) return 0;
    const int64_t taps = C.rfilter == 0 ? 0 : (int64_t) ceilf(C.radius - .5f);
    int64_t y0 = (int64_t) (lb / per_row) - (int64_t) C.border - taps, y1 = (int64_t) ((le - 1) / per_row) - (int64_t) C.border + taps;
    y0 = std::max<int64_t>(y0, 0); y1 = std::min<int64_t>(y1, (int64_t) C.crop_h - 1);
    if (y0 <= y1 && (y0 < (int64_t) I->film_row0 || y1 >= (int64_t) I->film_row0 + I->film_rows))
        return fail("har_integrator_set_film_window: the lanes splat into film rows [" + std::to_string(y0) + ", " + std::to_string(y1) + "], the window holds [" +
                    std::to_string(I->film_row0) + ", " + std::to_string(I->film_row0 + I->film_rows - 1) + "]");
    film -= (size_t) I->film_row0 * C.crop_w * channels;
    return 0;
}

int har_integrator_set_film_window(HarIntegrator I, uint32_t row_begin, uint32_t row_count) {
    if (!I) return fail("null integrator");
    I->film_row0 = row_count ? row_begin : 0; I->film_rows = row_count;
    return 0;
}

int har_render(HarScene S, HarIntegrator I, const HarSensor *sensor, uint32_t seed, uint32_t spp, uint64_t lb, uint64_t le, float *film, void *stream) {
    if (!S || !I || !sensor) return fail("null scene / integrator / sensor");
    if (!film) return fail("null film");
    float *const alpha_saved = I->set.alpha_film;
    if (I->film_rows) {
        if (apply_film_window(I, sensor, spp, lb, le, film)) return 1;
        if (I->set.alpha_film) { float *a = I->set.alpha_film; if (apply_film_window(I, sensor, spp, lb, le, a)) return 1; I->set.alpha_film = a; }
    }
    struct Restore { HarIntegrator I; float *a; ~Restore() { I->set.alpha_film = a; } } restore{ I, alpha_saved };
    uint64_t total_lb = lb, total_le = le;
    if (lb == 0 && le == 0) {                           /* "all lanes": resolve the range here so that it can be cut */
        uint32_t spp_pass = spp, n_passes = 1, grid_w = 0, grid_h = 0;
        if (sample_grid(sensor, grid_w, grid_h)) return 1;
        if (I->set.type == HAR_INTEGRATOR_PATH && pass_layout(I, grid_w, grid_h, spp, spp_pass, n_passes)) return 1;
        total_le = (uint64_t) grid_w * grid_h * spp_pass;
        if (total_le == 0 || total_le > 0xffffffffull) return render_range(S, I, sensor, seed, spp, lb, le, film, stream);      /* reports the error */
    }
    /* jobs small enough for the shadow-ray overlap run on one stream: that beats two half-jobs with or without overlap (overlap_applies) */
    const int streams_env = switches().streams;
    const bool single = streams_env != 2 && overlap_applies(S, I, std::min<uint64_t>(total_le - total_lb, I->set.chunk));
    const uint64_t mid = (total_le > total_lb && !single) ? dual_split(I, total_lb, total_le, (hipStream_t) stream) : total_le;
    if (mid >= total_le) { I->twin_used = false; return render_range(S, I, sensor, seed, spp, lb, le, film, stream); }
    /* HAR_DUAL_STAGGER=1 (A/B): the second half starts behind the first half's first closest-hit launch, so that one half's memory-bound shading launches
     * run next to the other half's issue-bound traversal launches instead of next to their own kind */
    const bool stagger_env = switches().dual_stagger;
    if (stagger_env && !I->ev_stagger && hipEventCreateWithFlags(&I->ev_stagger, hipEventDisableTiming) != hipSuccess) I->ev_stagger = nullptr;
    I->stagger_record = stagger_env && I->ev_stagger;
    int rc = render_range(S, I, sensor, seed, spp, total_lb, mid, film, stream);
    if (stagger_env && I->ev_stagger && !I->stagger_record) (void) hipStreamWaitEvent(I->side_stream, I->ev_stagger, 0);
    I->stagger_record = false;
    rc |= render_range(S, I->twin, sensor, seed, spp, mid, total_le, film, (void *) I->side_stream);
    rc |= dual_join(I, (hipStream_t) stream);
    return rc;
}

int har_render_backward(HarScene S, HarIntegrator I, const HarSensor *sensor, const float *grad_in, const float *weight_film, uint32_t seed,
                        uint32_t spp, uint64_t lb, uint64_t le, float *grad_reflectance, float *const *grad_textures, void *stream) {
    if (!S || !I || !sensor) return fail("null scene / integrator / sensor");
    uint64_t total_lb = lb, total_le = le;
    if (lb == 0 && le == 0) {
        uint32_t grid_w = 0, grid_h = 0;
        if (sample_grid(sensor, grid_w, grid_h)) return 1;
        total_le = (uint64_t) grid_w * grid_h * spp;
        if (total_le == 0 || total_le > 0xffffffffull) return backward_range(S, I, sensor, grad_in, weight_film, seed, spp, lb, le, grad_reflectance, grad_textures, stream);
    }
    /* as in har_render: one stream when the primal pass overlaps its shadow rays (PRB bands of 8 / 16 / 33 M lanes: 16.46 / 30.19 / 54.32 ms against 17.01 / 30.90 /
     * 55.34 ms on two streams, profiles/r03_ab_shadow_overlap.txt) */
    const int streams_env = switches().streams;
    const bool single = streams_env != 2 && overlap_applies(S, I, std::min<uint64_t>(total_le - total_lb, I->set.chunk));
    const uint64_t mid = (total_le > total_lb && I->set.type == HAR_INTEGRATOR_PRB && !I->shape_on && !single) ? dual_split(I, total_lb, total_le, (hipStream_t) stream) : total_le;
    if (mid >= total_le) I->twin_used = false;
    if (mid >= total_le) return backward_range(S, I, sensor, grad_in, weight_film, seed, spp, lb, le, grad_reflectance, grad_textures, stream);
    int rc = backward_range(S, I, sensor, grad_in, weight_film, seed, spp, total_lb, mid, grad_reflectance, grad_textures, stream);
    rc |= backward_range(S, I->twin, sensor, grad_in, weight_film, seed, spp, mid, total_le, grad_reflectance, grad_textures, (void *) I->side_stream);
    rc |= dual_join(I, (hipStream_t) stream);
    return rc;
}

int har_integrator_sample(HarScene S, HarIntegrator I, uint32_t seed, uint32_t lane_offset, uint32_t n, const float *o, const float *d, const float *maxt,
                          const uint64_t *state, const uint8_t *active, float *rgb, uint8_t *valid, uint64_t *state_out, void *stream) {
    if (!S || !I) return fail("null scene / integrator");
    if (n == 0) return 0;
    if (!o || !d || !maxt || !rgb) return fail("null ray / output arrays");
    if ((uint64_t) lane_offset + n > 0xffffffffull) return fail("lane_offset + n exceeds the 2^32 - 1 lanes of a wavefront");
    if (state_out && I->set.type != HAR_INTEGRATOR_PATH) return fail("state_out: only `path` reports the sampler state after sample()");
    hipStream_t s = (hipStream_t) stream;
    const uint32_t chunk = (uint32_t) std::min<uint64_t>(I->set.chunk, ((uint64_t) std::max<uint32_t>(n, 2048) + 2047) / 2048 * 2048);
    if (ensure_workspace(I, chunk, false)) return 1;
    if (!I->alpha_lane && ws_alloc(I, &I->alpha_lane, I->ws_lanes)) return 1;      /* the samples' masks use the per-lane alpha array of `rgba` films */
    HIP_TRY(hipMemsetAsync(I->totals, 0, 4 * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(I->status, 0, sizeof(int), s));
    I->last_stream = s; I->twin_used = false;
    if (prof_begin(I, s)) return 1;
    const int mode = I->set.type == HAR_INTEGRATOR_PATH ? MODE_PATH : MODE_PRB_PRIMAL;
    const DSensor C{};                                     /* no sensor on this entry point */
    for (uint64_t base = 0; base < n; base += chunk) {
        const uint32_t m = (uint32_t) std::min<uint64_t>(chunk, n - base);
        const RaySource rays{ o, d, maxt, state, active, n, (uint32_t) base };
        if (I->set.max_depth == 0) {                           /* path.cpp:102-103 / prb.py: no interaction at all */
            HIP_TRY(hipMemsetAsync(I->result, 0, (size_t) m * sizeof(float4), s));
            HIP_TRY(hipMemsetAsync(I->alpha_lane, 0, (size_t) m * sizeof(float), s));
            if (state_out) { if (!state) return fail("state_out with max_depth = 0 needs `state` (the sampler is not touched, path.cpp:102-103)"); HIP_TRY(hipMemcpyAsync(state_out + base, state + base, (size_t) m * sizeof(uint64_t), hipMemcpyDeviceToDevice, s)); }
        } else {
            /* the lanes' final sampler states come back through the multi-pass mechanism (PassState::rng is indexed by lane - lane_base) */
            const PassState ps{ state_out ? state_out + base : nullptr, nullptr, 1u };
            if (run_chunk(S, I, C, mode, seed, 1, 0, lane_offset + (uint32_t) base, m, nullptr, s, CACHE_NONE, ps, &rays, I->alpha_lane)) return 1;
            if (mode == MODE_PRB_PRIMAL) launch_accumulate_stats(s, I->counters, bounce_limit(I), I->totals, m);
        }
        launch_sample_out(s, m, n, (uint32_t) base, I->result, I->alpha_lane, mode == MODE_PATH ? 1 : 0, rgb, valid, active, seed, lane_offset + (uint32_t) base, state, state_out);
        prof_mark(I, s, CLS_OTHER);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int har_sampler_clone(uint32_t n, const uint64_t *state, const uint64_t *inc, uint64_t *state_dst, uint64_t *inc_dst, void *stream) {
    if (n == 0) return 0;
    if (!state || !inc || !state_dst || !inc_dst) return fail("null sampler state");
    HIP_TRY(hipMemcpyAsync(state_dst, state, (size_t) n * sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    HIP_TRY(hipMemcpyAsync(inc_dst, inc, (size_t) n * sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return 0;
}
int har_sampler_advance(uint32_t n, uint64_t *state, const uint64_t *inc, void *stream) {
    /* IndependentSampler::advance (src/samplers/independent.cpp:69-72 -> Sampler::advance, src/render/sampler.cpp:69-72) moves the sample index and
     * resets the dimension index; the PCG32 streams are untouched (no reseed), so the device state does not change */
    (void) n; (void) state; (void) inc; (void) stream;
    return 0;
}

int har_integrator_set_alpha_film(HarIntegrator I, float *alpha_film) {
    if (!I) return fail("null integrator");
    I->set.alpha_film = alpha_film;          /* the per-lane alpha values are allocated with the next render's workspace and kept */
    return 0;
}
int har_integrator_set_hide_emitters(HarIntegrator I, int hide) {
    if (!I) return fail("null integrator");
    I->set.hide_emitters = hide != 0;
    return 0;
}
int har_integrator_set_samples_per_pass(HarIntegrator I, uint32_t samples_per_pass) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PATH) return fail("samples_per_pass is a property of SamplingIntegrator (`path`); the AD integrators render a single wavefront");
    I->set.samples_per_pass = samples_per_pass ? samples_per_pass : 0xffffffffu;
    return 0;
}
int har_render_pass_layout(HarIntegrator I, const HarSensor *sensor, uint32_t spp, uint32_t *spp_per_pass, uint32_t *n_passes) {
    if (!I || !sensor || !spp_per_pass || !n_passes) return fail("null argument");
    *spp_per_pass = spp; *n_passes = 1;
    if (I->set.type != HAR_INTEGRATOR_PATH) return spp ? 0 : fail("spp must be > 0");
    uint32_t grid_w = 0, grid_h = 0;
    if (sample_grid(sensor, grid_w, grid_h)) return 1;
    return pass_layout(I, grid_w, grid_h, spp, *spp_per_pass, *n_passes);
}

int har_render_weights(const HarSensor *sensor, uint32_t seed, uint32_t spp, uint64_t lb, uint64_t le, float *film, void *stream) {
    if (!sensor || !film) return fail("null sensor / film");
    DSensor C; std::string e;
    if (!lower_sensor(*sensor, C, e)) return fail(e);
    uint64_t total = (uint64_t) C.samp_w * C.samp_h * spp;
    if (spp == 0 || total > 0xffffffffull) return fail("invalid sample count");
    if (lb == 0 && le == 0) le = total;
    if (lb > le || le > total) return fail("invalid lane range");
    uint32_t log_spp = log2_exact(spp);
    const uint64_t chunk = 1u << 24;
    for (uint64_t base = lb; base < le; base += chunk) {
        uint32_t n = (uint32_t) std::min<uint64_t>(chunk, le - base);
        launch_splat((hipStream_t) stream, C, seed, spp, log_spp, (uint32_t) base, n, nullptr, 1, film);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

static int backward_range(HarScene S, HarIntegrator I, const HarSensor *sensor, const float *grad_in, const float *weight_film, uint32_t seed,
                          uint32_t spp, uint64_t lb, uint64_t le, float *grad_reflectance, float *const *grad_textures, void *stream) {
    DSensor C; uint32_t log_spp;
    if (check_common(S, I, sensor, spp, lb, le, C, log_spp)) return 1;
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("render_backward is implemented by the `prb` integrator");
    if (!grad_in || !weight_film || !grad_reflectance) return fail("null gradient buffers");
    if (I->set.max_depth == 0) return 0;
    hipStream_t s = (hipStream_t) stream;
    uint32_t chunk = (uint32_t) std::min<uint64_t>(I->set.chunk, (std::max<uint64_t>(le - lb, 2048) + 2047) / 2048 * 2048);
    /* replay TAPE instead of the lane-indexed replay cache (TapeArrays, har_kernels.h) whenever the adjoint commits in place: the default.  Not with
     * vertex-position / instance gradients (their adjoint goes through items), hide_emitters (its device round trip re-traces into the ping-pong
     * buffers), the replay cache switched off, or more bounces than the tape holds.  HAR_PRB_TAPE=0: the round-2 cache (A/B). */
    const Switches &W = switches();
    const bool tape_env = W.prb_tape != 0;
    /* ... and the RECORD tape (primal pass writes one adjoint record per vertex, the adjoint pass is a streaming commit) unless alpha / eta / k gradients are
     * asked for (their fifteen extra vectors per vertex stay with the re-shading replay).  HAR_PRB_TAPE=1: the state tape (A/B) */
    const int tape_kind_env = W.prb_tape;
    const bool tape_ok = tape_env && W.adjoint_inline && I->set.use_cache && !I->shape_on && !I->set.hide_emitters && bounce_limit(I) <= HAR_REPLAY_CACHE_BOUNCES;
    /* what an earlier out-of-memory step-down settled on applies to THAT job (scene, film, lane count): another job starts from the full configuration again, and the
     * same job retries it every 16th call -- the failure may have been a transient state of the allocator pool the library shares with the caller's tensors */
    const uint64_t job_key = S->serial * 0x9e3779b97f4a7c15ull ^ ((uint64_t) C.crop_w << 40) ^ ((uint64_t) C.crop_h << 20) ^ (le - lb);
    if (I->bw_job_key != job_key || (++I->bw_calls_since_stepdown & 15u) == 0u) { I->bw_tape_max = 2; I->bw_chunk_max = 0xffffffffu; I->bw_job_key = job_key; }
    chunk = std::min(chunk, I->bw_chunk_max);
    /* texels of a light's bitmap radiance: committed in place by the re-shading replay as well (the record tape holds neither the sampled uv nor the unit weight) */
    const bool light_texels = I->set.grad_light_texels && (S->ds.bsdf_types & HAR_SCENE_TEXLIGHT) != 0u;
    /* a `blendbsdf` record: the nested records' gradients are deposited by the in-place commit of the re-shading replay (the record tape holds one record per vertex) */
    /* ... and a `mesh_attribute` texture: the transpose of its lookup needs the hit (face, barycentrics), which only the in-place commit has at hand */
    /* ... and a `normalmap` record: the normal map's gradient and the nested colours' are deposited by the in-place commit as well */
    const bool blend = (S->ds.bsdf_types & HAR_SCENE_WIDE_ROUTE) != 0u;
    const bool attr_only = (S->ds.bsdf_types & HAR_SCENE_WIDE_ROUTE) == HAR_SCENE_ATTR;
    const bool nmap = (S->ds.bsdf_types & HAR_SCENE_NORMALMAP) != 0u;
    const bool bump = (S->ds.bsdf_types & HAR_SCENE_BUMPMAP) != 0u;          /* ... and a `bumpmap` record: the height map's gradient and the nested colours' likewise */
    const bool amap = (S->ds.bsdf_types & HAR_SCENE_ALPHAMAP) != 0u;          /* ... and a roughness map: groups 0 / 1 of a textured record go into the map's texels, by the in-place commit too */
    const bool amap_only = amap && (S->ds.bsdf_types & HAR_SCENE_WIDE_ROUTE) == HAR_SCENE_ALPHAMAP;      /* ... without a composite record: the one wide-route scene whose alpha / eta / k gradients exist */
    const bool thin = (S->ds.bsdf_types & HAR_SCENE_THIN) != 0u;          /* ... and a `thindielectric` record: the pane has no gradient of its own; everything else in the scene takes the in-place commit of its set */
    const bool thin_only = thin && (S->ds.bsdf_types & HAR_SCENE_WIDE_ROUTE) == HAR_SCENE_THIN;      /* ... among plain models: the lean set, whose commit has the alpha / eta / k / slot-1 terms */
    const char *const comp = thin ? "thindielectric" : amap_only ? "roughness map" : bump ? "bumpmap" : nmap ? "normalmap" : attr_only ? "mesh_attribute" : (S->ds.bsdf_types & HAR_SCENE_MASK) ? "mask" : "blendbsdf";      /* (the refusals below are scene-wide: one such record anywhere in the scene) */
    /* ... and the texels of the environment map (har_integrator_set_grad_envmap): the same two terms, the same route */
    const bool env_texels = I->set.grad_envmap && S->hs.has_envmap;
    int tape = !tape_ok ? 0 : (tape_kind_env >= 2 && !I->set.grad_bsdf_params && !light_texels && !env_texels && !blend && !(S->ds.bsdf_types & HAR_SCENE_PROJECTOR) /* (the record tape does not carry ds.uv: a projector scene takes the state tape) */ && chunk <= (1u << 29)) ? 2 : 1;
    tape = std::min(tape, I->bw_tape_max);
    /* The tapes are the large workspaces (record tape 69 B, state tape 115 B per lane and bounce against 25 B for the lane-indexed cache: 28 - 90 GB for a 2^26-lane chunk
     * at max_depth 6 - 12).  When the device -- or the host's allocator pool, shared with the caller's tensors -- cannot hold one, step down instead of failing: record
     * tape -> lane-indexed replay cache (same gradients, more traffic), then halve the chunk (more launch tails) down to 2^20 lanes. */
    const size_t npx = (size_t) C.crop_w * C.crop_h, nt = S->hs.textures.size();
    /* the kernels accumulate into (bsdf_count + emitter_count) x 3 slots; the two halves are added to the caller's buffers at the end */
    const size_t nb3 = 3 * S->hs.bsdfs.size(), ne3 = 3 * S->hs.emitters.size();
    /* everything render_backward allocates, so that the step-down below sees every refusal (the texel queues are sized by the workspace's lanes) */
    auto allocate = [&]() -> int {
        if (ensure_workspace(I, chunk, true, tape)) return 1;
        if (I->adj_floats < 3 * npx) { if (ws_alloc(I, &I->adj, 3 * npx)) return 1; I->adj_floats = 3 * npx; }
        if (I->grad_tex_cap < std::max<size_t>(nt, 1)) { if (ws_alloc(I, &I->d_grad_tex, std::max<size_t>(nt, 1))) return 1; I->grad_tex_cap = std::max<size_t>(nt, 1); }
        if (ensure_texel_queues(S, I)) return 1;
        if (I->grad_slots_cap < nb3 + ne3 + 3) { if (ws_alloc(I, &I->grad_slots, nb3 + ne3 + 3)) return 1; I->grad_slots_cap = nb3 + ne3 + 3; }
        return 0;
    };
    for (;;) {
        g_alloc_failed = false;
        if (allocate() == 0) break;
        const std::string why = har_error_text();
        if (!g_alloc_failed) return 1;                                         /* not an allocation failure: the error stands */
        I->bw_calls_since_stepdown = 0;
        (void) hipDeviceSynchronize(); I->free_ws(); (void) hipGetLastError();
        if (tape != 0) { tape = 0; I->bw_tape_max = 0; }
        else if (chunk > (1u << 20)) { chunk = std::max<uint32_t>(1u << 20, (chunk / 2 + 2047) / 2048 * 2048); I->bw_chunk_max = chunk; }
        else return fail("render_backward: no workspace fits the device (" + why + ")");
        if (W.verbose) fprintf(stderr, "[hip_ad_rgb] render_backward: %s -- retrying with tape %d, chunk %u lanes\n", why.c_str(), tape, chunk);
    }
    if (nt) {
        if (!grad_textures) return fail("grad_textures is null but the scene has bitmap textures");
        for (size_t k = 0; k < nt; ++k) if (!grad_textures[k]) return fail("null texture gradient buffer");
        if (upload_pointer_table(I, (const void *const *) grad_textures, nt, s)) return 1;
    }
    if (light_texels) {
        if (!I->set.use_cache || I->shape_on) return fail("gradients of a light's texels need the replay cache and cannot be combined with vertex-position gradients");
        if (bounce_limit(I) > HAR_REPLAY_CACHE_BOUNCES) return fail("gradients of a light's texels: max_depth must not exceed " + std::to_string(HAR_REPLAY_CACHE_BOUNCES) + " (the cached bounces)");
        if (!W.adjoint_inline) return fail("gradients of a light's texels need the in-place commit (HAR_ADJOINT_INLINE=0 is set)");
    }
    if (env_texels) {
        if (!I->set.use_cache || I->shape_on) return fail("envmap gradients need the replay cache and cannot be combined with vertex-position gradients");
        if (bounce_limit(I) > HAR_REPLAY_CACHE_BOUNCES) return fail("envmap gradients: max_depth must not exceed " + std::to_string(HAR_REPLAY_CACHE_BOUNCES) + " (the cached bounces)");
        if (!W.adjoint_inline) return fail("envmap gradients need the in-place commit (HAR_ADJOINT_INLINE=0 is set)");
        /* the deposit addresses the REAL texels of the map, H x W: an image the constructor padded (to at least 2 x 3, envmap.cpp:125-131) has a smaller gradient buffer */
        const HostTexture &T = S->hs.textures[S->hs.envmap.tex_index];
        if (T.w != S->hs.envmap.w || T.h != S->hs.envmap.h) return fail("envmap gradients: an environment map smaller than 2 x 3 texels (padded by the emitter) is not differentiated");
    }
    if (blend) {
        if (I->set.grad_bsdf_params && attr_only) return fail("mesh_attribute: gradients of alpha / eta / k / specular colours are not produced for scenes with a `mesh_attribute` texture (the attributes' are)");
        if (I->set.grad_bsdf_params && amap && !amap_only)
            return fail(std::string("roughness map: alpha texel gradients (and alpha / eta / k / specular colours) are not produced for a scene that also holds a `") + comp + "` record: a roughconductor nested in a blendbsdf / mask / normalmap / bumpmap keeps its forward render only");
        if (I->set.grad_bsdf_params && !amap_only && !thin_only) return fail(std::string(comp) + ": gradients of alpha / eta / k / specular colours are not produced for scenes with a " + (thin ? "thindielectric record next to a blendbsdf / mask / normalmap / bumpmap record or a roughness map (colour slot 0 of the other BSDFs, texels and emitter radiances are)" : bump ? "bumpmap record (the height map and the nested BSDF's colour slot 0 are)" : nmap ? "normalmap record (the normal map and the nested BSDF's colour slot 0 are)" : (S->ds.bsdf_types & HAR_SCENE_MASK) ? "mask record (the opacity and the nested BSDF's colour slot 0 are)" : "blend record (the weight and the nested BSDFs' colour slot 0 are)"));
        if (!I->set.use_cache || I->shape_on) return fail(std::string(comp) + ": gradients need the replay cache and cannot be combined with vertex-position gradients");
        if (bounce_limit(I) > HAR_REPLAY_CACHE_BOUNCES) return fail(std::string(comp) + ": gradients of a scene with a " + (thin ? "thindielectric" : amap_only ? "roughness-map" : bump ? "bumpmap" : nmap ? "normalmap" : attr_only ? "mesh_attribute texture" : (S->ds.bsdf_types & HAR_SCENE_MASK) ? "mask" : "blend") + " record: max_depth must not exceed " + std::to_string(HAR_REPLAY_CACHE_BOUNCES) + " (the cached bounces)");
        if (!W.adjoint_inline) return fail(std::string(comp) + ": gradients need the in-place commit (HAR_ADJOINT_INLINE=0 is set)");
    }
    if (I->set.grad_bsdf_params) {
        /* the alpha / eta / k / slot-1 terms are committed in place by the cached-bounce shading kernel only */
        if (!I->set.use_cache || I->shape_on) return fail("gradients of alpha / eta / k / specular colours need the replay cache and cannot be combined with vertex-position gradients");
        if (bounce_limit(I) > HAR_REPLAY_CACHE_BOUNCES) return fail("gradients of alpha / eta / k / specular colours: max_depth must not exceed " + std::to_string(HAR_REPLAY_CACHE_BOUNCES) + " (the cached bounces)");
        if (!W.adjoint_inline) return fail("gradients of alpha / eta / k / specular colours need the in-place commit (HAR_ADJOINT_INLINE=0 is set)");
    }
    HIP_TRY(hipMemsetAsync(I->grad_slots, 0, (nb3 + ne3 + 3) * sizeof(float), s));
    if (I->shape_on) {
        if ((I->pos_verts && I->pos_offset.size() != S->hs.meshes.size()) || (I->inst_count && I->inst_count != S->hs.insts.size()))
            return fail("har_integrator_set_grad_positions / har_integrator_set_grad_instances was called for a different scene");
        if (I->pos_verts) HIP_TRY(hipMemsetAsync(I->grad_pos, 0, (size_t) 3 * I->pos_verts * sizeof(float), s));
        if (I->pos_verts && I->grad_nrm) HIP_TRY(hipMemsetAsync(I->grad_nrm, 0, (size_t) 3 * I->pos_verts * sizeof(float), s));
        if (I->inst_count) HIP_TRY(hipMemsetAsync(I->grad_inst, 0, (size_t) 12 * I->inst_count * sizeof(float), s));
    }
    HIP_TRY(hipMemsetAsync(I->totals, 0, 4 * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(I->status, 0, sizeof(int), s));
    I->last_stream = s;
    if (prof_begin(I, s)) return 1;
    launch_adjoint_image(s, grad_in, weight_film, (uint32_t) npx, I->adj);
    prof_mark(I, s, CLS_OTHER);
    for (uint64_t base = lb; base < le; base += chunk) {
        uint32_t n = (uint32_t) std::min<uint64_t>(chunk, le - base);
        /* pass 1: primal, keeps L per lane in `result` (common.py:752-762) */
        if (run_chunk(S, I, C, MODE_PRB_PRIMAL, seed, spp, log_spp, (uint32_t) base, n, I->grad_slots, s, tape == 2 ? RECORD_WRITE : tape == 1 ? TAPE_WRITE : I->cache_bounces ? CACHE_WRITE : CACHE_NONE)) return 1;
        /* pass 2: adjoint replay with the identical sample stream (common.py:765-775) */
        if (run_chunk(S, I, C, MODE_PRB_ADJOINT, seed, spp, log_spp, (uint32_t) base, n, I->grad_slots, s, tape == 2 ? RECORD_READ : tape == 1 ? TAPE_READ : I->cache_bounces ? CACHE_READ : CACHE_NONE)) return 1;
    }
    launch_add(s, I->grad_slots, grad_reflectance, (uint32_t) nb3);
    if (I->set.grad_emitters && ne3) launch_add(s, I->grad_slots + nb3, I->set.grad_emitters, (uint32_t) ne3);
    if (I->shape_on)
        for (size_t m = 0; m < I->pos_user.size(); ++m) {
            if (!I->pos_user[m]) continue;
            /* meshes with vertex normals: the summed adjoints of the vertex normals go through compute_normals once per face (second stage) */
            if (I->grad_nrm && (S->hs.meshes[m].flags & 1u))
                launch_normals_adjoint(s, S->ds, (uint32_t) m, S->hs.meshes[m].face_count, S->hs.meshes[m].vertex_count, I->nrm_acc + 3 * (size_t) I->pos_offset[m],
                                       I->grad_nrm + 3 * (size_t) I->pos_offset[m], I->grad_pos + 3 * (size_t) I->pos_offset[m]);
            launch_add(s, I->grad_pos + 3 * (size_t) I->pos_offset[m], I->pos_user[m], 3 * I->pos_count[m]);
        }
    if (I->shape_on && I->inst_count) launch_add(s, I->grad_inst, I->inst_user, 12 * I->inst_count);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* RBIntegrator.render_forward (src/python/python/ad/integrators/common.py:497-623): primal pass (L per lane), then the differential pass in
 * FORWARD mode -- the adjoint kernels read the parameters' tangents where render_backward accumulates gradients, and every lane sums
 * <d Lo / d theta, tangent> over its vertices (prb.py:313) -- then the lanes' differential radiance is splatted like an image. */
int har_render_forward(HarScene S, HarIntegrator I, const HarSensor *sensor, uint32_t seed, uint32_t spp, uint64_t lb, uint64_t le,
                       const float *tangent_reflectance, const float *const *tangent_textures, const float *tangent_emitters, float *film, void *stream) {
    DSensor C; uint32_t log_spp;
    if (check_common(S, I, sensor, spp, lb, le, C, log_spp)) return 1;
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("render_forward is implemented by the `prb` integrator");
    if (!film || !tangent_reflectance) return fail("null film / tangent buffers");
    if (I->shape_on) return fail("render_forward: tangents of vertex positions are not implemented (use render_backward for shape gradients)");
    if (S->ds.bsdf_types & HAR_SCENE_PROJECTOR) return fail("projector: render_forward is not implemented for a scene that holds a `projector` (forward-mode tangents of its irradiance and `scale`)");
    if ((S->ds.bsdf_types & HAR_SCENE_THIN) && (S->ds.bsdf_types & HAR_SCENE_WIDE_ROUTE) != HAR_SCENE_THIN)
        return fail("thindielectric: render_forward is not implemented for a scene that holds a `thindielectric` record next to a blendbsdf / mask / normalmap / bumpmap record, a roughness map or a `mesh_attribute` texture (that kernel set has no item-writing adjoint)");
    if (S->ds.bsdf_types & HAR_SCENE_ALPHAMAP) return fail("roughness map: render_forward is not implemented for a scene with a bitmap `alpha` (forward-mode tangents of alpha texels)");
    if (S->ds.bsdf_types & HAR_SCENE_BUMPMAP) return fail("bumpmap: render_forward is not implemented for a scene with a `bumpmap` record (forward-mode tangents of the height map and of nested parameters)");
    if (S->ds.bsdf_types & HAR_SCENE_NORMALMAP) return fail("normalmap: render_forward is not implemented for a scene with a `normalmap` record (forward-mode tangents of the normal map and of nested parameters)");
    /* forward mode commits through items, which carry a uv and no face: in a scene with a `mesh_attribute` texture the face comes from the replay cache's hit records,
     * so every bounce must be a cached one */
    if ((S->ds.bsdf_types & HAR_SCENE_ATTR) && (!I->set.use_cache || bounce_limit(I) > HAR_REPLAY_CACHE_BOUNCES))
        return fail("mesh_attribute: render_forward of a scene with a `mesh_attribute` texture needs the replay cache and max_depth must not exceed " + std::to_string(HAR_REPLAY_CACHE_BOUNCES) + " (the cached bounces)");
    hipStream_t s = (hipStream_t) stream;
    if (I->set.max_depth == 0) {        /* no interaction, no derivative: a zero image with the filter weights */
        return har_render_weights(sensor, seed, spp, lb, le, film, stream);
    }
    uint32_t chunk = (uint32_t) std::min<uint64_t>(I->set.chunk, (std::max<uint64_t>(le - lb, 2048) + 2047) / 2048 * 2048);
    if (ensure_workspace(I, chunk, true)) return 1;
    if ((S->ds.bsdf_types & HAR_SCENE_ATTR) && I->cache_bounces < bounce_limit(I)) return fail("mesh_attribute: render_forward of a scene with a `mesh_attribute` texture needs every bounce in the replay cache");
    const size_t nt = S->hs.textures.size();
    if (I->grad_tex_cap < std::max<size_t>(nt, 1)) { if (ws_alloc(I, &I->d_grad_tex, std::max<size_t>(nt, 1))) return 1; I->grad_tex_cap = std::max<size_t>(nt, 1); }
    if (nt) {
        if (!tangent_textures) return fail("tangent_textures is null but the scene has bitmap textures");
        for (size_t k = 0; k < nt; ++k) if (!tangent_textures[k]) return fail("null texture tangent buffer");
        if (upload_pointer_table(I, (const void *const *) tangent_textures, nt, s)) return 1;
    }
    /* tangent slots in the layout of the gradient slots: (bsdf_count + emitter_count) x 3 */
    const size_t nb3 = 3 * S->hs.bsdfs.size(), ne3 = 3 * S->hs.emitters.size();
    if (I->grad_slots_cap < nb3 + ne3 + 3) { if (ws_alloc(I, &I->grad_slots, nb3 + ne3 + 3)) return 1; I->grad_slots_cap = nb3 + ne3 + 3; }
    HIP_TRY(hipMemsetAsync(I->grad_slots, 0, (nb3 + ne3 + 3) * sizeof(float), s));
    if (nb3) HIP_TRY(hipMemcpyAsync(I->grad_slots, tangent_reflectance, nb3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (tangent_emitters && ne3) HIP_TRY(hipMemcpyAsync(I->grad_slots + nb3, tangent_emitters, ne3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(I->totals, 0, 4 * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(I->status, 0, sizeof(int), s));
    I->last_stream = s; I->twin_used = false;
    if (prof_begin(I, s)) return 1;
    float *saved_emitters = I->set.grad_emitters;
    I->set.grad_emitters = tangent_emitters ? I->grad_slots + nb3 : nullptr;       /* only its non-null-ness is read (HAR_SHADE_EMITTER_GRADS) */
    int rc = 0;
    for (uint64_t base = lb; base < le && !rc; base += chunk) {
        uint32_t n = (uint32_t) std::min<uint64_t>(chunk, le - base);
        rc = run_chunk(S, I, C, MODE_PRB_PRIMAL, seed, spp, log_spp, (uint32_t) base, n, nullptr, s, I->cache_bounces ? CACHE_WRITE : CACHE_NONE);
        I->forward_mode = true;
        if (!rc) rc = run_chunk(S, I, C, MODE_PRB_ADJOINT, seed, spp, log_spp, (uint32_t) base, n, I->grad_slots, s, I->cache_bounces ? CACHE_READ : CACHE_NONE);
        I->forward_mode = false;
        if (!rc) { launch_splat(s, C, seed, spp, log_spp, (uint32_t) base, n, I->dL, 0, film); prof_mark(I, s, CLS_SPLAT); }
    }
    I->set.grad_emitters = saved_emitters;
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

/* BSDFs with only delta lobes on MOVING geometry: bsdf.eval() is zero there, so prb.py:288 forms relative_grad(0) -- a 0 / 0 whose value the tree does not
 * pin -- and the sampled direction is a reflection / refraction of wi, not a direction the solid-angle-to-area Jacobian could hold fixed.  Refused. */
static bool record_has_smooth_lobe(const HostScene &hs, int32_t index) {
    if (index < 0 || (size_t) index >= hs.bsdfs.size()) return false;
    const DBsdf &b = hs.bsdfs[(size_t) index];
    return bsdf_is_smooth<HAR_SCENE_THIN>(b) && (b.back < 0 || bsdf_is_smooth<HAR_SCENE_THIN>(hs.bsdfs[(size_t) b.back]));
}

int har_integrator_set_grad_positions(HarIntegrator I, HarScene S, float *const *grad_positions) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("vertex-position gradients are computed by the `prb` integrator");
    std::vector<float *> user; std::vector<int32_t> offset; std::vector<uint32_t> count; uint32_t verts = 0; bool smooth = false;
    if (grad_positions) {
        if (!S) return fail("null scene");
        /* the hand-derived adjoint of har_shape_grad.h covers top-level meshes, flat-shaded or with (regenerated) vertex normals, carrying any BSDF with a non-delta lobe (the directional derivatives
         * of the models come from har_bsdf_dir.h); the rest of the scene may carry any model -- a vertex next to moving geometry contributes through its
         * attached si.wi (prb.py:128-140) */
        const size_t nm = S->hs.meshes.size();
        /* their adjoint goes through items, which carry one (record, direct, relative) triple per vertex: a blend vertex has three */
        /* ... and the barycentrics an attribute is looked up at move with the positions (Mesh::barycentric_coordinates): not differentiated */
        if (S->ds.bsdf_types & HAR_SCENE_PROJECTOR) return fail("projector: vertex-position gradients are not produced for a scene that holds a `projector` (the uv that eval_direction re-attaches to a moving shading point, projector.cpp:282-288, is not differentiated)");
        if (S->ds.bsdf_types & HAR_SCENE_THIN) return fail("thindielectric: vertex-position gradients are not produced for a scene with a `thindielectric` record");
        if (S->ds.bsdf_types & HAR_SCENE_ATTR) return fail("vertex-position gradients are not produced for a scene with a `mesh_attribute` texture");
        if (S->ds.bsdf_types & HAR_SCENE_ALPHAMAP) return fail("roughness map: vertex-position gradients are not produced for a scene with a bitmap `alpha`");
        if (S->ds.bsdf_types & HAR_SCENE_BUMPMAP) return fail("vertex-position gradients are not produced for a scene with a `bumpmap` record");
        if (S->ds.bsdf_types & HAR_SCENE_NORMALMAP) return fail("vertex-position gradients are not produced for a scene with a `normalmap` record");
        if (S->ds.bsdf_types & HAR_SCENE_MASK) return fail("vertex-position gradients are not produced for a scene with a `mask` record");
        if (S->ds.bsdf_types & HAR_SCENE_BLEND) return fail("vertex-position gradients are not produced for a scene with a `blendbsdf` record");
        offset.assign(nm, -1); user.assign(nm, nullptr); count.assign(nm, 0);
        for (size_t m = 0; m < nm; ++m) {          /* top-level meshes, then the meshes of the shape groups (vertex positions shared by all their instances) */
            if (!grad_positions[m]) continue;
            const DMesh &M = S->hs.meshes[m];
            if (m >= S->hs.top_mesh_count && I->inst_count) return fail("Cannot differentiate instance parameters and shapegroup internal parameters at the same time!");      /* instance.cpp:162-166 */
            const bool known = (I->pos_checked_scene == S->serial && m < I->pos_checked.size() && I->pos_checked[m]) ||      /* an optimisation loop calls this every step */
                               (m < S->normals_regenerated.size() && S->normals_regenerated[m]);                             /* k_vertex_normals wrote them (har_scene_update_vertices_device) */
            if ((M.flags & 1u) && known) smooth = true;
            else if (M.flags & 1u) {
                if (refresh_host_vertices(S, nullptr, (int) m)) return 1;
                /* a position update regenerates the vertex normals (mesh.cpp:876-878 -> compute_normals): the gradient is that of the REGENERATED normals, so the
                 * mesh must carry them -- stored normals of another origin (file, analytic) would render one surface and differentiate another */
                std::vector<float> copy(S->hs.verts.begin() + 8 * (size_t) M.voff, S->hs.verts.begin() + 8 * (size_t) (M.voff + M.vertex_count));
                if (har_mesh_compute_normals(M.vertex_count, copy.data(), M.face_count, S->hs.faces.data() + 4 * (size_t) M.foff)) return 1;
                float worst = 0.f;
                for (size_t v = 0; v < M.vertex_count; ++v) for (int c = 3; c < 6; ++c) worst = std::max(worst, std::fabs(copy[8 * v + c] - S->hs.verts[8 * ((size_t) M.voff + v) + c]));
                if (worst > 1e-4f) return fail("vertex-position gradients of a mesh with vertex normals: its normals are not the ones a position update regenerates (Mesh::compute_normals, mesh.cpp:876-878); write the positions once (params.update()) or regenerate the normals first");
                smooth = true;
                if (I->pos_checked_scene != S->serial) { I->pos_checked_scene = S->serial; I->pos_checked.assign(nm, 0); }
                I->pos_checked[m] = 1;
            }
            if (!record_has_smooth_lobe(S->hs, M.bsdf)) return fail("vertex-position gradients: a differentiated mesh cannot carry a BSDF made of delta lobes only (`dielectric`, `conductor`); other meshes of the scene may");
            offset[m] = (int32_t) verts; user[m] = grad_positions[m]; count[m] = M.vertex_count; verts += M.vertex_count;
        }
        if (verts == 0) { offset.clear(); user.clear(); count.clear(); }
    }
    if (offset != I->pos_offset || verts != I->pos_verts || smooth != I->pos_smooth) {      /* the geometry records and the offset table are part of the adjoint workspace */
        (void) hipDeviceSynchronize();
        I->free_ws();
    }
    I->pos_user = user; I->pos_offset = offset; I->pos_count = count; I->pos_verts = verts; I->pos_smooth = smooth; I->shape_on = verts != 0 || I->inst_count != 0;
    return 0;
}

int har_integrator_set_grad_instances(HarIntegrator I, HarScene S, float *grad_to_world) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("instance to_world gradients are computed by the `prb` integrator");
    uint32_t n = 0;
    if (grad_to_world) {
        if (!S) return fail("null scene");
        if (S->ds.bsdf_types & HAR_SCENE_PROJECTOR) return fail("projector: instance to_world gradients are not produced for a scene that holds a `projector` (the uv that eval_direction re-attaches to a moving shading point, projector.cpp:282-288, is not differentiated)");
        if (S->ds.bsdf_types & HAR_SCENE_THIN) return fail("thindielectric: instance to_world gradients are not produced for a scene with a `thindielectric` record");
        if (S->ds.bsdf_types & HAR_SCENE_ATTR) return fail("instance to_world gradients are not produced for a scene with a `mesh_attribute` texture");
        if (S->ds.bsdf_types & HAR_SCENE_ALPHAMAP) return fail("roughness map: instance to_world gradients are not produced for a scene with a bitmap `alpha`");
        if (S->ds.bsdf_types & HAR_SCENE_BUMPMAP) return fail("instance to_world gradients are not produced for a scene with a `bumpmap` record");
        if (S->ds.bsdf_types & HAR_SCENE_NORMALMAP) return fail("instance to_world gradients are not produced for a scene with a `normalmap` record");
        if (S->ds.bsdf_types & HAR_SCENE_MASK) return fail("instance to_world gradients are not produced for a scene with a `mask` record");
        if (S->ds.bsdf_types & HAR_SCENE_BLEND) return fail("instance to_world gradients are not produced for a scene with a `blendbsdf` record");
        /* as for the vertex positions: any BSDF with a non-delta lobe on the moving geometry, i.e. on the meshes of the shape groups */
        for (size_t m = S->hs.top_mesh_count; m < S->hs.meshes.size(); ++m)
            if (!record_has_smooth_lobe(S->hs, S->hs.meshes[m].bsdf)) return fail("instance to_world gradients: an instanced mesh cannot carry a BSDF made of delta lobes only (`dielectric`, `conductor`); top-level meshes may");
        n = (uint32_t) S->hs.insts.size();
        if (n == 0) return fail("the scene has no instances");
        for (size_t m = S->hs.top_mesh_count; m < I->pos_offset.size(); ++m)
            if (I->pos_offset[m] >= 0) return fail("Cannot differentiate instance parameters and shapegroup internal parameters at the same time!");      /* instance.cpp:162-166 */
        if (n >= (1u << (32 - HAR_SHAPE_INST_SHIFT)) - 1u) return fail("too many instances for the adjoint's geometry records");
    }
    if (n != I->inst_count) { (void) hipDeviceSynchronize(); I->free_ws(); }      /* the geometry records and the slot table are part of the adjoint workspace */
    I->inst_user = n ? grad_to_world : nullptr; I->inst_count = n; I->shape_on = I->pos_verts != 0 || n != 0;
    return 0;
}

int har_integrator_set_grad_bsdf_params(HarIntegrator I, float *grad) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("BSDF parameter gradients are computed by the `prb` integrator");
    I->set.grad_bsdf_params = grad;
    return 0;
}

int har_integrator_set_grad_light_texels(HarIntegrator I, int on) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("gradients of a light's texels are computed by the `prb` integrator");
    I->set.grad_light_texels = on != 0;
    return 0;
}

int har_integrator_set_grad_envmap(HarIntegrator I, int on) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("envmap gradients are computed by the `prb` integrator");
    I->set.grad_envmap = on != 0;
    return 0;
}

int har_integrator_set_grad_emitters(HarIntegrator I, float *grad_emitters) {
    if (!I) return fail("null integrator");
    if (I->set.type != HAR_INTEGRATOR_PRB) return fail("emitter gradients are computed by the `prb` integrator");
    I->set.grad_emitters = grad_emitters;
    return 0;
}

int har_render_stats(HarIntegrator I, HarStats *out) {
    if (!I || !out) return fail("null argument");
    memset(out, 0, sizeof(*out));
    if (!I->totals) return 0;
    hipStream_t s = I->last_stream;
    unsigned long long t[4] = { 0, 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(t, I->totals, sizeof(t), hipMemcpyDeviceToHost, s));
    if (read_status(I->status, s)) return 1;
    out->paths = t[0]; out->vertices = t[1]; out->closest_rays = t[2]; out->shadow_rays = t[3];
    if (I->twin_used && I->twin && I->twin->totals) {      /* the caller's stream has joined the side stream: one more copy on it sees the twin's counters */
        HIP_TRY(hipMemcpyAsync(t, I->twin->totals, sizeof(t), hipMemcpyDeviceToHost, s));
        if (read_status(I->twin->status, s)) return 1;
        out->paths += t[0]; out->vertices += t[1]; out->closest_rays += t[2]; out->shadow_rays += t[3];
    }
    return 0;
}

int har_integrator_set_top_seed(HarIntegrator I, int mode) {
    if (!I) return fail("null integrator");
    if (mode < -1 || mode > 1) return fail("har_integrator_set_top_seed: mode must be -1 (automatic), 0 (off) or 1 (on)");
    I->set.top_seed = mode;
    return 0;
}

int har_integrator_set_packet_tracing(HarIntegrator I, int mode) {
    if (!I) return fail("null integrator");
    if (mode < -1 || mode > 1) return fail("har_integrator_set_packet_tracing: mode must be -1 (automatic), 0 (off) or 1 (on)");
    I->set.packet_tracing = mode;
    return 0;
}

int har_integrator_set_material_queues(HarIntegrator I, int enable) {
    if (!I) return fail("null integrator");
    I->set.material_queues = enable != 0;
    return 0;
}

int har_integrator_set_replay_cache(HarIntegrator I, int enable) {
    if (!I) return fail("null integrator");
    if (I->set.use_cache != (enable != 0)) { (void) hipDeviceSynchronize(); I->free_ws(); I->set.use_cache = enable != 0; }
    return 0;
}

int har_integrator_set_profiling(HarIntegrator I, int enable) {
    if (!I) return fail("null integrator");
    /* (re)start: frames enqueued so far are dropped from the statistics (their events complete on their own and are reused later) */
    for (HarIntegratorImpl *J : { I, I->twin }) {
        if (!J) continue;
        J->set.profiling = enable != 0;
        if (!J->sets.empty()) { (void) hipDeviceSynchronize(); for (auto &E : J->sets) E.used = 0; }
        for (int k = 0; k < 8; ++k) { J->acc_ms[k] = 0.0; J->acc_launches[k] = 0; }
        J->acc_frames = 0;
    }
    return 0;
}

static int add_timing(HarIntegratorImpl *I, double ms[8], double launches[8], uint64_t &frames) {
    for (auto &E : I->sets) if (prof_collect(I, E)) return 1;
    for (int k = 0; k < 8; ++k) { ms[k] += I->acc_ms[k]; launches[k] += (double) I->acc_launches[k]; }
    frames = std::max(frames, I->acc_frames);
    return 0;
}
/* AVERAGE per frame over the frames rendered since har_integrator_set_profiling(1): ms[c] = device time between consecutive events of class c,
 * launches[c] = launches of class c per frame (rounded); ms[7] = number of frames averaged over.  In two-stream mode the launches of both
 * halves are summed: kernels of the two streams overlap, so the class totals exceed the wall time. */
int har_render_timing(HarIntegrator I, float ms[8], uint32_t launches[8]) {
    if (!I) return fail("null integrator");
    double m[8] = { 0 }, l[8] = { 0 }; uint64_t frames = 0;
    if (add_timing(I, m, l, frames)) return 1;
    if (I->twin && add_timing(I->twin, m, l, frames)) return 1;
    const double f = frames ? (double) frames : 1.0;
    for (int k = 0; k < 8; ++k) { ms[k] = (float) (m[k] / f); launches[k] = (uint32_t) (l[k] / f + 0.5); }
    ms[7] = (float) frames;
    return 0;
}

/* ------------------------------------------------------------------ AOV integrator (src/integrators/aov.cpp; kernels in har_aov.hip, per-lane code in har_aov.h) */
static int lower_aov_spec(uint32_t n_aovs, const uint32_t *types, AovSpec &spec) {
    const char *e = aov_spec_lower(n_aovs, types, spec);
    return e ? fail(e) : 0;
}

int har_aov_channel_count(uint32_t n_aovs, const uint32_t *types, uint32_t *count) {
    AovSpec spec;
    if (!count) return fail("null argument");
    if (lower_aov_spec(n_aovs, types, spec)) return 1;
    *count = spec.channels;
    return 0;
}

static bool aov_deep_stack(const HarSceneImpl *S) { return S->hs.stack_need() + HAR_STACK_MARGIN > (uint32_t) HAR_LDS_STACK_SMALL; }

int har_aov_sample(HarScene S, uint32_t n, const float *o, const float *d, const float *maxt, const uint8_t *active, uint32_t n_aovs, const uint32_t *types, float *out,
                   void *stream) {
    if (!S) return fail("null scene");
    AovSpec spec;
    if (lower_aov_spec(n_aovs, types, spec)) return 1;
    if (n == 0 || spec.channels == 0) return 0;
    if (!o || !d || !maxt || !out) return fail("null ray / output array");
    hipStream_t s = (hipStream_t) stream;
    float4 *h0 = nullptr; uint2 *h1 = nullptr; int *st = nullptr;
    HIP_TRY(dev_alloc((void **) &st, sizeof(int)));
    if (dev_alloc((void **) &h0, (size_t) n * sizeof(float4)) != hipSuccess || dev_alloc((void **) &h1, (size_t) n * sizeof(uint2)) != hipSuccess) {
        dev_free(st); dev_free(h0); return fail("har_aov_sample: out of device memory");
    }
    int rc = 0;
    if (hipMemsetAsync(st, 0, sizeof(int), s) != hipSuccess) rc = fail("har_aov_sample: hipMemsetAsync failed");
    if (!rc) {
        launch_aov_trace_rays(s, S->ds, aov_deep_stack(S), n, o, d, maxt, active, h0, h1, st);
        launch_aov_fill_rays(s, S->ds, spec, S->hs.top_mesh_count, n, d, active, h0, h1, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(std::string("har_aov_sample: ") + hipGetErrorString(e));
    }
    if (!rc) rc = read_status(st, s);              /* synchronises the stream: the blocks below are idle when they are freed */
    else (void) hipStreamSynchronize(s);
    dev_free(st); dev_free(h0); dev_free(h1);
    return rc;
}

int har_render_aovs(HarScene S, HarIntegrator I, const HarSensor *sensor, uint32_t seed, uint32_t spp, uint64_t lb, uint64_t le, uint32_t n_aovs, const uint32_t *types,
                    float *film, void *stream) {
    if (!S || !I || !sensor) return fail("null scene / integrator / sensor");
    if (!film) return fail("null film");
    AovSpec spec;
    if (lower_aov_spec(n_aovs, types, spec)) return 1;
    uint32_t spp_pass = spp, n_passes = 1, grid_w = 0, grid_h = 0;
    if (sample_grid(sensor, grid_w, grid_h)) return 1;
    if (pass_layout(I, grid_w, grid_h, spp, spp_pass, n_passes)) return 1;
    if (n_passes > 1) return fail("har_render_aovs: a render in several passes (samples_per_pass, more than 2^32 - 1 lanes) is not implemented by hip_ad_rgb for the aov integrator");
    DSensor C; uint32_t log_spp;
    if (check_common(S, I, sensor, spp, lb, le, C, log_spp)) return 1;
    if (I->film_rows && apply_film_window(I, sensor, spp, lb, le, film, spec.channels + 1u)) return 1;
    if (le == lb) return 0;
    hipStream_t s = (hipStream_t) stream;
    const uint32_t chunk = (uint32_t) std::min<uint64_t>(I->set.chunk, (std::max<uint64_t>(le - lb, 2048) + 2047) / 2048 * 2048);
    HarIntegratorImpl::AovWorkspace &W = I->aov;
    if (!W.status) { HIP_TRY(dev_alloc((void **) &W.status, sizeof(int))); }
    if (W.lanes < chunk) {
        if (W.h0 || W.h1) { (void) hipDeviceSynchronize(); dev_free(W.h0, true); dev_free(W.h1, true); W.h0 = nullptr; W.h1 = nullptr; W.lanes = 0; }
        HIP_TRY(dev_alloc((void **) &W.h0, (size_t) chunk * sizeof(float4)));
        HIP_TRY(dev_alloc((void **) &W.h1, (size_t) chunk * sizeof(uint2)));
        W.lanes = chunk;
    }
    const size_t floats = (size_t) chunk * std::max<uint32_t>(spec.channels, 1u);
    if (W.floats < floats) {
        if (W.val) { (void) hipDeviceSynchronize(); dev_free(W.val, true); W.val = nullptr; W.floats = 0; }
        HIP_TRY(dev_alloc((void **) &W.val, floats * sizeof(float)));
        W.floats = floats;
    }
    HIP_TRY(hipMemsetAsync(W.status, 0, sizeof(int), s));
    I->last_stream = s; I->twin_used = false;
    if (prof_begin(I, s)) return 1;
    const bool deep = aov_deep_stack(S);
    const bool aov_rays = I->set.batch.n || C.projection == 2u;      /* batch sensor / thin lens: the camera rays are made first (k_aov_batch_rays), then the array-valued flavours run */
    if (aov_rays && I->aov_rays_cap < chunk) {
        if (I->aov_rays) { (void) hipDeviceSynchronize(); dev_free(I->aov_rays, true); I->aov_rays = nullptr; I->aov_rays_cap = 0; }
        HIP_TRY(dev_alloc((void **) &I->aov_rays, (size_t) chunk * 7 * sizeof(float)));
        I->aov_rays_cap = chunk;
    }
    for (uint64_t base = lb; base < le; base += chunk) {
        const uint32_t n = (uint32_t) std::min<uint64_t>(chunk, le - base);
        if (aov_rays) {        /* the lanes' camera rays from the child table / through the lens, then the array-valued flavours of the pass (channel stride n) */
            float *ro = I->aov_rays, *rd = ro + 3 * (size_t) n, *rt = rd + 3 * (size_t) n;
            launch_aov_batch_rays(s, C, I->set.batch, seed, spp, log_spp, (uint32_t) base, n, ro, rd, rt);
            prof_mark(I, s, CLS_RAYGEN);
            launch_aov_trace_rays(s, S->ds, deep, n, ro, rd, rt, nullptr, W.h0, W.h1, W.status);
            prof_mark(I, s, CLS_TRACE);
            launch_aov_fill_rays(s, S->ds, spec, S->hs.top_mesh_count, n, rd, nullptr, W.h0, W.h1, W.val);
            prof_mark(I, s, CLS_SHADE);
            launch_splat_channels(s, C, seed, spp, log_spp, (uint32_t) base, n, W.val, (size_t) n, spec.channels, film);
            prof_mark(I, s, CLS_SPLAT);
            continue;
        }
        launch_aov_trace_lanes(s, S->ds, deep, C, seed, spp, log_spp, (uint32_t) base, n, W.h0, W.h1, W.status);
        prof_mark(I, s, CLS_TRACE);
        launch_aov_fill_lanes(s, S->ds, spec, S->hs.top_mesh_count, C, seed, spp, log_spp, (uint32_t) base, n, W.h0, W.h1, W.val, (size_t) chunk);
        prof_mark(I, s, CLS_SHADE);
        launch_splat_channels(s, C, seed, spp, log_spp, (uint32_t) base, n, W.val, (size_t) chunk, spec.channels, film);
        prof_mark(I, s, CLS_SPLAT);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

} // extern "C"
