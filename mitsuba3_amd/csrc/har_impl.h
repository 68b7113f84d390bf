/*
 * har_impl.h -- private header of the translation units that implement the C ABI of include/hip_ad_rgb.h (har_device_mem.hip, har_scene_api.hip,
 * har_capi.hip): the scene and integrator handles, error reporting, the device allocator and the profiling marks.
 * There is no CPU fallback anywhere in these files: without a HIP device every entry point that touches the GPU fails with an error.
 */
#pragma once
#include "../../include/hip_ad_rgb.h"
#include "har_kernels.h"
#include "har_scene_host.h"
#include "har_refit.h"
#include "har_plan.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace har;

int har_set_error(const std::string &msg);       /* har_device_mem.hip; also used by har_mesh_io.cpp */
inline int fail(const std::string &msg) { return har_set_error(msg); }
const std::string &har_error_text();

#define HIP_TRY(expr)                                                                          \
    do { hipError_t _e = (expr); if (_e != hipSuccess) {                                       \
        return fail(std::string(#expr) + ": " + hipGetErrorString(_e)); } } while (0)

/* device allocations of the library (har_device_mem.hip) */
hipError_t dev_alloc(void **out, size_t bytes);
void dev_free(void *p, bool device_is_idle = false);      /* device_is_idle: the caller has synchronised the device (free_ws: once for all its blocks) */

template <typename T> hipError_t upload(const std::vector<T> &v, const T **dst, std::vector<void *> &owned) {
    *dst = nullptr;
    size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    void *p = nullptr;
    hipError_t e = dev_alloc(&p, bytes);
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (!v.empty()) { e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); if (e != hipSuccess) return e; }
    *dst = (const T *) p;
    return hipSuccess;
}

inline uint64_t g_scene_serial = 0;
struct HarSceneImpl {
    uint64_t serial = ++g_scene_serial;       /* identifies the scene in per-integrator caches (a freed scene's address may be reused) */
    uint32_t mat_classes = 0, mat_miss_class = 0;   /* material classes (MaterialQueues) the scene's BSDF records fall into: bit mask, and the class escaped paths ride in */
    HostScene hs;
    DScene ds{};
    std::vector<void *> owned;
    std::vector<float *> tex_dev;
    DBsdf *d_bsdfs = nullptr;
    /* har_scene_set_*_device: the host mirrors (hs.textures[k].data, hs.bsdfs, hs.emitters) that no longer hold the device's values */
    std::vector<uint8_t> tex_host_stale; bool bsdf_host_stale = false, emitter_host_stale = false;
    /* incremental accel updates (har_scene_update_instances / har_scene_update_vertices): capacity of the node array (BLAS nodes + the largest TLAS the instances can
     * need), scratch of the device refit -- boxes of the triangle records and of the nodes, the nodes of every BLAS by depth, one surface-area accumulator per BLAS
     * (+ the root box read-back) */
    size_t nodes_cap = 0;
    RefitBox *tri_box = nullptr, *node_box = nullptr; uint32_t *d_refit_order = nullptr; float *d_area = nullptr;
    double last_refit_cost = 0.0, last_refit_ratio = 1.0;
    float *d_emitter_distr = nullptr; DTexture *d_textures = nullptr;
    /* device-resident vertex updates (har_scene_update_vertices_device): per mesh -- the host mirror of its vertex records (hs.verts, hs.shade_tris) is older than
     * the device's; its normals are the ones k_vertex_normals regenerated; its corner list (har_vertex_update.h) on the device.  `pend`: one pinned record the last
     * update's refit writes its figures to (surface-area sum, root box, non-finite flag) behind `pend_ev` -- read by the NEXT call, nothing waits for it */
    std::vector<uint8_t> verts_host_stale, normals_regenerated;
    std::vector<uint32_t *> d_corner_begin, d_corners;
    struct PendingRefit { float area; RefitBox root; uint32_t bad; } *pend = nullptr;
    hipEvent_t pend_ev = nullptr; bool pend_active = false; BlasInfo *pend_blas = nullptr; uint32_t *d_bad = nullptr;
    /* device refit of the instance level (instanced meshes): TLAS nodes by depth, {first vertex, count} of every leaf record's group, the records' boxes; valid for tlas_serial */
    uint32_t *d_tlas_order = nullptr; uint2 *d_inst_vrange = nullptr; RefitBox *d_inst_box = nullptr; uint64_t d_tlas_serial = 0; size_t d_tlas_cap = 0, d_inst_cap = 0;
    /* device-resident instance transforms (har_scene_update_instances_device): TLAS leaf record of every instance, the "singular / not finite" flag of the last update in a
     * pinned word behind an event (read by the next call), and whether hs.insts (the host mirror of the transforms) is older than the device's */
    uint32_t *d_rec_of = nullptr; size_t d_rec_of_cap = 0; uint32_t *pend_inst = nullptr, *d_bad_inst = nullptr; hipEvent_t pend_inst_ev = nullptr; bool pend_inst_active = false;
    bool insts_host_stale = false;
    hipStream_t last_push_stream = nullptr; bool last_push_valid = false;      /* stream of the last har_scene_set_*_device copy: the blocking host read-backs order themselves after it */
    ~HarSceneImpl() {
        if (pend) (void) hipHostFree(pend); if (pend_ev) (void) hipEventDestroy(pend_ev);
        if (pend_inst) (void) hipHostFree(pend_inst); if (pend_inst_ev) (void) hipEventDestroy(pend_inst_ev);
    }
};

struct HarIntegratorImpl {
    Settings set;                         /* har_plan.h: everything the twin of two-stream mode shares with this integrator */
    DCamera *batch_cams = nullptr; uint32_t batch_cap = 0;      /* the block behind set.batch (har_integrator_set_batch_sensors) */
    float *aov_rays = nullptr; size_t aov_rays_cap = 0;      /* AOV pass of a batch sensor: the chunk's camera rays (7 floats per lane) */
    bool forward_mode = false;            /* har_render_forward in progress: the adjoint kernels read tangents and accumulate differential radiance */
    uint32_t film_row0 = 0, film_rows = 0; /* har_integrator_set_film_window: the film buffers of har_render hold rows [film_row0, film_row0 + film_rows) of the crop window (0 rows = all) */
    float *alpha_lane = nullptr;          /* alpha value per lane of the chunk */
    /* AOV pass (har_render_aovs): hit records and channel-major values of one chunk -- blocks of their own, not part of the path tracer's workspace */
    struct AovWorkspace { float4 *h0 = nullptr; uint2 *h1 = nullptr; float *val = nullptr; int *status = nullptr; size_t lanes = 0, floats = 0; } aov;
    uint32_t *skip_counters = nullptr;    /* hide_emitters: count + cursor of the two continuation lists of skip_area_emitters */
    uint32_t *pk_list = nullptr, *pk_counters = nullptr;      /* wave-shared descent of the camera rays (k_trace_packet): the packets left to the per-lane kernel, their count + cursor */
    // workspace
    uint32_t ws_lanes = 0; bool ws_adjoint = false; uint32_t shard_cap = 0;
    std::vector<void *> owned;
    WaveState st[2]{};
    float4 *h0 = nullptr; uint2 *h1 = nullptr; float4 *hit_scratch = nullptr;      /* hit records (32 B per lane, two views); scratch records of hide_emitters */
    ItemArrays items{};
    float4 *result = nullptr, *dL = nullptr;
    /* PRB replay cache (see ReplayCache): cache_bounces arrays of ws_lanes entries each */
    float4 *rc_h0 = nullptr; uint2 *rc_h1 = nullptr; uint8_t *rc_vis = nullptr; uint32_t cache_bounces = 0;
    /* PRB replay tape (TapeArrays, har_kernels.h): per bounce the wavefront's path state, its hit records, a visibility byte and the next-slot word per
     * vertex slot; two slot-ordered (L, dL) array pairs that alternate from bounce to bounce */
    int ws_tape = 0 /* 0 none, 1 state tape, 2 record tape */; uint32_t tape_bounces = 0;
    float4 *tape_rec[4] = { nullptr, nullptr, nullptr, nullptr };      /* record tape: rec0, rec1, rec2, rec_em (lanes x bounces each) */
    WaveState tape_st[HAR_REPLAY_CACHE_BOUNCES + 1]{}; float4 *tape_h0 = nullptr; uint8_t *tape_vis = nullptr; uint32_t *tape_next = nullptr;
    float4 *tape_la[2] = { nullptr, nullptr }; float2 *tape_lb[2] = { nullptr, nullptr };
    float *adj = nullptr; size_t adj_floats = 0;
    float *grad_slots = nullptr; size_t grad_slots_cap = 0;   /* adjoint accumulators: (bsdf_count + emitter_count) x 3 */
    /* vertex-position gradients (har_integrator_set_grad_positions): user buffers per top-level mesh, the flat accumulation buffer + offsets */
    bool shape_on = false; std::vector<float *> pos_user; std::vector<int32_t> pos_offset; std::vector<uint32_t> pos_count;
    int32_t *d_pos_offset = nullptr; float *grad_pos = nullptr; uint32_t pos_verts = 0; ShapeArrays geo{};
    /* differentiated meshes WITH vertex normals: adjoints of the vertex normals and scratch for the normal sums, laid out like grad_pos (har_shape_grad.h) */
    bool pos_smooth = false; float *grad_nrm = nullptr, *nrm_acc = nullptr;
    uint64_t pos_checked_scene = 0; std::vector<uint8_t> pos_checked;      /* meshes of scene `pos_checked_scene` whose normals were found to be the regenerated ones */
    /* instance to_world gradients (har_integrator_set_grad_instances): user buffer (DEVICE, instance_count x 12), per-instance slot table, accumulation buffer */
    float *inst_user = nullptr; uint32_t inst_count = 0; int32_t *d_inst_slot = nullptr; float *grad_inst = nullptr;
    int bw_tape_max = 2; uint32_t bw_chunk_max = 0xffffffffu;      /* render_backward: what the last out-of-memory fallback settled on (tape kind, chunk lanes) */
    uint64_t bw_job_key = 0; uint32_t bw_calls_since_stepdown = 0;   /* ... for which job (scene, film, lanes), and how many calls ago */
    uint32_t *mq_idx = nullptr, *mq_count = nullptr;      /* per-material shading queues (MaterialQueues): HAR_MAT_CLASSES index lists of ws_lanes entries, their counters */
    uint2 *stack_spill = nullptr;         /* HBM part of the traversal stacks: HAR_STACK_SPILL entries per thread of the largest traversal grid */
    /* multi-pass rendering: sampler state per lane of the rendered lane range, pixel jitter per chunk lane (see PassState) */
    uint64_t *pass_rng = nullptr; size_t pass_rng_cap = 0; float2 *pass_jitter = nullptr; size_t pass_jitter_cap = 0;
    uint32_t *counters = nullptr;
    unsigned long long *totals = nullptr;
    int *status = nullptr;
    float **d_grad_tex = nullptr; size_t grad_tex_cap = 0;
    /* staging of the per-call pointer table (upload_pointer_table): a ring of pinned slots with one event each */
    void **ptr_ring = nullptr; size_t ptr_ring_cap = 0; hipEvent_t ptr_ring_ev[8]{}; bool ptr_ring_used[8]{}; uint32_t ptr_ring_next = 0;
    /* texel-gradient queues of the adjoint pass (TexelQueues, har_kernels.h): records, counters, band tables; built for `tq_scene` */
    TexelQueues tq{ nullptr, nullptr, nullptr, nullptr, 0u, 0u, nullptr }; uint64_t tq_scene = 0; uint32_t tq_lanes = 0, tq_lds = 0;
    // profiling
    /* Per-launch HIP events of the frames rendered since har_integrator_set_profiling(1).  An event is NEVER re-recorded while an earlier record of it
     * may still be pending: every frame (render_range / backward_range call) takes its own event set from a ring, and a set is only reused after its
     * last event has completed and its durations have been folded into the accumulators -- a render loop that enqueues tens of frames without a
     * synchronisation (bench.py) therefore neither waits nor touches in-flight events. */
    struct EventSet { std::vector<hipEvent_t> ev; std::vector<int> cls; size_t used = 0; };
    std::vector<EventSet> sets; size_t cur_set = 0;
    double acc_ms[8] = { 0 }; uint64_t acc_launches[8] = { 0 }; uint64_t acc_frames = 0;
    hipStream_t last_stream = nullptr;
    /* two-stream mode: a job of >= HAR_DUAL_MIN_LANES lanes is cut in two halves that run concurrently -- this integrator on the caller's stream, a
     * private twin (own workspace) on `side_stream`.  Every persistent traversal launch ends with a tail of a few hundred microseconds in which
     * the chip waits for the launch's longest rays (a chain of dependent node fetches); with two independent launch sequences in flight the blocks
     * of one fill the CUs the other's tail leaves idle. */
    HarIntegratorImpl *twin = nullptr; bool twin_used = false;
    hipStream_t side_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_stagger = nullptr; bool stagger_record = false;      /* staggered halves (HAR_DUAL_STAGGER): recorded behind the first half's first closest-hit launch, the second half starts there */
    /* shadow-ray overlap (small jobs): bounce b's shadow rays (k_resolve) do not depend on bounce b + 1's closest-hit rays (k_trace_closest) -- both only need
     * bounce b's shading -- so k_resolve runs on `aux_stream` next to the trace launch (and, with the second item set below, next to bounce b + 1's shading too).  One traversal
     * tail per bounce instead of two (see run_chunk). */
    hipStream_t aux_stream = nullptr; hipEvent_t ev_shaded = nullptr, ev_resolved = nullptr, ev_resolved2 = nullptr;
    /* ... with a second set of item arrays and a second radiance accumulator the shadow rays of bounce b only have to be done before bounce b + 2 is SHADED (the item
     * set is free again); `result2` collects what they add and is folded into `result` at the end of the chunk */
    ItemArrays items2{}; float4 *result2 = nullptr;
    void free_ws();
};
#define HAR_DUAL_MIN_LANES (1u << 20)
#define HAR_DUAL_MAX_LANES (1u << 24)

void prof_mark(HarIntegratorImpl *I, hipStream_t s, int cls);
enum { CLS_RAYGEN = 0, CLS_TRACE = 1, CLS_SHADE = 2, CLS_RESOLVE = 3, CLS_SPLAT = 4, CLS_OTHER = 6, CLS_START = 7 };

/* set by every failed workspace allocation, cleared by whoever handles it (render_backward's step-down): the condition "out of device memory", as a flag rather
 * than as a substring of the error text */
extern thread_local bool g_alloc_failed;
template <typename T> int ws_alloc(HarIntegratorImpl *I, T **p, size_t count) {
    void *q = nullptr;
    hipError_t e = dev_alloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { g_alloc_failed = true; return fail(std::string("hipMalloc(workspace): ") + hipGetErrorString(e)); }
    I->owned.push_back(q); *p = (T *) q;
    return 0;
}

inline uint32_t bounce_limit(const HarIntegratorImpl *I) { return std::min<uint32_t>(I->set.max_depth, HAR_MAX_BOUNCE_SLOTS - 2); }

/* har_device_mem.hip */
int ensure_workspace(HarIntegratorImpl *I, uint32_t lanes, bool adjoint, int tape = 0);
int ensure_texel_queues(HarSceneImpl *S, HarIntegratorImpl *I);
int prof_collect(HarIntegratorImpl *I, HarIntegratorImpl::EventSet &E);
int prof_begin(HarIntegratorImpl *I, hipStream_t s);
void prof_destroy(HarIntegratorImpl *I);
/* har_scene_api.hip */
int read_status(int *d_status, hipStream_t s);
int refresh_host_vertices(HarSceneImpl *S, hipStream_t s, int only_mesh);
