/*
 * har_device_mem.hip -- device memory of the library: the allocator hook and its guard ranges, the integrator's workspace and texel-gradient
 * queues, the per-launch profiling events, and the error text of the C ABI.
 */
#include "har_impl.h"

#include <map>
#include <mutex>

static thread_local std::string g_error;
int har_set_error(const std::string &msg) { g_error = msg; return 1; }
const std::string &har_error_text() { return g_error; }
thread_local bool g_alloc_failed = false;

/*
 * Device allocations of the library.  HAR_DEBUG_GUARD = 1 | 2 (debug switch, tests/test_gpu_parity.py::test_guarded_*): every buffer gets a private
 * virtual-address reservation (hipMemAddressReserve / hipMemCreate / hipMemMap) with UNMAPPED ranges on both sides, and sits flush against the
 * end (1) or the start (2) of its mapped pages -- an access past the end (before the start) of any workspace or scene array is then a GPU
 * memory-access fault whatever the neighbouring allocations are, instead of a silent read of another array.  Default: plain hipMalloc.
 */
namespace {
struct GuardedBlock { void *base; size_t reserved; void *mapped; size_t mapped_bytes; hipMemGenericAllocationHandle_t handle; };
std::map<void *, GuardedBlock> g_guarded;
std::mutex g_guarded_mutex;
int guard_mode() { return switches().debug_guard; }
/* har_set_allocator: the host's device allocator (the Python host installs PyTorch's caching allocator, so that workspaces and scene arrays show up in -- and are
 * reused through -- the process's one memory pool).  Every block remembers who has to free it, so the hook can be changed while blocks are alive. */
HarAllocFn g_alloc_fn = nullptr; HarFreeFn g_free_fn = nullptr; void *g_alloc_user = nullptr;
struct HostBlock { HarFreeFn free_fn; void *user; };
std::map<void *, HostBlock> g_host_blocks;
std::mutex g_alloc_mutex;
}
int har_set_allocator(HarAllocFn alloc_fn, HarFreeFn free_fn, void *user) {
    if ((alloc_fn == nullptr) != (free_fn == nullptr)) return fail("har_set_allocator: give both functions, or neither (hipMalloc / hipFree)");
    std::lock_guard<std::mutex> lock(g_alloc_mutex);
    g_alloc_fn = alloc_fn; g_free_fn = free_fn; g_alloc_user = user;
    return 0;
}
hipError_t dev_alloc(void **out, size_t bytes) {
    bytes = std::max<size_t>(bytes, 1);
    if (!guard_mode()) {
        HarAllocFn fn; HarFreeFn ffn; void *user;
        { std::lock_guard<std::mutex> lock(g_alloc_mutex); fn = g_alloc_fn; ffn = g_free_fn; user = g_alloc_user; }
        if (!fn) return hipMalloc(out, bytes);
        void *p = fn(bytes, user);
        if (!p) return hipErrorOutOfMemory;
        std::lock_guard<std::mutex> lock(g_alloc_mutex);
        g_host_blocks[p] = HostBlock{ ffn, user }; *out = p;
        return hipSuccess;
    }
    int dev = 0; hipError_t e = hipGetDevice(&dev); if (e != hipSuccess) return e;
    hipMemAllocationProp prop{}; prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = dev;
    size_t gran = 0; e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum); if (e != hipSuccess) return e;
    gran = std::max<size_t>(gran, 4096);
    GuardedBlock B{};
    B.mapped_bytes = (bytes + gran - 1) / gran * gran;
    const size_t guard = std::max<size_t>(gran, (size_t) 64 << 20);          /* 64 MB of nothing on either side */
    B.reserved = B.mapped_bytes + 2 * guard;
    e = hipMemAddressReserve(&B.base, B.reserved, gran, nullptr, 0); if (e != hipSuccess) return e;
    e = hipMemCreate(&B.handle, B.mapped_bytes, &prop, 0); if (e != hipSuccess) { (void) hipMemAddressFree(B.base, B.reserved); return e; }
    B.mapped = (char *) B.base + guard;
    e = hipMemMap(B.mapped, B.mapped_bytes, 0, B.handle, 0);
    if (e == hipSuccess) {
        hipMemAccessDesc acc{}; acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(B.mapped, B.mapped_bytes, &acc, 1);
    }
    if (e != hipSuccess) { (void) hipMemRelease(B.handle); (void) hipMemAddressFree(B.base, B.reserved); return e; }
    /* end-flush placement keeps 256-byte alignment (every array of the library is accessed with <= 16-byte vectors) */
    void *user = guard_mode() == 2 ? B.mapped : (char *) B.mapped + (B.mapped_bytes - bytes) / 256 * 256;
    std::lock_guard<std::mutex> lock(g_guarded_mutex);
    g_guarded[user] = B; *out = user;
    return hipSuccess;
}
void dev_free(void *p, bool device_is_idle) {
    if (!p) return;
    if (guard_mode()) {
        std::lock_guard<std::mutex> lock(g_guarded_mutex);
        auto it = g_guarded.find(p);
        if (it != g_guarded.end()) {
            const GuardedBlock B = it->second; g_guarded.erase(it);
            (void) hipDeviceSynchronize();
            (void) hipMemUnmap(B.mapped, B.mapped_bytes); (void) hipMemRelease(B.handle);
            /* the address range stays reserved for the life of the process (quarantine): a stale pointer faults instead of reaching a later allocation */
            return;
        }
    }
    {
        HostBlock B{ nullptr, nullptr };
        {
            std::lock_guard<std::mutex> lock(g_alloc_mutex);
            auto it = g_host_blocks.find(p);
            if (it != g_host_blocks.end()) { B = it->second; g_host_blocks.erase(it); }
        }
        /* hipFree synchronises the device before it releases a block; a pooling allocator hands the block to its next user at once, so do the same here
         * (the library's private streams may still be reading it) */
        if (B.free_fn) { if (!device_is_idle) (void) hipDeviceSynchronize(); B.free_fn(p, B.user); return; }
    }
    (void) hipFree(p);
}

/* One device synchronisation for the whole workspace: blocks handed back to a pooling allocator (har_set_allocator) are reused at once, and the library's private
 * streams may still be reading them -- the invariant is "no block of this library is freed while the device runs"; dev_free keeps it per block for single frees. */
void HarIntegratorImpl::free_ws() { if (!owned.empty()) (void) hipDeviceSynchronize(); for (void *p : owned) dev_free(p, true); owned.clear(); ws_lanes = 0; }

int ensure_workspace(HarIntegratorImpl *I, uint32_t lanes, bool adjoint, int tape) {
    if (I->ws_lanes >= lanes && (I->ws_adjoint || !adjoint) && (!adjoint || I->ws_tape == tape)) {
        if (I->set.alpha_film && !I->alpha_lane) return ws_alloc(I, &I->alpha_lane, I->ws_lanes);      /* `rgba` film on an existing workspace */
        return 0;
    }
    I->free_ws();
    I->counters = nullptr; I->totals = nullptr; I->status = nullptr; I->adj = nullptr; I->adj_floats = 0; I->d_grad_tex = nullptr; I->grad_tex_cap = 0;
    I->tq = TexelQueues{ nullptr, nullptr, nullptr, nullptr, 0u, 0u, nullptr }; I->tq_scene = 0; I->tq_lanes = 0;
    I->pass_rng = nullptr; I->pass_rng_cap = 0; I->pass_jitter = nullptr; I->pass_jitter_cap = 0;
    I->grad_slots = nullptr; I->grad_slots_cap = 0; I->mq_idx = nullptr; I->mq_count = nullptr;
    for (int k = 0; k < 2; ++k) {
        if (ws_alloc(I, &I->st[k].a0, lanes) || ws_alloc(I, &I->st[k].a1, lanes) || ws_alloc(I, &I->st[k].a2, lanes) ||
            ws_alloc(I, &I->st[k].a3, lanes) || ws_alloc(I, &I->st[k].a4, lanes)) return 1;
    }
    /* closest-hit records: one 32-byte record per lane, viewed as h0 (float4, stride 2) and h1 (uint2, stride 4) -- see HIT0 / HIT1 in har_kernels.hip */
    if (ws_alloc(I, &I->h0, (size_t) 2 * lanes)) return 1;
    I->h1 = HAR_HIT_INTERLEAVED ? reinterpret_cast<uint2 *>(I->h0 + 1) : reinterpret_cast<uint2 *>(I->h0 + lanes); I->hit_scratch = nullptr;
    if (ws_alloc(I, &I->items.s0, lanes) || ws_alloc(I, &I->items.s1, lanes) || ws_alloc(I, &I->items.s2, lanes)) return 1;
    I->items.s3 = I->items.s4 = nullptr; I->dL = nullptr; I->items2 = ItemArrays{}; I->result2 = nullptr;
    if (adjoint && (ws_alloc(I, &I->items.s3, lanes) || ws_alloc(I, &I->items.s4, lanes) || ws_alloc(I, &I->dL, lanes))) return 1;
    I->geo = ShapeArrays{}; I->d_pos_offset = nullptr; I->grad_pos = nullptr; I->d_inst_slot = nullptr; I->grad_inst = nullptr; I->grad_nrm = nullptr; I->nrm_acc = nullptr;
    if (adjoint && I->shape_on) {
        if (ws_alloc(I, &I->geo.g0, lanes) || ws_alloc(I, &I->geo.g1, lanes) || ws_alloc(I, &I->geo.g2, lanes) || ws_alloc(I, &I->geo.g3, lanes) || ws_alloc(I, &I->geo.g4, lanes) ||
            ws_alloc(I, &I->geo.g5, lanes) || ws_alloc(I, &I->geo.g6, lanes) || ws_alloc(I, &I->geo.pv0, lanes) || ws_alloc(I, &I->geo.pv1, lanes) || ws_alloc(I, &I->geo.vis, lanes)) return 1;
        if (I->pos_verts) {
            if (ws_alloc(I, &I->d_pos_offset, I->pos_offset.size()) || ws_alloc(I, &I->grad_pos, (size_t) 3 * I->pos_verts)) return 1;
            if (I->pos_smooth && (ws_alloc(I, &I->grad_nrm, (size_t) 3 * I->pos_verts) || ws_alloc(I, &I->nrm_acc, (size_t) 3 * I->pos_verts))) return 1;
            HIP_TRY(hipMemcpy(I->d_pos_offset, I->pos_offset.data(), I->pos_offset.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        if (I->inst_count) {
            std::vector<int32_t> slots(I->inst_count); for (uint32_t k = 0; k < I->inst_count; ++k) slots[k] = (int32_t) k;
            if (ws_alloc(I, &I->d_inst_slot, I->inst_count) || ws_alloc(I, &I->grad_inst, (size_t) 12 * I->inst_count)) return 1;
            HIP_TRY(hipMemcpy(I->d_inst_slot, slots.data(), slots.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
    }
    I->rc_h0 = nullptr; I->rc_h1 = nullptr; I->rc_vis = nullptr; I->cache_bounces = 0;
    I->ws_tape = 0; I->tape_bounces = 0; I->tape_h0 = nullptr; I->tape_vis = nullptr; I->tape_next = nullptr;
    for (int k = 0; k < 2; ++k) { I->tape_la[k] = nullptr; I->tape_lb[k] = nullptr; }
    for (int k = 0; k < 4; ++k) I->tape_rec[k] = nullptr;
    for (auto &w : I->tape_st) w = WaveState{};
    if (adjoint && tape == 2) {
        /* record tape (TapeArrays): 3 x 16 B of adjoint record + 16 B of emission + 1 B visibility + 4 B next slot per lane and bounce, 2 x 24 B for L / dL:
         * 37 GB for a 2^26-lane chunk at max_depth = 8 */
        const uint32_t nb = bounce_limit(I);
        for (int k = 0; k < 4; ++k) if (ws_alloc(I, &I->tape_rec[k], (size_t) lanes * nb)) return 1;
        if (ws_alloc(I, &I->tape_vis, (size_t) lanes * nb) || ws_alloc(I, &I->tape_next, (size_t) lanes * nb)) return 1;
        for (int k = 0; k < 2; ++k) if (ws_alloc(I, &I->tape_la[k], lanes) || ws_alloc(I, &I->tape_lb[k], lanes)) return 1;
        I->ws_tape = 2; I->tape_bounces = nb;
    } else
    if (adjoint && tape == 1) {
        /* the tape instead of the lane-indexed cache: (nb + 1) x 72 B of path state + nb x (32 B hit + 1 B visibility + 4 B next slot) per lane, 2 x 24 B for
         * L / dL: 62 GB for a 2^26-lane chunk at max_depth = 8 -- what 288 GB of HBM are for (the adjoint shading pass moves 40 % fewer bytes) */
        const uint32_t nb = bounce_limit(I);
        for (uint32_t b = 0; b <= nb; ++b)
            if (ws_alloc(I, &I->tape_st[b].a0, lanes) || ws_alloc(I, &I->tape_st[b].a1, lanes) || ws_alloc(I, &I->tape_st[b].a2, lanes) ||
                ws_alloc(I, &I->tape_st[b].a3, lanes) || ws_alloc(I, &I->tape_st[b].a4, lanes)) return 1;
        if (ws_alloc(I, &I->tape_h0, (size_t) 2 * lanes * nb) || ws_alloc(I, &I->tape_vis, (size_t) lanes * nb) || ws_alloc(I, &I->tape_next, (size_t) lanes * nb)) return 1;
        for (int k = 0; k < 2; ++k) if (ws_alloc(I, &I->tape_la[k], lanes) || ws_alloc(I, &I->tape_lb[k], lanes)) return 1;
        I->ws_tape = 1; I->tape_bounces = nb;
    } else
    if (adjoint && I->set.use_cache) {
        /* 25 B per lane and cached bounce; bounces beyond the cache are simply traced again */
        const uint32_t nb = std::min<uint32_t>(bounce_limit(I), HAR_REPLAY_CACHE_BOUNCES);
        if (nb && (ws_alloc(I, &I->rc_h0, (size_t) lanes * nb) || ws_alloc(I, &I->rc_h1, (size_t) lanes * nb) || ws_alloc(I, &I->rc_vis, (size_t) lanes * nb))) return 1;
        I->cache_bounces = nb;
    }
    if (ws_alloc(I, &I->result, lanes)) return 1;
    if (ws_alloc(I, &I->stack_spill, (size_t) HAR_STACK_SPILL * HAR_MAX_TRAVERSAL_BLOCKS * 256)) return 1;
    if (ws_alloc(I, &I->skip_counters, (size_t) 4 * HAR_SHARDS * HAR_COUNTER_STRIDE)) return 1;
    if (ws_alloc(I, &I->pk_list, (size_t) lanes / 64 + HAR_SHARDS) || ws_alloc(I, &I->pk_counters, (size_t) 2 * HAR_SHARDS * HAR_COUNTER_STRIDE)) return 1;
    I->alpha_lane = nullptr;
    if (I->set.alpha_film && ws_alloc(I, &I->alpha_lane, lanes)) return 1;
    if (ws_alloc(I, &I->counters, (size_t) 4 * HAR_MAX_BOUNCE_SLOTS * HAR_SHARDS * HAR_COUNTER_STRIDE) || ws_alloc(I, &I->totals, 4) || ws_alloc(I, &I->status, 1)) return 1;
    /* totals / status are cleared by every render call ON ITS STREAM before use.  (Round 1 also cleared them here with hipMemset: that memset is
     * enqueued on the NULL stream and runs after whatever is queued there -- in two-stream mode after the first half of the frame -- while the twin
     * renders on its non-blocking stream; when the twin finished first, the late memset wiped its counters: half the paths in har_render_stats,
     * seen as an intermittent test failure when scenes of different cost alternate.) */
    I->ws_lanes = lanes; I->ws_adjoint = adjoint; I->shard_cap = lanes / HAR_SHARDS;
    return 0;
}

/* HAR_DEBUG_SYNC=1 (debug switch): name every launch class on stderr and wait for it, so that a GPU fault is attributed to a kernel */
static void dbg_sync(hipStream_t s, int cls) {
    if (!switches().debug_sync) return;
    static const char *names[8] = { "raygen", "trace_closest", "shade", "resolve", "splat", "?", "other", "start" };
    fprintf(stderr, "[hip_ad_rgb] sync after %s ...", names[cls & 7]); fflush(stderr);
    hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, " %s\n", hipGetErrorString(e)); fflush(stderr);
}

#define HAR_PROFILE_RING 32       /* event sets (frames in flight) before prof_begin has to wait for the oldest */
/* fold a finished event set into the accumulators (waits for its last event) */
int prof_collect(HarIntegratorImpl *I, HarIntegratorImpl::EventSet &E) {
    if (E.used >= 2) {
        HIP_TRY(hipEventSynchronize(E.ev[E.used - 1]));
        for (size_t k = 1; k < E.used; ++k) {
            float dt = 0.f;
            HIP_TRY(hipEventElapsedTime(&dt, E.ev[k - 1], E.ev[k]));
            int c = E.cls[k]; if (c < 0 || c > 6) c = CLS_OTHER;
            I->acc_ms[c] += dt; I->acc_launches[c]++; I->acc_ms[5] += dt;
        }
        I->acc_frames++;
    }
    E.used = 0;
    return 0;
}
/* start of a frame: take the next event set of the ring */
int prof_begin(HarIntegratorImpl *I, hipStream_t s) {
    if (!I->set.profiling) return 0;
    if (I->sets.empty()) { I->sets.resize(1); I->cur_set = 0; }
    else {
        const size_t next = (I->cur_set + 1) % HAR_PROFILE_RING;
        if (next >= I->sets.size()) I->sets.resize(next + 1);
        I->cur_set = next;
    }
    if (prof_collect(I, I->sets[I->cur_set])) return 1;
    prof_mark(I, s, CLS_START);
    return 0;
}
void prof_mark(HarIntegratorImpl *I, hipStream_t s, int cls) {
    dbg_sync(s, cls);
    if (!I->set.profiling || I->sets.empty()) return;
    HarIntegratorImpl::EventSet &E = I->sets[I->cur_set];
    if (E.used == E.ev.size()) {
        hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return;
        E.ev.push_back(e); E.cls.push_back(cls);
    }
    E.cls[E.used] = cls;
    (void) hipEventRecord(E.ev[E.used++], s);
}
void prof_destroy(HarIntegratorImpl *I) {
    for (auto &E : I->sets) for (hipEvent_t e : E.ev) (void) hipEventDestroy(e);
    I->sets.clear();
}

/* texel-gradient queues for the bitmap textures of scene S (see TexelQueues): row bands whose LDS copy fits HAR_TQ_LDS_BYTES, at most HAR_TQ_MAX of
 * them; textures that do not fit keep the direct atomics.  HAR_TEXEL_QUEUES=0 switches the queues off (A/B). */
int ensure_texel_queues(HarSceneImpl *S, HarIntegratorImpl *I) {
    const bool enabled = switches().texel_queues;
    if (I->tq_scene == S->serial && I->tq_lanes == I->ws_lanes) return 0;
    /* queues of another scene (params.update() re-creates the scene handle; one integrator may alternate between scenes): give their buffers back
     * first -- the record buffer alone is 64 B per workspace lane */
    {
        void *old[4] = { I->tq.rec, I->tq.count, const_cast<uint2 *>(I->tq.band), const_cast<uint4 *>(I->tq.qinfo) };
        for (void *q : old) {
            if (!q) continue;
            auto it = std::find(I->owned.begin(), I->owned.end(), q);
            if (it != I->owned.end()) { I->owned.erase(it); dev_free(q); }
        }
    }
    I->tq = TexelQueues{ nullptr, nullptr, nullptr, nullptr, 0u, 0u, nullptr }; I->tq_scene = S->serial; I->tq_lanes = I->ws_lanes;
    const size_t nt = S->hs.textures.size();
    if (!enabled || nt == 0) return 0;
    /* LDS copy of a band: the smallest of 24 / 32 / 48 / 64 KB that keeps the texture within HAR_TQ_MAX queues (three 64-bit accumulators per texel: a 256-wide
     * texture gets 4-row bands in 32 KB, five blocks per CU).  Round 2 measured the float version at 24 / 48 / 64 KB: 125.9 / 130.4 / 127.7 ms per PRB step --
     * what matters is that every CU holds several blocks.  HAR_TQ_LDS forces one size (A/B). */
    const size_t lds_forced = switches().tq_lds;
    std::vector<uint2> band(nt); std::vector<uint4> qinfo, heights; uint32_t nq = 0; size_t lds_used = 0;
    for (size_t t = 0; t < nt; ++t) {
        const uint32_t W = S->hs.textures[t].w, H = S->hs.textures[t].h;
        band[t] = make_uint2(0xffffffffu, 1u);
        if (W == 0 || H == 0 || W > 65535u || H > 65535u) continue;
        if (S->hs.textures[t].mode != 0u) continue;          /* the queue records assume the bilinear + repeat neighbourhood (x0 + 1, y0 + 1 wrapped): other modes keep the direct atomics */
        const size_t sizes[4] = { (size_t) HAR_TQ_LDS_BYTES, 32768, 49152, 65536 };
        for (int k = 0; k < 4; ++k) {
            const size_t lds = lds_forced ? lds_forced : sizes[k];
            const size_t row_bytes = (size_t) W * 3 * HAR_TQ_ACC_BYTES;                /* three 64-bit fixed-point accumulators per texel */
            if (row_bytes * 2 > lds) { if (lds_forced) break; continue; }
            /* the LDS copy of a band holds its rows + the row after it (k_texel_accumulate) */
            const uint32_t rows = std::min<uint32_t>(H, (uint32_t) (lds / row_bytes) - 1u), nb = (H + rows - 1) / rows;
            if (nq + nb > HAR_TQ_MAX) { if (lds_forced) break; continue; }
            band[t] = make_uint2(nq, rows);
            for (uint32_t b = 0; b < nb; ++b) { qinfo.push_back(make_uint4((uint32_t) t, b * rows, std::min(rows, H - b * rows), W)); heights.push_back(make_uint4(H, 0u, 0u, 0u)); }
            nq += nb; lds_used = std::max(lds_used, lds);
            break;
        }
    }
    if (nq == 0) return 0;
    qinfo.insert(qinfo.end(), heights.begin(), heights.end());
    uint2 *d_band = nullptr; uint4 *d_qinfo = nullptr; float4 *rec = nullptr; uint32_t *count = nullptr;
    /* every (shard, band) queue holds twice its mean share of a shard's lanes: 2 x lanes records of 32 bytes in total */
    const uint32_t cap = std::max<uint32_t>(1024u, (uint32_t) (2ull * I->shard_cap / nq));
    if (ws_alloc(I, &d_band, nt) || ws_alloc(I, &d_qinfo, qinfo.size()) || ws_alloc(I, &rec, (size_t) 2 * HAR_SHARDS * nq * cap) ||
        ws_alloc(I, &count, (size_t) (HAR_SHARDS * nq + 1) * HAR_COUNTER_STRIDE)) return 1;          /* + the launch's gmax word (cleared with the counters) */
    HIP_TRY(hipMemcpy(d_band, band.data(), nt * sizeof(uint2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_qinfo, qinfo.data(), qinfo.size() * sizeof(uint4), hipMemcpyHostToDevice));
    I->tq = TexelQueues{ rec, count, d_band, d_qinfo, nq, cap, count + (size_t) HAR_SHARDS * nq * HAR_COUNTER_STRIDE }; I->tq_lds = (uint32_t) lds_used;
    return 0;
}

extern "C" {

const char *har_last_error(void) { return g_error.c_str(); }

const char *har_device_arch(void) {
    static thread_local std::string arch;
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return nullptr;
    arch = prop.gcnArchName;
    return arch.c_str();
}

} // extern "C"
