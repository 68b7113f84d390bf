/*
 * seed_model.cpp -- host model of the SEEDED closest-hit launches (Accel::top_seed, har_accel.h) next to the parent's, driven by tools/seed_model.py.
 * The product's own host code lowers the scene and walks the paths (raygen_lane / shade_lane); for the closest-hit rays of every bounce >= 1 the steps of
 * Traversal<0> are recorded twice -- begin() in the order the scene was lowered with (parent) and top_seed_hit() + begin_seeded() -- and both event lists go
 * through the same lock-step model of the persistent kernel: waves of 64 lanes that draw 128-ray batches and refill when `refill` lanes are idle; a wave step
 * issues a node block when any lane visits a node, a triangle block when any lane tests one, an instance block when any lane enters one.  The seeded variant
 * adds its prologue: one pass of `top_count` full-wave triangle tests per 64 rays of a batch.  Model tool only; nothing of the shipped library uses it.
 */
#include "../mitsuba3_amd/csrc/har_cpu.h"
#include "../mitsuba3_amd/csrc/har_path.h"
#include "../mitsuba3_amd/csrc/har_scene_host.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace har;

namespace {
struct HostStack {
    static constexpr int Capacity = 24;
    uint32_t x[Capacity], y[Capacity];
    void push(int l, uint32_t a, uint32_t b) { x[l] = a; y[l] = b; }
    void pop(int l, uint32_t &a, uint32_t &b) { a = x[l]; b = y[l]; }
};
struct EvProbe : NoProbe {
    std::vector<uint32_t> *ev;     /* one entry per step: bit 0 node visit, bit 1 instance entry, bits 8.. triangle tests */
    explicit EvProbe(std::vector<uint32_t> *e) : ev(e) {}
    void iter() { ev->push_back(0u); }
    void node() { ev->back() |= 1u; }
    void inst() { ev->back() |= 2u; }
    void tri()  { ev->back() += 256u; }
};
struct MScene { HostScene hs; std::vector<DTexture> dtex; DScene ds; };

/* out: 0 rays, 1 steps, 2 node blocks, 3 triangle blocks, 4 instance blocks, 5 waves, 6 prologue passes (64 rays each), 7 node visits, 8 triangle tests, 9 instance entries */
void account(const std::vector<std::vector<uint32_t>> &evs, int refill, bool seeded, double *q) {
    const size_t n = evs.size();
    const size_t W = std::max<size_t>(1, std::min<size_t>(n / 1024, 4096));
    for (size_t w = 0; w < W; ++w) {
        size_t ray[64], pos[64]; bool busy[64]; for (int l = 0; l < 64; ++l) busy[l] = false;
        size_t pool = 0, pool_end = 0, cursor = 0; bool exhausted = false;
        q[5] += 1;
        for (;;) {
            int idle = 0; for (int l = 0; l < 64; ++l) idle += !busy[l];
            if (idle >= refill) {
                for (int l = 0; l < 64; ++l) {
                    if (busy[l]) continue;
                    if (pool == pool_end && !exhausted) {
                        const size_t b = w + W * cursor++;
                        if (b * 128 >= n) exhausted = true;
                        else { pool = b * 128; pool_end = std::min(n, pool + 128); if (seeded) q[6] += (double) ((pool_end - pool + 63) / 64); }
                    }
                    if (pool < pool_end) { busy[l] = true; ray[l] = pool++; pos[l] = 0; }
                }
                idle = 0; for (int l = 0; l < 64; ++l) idle += !busy[l];
                if (idle == 64) break;
            }
            uint32_t anyn = 0, anyi = 0, mt = 0;
            for (int l = 0; l < 64; ++l) if (busy[l]) {
                const uint32_t v = evs[ray[l]][pos[l]++];
                anyn |= v & 1u; anyi |= (v >> 1) & 1u; mt = std::max(mt, v >> 8);
                if (pos[l] == evs[ray[l]].size()) busy[l] = false;
            }
            q[1] += 1; q[2] += anyn; q[3] += mt; q[4] += anyi;
        }
    }
    for (const auto &v : evs) { q[0] += 1; for (uint32_t x : v) { q[7] += x & 1u; q[9] += (x >> 1) & 1u; q[8] += x >> 8; } }
}
}

extern "C" {

void *sm_scene_create(const HarSceneDesc *d, char *err, int errlen) {
    MScene *H = new MScene();
    std::string e;
    if (!lower_scene(*d, H->hs, e)) { snprintf(err, errlen, "%s", e.c_str()); delete H; return nullptr; }
    HostScene &hs = H->hs; DScene &S = H->ds;
    for (size_t k = 0; k < hs.textures.size(); ++k) H->dtex.push_back(hs.device_texture(k, hs.textures[k].data.data()));
    S.accel.nodes = hs.nodes.data(); S.accel.tris = hs.tris.data(); S.accel.insts = hs.inst_recs.data(); S.accel.mesh_info = nullptr;
    S.accel.root = hs.root; S.accel.has_tlas = hs.has_tlas; S.accel.n_tris = (uint32_t) hs.tris.size(); S.accel.n_insts = (uint32_t) hs.inst_recs.size();
    S.accel.top_root = hs.top_root; S.accel.top_first = hs.top_first; S.accel.top_count = hs.top_count; S.accel.top_last = hs.top_last;
    S.blas_tri_ranges = hs.blas_tri_ranges.data();
#if HAR_SHADING_TRIS
    S.shade_tris = hs.shade_tris.data();
#endif
    S.verts = hs.verts.data(); S.faces = hs.faces.data(); S.meshes = hs.meshes.data(); S.bsdfs = hs.bsdfs.data();
    S.textures = H->dtex.data(); S.emitters = hs.emitters.data(); S.insts = hs.insts.data(); S.bsdf_tables = hs.bsdf_tables.data();
    S.n_emitters = (uint32_t) hs.emitters.size(); S.n_meshes = (uint32_t) hs.meshes.size();
    S.n_bsdfs = (uint32_t) hs.bsdfs.size(); S.n_insts = (uint32_t) hs.insts.size(); S.n_textures = (uint32_t) hs.textures.size();
    S.env_emitter = hs.env_emitter;
    S.bsdf_types = 0; for (const DBsdf &b : hs.bsdfs) S.bsdf_types |= (1u << b.type) | ((b.flags & BF_TWOSIDED) ? 0x80000000u : 0u);
    S.envmap = nullptr; S.emitter_cdf = hs.emitter_cdf.data();
    hs.bind_tables(S, hs.emitter_distr.data());
    if (hs.has_mesh_emitters || hs.has_point_emitters || !hs.emitter_distr.empty()) S.bsdf_types |= HAR_SCENE_ENVMAP;
    return H;
}
void sm_scene_destroy(void *h) { delete (MScene *) h; }
uint32_t sm_top_count(void *h) { const MScene *H = (const MScene *) h; return H->ds.accel.top_root != HAR_NO_NODE ? H->ds.accel.top_count : 0u; }

/* out[2][10]: parent, seeded (see account); returns the number of rays whose two hit records differ (must be 0), or -1 */
int sm_model(void *h, const HarSensor *sensor, uint32_t seed, uint32_t spp, int32_t max_depth, int32_t rr_depth, uint64_t n_lanes, uint32_t max_bounces, int refill, double *out) {
    MScene *H = (MScene *) h; const DScene &S = H->ds; const Accel &A = S.accel;
    if (!(A.has_tlas && A.top_root != HAR_NO_NODE && A.top_count >= 1u)) return -1;
    DSensor C; std::string e; if (!lower_sensor(*sensor, C, e)) return -1;
    uint32_t log_spp = 0xffffffffu; for (uint32_t k = 0; k < 32; ++k) if ((1u << k) == spp) log_spp = k;
    ShadeParams P{ seed, (uint32_t) max_depth, (uint32_t) rr_depth };
    std::vector<PathState> cur, next; LaneSample ls;
    for (uint64_t lane = 0; lane < n_lanes; ++lane) cur.push_back(raygen_lane(C, seed, spp, log_spp, (uint32_t) lane, ls));
    int status = 0, mismatches = 0;
    for (uint32_t b = 0; b < max_bounces && !cur.empty(); ++b) {
        std::vector<std::vector<uint32_t>> ev0(cur.size()), ev1(cur.size());
        std::vector<Hit> hits(cur.size());
        next.clear();
        for (size_t i = 0; i < cur.size(); ++i) {
            { HostStack st; EvProbe pr{ &ev0[i] }; Traversal<0> T; T.begin(A, cur[i].o, cur[i].d, cur[i].maxt, (A.top_last & 2u) != 0u);
              while (!T.template step<false, HostStack, EvProbe, 2>(A, st, status, pr)) { }
              hits[i] = T.hit; }
            { HostStack st; EvProbe pr{ &ev1[i] }; Traversal<0> T; Hit sd; top_seed_hit(A, cur[i].o, cur[i].d, cur[i].maxt, sd); T.begin_seeded(A, cur[i].o, cur[i].d, cur[i].maxt, sd);
              while (!T.template step<false, HostStack, EvProbe, 2>(A, st, status, pr)) { }
              if (memcmp(&T.hit, &hits[i], sizeof(Hit)) != 0) ++mismatches; }
        }
        if (b >= 1) { account(ev0, refill, false, out); account(ev1, refill, true, out + 10); }        /* bounce 0 belongs to the packet kernel */
        for (size_t i = 0; i < cur.size(); ++i) {
            ShadeResult R; shade_lane<MODE_PATH>(S, P, cur[i], hits[i], R);
            if (R.alive) next.push_back(R.next);
        }
        cur.swap(next);
    }
    return status ? -1 : mismatches;
}

}
