/*
 * top_seed_lib.cpp -- test tool of tests/test_top_seed_cpu.py (not a product path): the seeded closest-hit query of the persistent kernel (top_seed_hit +
 * Traversal::begin_seeded, har_accel.h) stepped to the end on the host, next to the brute-force loop and the unseeded traversal, over a scene lowered by the
 * product's own host code.  Built by the test into a temporary directory together with har_scene_host.cpp and har_accel_build.cpp.
 */
#include "../../mitsuba3_amd/csrc/har_cpu.h"
#include "../../mitsuba3_amd/csrc/har_scene_host.h"
#include <cstdio>
#include <string>

using namespace har;

namespace {
struct HostStack {
    static constexpr int Capacity = 24;
    uint32_t x[Capacity], y[Capacity];
    void push(int l, uint32_t a, uint32_t b) { x[l] = a; y[l] = b; }
    void pop(int l, uint32_t &a, uint32_t &b) { a = x[l]; b = y[l]; }
};
struct Scene { HostScene hs; Accel A; };
}

extern "C" {

void *ts_scene_create(const HarSceneDesc *d, char *err, int errlen) {
    Scene *S = new Scene();
    std::string e;
    if (!lower_scene(*d, S->hs, e)) { snprintf(err, errlen, "%s", e.c_str()); delete S; return nullptr; }
    const HostScene &hs = S->hs; Accel &A = S->A;
    A.nodes = hs.nodes.data(); A.tris = hs.tris.data(); A.insts = hs.inst_recs.data(); A.mesh_info = nullptr;
    A.root = hs.root; A.has_tlas = hs.has_tlas; A.n_tris = (uint32_t) hs.tris.size(); A.n_insts = (uint32_t) hs.inst_recs.size();
    A.top_root = hs.top_root; A.top_first = hs.top_first; A.top_count = hs.top_count; A.top_last = hs.top_last;
    return S;
}
void ts_scene_destroy(void *h) { delete (Scene *) h; }

/* out: has_tlas, top-level triangles (0: none), Accel::top_seed as lowered, eligible for the automatic choice, HAR_TOP_SEED_MAX, HAR_TOP_SEED_DEFAULT */
void ts_scene_info(void *h, uint32_t out[6]) {
    const Scene *S = (const Scene *) h;
    out[0] = S->A.has_tlas; out[1] = S->A.top_root != HAR_NO_NODE ? S->A.top_count : 0u; out[2] = S->A.top_seed() ? 1u : 0u;
    out[3] = S->hs.top_seed_eligible ? 1u : 0u; out[4] = HAR_TOP_SEED_MAX; out[5] = HAR_TOP_SEED_DEFAULT;
}

/* mode 0: accel_trace_naive; 1: the seeded query (what k_trace_closest<.., SEED> does per ray); 2: the unseeded traversal in the order the scene was lowered with;
 * 3: the seed alone (top_seed_hit).  Rays as o[3][n], d[3][n].  Returns the traversal status (0, or HAR_STACK_OVERFLOW) or -1 when mode 1 / 3 is asked of a scene
 * without a TLAS or without top-level geometry. */
int ts_trace(void *h, int mode, uint32_t n, const float *o, const float *d, const float *maxt,
             float *t, float *u, float *v, uint32_t *prim, uint32_t *shape, uint32_t *inst) {
    const Scene *S = (const Scene *) h; const Accel &A = S->A; int status = 0;
    if ((mode == 1 || mode == 3) && !(A.has_tlas && A.top_root != HAR_NO_NODE && A.top_count >= 1u)) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        const Vec3 O(o[i], o[n + i], o[2 * (size_t) n + i]), D(d[i], d[n + i], d[2 * (size_t) n + i]);
        Hit hit;
        if (mode == 0) accel_trace_naive<false>(A, S->hs.blas_tri_ranges.data(), O, D, maxt[i], hit);
        else if (mode == 3) top_seed_hit(A, O, D, maxt[i], hit);
        else {
            HostStack st; Traversal<0, false> T;
            if (mode == 1) { Hit seed; top_seed_hit(A, O, D, maxt[i], seed); T.begin_seeded(A, O, D, maxt[i], seed); }
            else T.begin(A, O, D, maxt[i], (A.top_last & 2u) != 0u);
            while (!T.template step<false, HostStack, NoProbe, 0>(A, st, status)) { }
            hit = T.hit;
        }
        t[i] = hit.t; u[i] = hit.u; v[i] = hit.v; prim[i] = hit.prim; shape[i] = hit.shape; inst[i] = hit.inst;
    }
    return status;
}

}
