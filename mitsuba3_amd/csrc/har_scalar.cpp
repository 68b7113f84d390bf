/*
 * har_scalar.cpp -- BASELINE config 1 / SURVEY.md 8 row a20: the `scalar_rgb` plumbing path (CPU, no GPU).
 *
 * SamplingIntegrator::render's NON-JIT branch (src/render/integrator.cpp:190-274): block size against the thread
 * count, Spiral::next_block (src/render/spiral.cpp:27-73), render_block (integrator.cpp:398-446: Morton pixel order,
 * per-pixel reseed, `seed *= prod(film_size)`, `seed += block_id * block_size^2`), render_sample (:448-520) and
 * ImageBlock::put's scalar branch on a bordered block with the DISCRETISED reconstruction filter
 * (src/render/imageblock.cpp:228-375, include/mitsuba/core/rfilter.h:70-79, src/core/rfilter.cpp:11-26), then
 * put_block into the film (imageblock.cpp:160-186).
 *
 * This is an explicit, separately named entry point (`har_render_scalar`, Python variant 'scalar_rgb'): the
 * `hip_ad_rgb` entry points never call it and never fall back to it.  It runs the SAME path code as the HIP
 * kernels -- the HAR_HD headers compiled for the host: BVH8 traversal, compute_si, shade_lane<MODE_PATH> -- with
 * the scalar variants' draw semantics (path.cpp:226-227 `break`, :244-249 conditional emitter samples).
 */
#include "../../include/hip_ad_rgb.h"
#include "har_cpu.h"
#include "har_path.h"
#include "har_aov.h"
#include "har_normalmap_grad.h"
#include "har_bumpmap_grad.h"
#include "har_scene_host.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <exception>
#include <thread>
#include <vector>

extern int har_set_error(const std::string &msg);

namespace {

using namespace har;

struct ScalarStack {                  /* traversal stack of accel_trace (depth-first bound checked by the caller) */
    static constexpr int Capacity = 64;
    uint32_t x[Capacity], y[Capacity];
    void push(int l, uint32_t a, uint32_t b) { x[l] = a; y[l] = b; }
    void pop(int l, uint32_t &a, uint32_t &b) { a = x[l]; b = y[l]; }
};

/* host view of a lowered scene: DScene over the HostScene's own vectors */
struct BoundScene {
    HostScene hs; std::vector<DTexture> dtex; DScene ds{};
    void bind() {
        dtex.clear();
        for (size_t k = 0; k < hs.textures.size(); ++k) dtex.push_back(hs.device_texture(k, hs.textures[k].data.data()));
        DScene &S = ds;
        S.accel.nodes = hs.nodes.data(); S.accel.tris = hs.tris.data(); S.accel.insts = hs.inst_recs.data(); S.accel.mesh_info = nullptr;
        S.accel.root = hs.root; S.accel.has_tlas = hs.has_tlas; S.accel.n_tris = (uint32_t) hs.tris.size(); S.accel.n_insts = (uint32_t) hs.inst_recs.size();
        S.accel.top_root = hs.top_root; S.accel.top_first = hs.top_first; S.accel.top_count = hs.top_count; S.accel.top_last = hs.top_last;
        S.blas_tri_ranges = hs.blas_tri_ranges.data();
#if HAR_SHADING_TRIS
        S.shade_tris = hs.shade_tris.data();
#endif
        S.verts = hs.verts.data(); S.faces = hs.faces.data(); S.meshes = hs.meshes.data(); S.bsdfs = hs.bsdfs.data();
        S.textures = dtex.data(); S.emitters = hs.emitters.data(); S.insts = hs.insts.data(); S.bsdf_tables = hs.bsdf_tables.data();
        S.n_emitters = (uint32_t) hs.emitters.size(); S.n_meshes = (uint32_t) hs.meshes.size();
        S.n_bsdfs = (uint32_t) hs.bsdfs.size(); S.n_insts = (uint32_t) hs.insts.size(); S.n_textures = (uint32_t) hs.textures.size();
        S.env_emitter = hs.env_emitter;
        S.bsdf_types = 0; for (const DBsdf &b : hs.bsdfs) S.bsdf_types |= bsdf_scene_bit(b.type) | ((b.flags & BF_TWOSIDED) ? 0x80000000u : 0u);
        for (const HostTexture &t : hs.textures) if (t.mode & HAR_TEX_ATTRIBUTE) S.bsdf_types |= HAR_SCENE_ATTR;
        for (const DBsdf &b : hs.bsdfs) if (b.type == BSDF_ROUGHCONDUCTOR && (b.flags & BF_ALPHA_TEX)) S.bsdf_types |= HAR_SCENE_ALPHAMAP;
        S.envmap = nullptr; S.emitter_cdf = hs.emitter_cdf.data();
        hs.bind_tables(S, hs.emitter_distr.data());
        if (hs.has_mesh_emitters || hs.has_point_emitters || !hs.emitter_distr.empty()) S.bsdf_types |= HAR_SCENE_ENVMAP;
        if (hs.has_envmap) { hs.envmap.tex = hs.env_tex.data(); hs.envmap.warp = hs.env_warp.data(); S.envmap = &hs.envmap; S.bsdf_types |= HAR_SCENE_ENVMAP; }
    }
};

/* dr::morton_decode<Point2u>: even bits -> x, odd bits -> y */
inline uint32_t compact_bits(uint32_t v) {
    v &= 0x55555555u; v = (v | (v >> 1)) & 0x33333333u; v = (v | (v >> 2)) & 0x0f0f0f0fu; v = (v | (v >> 4)) & 0x00ff00ffu; v = (v | (v >> 8)) & 0x0000ffffu;
    return v;
}

struct Block { int32_t off_x, off_y; uint32_t size_x, size_y, id; };

/* Spiral (src/render/spiral.cpp): blocks of one pass in the order next_block() hands them out */
std::vector<Block> spiral(uint32_t w, uint32_t h, uint32_t off_x, uint32_t off_y, uint32_t bs) {
    const int32_t nbx = (int32_t) ((w + bs - 1) / bs), nby = (int32_t) ((h + bs - 1) / bs);
    const uint32_t count = (uint32_t) (nbx * nby);
    std::vector<Block> out; out.reserve(count);
    int32_t px = nbx / 2, py = nby / 2; int dir = 0 /* right, down, left, up */; uint32_t steps_left = 1, spiral_size = 1;
    for (uint32_t k = 0; k < count; ++k) {
        Block b; b.id = k;
        const uint32_t ox = (uint32_t) px * bs, oy = (uint32_t) py * bs;
        b.size_x = std::min(bs, w - ox); b.size_y = std::min(bs, h - oy); b.off_x = (int32_t) (ox + off_x); b.off_y = (int32_t) (oy + off_y);
        out.push_back(b);
        if (k + 1 == count) break;
        do {
            if (dir == 0) ++px; else if (dir == 1) ++py; else if (dir == 2) --px; else --py;
            if (--steps_left == 0) {
                dir = (dir + 1) % 4;
                if (dir == 0 || dir == 2) ++spiral_size;
                steps_left = spiral_size;
            }
        } while (px < 0 || py < 0 || px >= nbx || py >= nby);
    }
    return out;
}

/* PathIntegrator::sample, scalar variant, on the host-compiled path code: radiance + valid_ray */
Vec3 sample_scalar(const DScene &S, const ShadeParams &P, uint64_t &rng, Vec3 o, Vec3 d, float maxt, bool &valid_ray, int &status, uint32_t lane = 0u, HarStats *stats = nullptr) {
    Vec3 result(0.f);
    valid_ray = S.env_emitter >= 0;                               /* path.cpp:114-115 (hide_emitters is refused by the caller) */
    if (P.max_depth == 0) return result;                          /* path.cpp:102-103 */
    PathState st; st.o = o; st.d = d; st.maxt = maxt; st.throughput = Vec3(1.f); st.rng = rng; st.lane = lane; st.prev_p = Vec3(0.f); st.prev_bsdf_pdf = 1.f;
    st.flags = 1u << 16; st.eta = 1.f;
    for (;;) {
        Hit hit; ScalarStack stack;
        accel_trace<false>(S.accel, st.o, st.d, st.maxt, hit, stack, status);
        if (stats) { stats->vertices++; stats->closest_rays++; }   /* one loop iteration of PathIntegrator::sample: what the wavefront's bounce counters add up to */
        ShadeResult R;
        R.next.rng = st.rng;                                      /* a path that ends before this iteration's draws (path.cpp:226-227 `break`) leaves the stream where it is */
        if (S.bsdf_types & HAR_SCENE_THIN) shade_lane<MODE_PATH, HAR_SCENE_THIN_TYPES>(S, P, st, hit, R);      /* a thin dielectric: the roughness-map set plus the thin leaf and the null-lobe bookkeeping by lobe type */
        else if (S.bsdf_types & HAR_SCENE_ALPHAMAP) shade_lane<MODE_PATH, HAR_SCENE_ALPHAMAP_TYPES>(S, P, st, hit, R);      /* a roughness map: the bumpmap set plus the lookup (no `mesh_attribute` texture next to it) */
        else if (S.bsdf_types & HAR_SCENE_ATTR) shade_lane<MODE_PATH, HAR_SCENE_ATTR_TYPES>(S, P, st, hit, R);        /* only scenes with a `mesh_attribute` texture solve the barycentrics */
        else if (S.bsdf_types & HAR_SCENE_BUMPMAP) shade_lane<MODE_PATH, HAR_SCENE_BUMPMAP_TYPES>(S, P, st, hit, R);      /* ... with a `bumpmap` record the bump frame as well */
        else if (S.bsdf_types & HAR_SCENE_NORMALMAP) shade_lane<MODE_PATH, HAR_SCENE_NORMALMAP_TYPES>(S, P, st, hit, R);      /* ... with a `normalmap` record the perturbed and the tangent frames */
        else shade_lane<MODE_PATH, HAR_SCENE_MASK_TYPES>(S, P, st, hit, R);
        /* path.cpp:307-308; in a scene with a `mask` record the vertex decides (a null lobe does not make the sample valid: ShadeResult::non_null, which also follows the
         * scalar branch's early exit, :227-231, where HAR_SHADE_SCALAR_DRAWS is set) */
        valid_ray = valid_ray || ((S.bsdf_types & (HAR_SCENE_MASK | HAR_SCENE_THIN)) ? R.non_null : hit.t != HAR_INF);
        if (R.add_emission) result = Vec3(fma_(R.em_a.x, R.em_b.x, result.x), fma_(R.em_a.y, R.em_b.y, result.y), fma_(R.em_a.z, R.em_b.z, result.z));
        if (R.item && R.item_ray) {                                /* the emitter sample's shadow ray (path.cpp:271-281; ray_test inside sample_emitter_direction) */
            Hit h2; ScalarStack s2;
            if (stats) stats->shadow_rays++;
            if (!accel_trace<true>(S.accel, R.sh_o, R.sh_d, R.sh_maxt, h2, s2, status)) result = fma3(st.throughput, R.contrib_b, result);      /* path.cpp:279 */
        }
        if (!R.alive) { rng = R.next.rng; break; }
        st = R.next;
    }
    return valid_ray ? result : Vec3(0.f);                        /* path.cpp:341-345 */
}

} // namespace

extern "C" int har_render_scalar(const HarSceneDesc *desc, const HarSensor *sensor, uint32_t seed, uint32_t spp, int32_t max_depth, int32_t rr_depth,
                                 uint32_t block_size, uint32_t n_threads, float *film, uint32_t *block_size_used) {
    try {
        if (!desc || !sensor || !film) return har_set_error("null argument");
        if (spp == 0) return har_set_error("spp must be > 0");
        if (max_depth < 0 && max_depth != -1) return har_set_error("\"max_depth\" must be set to -1 (infinite) or a value >= 0");
        if (rr_depth <= 0) return har_set_error("\"rr_depth\" must be set to a value greater than zero!");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        if (B.hs.stack_need() > (uint32_t) ScalarStack::Capacity) return har_set_error("scene too deep for the scalar traversal stack");
        B.bind();
        DSensor C;
        if (!lower_sensor(*sensor, C, e)) return har_set_error(e);
        if (C.projection == 2u) return har_set_error("scalar_rgb: the `thinlens` sensor is not implemented by the scalar_rgb variant (hip_ad_rgb only)");
        const DScene &S = B.ds;
        const uint32_t W = C.crop_w, H = C.crop_h;
        /* Film::sample_border: the spiral runs over the enlarged film, every block is shifted back by the border (integrator.cpp:162-165, 248-249) */
        const uint32_t Wg = C.samp_w, Hg = C.samp_h; const int32_t sample_shift = (int32_t) C.border;
        if (n_threads == 0) n_threads = har_usable_cores();         /* affinity mask and container quota, not the machine's CPU count */

        /* ReconstructionFilter::init_discretization (rfilter.cpp:11-26) */
        constexpr int RES = 31;                                   /* MI_FILTER_RESOLUTION */
        const bool box = C.rfilter == 0;
        const float radius = box ? .5f : C.radius;
        float values[RES + 1];
        for (int i = 0; i < RES; ++i) { const float x = (radius * (float) i) / (float) RES; values[i] = box ? (x <= .5f ? 1.f : 0.f) : rfilter_eval(C, x); }
        values[RES] = 0.f;
        const float scale_factor = (float) RES / radius;
        const int border = (int) std::ceil(radius - .5f - 2.f * HAR_RAY_EPS);
        auto eval_discretized = [&](float x) { const uint32_t idx = std::min<uint32_t>((uint32_t) std::fabs(x * scale_factor), (uint32_t) RES); return values[idx]; };

        /* integrator.cpp:203-214: a block for every thread */
        if (block_size == 0) {
            block_size = 32;                                      /* MI_BLOCK_SIZE */
            while (!(block_size == 1 || ((Wg + block_size - 1) / block_size) * ((Hg + block_size - 1) / block_size) >= n_threads)) block_size /= 2;
        }
        if (block_size_used) *block_size_used = block_size;
        std::vector<Block> blocks = spiral(Wg, Hg, C.crop_x, C.crop_y, block_size);
        for (Block &b : blocks) { b.off_x -= sample_shift; b.off_y -= sample_shift; }
        const uint32_t seed_scaled = seed * (Wg * Hg);              /* integrator.cpp:231: seed *= prod(film_size), film_size = crop_size (:162) */
        const ShadeParams P0{ 0u, (uint32_t) max_depth, (uint32_t) rr_depth, HAR_SHADE_SCALAR_DRAWS };

        std::mutex film_mutex; std::atomic<uint32_t> next(0); std::atomic<int> status_all(0);
        std::exception_ptr worker_error; std::mutex error_mutex;
        auto worker_body = [&]() {
            std::vector<float> blk; ShadeParams P = P0;            /* per worker: P.seed names the current pixel's stream */
            for (;;) {
                if (status_all.load()) break;                     /* an overflow reported by any worker ends the render early */
                const uint32_t bi = next.fetch_add(1);
                if (bi >= blocks.size()) break;
                const Block &b = blocks[bi];
                /* ImageBlock(size, border = true): (size + 2 * border)^2 x {R, G, B, W}, cleared (integrator.cpp:419) */
                const uint32_t bw = b.size_x + 2u * (uint32_t) border, bh = b.size_y + 2u * (uint32_t) border;
                blk.assign((size_t) bw * bh * 4, 0.f);
                const uint32_t bseed = seed_scaled + b.id * block_size * block_size;          /* integrator.cpp:412 */
                int status = 0;
                for (uint32_t i = 0; i < block_size * block_size; ++i) {
                    /* sampler->seed(seed + i) with a wavefront of one lane: Sampler::seed (sampler.cpp:129-148), lane index 0 */
                    uint64_t rng, inc; sampler_seed(bseed + i, 0u, rng, inc);
                    const uint32_t px = compact_bits(i), py = compact_bits(i >> 1);
                    if (px >= b.size_x || py >= b.size_y) continue;
                    const float pos_x = (float) ((int32_t) px + b.off_x), pos_y = (float) ((int32_t) py + b.off_y);
                    for (uint32_t j = 0; j < spp; ++j) {
                        /* render_sample (integrator.cpp:448-520) */
                        const float jx = pcg32_next_float(rng, inc), jy = pcg32_next_float(rng, inc);
                        const float spx = pos_x + jx, spy = pos_y + jy;
                        const float sx = 1.f / (float) W, sy = 1.f / (float) H;
                        Vec3 o, d; float maxt;
                        /* the pinhole models only: projection 2 was refused above (sensor_sample_ray would read the lens parameters as principal point offsets) */
                        sensor_sample_ray(C, fma_(spx, sx, -(float) C.crop_x * sx), fma_(spy, sy, -(float) C.crop_y * sy), o, d, maxt);
                        P.seed = bseed + i;                       /* the stream's increment is a function of (seed value, lane 0) */
                        bool valid = false;
                        const Vec3 rgb = sample_scalar(S, P, rng, o, d, maxt, valid, status);
                        const float v[4] = { rgb.x, rgb.y, rgb.z, 1.f };
                        /* block->put(box_filter ? pos : sample_pos, aovs) */
                        const float ppx = box ? pos_x : spx, ppy = box ? pos_y : spy;
                        if (box) {                                /* imageblock.cpp:228-250 (no filter object) -- the film hands box-filtered blocks no rfilter */
                            const int32_t x = (int32_t) std::floor(ppx) - b.off_x + border, y = (int32_t) std::floor(ppy) - b.off_y + border;
                            if ((uint32_t) x < bw && (uint32_t) y < bh) { float *p = blk.data() + 4 * ((size_t) y * bw + x); for (int k = 0; k < 4; ++k) p[k] += v[k]; }
                            continue;
                        }
                        const float pfx = ppx + ((float) border - (float) b.off_x - .5f), pfy = ppy + ((float) border - (float) b.off_y - .5f);
                        const int32_t x0 = std::max((int32_t) std::ceil(pfx - radius), 0), y0 = std::max((int32_t) std::ceil(pfy - radius), 0);
                        const int32_t x1 = std::min((int32_t) std::floor(pfx + radius), (int32_t) bw - 1), y1 = std::min((int32_t) std::floor(pfy + radius), (int32_t) bh - 1);
                        if (x0 > x1 || y0 > y1) continue;
                        float wx[32], wy[32];
                        const int cx = x1 - x0 + 1, cy = y1 - y0 + 1;
                        if (cx > 32 || cy > 32) { status = HAR_STACK_OVERFLOW; continue; }
                        float relx = (float) x0 - pfx, rely = (float) y0 - pfy;
                        for (int k = 0; k < cx; ++k) { wx[k] = eval_discretized(relx); relx += 1.f; }
                        for (int k = 0; k < cy; ++k) { wy[k] = eval_discretized(rely); rely += 1.f; }
                        for (int yy = 0; yy < cy; ++yy)
                            for (int xx = 0; xx < cx; ++xx) {
                                const float w = wx[xx] * wy[yy];
                                float *p = blk.data() + 4 * ((size_t) (y0 + yy) * bw + (x0 + xx));
                                for (int k = 0; k < 4; ++k) p[k] = fma_(v[k], w, p[k]);
                            }
                    }
                }
                if (status) status_all.store(status);
                /* film->put_block (imageblock.cpp:160-186): the bordered block is added where it overlaps the crop window */
                std::lock_guard<std::mutex> lock(film_mutex);
                for (uint32_t y = 0; y < bh; ++y) {
                    const int32_t fy = b.off_y - border + (int32_t) y - (int32_t) C.crop_y;
                    if ((uint32_t) fy >= H) continue;
                    for (uint32_t x = 0; x < bw; ++x) {
                        const int32_t fx = b.off_x - border + (int32_t) x - (int32_t) C.crop_x;
                        if ((uint32_t) fx >= W) continue;
                        const float *src = blk.data() + 4 * ((size_t) y * bw + x); float *dst = film + 4 * ((size_t) fy * W + (size_t) fx);
                        for (int k = 0; k < 4; ++k) dst[k] += src[k];
                    }
                }
            }
        };
        /* an exception in a pool thread (std::bad_alloc of a block buffer) must not reach std::terminate: it is kept, the other workers stop at
         * their next block, and the calling thread rethrows it after the join (into the catch clauses below) */
        auto worker = [&]() {
            try { worker_body(); }
            catch (...) {
                std::lock_guard<std::mutex> lock(error_mutex);
                if (!worker_error) worker_error = std::current_exception();
                next.store((uint32_t) blocks.size());
            }
        };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < n_threads; ++t) { try { pool.emplace_back(worker); } catch (...) { break; } }
        worker();
        for (auto &t : pool) t.join();
        if (worker_error) std::rethrow_exception(worker_error);
        if (status_all.load()) return har_set_error("scalar render: traversal stack / filter footprint overflow");
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_render_scalar: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_render_scalar: ") + ex.what()); }
}

/* AOVIntegratorImpl::sample (src/integrators/aov.cpp:175-306) on the host: the scene lowered as above, accel_trace for the closest hit, aov_lane (har_aov.h) -- the
 * function the kernels of har_aov.hip run -- for the channels.  The twin of har_aov_sample: a test of the feature without a GPU, and the other side of the
 * device / host bit comparison. */
extern "C" int har_aov_sample_host(const HarSceneDesc *desc, uint32_t n, const float *o, const float *d, const float *maxt, const uint8_t *active, uint32_t n_aovs,
                                   const uint32_t *types, float *out) {
    try {
        if (!desc) return har_set_error("null argument");
        AovSpec spec;
        if (const char *e = aov_spec_lower(n_aovs, types, spec)) return har_set_error(e);
        if (n == 0 || spec.channels == 0) return 0;
        if (!o || !d || !maxt || !out) return har_set_error("null ray / output array");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        if (B.hs.stack_need() > (uint32_t) ScalarStack::Capacity) return har_set_error("scene too deep for the scalar traversal stack");
        B.bind();
        const DScene &S = B.ds;
        int status = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const Vec3 O(o[i], o[n + i], o[2 * (size_t) n + i]), D(d[i], d[n + i], d[2 * (size_t) n + i]);
            const bool act = !(active && !active[i]);
            Hit hit; hit.t = HAR_INF; hit.u = 0.f; hit.v = 0.f; hit.prim = 0; hit.shape = 0; hit.inst = 0xffffffffu;
            if (act) { ScalarStack stack; accel_trace<false>(S.accel, O, D, maxt[i], hit, stack, status); }
            if (S.bsdf_types & HAR_SCENE_ATTR) aov_lane<HAR_SCENE_WIDEST>(S, spec, B.hs.top_mesh_count, D, hit, act, out + i, (size_t) n);
            else if (S.bsdf_types & HAR_SCENE_BUMPMAP) aov_lane<HAR_SCENE_RECORD_BITS>(S, spec, B.hs.top_mesh_count, D, hit, act, out + i, (size_t) n);
            else if (S.bsdf_types & HAR_SCENE_NORMALMAP) aov_lane<HAR_SCENE_NMAP_RECORD_BITS>(S, spec, B.hs.top_mesh_count, D, hit, act, out + i, (size_t) n);
            else aov_lane<HAR_SCENE_COMPOSITE>(S, spec, B.hs.top_mesh_count, D, hit, act, out + i, (size_t) n);
        }
        if (status) return har_set_error("har_aov_sample_host: traversal stack overflow");
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_aov_sample_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_aov_sample_host: ") + ex.what()); }
}

/* PreliminaryIntersection::compute_surface_interaction on the host for n given hits (t, prim_uv, prim, shape, inst as Scene::ray_intersect_preliminary returns them;
 * d = the ray directions, 3 x n): the 33 rows of har_compute_surface_interaction, by the function its kernel runs in a scene with a `normalmap` record (si_rows_tangent:
 * compute_si + the tangent frame of the shapes that pack one; for every other shape that IS compute_si).  The twin of that entry: the frames without a GPU. */
extern "C" int har_surface_interaction_host(const HarSceneDesc *desc, uint32_t n, const float *d, const float *t, const float *u, const float *v, const uint32_t *prim,
                                            const uint32_t *shape, const uint32_t *inst, uint32_t ray_flags, const uint8_t *active, float *out) {
    try {
        if (!desc) return har_set_error("null argument");
        if (ray_flags & ~(uint32_t) RAY_KNOWN_FLAGS) return har_set_error("unknown RayFlags bits");
        if (n == 0) return 0;
        if (!d || !t || !u || !v || !prim || !shape || !inst || !out) return har_set_error("null input / output arrays");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        const DScene &S = B.ds;
        for (uint32_t i = 0; i < n; ++i) {
            const bool act = !(active && !active[i]);
            if (act && t[i] != HAR_INF) {
                if (shape[i] >= S.n_meshes || prim[i] >= S.meshes[shape[i]].face_count || (inst[i] != 0xffffffffu && inst[i] >= S.n_insts)) return har_set_error("har_surface_interaction_host: hit record out of bounds");
            }
            si_rows_tangent(S, n, i, Vec3(d[i], d[n + i], d[2 * (size_t) n + i]), t[i], u[i], v[i], prim[i], shape[i], inst[i], ray_flags, act, out);
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_surface_interaction_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_surface_interaction_host: ") + ex.what()); }
}

/* d F / d c of a `normalmap` record on the host (normalmap_weighted_value_grad, har_normalmap_grad.h): n tuples (wi 3 x n, uv 2 x n, wo 3 x n, A 3 x n) on record
 * `bsdf` -- a normalmap record, possibly under an outer one-BSDF `twosided` --, c = the record's colour looked up at uv.  value (n, may be NULL) = F = sum_k A_k value_k,
 * grad (3 x n) = the three partials with respect to the looked-up colour.  Default context. */
extern "C" int har_normalmap_grad_host(const HarSceneDesc *desc, uint32_t bsdf, uint32_t n, const float *wi, const float *uv, const float *wo, const float *A,
                                       float *value, float *grad) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.hs.bsdfs[bsdf].type != BSDF_NORMALMAP) return har_set_error("har_normalmap_grad_host: not a normalmap record");
        if (n == 0) return 0;
        if (!wi || !uv || !wo || !A || !grad) return har_set_error("null input / output arrays");
        const DScene &S = B.ds;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t i1 = n + (size_t) i, i2 = 2 * (size_t) n + i;
            float dc[3] = { 0.f, 0.f, 0.f }, f = 0.f;
            BsdfSide side;
            if (bsdf_side(S, bsdf, Vec3(wi[i], wi[i1], wi[i2]), side)) {
                TexTaps taps; const BsdfInputs in = bsdf_inputs(S, S.bsdfs[side.index], uv[i], uv[i1], taps);
                f = normalmap_weighted_value_grad<HAR_SCENE_ALPHAMAP>(S, S.bsdfs[side.index], in.slot0, side.wi, Vec3(wo[i], wo[i1], wo[i2] * side.wo_sign), uv[i], uv[i1], Vec3(A[i], A[i1], A[i2]), dc);
            }
            if (value) value[i] = f;
            grad[i] = dc[0]; grad[i1] = dc[1]; grad[i2] = dc[2];
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_normalmap_grad_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_normalmap_grad_host: ") + ex.what()); }
}

/* The twins of har_bsdf_eval_pdf_si / har_bsdf_sample_si: the lane functions their kernels run (bsdf_eval_pdf_si_lane / bsdf_sample_si_lane, har_scene.h) over HOST arrays;
 * geom = 18 x n (si.n, sh_frame.n, .s, .t, dp_du, dp_dv), read for a bumpmap record */
extern "C" int har_bsdf_eval_pdf_si_host(const HarSceneDesc *desc, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo,
                                         const float *geom, const uint8_t *active, float *value, float *pdf) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.ds.bsdf_types & HAR_SCENE_ATTR) return har_set_error("mesh_attribute: BSDF::eval / pdf / sample see a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
        BsdfCtx c; c = BsdfCtx();
        if (ctx) { if (ctx->mode > 1u) return har_set_error("HarBSDFContext::mode must be 0 (TransportMode::Radiance) or 1 (TransportMode::Importance)"); c.mode = ctx->mode; c.type_mask = ctx->type_mask; c.component = ctx->component; }
        if (n == 0) return 0;
        if (!wi || !uv || !wo || !geom) return har_set_error("null input arrays");
        for (uint32_t i = 0; i < n; ++i) bsdf_eval_pdf_si_lane<HAR_SCENE_ALPHAMAP | HAR_SCENE_THIN>(B.ds, bsdf, c, n, i, wi, uv, wo, geom, !(active && !active[i]), value, pdf);
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bsdf_eval_pdf_si_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bsdf_eval_pdf_si_host: ") + ex.what()); }
}
extern "C" int har_bsdf_sample_si_host(const HarSceneDesc *desc, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *sample1,
                                       const float *sample2, const float *geom, const uint8_t *active, float *wo, float *pdf, float *weight, float *eta,
                                       uint32_t *sampled_type, uint32_t *sampled_component) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.ds.bsdf_types & HAR_SCENE_ATTR) return har_set_error("mesh_attribute: BSDF::eval / pdf / sample see a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
        BsdfCtx c; c = BsdfCtx();
        if (ctx) { if (ctx->mode > 1u) return har_set_error("HarBSDFContext::mode must be 0 (TransportMode::Radiance) or 1 (TransportMode::Importance)"); c.mode = ctx->mode; c.type_mask = ctx->type_mask; c.component = ctx->component; }
        if (n == 0) return 0;
        if (!wi || !uv || !sample2 || !geom || !wo || !pdf || !weight) return har_set_error("null input / output arrays");
        for (uint32_t i = 0; i < n; ++i) bsdf_sample_si_lane<HAR_SCENE_ALPHAMAP | HAR_SCENE_THIN>(B.ds, bsdf, c, n, i, wi, uv, sample1, sample2, geom, !(active && !active[i]), wo, pdf, weight, eta, sampled_type, sampled_component);
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bsdf_sample_si_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bsdf_sample_si_host: ") + ex.what()); }
}

/* BitmapTexture::eval_1_grad and its transpose on the host, by the functions the kernels run (tex_eval_1_grad, tex_eval_1_grad_transpose): n lookups of texture record
 * `texture` -- a bitmap; HAR_BSDF_MONO among the flags of a BSDF record that names it: ONE channel, else the luminance of three -- at uv (2 x n).  grad (2 x n) = the
 * gradient with respect to the surface's uv, WITHOUT a bump map's `scale`.  With g (2 x n) and deposit (h x w x 3, ACCUMULATED into; both or neither) the adjoint:
 * deposit += the four signed tap weights of (g_u, g_v) at every lookup, times the channel's luminance coefficient (one channel: into channel 0). */
extern "C" int har_texture_eval_1_grad_host(const HarSceneDesc *desc, uint32_t texture, uint32_t n, const float *uv, float *grad, const float *g, float *deposit) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        const DScene &S = B.ds;
        if (texture >= S.n_textures) return har_set_error("invalid texture index");
        const DTexture T = S.textures[texture];
        if (T.mode & HAR_TEX_ATTRIBUTE) return har_set_error("eval_1_grad: not a bitmap texture (a `mesh_attribute` record)");
        bool mono = false; for (const DBsdf &b : B.hs.bsdfs) if (b.texture == (int32_t) texture && (b.flags & BF_MONO)) mono = true;
        if (n == 0) return 0;
        if (!uv || !grad || (!g != !deposit)) return har_set_error("null input / output arrays");
        const Vec3 ch = tex_eval_1_grad_channels(mono);
        for (uint32_t i = 0; i < n; ++i) {
            float gu, gv; tex_eval_1_grad(T, mono, uv[i], uv[n + (size_t) i], gu, gv);
            grad[i] = gu; grad[n + (size_t) i] = gv;
            if (g) {
                TexTaps l; float w[4]; tex_eval_1_grad_transpose(T, uv[i], uv[n + (size_t) i], g[i], g[n + (size_t) i], 1.f, l, w);
                for (int k = 0; k < 4; ++k) { float *q = deposit + 3 * (size_t) l.idx[k]; q[0] += ch.x * w[k]; q[1] += ch.y * w[k]; q[2] += ch.z * w[k]; }
            }
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_texture_eval_1_grad_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_texture_eval_1_grad_host: ") + ex.what()); }
}

/* d F / d grad_uv of a `bumpmap` record on the host (bumpmap_weighted_value_grad, har_bumpmap_grad.h): n tuples (wi 3 x n, uv 2 x n, wo 3 x n, geom 18 x n, A 3 x n) on
 * record `bsdf` -- a bumpmap record, possibly under an outer one-BSDF `twosided`.  grad_uv (2 x n, may be NULL) overrides scale * eval_1_grad of the record's height map
 * at uv (for finite differences in grad_uv).  value (n, may be NULL) = F = sum_k A_k value_k, grad (2 x n) = the two partials.  Default context. */
extern "C" int har_bumpmap_grad_host(const HarSceneDesc *desc, uint32_t bsdf, uint32_t n, const float *wi, const float *uv, const float *wo, const float *geom, const float *A,
                                     const float *grad_uv, float *value, float *grad) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.hs.bsdfs[bsdf].type != BSDF_BUMPMAP) return har_set_error("har_bumpmap_grad_host: not a bumpmap record");
        if (n == 0) return 0;
        if (!wi || !uv || !wo || !geom || !A || !grad) return har_set_error("null input / output arrays");
        const DScene &S = B.ds;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t i1 = n + (size_t) i, i2 = 2 * (size_t) n + i;
            float dg[2] = { 0.f, 0.f }, f = 0.f;
            BsdfSide side;
            if (bsdf_side(S, bsdf, Vec3(wi[i], wi[i1], wi[i2]), side)) {
                const DBsdf &R = S.bsdfs[side.index];
                BumpGeom G = bump_geom_rows(S, R, n, i, geom, uv[i], uv[i1]);
                if (grad_uv) { G.gx = grad_uv[i]; G.gy = grad_uv[i1]; }
                f = bumpmap_weighted_value_grad(S, R, G, G.gx, G.gy, side.wi, Vec3(wo[i], wo[i1], wo[i2] * side.wo_sign), uv[i], uv[i1], Vec3(A[i], A[i1], A[i2]), dg);
            }
            if (value) value[i] = f;
            grad[i] = dg[0]; grad[i1] = dg[1];
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bumpmap_grad_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bumpmap_grad_host: ") + ex.what()); }
}

/* The lookup of a `mesh_attribute` record and its transpose on the host, by the functions the kernels run (attr_addr, attr_taps, attr_fetch, tap_weights): n hits on the
 * record's mesh, face `prim[i]` at point p (3 x n).  value (3 x n, may be NULL) = the looked-up colour; with g (3 x n) and grad (rows x 3, ACCUMULATED into) the deposit of
 * the in-place commit: grad[row_k] += g * b_k * scale for the three rows of the lookup (a face attribute: its row, weight scale) */
extern "C" int har_attribute_lookup_host(const HarSceneDesc *desc, uint32_t texture, uint32_t n, const uint32_t *prim, const float *p, float *value, const float *g, float *grad) {
    try {
        if (!desc || (n && (!prim || !p)) || (!g != !grad)) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (texture >= B.hs.textures.size() || !(B.hs.textures[texture].mode & HAR_TEX_ATTRIBUTE)) return har_set_error("mesh_attribute: not a HAR_TEX_MESH_ATTRIBUTE record");
        const DScene &S = B.ds; const DTexture T = S.textures[texture]; const uint32_t shape = B.hs.textures[texture].mesh;
        for (uint32_t i = 0; i < n; ++i) {
            if (prim[i] >= S.meshes[shape].face_count) return har_set_error("mesh_attribute: face index out of bounds");
            const AttrAddr a = attr_addr(S, Vec3(p[i], p[n + i], p[2 * (size_t) n + i]), prim[i], shape);
            TexTaps taps; attr_taps(S, T, a, taps);
            if (value) { const Vec3 v = attr_fetch(T, taps); value[i] = v.x; value[n + i] = v.y; value[2 * (size_t) n + i] = v.z; }
            if (grad) {
                float w[4]; tap_weights(taps, true, w);
                for (int k = 0; k < 3; ++k) for (int c = 0; c < 3; ++c) grad[3 * (size_t) taps.idx[k] + c] += g[c * (size_t) n + i] * w[k];
            }
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_attribute_lookup_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_attribute_lookup_host: ") + ex.what()); }
}

/* The lookup of the environment map and its transpose on the host, by the functions the kernels run (envmap_taps, envmap_eval_uv): n lookups at uv (2 x n).  idx / weight
 * (4 x n): the taps in the REAL image; value (3 x n) = scale * sum_k w_k image[idx_k]; eval (3 x n) = envmap_eval_uv; with g (3 x n) and grad (h x w x 3, ACCUMULATED into)
 * the deposit of the in-place commit under HAR_SHADE_ENV_TEXELS: grad[idx_k] += g * w_k */
extern "C" int har_envmap_taps_host(const HarSceneDesc *desc, uint32_t n, const float *uv, uint32_t *idx, float *weight, float *value, float *eval, const float *g, float *grad) {
    try {
        if (!desc || (n && !uv) || (!g != !grad)) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (!B.hs.has_envmap || !B.ds.envmap) return har_set_error("har_envmap_taps_host: the scene has no environment map");
        const DEnvmap &E = *B.ds.envmap;
        const HostTexture &T = B.hs.textures[E.tex_index];
        if (T.w != E.w || T.h != E.h) return har_set_error("envmap gradients: an environment map smaller than 2 x 3 texels (padded by the emitter) is not differentiated");
        const size_t texels = (size_t) E.w * E.h;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t i1 = n + (size_t) i, i2 = 2 * (size_t) n + i;
            EnvTaps t; envmap_taps(E, uv[i], uv[i1], t);
            for (int k = 0; k < 4; ++k) {
                if (t.idx[k] >= texels) return har_set_error("har_envmap_taps_host: tap out of bounds");
                if (idx) idx[k * (size_t) n + i] = t.idx[k];
                if (weight) weight[k * (size_t) n + i] = t.w[k];
            }
            if (value) {
                float acc[3] = { 0.f, 0.f, 0.f };
                for (int k = 0; k < 4; ++k) for (int c = 0; c < 3; ++c) acc[c] += t.w[k] * T.data[3 * (size_t) t.idx[k] + c];
                value[i] = acc[0] * E.scale; value[i1] = acc[1] * E.scale; value[i2] = acc[2] * E.scale;
            }
            if (eval) { const Vec3 v = envmap_eval_uv(E, uv[i], uv[i1]); eval[i] = v.x; eval[i1] = v.y; eval[i2] = v.z; }
            if (grad) for (int k = 0; k < 4; ++k) for (int c = 0; c < 3; ++c) grad[3 * (size_t) t.idx[k] + c] += g[c * (size_t) n + i] * t.w[k];
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_envmap_taps_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_envmap_taps_host: ") + ex.what()); }
}

/* BSDF::eval_pdf / BSDF::sample of record `bsdf` of a scene on the host: the functions k_api_bsdf_eval_pdf / k_api_bsdf_sample run per lane (bsdf_side, bsdf_inputs,
 * bsdf_eval_pdf / bsdf_sample with the caller's context, the blend-carrying instantiation).  The twins of har_bsdf_eval_pdf / har_bsdf_sample: `value` / `pdf` may be
 * NULL, a masked lane returns zeros.  wi, wo, value, weight: 3 x n; uv, sample2: 2 x n. */
static bool lower_ctx_host(const HarBSDFContext *ctx, BsdfCtx &out) {
    out = BsdfCtx();
    if (!ctx) return true;
    if (ctx->mode > 1u) return false;
    out.mode = ctx->mode; out.type_mask = ctx->type_mask; out.component = ctx->component;
    return true;
}
extern "C" int har_bsdf_eval_pdf_host(const HarSceneDesc *desc, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo,
                                      const uint8_t *active, float *value, float *pdf) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.ds.bsdf_types & HAR_SCENE_ATTR) return har_set_error("mesh_attribute: BSDF::eval / pdf / sample see a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
        if (B.hs.bsdfs[bsdf].type == BSDF_BUMPMAP) return har_set_error("bumpmap: BSDF::eval / pdf / sample of a `bumpmap` record read si.n, si.sh_frame, si.dp_du and si.dp_dv: use har_bsdf_eval_pdf_si_host / har_bsdf_sample_si_host");
        BsdfCtx c; if (!lower_ctx_host(ctx, c)) return har_set_error("HarBSDFContext::mode must be 0 (TransportMode::Radiance) or 1 (TransportMode::Importance)");
        if (n == 0) return 0;
        if (!wi || !uv || !wo) return har_set_error("null input arrays");
        const DScene &S = B.ds;
        for (uint32_t i = 0; i < n; ++i) {
            BsdfEval ev; ev.value = Vec3(0.f); ev.pdf = 0.f;
            if (!(active && !active[i])) {
                BsdfSide side; const bool ok = bsdf_side(S, bsdf, Vec3(wi[i], wi[n + i], wi[2 * (size_t) n + i]), side);
                TexTaps taps; const BsdfInputs in = bsdf_inputs<HAR_SCENE_ALPHAMAP>(S, S.bsdfs[side.index], uv[i], uv[n + i], taps);          /* (the host entries always carry the roughness lookup) */
                bsdf_eval_pdf<HAR_BSDF_ALL_TYPES | HAR_SCENE_NMAP_RECORD_BITS | HAR_SCENE_ALPHAMAP | HAR_SCENE_THIN, true>(S, side, in, ok, Vec3(wo[i], wo[n + i], wo[2 * (size_t) n + i]), ev, bsdf_side_ctx<true>(S, bsdf, side, c), uv[i], uv[n + i]);
            }
            if (value) { value[i] = ev.value.x; value[n + i] = ev.value.y; value[2 * (size_t) n + i] = ev.value.z; }
            if (pdf) pdf[i] = ev.pdf;
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bsdf_eval_pdf_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bsdf_eval_pdf_host: ") + ex.what()); }
}
extern "C" int har_bsdf_sample_host(const HarSceneDesc *desc, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *sample1,
                                    const float *sample2, const uint8_t *active, float *wo, float *pdf, float *weight, float *eta, uint32_t *sampled_type, uint32_t *sampled_component) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.ds.bsdf_types & HAR_SCENE_ATTR) return har_set_error("mesh_attribute: BSDF::eval / pdf / sample see a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
        if (B.hs.bsdfs[bsdf].type == BSDF_BUMPMAP) return har_set_error("bumpmap: BSDF::eval / pdf / sample of a `bumpmap` record read si.n, si.sh_frame, si.dp_du and si.dp_dv: use har_bsdf_eval_pdf_si_host / har_bsdf_sample_si_host");
        BsdfCtx c; if (!lower_ctx_host(ctx, c)) return har_set_error("HarBSDFContext::mode must be 0 (TransportMode::Radiance) or 1 (TransportMode::Importance)");
        if (n == 0) return 0;
        if (!wi || !uv || !sample2 || !wo || !pdf || !weight) return har_set_error("null input / output arrays");
        const DScene &S = B.ds;
        for (uint32_t i = 0; i < n; ++i) {
            BsdfSample b; b.wo = Vec3(0.f); b.pdf = 0.f; b.weight = Vec3(0.f); b.eta = 0.f; b.delta = false; b.type = 0u; b.comp = 0u;
            if (!(active && !active[i])) {
                BsdfSide side; const bool ok = bsdf_side(S, bsdf, Vec3(wi[i], wi[n + i], wi[2 * (size_t) n + i]), side);
                TexTaps taps; const BsdfInputs in = bsdf_inputs<HAR_SCENE_ALPHAMAP>(S, S.bsdfs[side.index], uv[i], uv[n + i], taps);
                bsdf_sample<HAR_BSDF_ALL_TYPES | HAR_SCENE_NMAP_RECORD_BITS | HAR_SCENE_ALPHAMAP | HAR_SCENE_THIN, true>(S, side, in, ok, sample1 ? sample1[i] : 0.f, sample2[i], sample2[n + i], b, bsdf_side_ctx<true>(S, bsdf, side, c), uv[i], uv[n + i]);
            }
            wo[i] = b.wo.x; wo[n + i] = b.wo.y; wo[2 * (size_t) n + i] = b.wo.z; pdf[i] = b.pdf;
            weight[i] = b.weight.x; weight[n + i] = b.weight.y; weight[2 * (size_t) n + i] = b.weight.z;
            if (eta) eta[i] = b.eta;
            if (sampled_type) sampled_type[i] = b.type;
            if (sampled_component) sampled_component[i] = b.comp;
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bsdf_sample_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bsdf_sample_host: ") + ex.what()); }
}

/* Emitter::sample_direction of a projector on the host: projector_sample_direction_lane (har_scene.h), the function k_api_emitter_sample_direction runs per lane.  The
 * twin of har_emitter_sample_direction. */
extern "C" int har_emitter_sample_direction_host(const HarSceneDesc *desc, uint32_t emitter, uint32_t n, const float *ref_p, const float *sample, const uint8_t *active,
                                                 float *d, float *dist, float *pdf, float *p, float *nrm, float *uv, float *spec) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (emitter >= B.hs.emitters.size()) return har_set_error("invalid emitter index");
        if (B.hs.emitters[emitter].type != 8u) return har_set_error("har_emitter_sample_direction_host: implemented for a `projector` (emitter type 8); the other emitters are sampled by the renders only");
        (void) sample;          /* Projector::sample_direction ignores its sample (projector.cpp:203) */
        if (n == 0) return 0;
        if (!ref_p || !d || !dist || !pdf || !p || !nrm || !uv || !spec) return har_set_error("null input / output arrays");
        for (uint32_t i = 0; i < n; ++i) projector_sample_direction_lane(B.ds, emitter, n, i, ref_p, !(active && !active[i]), d, dist, pdf, p, nrm, uv, spec);
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_emitter_sample_direction_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_emitter_sample_direction_host: ") + ex.what()); }
}

/* The looked-up roughness of record `bsdf` at n uv points (uv 2 x n) on the host: bsdf_alpha_lane (har_scene.h), the function k_api_bsdf_alpha runs per lane -- alpha_u,
 * alpha_v after the lookup and before Microfacet's max(., 1e-4); the constants of a record without a roughness map.  The twin of har_bsdf_alpha. */
extern "C" int har_bsdf_alpha_host(const HarSceneDesc *desc, uint32_t bsdf, uint32_t n, const float *uv, float *alpha_u, float *alpha_v) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (n == 0) return 0;
        if (!uv || !alpha_u || !alpha_v) return har_set_error("null uv / alpha_u / alpha_v");
        for (uint32_t i = 0; i < n; ++i) bsdf_alpha_lane(B.ds, bsdf, n, i, uv, alpha_u, alpha_v);
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bsdf_alpha_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bsdf_alpha_host: ") + ex.what()); }
}

/* d value / d {alpha_u, alpha_v, eta, k} of record `bsdf` on the host (bsdf_eval_extra, har_scene.h: what the EXTRA shading kernels form at a vertex), n tuples (wi 3 x n,
 * uv 2 x n, wo 3 x n) under the default context; a `twosided` record is resolved, a roughness map is looked up at uv.  d_alpha_u, d_alpha_v, d_eta, d_k: 3 x n each. */
extern "C" int har_bsdf_eval_extra_host(const HarSceneDesc *desc, uint32_t bsdf, uint32_t n, const float *wi, const float *uv, const float *wo,
                                        float *d_alpha_u, float *d_alpha_v, float *d_eta, float *d_k) {
    try {
        if (!desc) return har_set_error("null argument");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        B.bind();
        if (bsdf >= B.hs.bsdfs.size()) return har_set_error("invalid bsdf index");
        if (B.hs.bsdfs[bsdf].type >= BSDF_TYPE_COUNT) return har_set_error("har_bsdf_eval_extra_host: a plain BSDF model (possibly twosided) is expected");
        if (n == 0) return 0;
        if (!wi || !uv || !wo || !d_alpha_u || !d_alpha_v || !d_eta || !d_k) return har_set_error("null input / output arrays");
        const DScene &S = B.ds;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t i1 = n + (size_t) i, i2 = 2 * (size_t) n + i;
            BsdfSide side; const bool ok = bsdf_side(S, bsdf, Vec3(wi[i], wi[i1], wi[i2]), side);
            TexTaps taps; const BsdfInputs in = bsdf_inputs<HAR_SCENE_ALPHAMAP>(S, S.bsdfs[side.index], uv[i], uv[i1], taps);
            BsdfEvalExtra x; bsdf_eval_extra<HAR_BSDF_ALL_TYPES | HAR_SCENE_ALPHAMAP>(S, side, in, ok, Vec3(wo[i], wo[i1], wo[i2]), x);
            const Vec3 v[4] = { x.d_alpha_u, x.d_alpha_v, x.d_eta, x.d_k }; float *const out[4] = { d_alpha_u, d_alpha_v, d_eta, d_k };
            for (int k = 0; k < 4; ++k) { out[k][i] = v[k].x; out[k][i1] = v[k].y; out[k][i2] = v[k].z; }
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_bsdf_eval_extra_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_bsdf_eval_extra_host: ") + ex.what()); }
}

/* BatchSensor::sample_ray (src/sensors/batch.cpp:132-159) on the host: batch_sample_ray (har_scene.h) -- the function k_raygen_batch runs per lane -- over the children
 * lowered as har_integrator_set_batch_sensors lowers them.  The twin of har_batch_sample_ray. */
static int lower_batch_children_host(const HarSensor *children, uint32_t n_children, std::vector<DCamera> &cams, uint32_t &aperture) {
    if (n_children == 0) return har_set_error("BatchSensor: at least one child sensor must be specified!");
    std::string e;
    return lower_batch_children(children, n_children, cams, aperture, e) ? 0 : har_set_error(e);
}
extern "C" int har_batch_sample_ray_aperture_host(const HarSensor *children, uint32_t n_children, uint32_t n, const float *px, const float *py, const float *ax, const float *ay,
                                                  float *o, float *d, float *maxt) {
    try {
        std::vector<DCamera> cams; uint32_t aperture = 0u;
        if (lower_batch_children_host(children, n_children, cams, aperture)) return 1;
        if (n == 0) return 0;
        if (!px || !py || !o || !d || !maxt || (!ax != !ay)) return har_set_error("null input / output arrays");
        const DBatch B{ cams.data(), n_children, aperture };
        for (uint32_t i = 0; i < n; ++i) {
            Vec3 O, D; float mt; batch_sample_ray<true>(B, px[i], py[i], O, D, mt, ax ? ax[i] : .5f, ay ? ay[i] : .5f);
            o[i] = O.x; o[n + i] = O.y; o[2 * (size_t) n + i] = O.z; d[i] = D.x; d[n + i] = D.y; d[2 * (size_t) n + i] = D.z; maxt[i] = mt;
        }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_batch_sample_ray_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_batch_sample_ray_host: ") + ex.what()); }
}
extern "C" int har_batch_sample_ray_host(const HarSensor *children, uint32_t n_children, uint32_t n, const float *px, const float *py, float *o, float *d, float *maxt) {
    return har_batch_sample_ray_aperture_host(children, n_children, n, px, py, nullptr, nullptr, o, d, maxt);
}

/* Sensor::sample_ray of one camera on the host: camera_sample_ray (har_scene.h) -- what k_api_sensor_ray and, through raygen_lane, the ray generation kernels run per
 * lane.  The twin of har_sensor_sample_ray_aperture. */
extern "C" int har_sensor_sample_ray_aperture_host(const HarSensor *sensor, uint32_t n, const float *px, const float *py, const float *ax, const float *ay,
                                                   float *o, float *d, float *maxt) {
    try {
        DSensor C; std::string e;
        if (!sensor || !lower_sensor(*sensor, C, e)) return har_set_error(e.empty() ? "null sensor" : e);
        if (n == 0) return 0;
        if (!px || !py || !o || !d || !maxt || (!ax != !ay)) return har_set_error("null input / output arrays");
        for (uint32_t i = 0; i < n; ++i) {
            Vec3 O, D; float mt; camera_sample_ray<true>(C, px[i], py[i], ax ? ax[i] : .5f, ay ? ay[i] : .5f, O, D, mt);
            o[i] = O.x; o[n + i] = O.y; o[2 * (size_t) n + i] = O.z; d[i] = D.x; d[n + i] = D.y; d[2 * (size_t) n + i] = D.z; maxt[i] = mt;
        }
        return 0;
    } catch (const std::exception &ex) { return har_set_error(std::string("har_sensor_sample_ray_aperture_host: ") + ex.what()); }
}

/* The forward `path` render of hip_ad_rgb on the host, lane by lane and serially: raygen_lane, the closest-hit traversal and shade_lane<MODE_PATH> with the JIT variants'
 * draws (every lane of the wavefront draws its emitter samples), the splat of ImageBlock::put's coalesced branch (film_footprint).  A test instrument for small films: it
 * runs the functions the kernels run, in the order the wavefront runs them per lane, without a GPU.  `film`: H x W x 4 of the crop window, accumulated into. */
extern "C" int har_render_lanes_stats_host(const HarSceneDesc *desc, const HarSensor *sensor, const HarSensor *children, uint32_t n_children, uint32_t seed, uint32_t spp,
                                           int32_t max_depth, int32_t rr_depth, float *film, HarStats *stats) {
    try {
        if (!desc || !sensor || !film) return har_set_error("null argument");
        if (spp == 0) return har_set_error("spp must be > 0");
        if (max_depth < 0 && max_depth != -1) return har_set_error("\"max_depth\" must be set to -1 (infinite) or a value >= 0");
        if (rr_depth <= 0) return har_set_error("\"rr_depth\" must be set to a value greater than zero!");
        BoundScene B; std::string e;
        if (!lower_scene(*desc, B.hs, e)) return har_set_error(e);
        if (B.hs.stack_need() > (uint32_t) ScalarStack::Capacity) return har_set_error("scene too deep for the scalar traversal stack");
        B.bind();
        DSensor C;
        if (!lower_sensor(*sensor, C, e)) return har_set_error(e);
        std::vector<DCamera> cams; uint32_t aperture = 0u;
        if (n_children && lower_batch_children_host(children, n_children, cams, aperture)) return 1;
        if (n_children && (C.crop_x || C.crop_y || C.crop_w != sensor->film_width || C.crop_h != sensor->film_height || C.border || C.crop_w % n_children))
            return har_set_error("batch sensor: the wide film must have no crop window or sample border, and a width divisible by the child count");
        const uint64_t total = (uint64_t) C.samp_w * C.samp_h * spp;
        if (total > (1u << 22)) return har_set_error("har_render_lanes_host: a serial host render for small films (at most 2^22 lanes)");
        const DBatch T{ cams.data(), n_children, aperture };
        uint32_t log_spp = 0xffffffffu; for (uint32_t k = 0; k < 32; ++k) if ((1u << k) == spp) log_spp = k;
        ShadeParams P{ seed, (uint32_t) max_depth, (uint32_t) rr_depth, 0u };
        int status = 0;
        HarStats count{}; count.paths = total;
        for (uint32_t lane = 0; lane < (uint32_t) total; ++lane) {
            LaneSample ls;
            const PathState st = raygen_lane<true>(C, seed, spp, log_spp, lane, ls, nullptr, nullptr, n_children ? &T : nullptr);
            uint64_t rng = st.rng; bool valid = false;
            const Vec3 rgb = sample_scalar(B.ds, P, rng, st.o, st.d, st.maxt, valid, status, lane, &count);
            const float v[4] = { rgb.x, rgb.y, rgb.z, 1.f };
            Footprint F; film_footprint(C, ls, F);
            for (uint32_t ys = 0; ys < F.count; ++ys)
                for (uint32_t xs = 0; xs < F.count; ++xs) {
                    const uint32_t x = F.x0 + xs, y = F.y0 + ys;
                    if (!(x < C.crop_w && y < C.crop_h)) continue;
                    const float w = F.wx[xs] * F.wy[ys];
                    float *p = film + 4 * ((size_t) y * C.crop_w + x);
                    for (int k = 0; k < 4; ++k) p[k] += v[k] * w;
                }
        }
        if (status) return har_set_error("host render: traversal stack overflow");
        if (stats) { stats->paths += count.paths; stats->vertices += count.vertices; stats->closest_rays += count.closest_rays; stats->shadow_rays += count.shadow_rays; }
        return 0;
    } catch (const std::bad_alloc &) { return har_set_error("har_render_lanes_host: out of memory"); }
    catch (const std::exception &ex) { return har_set_error(std::string("har_render_lanes_host: ") + ex.what()); }
}
extern "C" int har_render_lanes_host(const HarSceneDesc *desc, const HarSensor *sensor, const HarSensor *children, uint32_t n_children, uint32_t seed, uint32_t spp,
                                     int32_t max_depth, int32_t rr_depth, float *film) {
    return har_render_lanes_stats_host(desc, sensor, children, n_children, seed, spp, max_depth, rr_depth, film, nullptr);
}

/* raygen_lane on the host over a lane range: the rays, film positions and sampler states the ray generation kernels produce (k_raygen for pinhole cameras,
 * k_raygen_batch, k_raygen_lens) */
extern "C" int har_raygen_lanes_host(const HarSensor *sensor, const HarSensor *children, uint32_t n_children, uint32_t seed, uint32_t spp, uint32_t lane_begin, uint32_t n,
                                     const uint64_t *resume, float *o, float *d, float *maxt, float *pos, uint64_t *state) {
    try {
        DSensor C; std::string e;
        if (!sensor || !lower_sensor(*sensor, C, e)) return har_set_error(e.empty() ? "null sensor" : e);
        if (spp == 0) return har_set_error("spp must be > 0");
        std::vector<DCamera> cams; uint32_t aperture = 0u;
        if (n_children && lower_batch_children_host(children, n_children, cams, aperture)) return 1;
        if (n_children && (C.crop_x || C.crop_y || C.crop_w != sensor->film_width || C.crop_h != sensor->film_height || C.border || C.crop_w % n_children))
            return har_set_error("batch sensor: the wide film must have no crop window or sample border, and a width divisible by the child count");
        if ((uint64_t) lane_begin + n > (uint64_t) C.samp_w * C.samp_h * spp) return har_set_error("lane range beyond the render's lanes");
        const DBatch B{ cams.data(), n_children, aperture };
        uint32_t log_spp = 0xffffffffu; for (uint32_t k = 0; k < 32; ++k) if ((1u << k) == spp) log_spp = k;
        for (uint32_t i = 0; i < n; ++i) {
            LaneSample ls;
            const PathState st = raygen_lane<true>(C, seed, spp, log_spp, lane_begin + i, ls, resume ? resume + i : nullptr, nullptr, n_children ? &B : nullptr);
            if (o) { o[i] = st.o.x; o[n + i] = st.o.y; o[2 * (size_t) n + i] = st.o.z; }
            if (d) { d[i] = st.d.x; d[n + i] = st.d.y; d[2 * (size_t) n + i] = st.d.z; }
            if (maxt) maxt[i] = st.maxt;
            if (pos) { pos[i] = ls.pos_x; pos[n + i] = ls.pos_y; }
            if (state) state[i] = st.rng;
        }
        return 0;
    } catch (const std::exception &ex) { return har_set_error(std::string("har_raygen_lanes_host: ") + ex.what()); }
}
