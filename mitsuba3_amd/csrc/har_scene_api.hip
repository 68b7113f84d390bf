/*
 * har_scene_api.hip -- the scene half of the C ABI: scene create / destroy / set, instance and vertex updates, refit, and the ray, sampler,
 * BSDF, sensor and film queries.
 */
#include "har_impl.h"
#include "har_refit_launch.h"
#include "har_vertex_update.h"

extern "C" {

int har_scene_create(const HarSceneDesc *desc, HarScene *out) {
    if (!desc || !out) return fail("null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("hip_ad_rgb requires a HIP device (no CPU fallback)");
    HarSceneImpl *S = new HarSceneImpl();
    std::string e;
    if (!lower_scene(*desc, S->hs, e)) { delete S; return fail(e); }
    HostScene &hs = S->hs; DScene &D = S->ds;
    hipError_t err = hipSuccess;
    auto up = [&](auto &vec, auto **dst) { if (err == hipSuccess) err = upload(vec, dst, S->owned); };
    /* the node array keeps room for the largest TLAS the scene's instances can need (a TLAS over n leaves has at most n nodes): an instance update rebuilds the
     * TLAS on the host and rewrites the tail of this array in place */
    S->nodes_cap = hs.nodes.size() + (hs.has_tlas ? hs.insts.size() + 2 : 0);
    {
        void *p = nullptr;
        if (err == hipSuccess) err = dev_alloc(&p, std::max<size_t>(S->nodes_cap, 1) * sizeof(Node8));
        if (err == hipSuccess) { S->owned.push_back(p); if (!hs.nodes.empty()) err = hipMemcpy(p, hs.nodes.data(), hs.nodes.size() * sizeof(Node8), hipMemcpyHostToDevice); }
        D.accel.nodes = (const Node8 *) p;
    }
    up(hs.tris, &D.accel.tris); up(hs.inst_recs, &D.accel.insts);
    up(hs.blas_tri_ranges, &D.blas_tri_ranges); up(hs.verts, &D.verts); up(hs.faces, &D.faces);
#if HAR_SHADING_TRIS
    up(hs.shade_tris, &D.shade_tris);
#endif
    /* material class of every BSDF record and mesh (MaterialQueues; the mesh's class rides in DMesh::pad1 so that k_classify needs ONE dependent load) */
    S->mat_classes = 0;
    {
        std::vector<uint32_t> cls(hs.bsdfs.size());
        for (size_t k = 0; k < hs.bsdfs.size(); ++k) {
            const DBsdf &b = hs.bsdfs[k];
            uint32_t c = std::min<uint32_t>(b.type, BSDF_TYPE_COUNT - 1u);
            if ((b.flags & BF_TWOSIDED) && b.back >= 0 && hs.bsdfs[(size_t) b.back].type != b.type) c = HAR_MAT_GENERIC;
            if (b.type == BSDF_BLEND || b.type == BSDF_MASK || b.type == BSDF_NORMALMAP || b.type == BSDF_BUMPMAP || b.type == BSDF_THINDIELECTRIC) c = HAR_MAT_GENERIC;      /* two models at one vertex / a nested model and a null lobe / the thin leaf, which has no class of its own: the generic bucket of the block-local sort */
            cls[k] = c;
        }
        for (DMesh &m : hs.meshes) { m.pad1 = m.bsdf < cls.size() ? cls[m.bsdf] : 0u; S->mat_classes |= 1u << m.pad1; }
    }
    S->mat_miss_class = 0; while (S->mat_miss_class < HAR_MAT_CLASSES && !(S->mat_classes & (1u << S->mat_miss_class))) ++S->mat_miss_class;
    up(hs.meshes, &D.meshes); up(hs.bsdfs, &D.bsdfs); up(hs.emitters, &D.emitters); up(hs.insts, &D.insts);
    {   /* Accel::mesh_info: what a retiring closest-hit ray copies into its record (HAR_HIT_MATINFO) */
        std::vector<MeshInfo> info(hs.meshes.size());
        for (size_t k = 0; k < hs.meshes.size(); ++k) {
            const DMesh &m = hs.meshes[k];
            if (m.bsdf > 0xfffffu) { for (void *p : S->owned) dev_free(p); delete S; return fail("more than 2^20 BSDF records"); }
            info[k] = MeshInfo{ m.foff, m.bsdf | ((m.flags & 3u) << 20) | ((m.emitter >= 0 ? 1u : 0u) << 22) | ((m.pad1 & 0xfu) << 24) };
        }
        up(info, &D.accel.mesh_info);
    }
    std::vector<DTexture> dt;
    for (auto &t : hs.textures) {
        const float *p = nullptr; up(t.data, &p);
        S->tex_dev.push_back(const_cast<float *>(p)); dt.push_back(hs.device_texture(dt.size(), p));
    }
    S->tex_host_stale.assign(hs.textures.size(), 0);
    up(dt, &D.textures); S->d_textures = const_cast<DTexture *>(D.textures);
    up(hs.bsdf_tables, &D.bsdf_tables);
    D.envmap = nullptr;
    if (hs.has_envmap) {
        const float *tex = nullptr, *warp = nullptr; up(hs.env_tex, &tex); up(hs.env_warp, &warp);
        hs.envmap.tex = tex; hs.envmap.warp = warp;
        std::vector<DEnvmap> one(1, hs.envmap); up(one, &D.envmap);
    }
    up(hs.emitter_cdf, &D.emitter_cdf);
    {   /* the emitter-selection table always gets room for 2 x emitter_count floats: har_scene_set_emitter_sampling_weights rewrites it in place */
        std::vector<float> table(std::max<size_t>(2 * hs.emitters.size(), 1), 0.f);
        std::copy(hs.emitter_distr.begin(), hs.emitter_distr.end(), table.begin());
        const float *distr = nullptr; up(table, &distr); S->d_emitter_distr = const_cast<float *>(distr); hs.bind_tables(D, distr);
    }
    if (err != hipSuccess) { for (void *p : S->owned) dev_free(p); delete S; return fail(std::string("scene upload: ") + hipGetErrorString(err)); }
    S->d_bsdfs = const_cast<DBsdf *>(D.bsdfs);
    D.accel.root = hs.root; D.accel.has_tlas = hs.has_tlas; D.accel.n_tris = (uint32_t) hs.tris.size(); D.accel.n_insts = (uint32_t) hs.inst_recs.size();
    D.accel.top_root = hs.top_root; D.accel.top_first = hs.top_first; D.accel.top_count = hs.top_count; D.accel.top_last = hs.top_last;
    D.n_emitters = (uint32_t) hs.emitters.size(); D.n_meshes = (uint32_t) hs.meshes.size();
    D.n_bsdfs = (uint32_t) hs.bsdfs.size(); D.n_insts = (uint32_t) hs.insts.size(); D.n_textures = (uint32_t) hs.textures.size();
    D.env_emitter = hs.env_emitter;
    D.bsdf_types = 0; for (const DBsdf &b : hs.bsdfs) D.bsdf_types |= bsdf_scene_bit(b.type) | ((b.flags & BF_TWOSIDED) ? 0x80000000u : 0u);
    for (const DBsdf &b : hs.bsdfs) if (b.type == BSDF_ROUGHCONDUCTOR && (b.flags & BF_ALPHA_TEX)) D.bsdf_types |= HAR_SCENE_ALPHAMAP;      /* a roughness map: the set that also looks the roughness up */
    if (hs.has_envmap || hs.has_mesh_emitters || hs.has_point_emitters || !hs.emitter_distr.empty()) D.bsdf_types |= HAR_SCENE_ENVMAP;
    for (const DEmitter &e : hs.emitters) if (e.type == 7u) D.bsdf_types |= HAR_SCENE_TEXLIGHT;      /* (has_mesh_emitters is set with it: the generic emitter kernels + the texel-distribution code) */
    if (hs.has_projector) D.bsdf_types |= HAR_SCENE_TEXLIGHT | HAR_SCENE_PROJECTOR;      /* a projector: the same set (har_bsdf.h) */
    for (const HostTexture &t : hs.textures) if (t.mode & HAR_TEX_ATTRIBUTE) D.bsdf_types |= HAR_SCENE_ATTR;      /* a `mesh_attribute` texture: the widest set that also looks attributes up */
    /* the depth-first bound of the BVH must fit the traversal stacks (LDS entries + HBM spill columns): a deeper scene is refused here instead of
     * rendering with rays that overflow (an overflowing ray is a miss + a status word that only har_render_stats reads) */
    const uint32_t stack_cap = (uint32_t) std::min(HAR_LDS_STACK_DEPTH, HAR_LDS_STACK_SMALL + HAR_STACK_SPILL);
    if (hs.stack_need() + HAR_STACK_MARGIN > stack_cap) {
        const std::string msg = "the scene's BVH needs " + std::to_string(hs.stack_need() + HAR_STACK_MARGIN) + " traversal stack entries per ray, the kernels hold " +
                                std::to_string(stack_cap) + " (HAR_LDS_STACK_DEPTH / HAR_LDS_STACK_SMALL + HAR_STACK_SPILL in har_kernels.h)";
        for (void *p : S->owned) dev_free(p);
        delete S;
        return fail(msg);
    }
    *out = S;
    return 0;
}

int har_scene_destroy(HarScene S) {
    if (!S) return 0;
    (void) hipDeviceSynchronize();     /* accel must outlive in-flight launches (scene_native.inl:44-57) */
    for (void *p : S->owned) dev_free(p);
    delete S;
    return 0;
}

/* device -> host refresh of the mirrors that har_scene_set_*_device left stale (the host setters below rewrite whole records from the mirror) */
/* The values were written by hipMemcpyAsync on the CALLER's stream (har_scene_set_*_device); the blocking copies below run on the null stream, which does not order
 * itself against a non-blocking stream (torch side streams): wait for the last push first, or the mirror picks up the pre-update value and writes it back. */
static void wait_for_device_pushes(HarSceneImpl *S) {
    if (S->last_push_valid) { (void) hipStreamSynchronize(S->last_push_stream); S->last_push_valid = false; }
}
static int sync_host_records(HarSceneImpl *S) {
    if (S->bsdf_host_stale || S->emitter_host_stale) wait_for_device_pushes(S);
    if (S->bsdf_host_stale) { HIP_TRY(hipMemcpy(S->hs.bsdfs.data(), S->d_bsdfs, S->hs.bsdfs.size() * sizeof(DBsdf), hipMemcpyDeviceToHost)); S->bsdf_host_stale = false; }
    if (S->emitter_host_stale) { HIP_TRY(hipMemcpy(S->hs.emitters.data(), S->ds.emitters, S->hs.emitters.size() * sizeof(DEmitter), hipMemcpyDeviceToHost)); S->emitter_host_stale = false; }
    return 0;
}
int har_scene_set_reflectance(HarScene S, uint32_t bsdf, const float rgb[3]) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (sync_host_records(S)) return 1;
    DBsdf &b = S->hs.bsdfs[bsdf]; b.r = rgb[0]; b.g = rgb[1]; b.b = rgb[2];
    if (b.type == BSDF_ROUGHPLASTIC || b.type == BSDF_PLASTIC) update_roughplastic_sampling_weight(S->hs, bsdf);     /* RoughPlastic::parameters_changed */
    HIP_TRY(hipMemcpy(S->d_bsdfs + bsdf, &b, sizeof(DBsdf), hipMemcpyHostToDevice));
    return 0;
}
static int refresh_host_geometry(HarSceneImpl *S, hipStream_t s);
int har_scene_set_delta_emitter(HarScene S, uint32_t emitter, const HarEmitter *record) {
    if (!S || !record || emitter >= S->hs.emitters.size()) return fail("invalid emitter index");
    if (sync_host_records(S)) return 1;
    if (refresh_host_geometry(S, nullptr)) return 1;            /* a directional light's record follows the scene's bounding sphere: the host's vertices / transforms must be current */
    std::string e;
    if (!scene_set_delta_emitter_host(S->hs, emitter, *record, e)) return fail(e);
    if (S->hs.emitters[emitter].type == 8u) {          /* a projector: its block of the side table was re-derived with the record */
        const uint32_t off = as_u32(S->hs.emitters[emitter].inv_area);
        HIP_TRY(hipMemcpy(const_cast<float *>(S->ds.emitter_cdf) + off, S->hs.emitter_cdf.data() + off, HAR_PROJECTOR_TABLE * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(const_cast<DEmitter *>(S->ds.emitters), S->hs.emitters.data(), S->hs.emitters.size() * sizeof(DEmitter), hipMemcpyHostToDevice));
    if (S->hs.emitters.size() == 1) { S->ds.emitter0 = S->hs.emitters[0]; S->ds.emitter0_valid = 1u; }
    return 0;
}
int har_scene_set_bsdf_params(HarScene S, uint32_t bsdf, const HarBSDF *params) {
    if (!S || !params || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (sync_host_records(S)) return 1;
    std::string e;
    if (!scene_set_bsdf_params_host(S->hs, bsdf, *params, e)) return fail(e);
    const DBsdf &b = S->hs.bsdfs[bsdf];
    if (b.type == BSDF_ROUGHPLASTIC && b.table >= 0)
        HIP_TRY(hipMemcpy(const_cast<float *>(S->ds.bsdf_tables) + b.table, S->hs.bsdf_tables.data() + b.table, HAR_ROUGH_TRANSMITTANCE_RES * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(S->d_bsdfs + bsdf, &b, sizeof(DBsdf), hipMemcpyHostToDevice));
    return 0;
}
int har_scene_set_emitter_radiance(HarScene S, uint32_t emitter, const float rgb[3]) {
    if (!S || emitter >= S->hs.emitters.size()) return fail("invalid emitter index");
    if (sync_host_records(S)) return 1;
    DEmitter &e = S->hs.emitters[emitter];
    if (e.type == 2u) return fail("an environment map has no constant radiance");
    if (e.type == 7u) return fail("this area light radiates a bitmap: update the texture (har_scene_set_texture)");
    if (e.type == 8u) return fail(e.mesh != 0xffffffffu ? "projector: this projector's irradiance is a bitmap: update the texture (har_scene_set_texture)"
                                                       : "projector: the record's colour is irradiance * scale: replace the record (har_scene_set_delta_emitter), which takes both");
    e.radiance[0] = rgb[0]; e.radiance[1] = rgb[1]; e.radiance[2] = rgb[2];
    HIP_TRY(hipMemcpy(const_cast<DEmitter *>(S->ds.emitters) + emitter, &e, sizeof(DEmitter), hipMemcpyHostToDevice));
    if (S->hs.emitters.size() == 1) { S->ds.emitter0 = e; S->ds.emitter0_valid = 1u; }
    return 0;
}
/* the records whose lobe-selection weight depends on the MEAN of texture `tex` (RoughPlastic / SmoothPlastic::parameters_changed, roughplastic.cpp:204-242,
 * plastic.cpp:188-205: m_specular_sampling_weight from the means of the two reflectances) */
static bool texture_lights_an_emitter(const HostScene &hs, uint32_t tex) {
    for (const DEmitter &e : hs.emitters) if (e.type == 7u && as_u32(e.radiance[0]) == tex) return true;
    return false;
}
static bool texture_feeds_sampling_weight(const HostScene &hs, uint32_t tex) {
    for (const DBsdf &b : hs.bsdfs) if (b.texture == (int32_t) tex && (b.type == BSDF_ROUGHPLASTIC || b.type == BSDF_PLASTIC)) return true;
    return texture_lights_an_emitter(hs, tex);      /* an area light radiates it: its texel distribution is derived on the host */
}
/* the texel distributions of the area lights that radiate bitmap `tex` (BitmapTexture::parameters_changed -> rebuild_internals, bitmap.cpp:484-493): re-derived from the
 * host mirror of the texels and copied over their slice of the device table */
static int refresh_texel_tables(HarSceneImpl *S, uint32_t tex) {
    for (const DEmitter &e : S->hs.emitters) {
        if (e.type != 7u || as_u32(e.radiance[0]) != tex) continue;
        const HostTexture &t = S->hs.textures[tex];
        const uint32_t off = as_u32(e.radiance[1]);
        std::string err;
        if (!texel_table_fill(S->hs, t, off, err)) return fail(err);
        const size_t n = HAR_TEXEL_TABLE_HEADER + (size_t) t.h + (size_t) t.w * t.h;
        HIP_TRY(hipMemcpy(const_cast<float *>(S->ds.emitter_cdf) + off, S->hs.emitter_cdf.data() + off, n * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}
static int refresh_sampling_weights(HarSceneImpl *S, uint32_t tex) {
    for (uint32_t k = 0; k < S->hs.bsdfs.size(); ++k) {
        DBsdf &b = S->hs.bsdfs[k];
        if (b.texture != (int32_t) tex || !(b.type == BSDF_ROUGHPLASTIC || b.type == BSDF_PLASTIC)) continue;
        update_roughplastic_sampling_weight(S->hs, k);
        HIP_TRY(hipMemcpy(S->d_bsdfs + k, &b, sizeof(DBsdf), hipMemcpyHostToDevice));
    }
    return refresh_texel_tables(S, tex);
}
int har_scene_set_texture(HarScene S, uint32_t tex, const float *data) {
    if (!S || tex >= S->hs.textures.size()) return fail("invalid texture index");
    HostTexture &t = S->hs.textures[tex];
    if (texture_lights_an_emitter(S->hs, tex)) { std::string err; if (!texel_table_inputs_ok(t.uvm, data, t.w, t.h, err)) return fail(err); }      /* before anything changes */
    t.data.assign(data, data + t.data.size());
    HIP_TRY(hipMemcpy(S->tex_dev[tex], data, t.data.size() * sizeof(float), hipMemcpyHostToDevice));
    S->tex_host_stale[tex] = 0;
    return refresh_sampling_weights(S, tex);
}
/* The same three updates from DEVICE memory, ordered on `stream`, without a host round trip: what an optimisation loop calls every step (mi.traverse +
 * params.update(), src/python/python/util.py:344-528 -- in the reference the parameters ARE device arrays and update() copies nothing).  The library's host
 * mirror of the value goes stale and is refreshed from the device only when something needs it (har_scene_set_* from the host overwrite it anyway).
 * Exception: a bitmap / colour that feeds the lobe-selection weight of a `plastic` / `roughplastic` record (the mean of the reflectance) -- that weight is
 * computed on the host, so these records take one synchronous device-to-host copy. */
int har_scene_set_texture_device(HarScene S, uint32_t tex, const float *dev, void *stream) {
    if (!S || tex >= S->hs.textures.size()) return fail("invalid texture index");
    if (!dev) return fail("null device pointer");
    HostTexture &t = S->hs.textures[tex];
    hipStream_t s = (hipStream_t) stream;
    if (texture_lights_an_emitter(S->hs, tex)) {          /* its texel distribution is derived on the host; the new texels are checked before anything changes */
        std::vector<float> incoming(t.data.size());
        HIP_TRY(hipMemcpyAsync(incoming.data(), dev, incoming.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::string err;
        if (!texel_table_inputs_ok(t.uvm, incoming.data(), t.w, t.h, err)) return fail(err);
    }
    if (texture_feeds_sampling_weight(S->hs, tex)) {
        HIP_TRY(hipMemcpyAsync(t.data.data(), dev, t.data.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        if (dev != S->tex_dev[tex]) HIP_TRY(hipMemcpyAsync(S->tex_dev[tex], dev, t.data.size() * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        S->tex_host_stale[tex] = 0;
        return refresh_sampling_weights(S, tex);
    }
    if (dev != S->tex_dev[tex]) HIP_TRY(hipMemcpyAsync(S->tex_dev[tex], dev, t.data.size() * sizeof(float), hipMemcpyDeviceToDevice, s));
    S->tex_host_stale[tex] = 1; S->last_push_stream = s; S->last_push_valid = true;
    return 0;
}
int har_scene_set_reflectance_device(HarScene S, uint32_t bsdf, const float *dev_rgb, void *stream) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (!dev_rgb) return fail("null device pointer");
    DBsdf &b = S->hs.bsdfs[bsdf];
    hipStream_t s = (hipStream_t) stream;
    if (b.type == BSDF_ROUGHPLASTIC || b.type == BSDF_PLASTIC) {           /* its sampling weight depends on the colour: through the host */
        float rgb[3];
        HIP_TRY(hipMemcpyAsync(rgb, dev_rgb, sizeof(rgb), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return har_scene_set_reflectance(S, bsdf, rgb);
    }
    static_assert(offsetof(DBsdf, g) == offsetof(DBsdf, r) + 4 && offsetof(DBsdf, b) == offsetof(DBsdf, r) + 8, "slot 0 is three consecutive floats");
    HIP_TRY(hipMemcpyAsync(&S->d_bsdfs[bsdf].r, dev_rgb, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    S->bsdf_host_stale = true; S->last_push_stream = (hipStream_t) stream; S->last_push_valid = true;
    return 0;
}
int har_scene_set_emitter_radiance_device(HarScene S, uint32_t emitter, const float *dev_rgb, void *stream) {
    if (!S || emitter >= S->hs.emitters.size()) return fail("invalid emitter index");
    if (!dev_rgb) return fail("null device pointer");
    if (S->hs.emitters[emitter].type == 2u) return fail("an environment map has no constant radiance");
    if (S->hs.emitters[emitter].type == 7u) return fail("this area light radiates a bitmap: update the texture (har_scene_set_texture_device)");
    if (S->hs.emitters[emitter].type == 8u) return fail(S->hs.emitters[emitter].mesh != 0xffffffffu ? "projector: this projector's irradiance is a bitmap: update the texture (har_scene_set_texture_device)"
                                                                                                    : "projector: the record's colour is irradiance * scale: replace the record (har_scene_set_delta_emitter), which takes both");
    HIP_TRY(hipMemcpyAsync(const_cast<float *>(S->ds.emitters[0].radiance) + (size_t) emitter * (sizeof(DEmitter) / sizeof(float)), dev_rgb, 3 * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t) stream));
    S->emitter_host_stale = true; S->last_push_stream = (hipStream_t) stream; S->last_push_valid = true;
    if (S->ds.emitter0_valid) S->ds.emitter0_valid = 2u;      /* the argument copy no longer holds the radiance: the kernels take those three floats from the array, the rest of the record stays in scalar registers */
    return 0;
}
int har_scene_accel_info(HarScene S, uint64_t info[4]) {
    if (!S) return fail("null scene");
    info[0] = S->hs.nodes.size(); info[1] = S->hs.tris.size();
    info[2] = S->hs.nodes.size() * sizeof(Node8) + S->hs.tris.size() * sizeof(TriRec) + S->hs.inst_recs.size() * sizeof(InstRec);
    info[3] = S->hs.stack_need();
    return 0;
}

/* Scene::sample_emitter / pdf_emitter (src/render/scene.cpp:248-279), array-valued */
int har_scene_sample_emitter(HarScene S, uint32_t n, const float *index_sample, const uint8_t *active, uint32_t *index, float *weight, float *reused_sample, void *stream) {
    if (!S) return fail("null scene");
    if (n == 0) return 0;
    if (!index_sample || !index || !weight || !reused_sample) return fail("null sample / output arrays");
    launch_api_sample_emitter((hipStream_t) stream, S->ds, n, index_sample, active, index, weight, reused_sample);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_scene_pdf_emitter(HarScene S, uint32_t n, const uint32_t *index, const uint8_t *active, float *pdf, void *stream) {
    if (!S) return fail("null scene");
    if (n == 0) return 0;
    if (!index || !pdf) return fail("null index / output arrays");
    launch_api_pdf_emitter((hipStream_t) stream, S->ds, n, index, active, pdf);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* params['<emitter>.sampling_weight'] + update(): Scene::parameters_changed -> update_emitter_sampling_distribution (scene.cpp:120-141, 523-528) */
int har_scene_set_emitter_sampling_weights(HarScene S, const float *weights, uint32_t count) {
    if (!S || !weights) return fail("null argument");
    if (count != S->hs.emitters.size()) return fail("one sampling weight per emitter of the scene");
    std::string e;
    if (!build_emitter_distribution(S->hs, weights, count, e)) return fail(e);
    if (!S->hs.emitter_distr.empty()) HIP_TRY(hipMemcpy(S->d_emitter_distr, S->hs.emitter_distr.data(), S->hs.emitter_distr.size() * sizeof(float), hipMemcpyHostToDevice));
    S->hs.bind_tables(S->ds, S->d_emitter_distr);
    if (S->emitter_host_stale && S->ds.emitter0_valid) S->ds.emitter0_valid = 2u;      /* a radiance pushed device-to-device is newer than the mirror bind_tables copies */
    /* scenes with a distribution run the kernels that carry the generic emitter code */
    const bool generic = S->hs.has_envmap || S->hs.has_mesh_emitters || S->hs.has_point_emitters || !S->hs.emitter_distr.empty();
    S->ds.bsdf_types = generic ? (S->ds.bsdf_types | HAR_SCENE_ENVMAP) : (S->ds.bsdf_types & ~HAR_SCENE_ENVMAP);
    return 0;
}
/* params['<texture>.to_uv'] + update(): BitmapTexture::parameters_changed with a new m_transform (bitmap.cpp:175); six zeros or the identity switch the transform off */
int har_scene_set_texture_to_uv(HarScene S, uint32_t tex, const float to_uv[6]) {
    if (!S || tex >= S->hs.textures.size() || !to_uv) return fail("invalid texture index");
    HostTexture &t = S->hs.textures[tex];
    if (t.mode & HAR_TEX_ATTRIBUTE) {          /* a `mesh_attribute` record keeps its `scale` there (MeshAttribute::traverse: "scale") */
        if (!std::isfinite(to_uv[0])) return fail("mesh_attribute: `scale` must be finite");
        t.uvm[0] = to_uv[0];
        const DTexture d = S->hs.device_texture(tex, S->tex_dev[tex]);
        HIP_TRY(hipMemcpy(S->d_textures + tex, &d, sizeof(DTexture), hipMemcpyHostToDevice));
        return 0;
    }
    const float id6[6] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f };
    bool zero = true, ident = true;
    for (int k = 0; k < 6; ++k) { if (!std::isfinite(to_uv[k])) return fail("HarTexture::to_uv must be finite"); zero = zero && to_uv[k] == 0.f; ident = ident && to_uv[k] == id6[k]; }
    if (!zero && !ident && to_uv[0] * to_uv[4] - to_uv[1] * to_uv[3] == 0.f) return fail("HarTexture::to_uv is singular");
    if (texture_lights_an_emitter(S->hs, tex)) {          /* the emitter's texel distribution needs a to_uv that keeps the unit square (bitmap.cpp:976-992): checked before anything changes */
        if (S->tex_host_stale[tex]) { wait_for_device_pushes(S); HIP_TRY(hipMemcpy(t.data.data(), S->tex_dev[tex], t.data.size() * sizeof(float), hipMemcpyDeviceToHost)); S->tex_host_stale[tex] = 0; }
        std::string err;
        if (!texel_table_inputs_ok((zero || ident) ? id6 : to_uv, t.data.data(), t.w, t.h, err)) return fail(err);
    }
    t.mode &= ~HAR_TEX_HAS_UV_XF;
    for (int k = 0; k < 6; ++k) t.uvm[k] = id6[k];
    if (!zero && !ident) {
        for (int k = 0; k < 6; ++k) t.uvm[k] = to_uv[k];
        t.mode |= HAR_TEX_HAS_UV_XF;
    }
    const DTexture d = S->hs.device_texture(tex, S->tex_dev[tex]);
    HIP_TRY(hipMemcpy(S->d_textures + tex, &d, sizeof(DTexture), hipMemcpyHostToDevice));
    return refresh_texel_tables(S, tex);
}

/* ---- incremental updates of the acceleration data (Scene::parameters_changed rebuilds only what a dirty shape needs, scene.cpp:517-540; scene_optix.inl:351-372) */
static int stack_fits(const HostScene &hs) {
    const uint32_t stack_cap = (uint32_t) std::min(HAR_LDS_STACK_DEPTH, HAR_LDS_STACK_SMALL + HAR_STACK_SPILL);
    if (hs.stack_need() + HAR_STACK_MARGIN > stack_cap) return fail("the updated scene's BVH needs " + std::to_string(hs.stack_need() + HAR_STACK_MARGIN) + " traversal stack entries per ray, the kernels hold " + std::to_string(stack_cap));
    return 0;
}
/* the arrays build_tlas / update_scene_bounds rewrote on the host -> device, in stream order; the copies read pageable host memory, so the call waits for them */
static int upload_instance_level(HarSceneImpl *S, hipStream_t s) {
    HostScene &hs = S->hs; DScene &D = S->ds;
    if (hs.nodes.size() > S->nodes_cap) return fail("TLAS does not fit the node array");           /* cannot happen: capacity = BLAS nodes + instance count + 2 */
    if (stack_fits(hs)) return 1;
    const size_t tail = hs.nodes.size() - hs.tlas_first;
    if (tail) HIP_TRY(hipMemcpyAsync(const_cast<Node8 *>(D.accel.nodes) + hs.tlas_first, hs.nodes.data() + hs.tlas_first, tail * sizeof(Node8), hipMemcpyHostToDevice, s));
    if (!hs.inst_recs.empty()) HIP_TRY(hipMemcpyAsync(const_cast<InstRec *>(D.accel.insts), hs.inst_recs.data(), hs.inst_recs.size() * sizeof(InstRec), hipMemcpyHostToDevice, s));
    if (!hs.blas_tri_ranges.empty()) HIP_TRY(hipMemcpyAsync(const_cast<uint32_t *>(D.blas_tri_ranges), hs.blas_tri_ranges.data(), hs.blas_tri_ranges.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (!hs.insts.empty()) HIP_TRY(hipMemcpyAsync(const_cast<DInst *>(D.insts), hs.insts.data(), hs.insts.size() * sizeof(DInst), hipMemcpyHostToDevice, s));
    D.accel.root = hs.root; D.accel.n_insts = (uint32_t) hs.inst_recs.size();
    D.accel.top_root = hs.top_root; D.accel.top_first = hs.top_first; D.accel.top_count = hs.top_count; D.accel.top_last = hs.top_last;
    return 0;
}
/* the records update_scene_bounds touches: the environment / directional emitters' bounding sphere */
static int upload_scene_bounds(HarSceneImpl *S, hipStream_t s) {
    HostScene &hs = S->hs;
    bool any = hs.env_emitter >= 0; for (const DEmitter &E : hs.emitters) any = any || E.type == 6u;
    if (!any) return 0;
    if (S->emitter_host_stale) {          /* radiances pushed device-to-device are newer than the mirror: fetch them before the records are rewritten */
        std::vector<DEmitter> cur(hs.emitters.size());
        HIP_TRY(hipMemcpyAsync(cur.data(), S->ds.emitters, cur.size() * sizeof(DEmitter), hipMemcpyDeviceToHost, s)); HIP_TRY(hipStreamSynchronize(s));
        for (size_t k = 0; k < cur.size(); ++k) std::memcpy(hs.emitters[k].radiance, cur[k].radiance, 12);
        S->emitter_host_stale = false;
    }
    HIP_TRY(hipMemcpyAsync(const_cast<DEmitter *>(S->ds.emitters), hs.emitters.data(), hs.emitters.size() * sizeof(DEmitter), hipMemcpyHostToDevice, s));
    if (hs.emitters.size() == 1) { S->ds.emitter0 = hs.emitters[0]; S->ds.emitter0_valid = 1u; }
    if (hs.has_envmap && S->ds.envmap) {
        DEnvmap E = hs.envmap;         /* tex / warp already hold the device pointers (har_scene_create) */
        HIP_TRY(hipMemcpyAsync(const_cast<DEnvmap *>(S->ds.envmap), &E, sizeof(DEnvmap), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}
static int refresh_host_geometry(HarSceneImpl *S, hipStream_t s);
int har_scene_update_instances(HarScene S, uint32_t first, uint32_t count, const float *to_world, const float *to_object, void *stream) {
    if (!S || !to_world || !to_object) return fail("null argument");
    if (count == 0) return 0;
    std::string e;
    hipStream_t s = (hipStream_t) stream;
    if (refresh_host_geometry(S, s)) return 1;              /* the instance boxes and the scene bounds are host builds over the vertex positions and the other instances' transforms */
    if (!scene_set_instances_host(S->hs, first, count, to_world, to_object, e)) return fail(e);
    if (upload_instance_level(S, s) || upload_scene_bounds(S, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
/* refit scratch, on first use; S->tri_box (the "scratch exists" flag) is set last, so a failed allocation leaves no half-made set behind */
static int ensure_refit_scratch(HarSceneImpl *S, hipStream_t s) {
    if (S->tri_box) return 0;
    HostScene &hs = S->hs;
    const size_t n_blas = 1 + hs.blas_groups.size();
    void *p = nullptr;
    HIP_TRY(dev_alloc(&p, std::max<size_t>(hs.tris.size(), 1) * sizeof(RefitBox))); S->owned.push_back(p); RefitBox *tri_box = (RefitBox *) p;
    HIP_TRY(dev_alloc(&p, std::max<size_t>(S->nodes_cap, 1) * sizeof(RefitBox))); S->owned.push_back(p); S->node_box = (RefitBox *) p;
    HIP_TRY(dev_alloc(&p, std::max<size_t>(hs.refit_order.size(), 1) * sizeof(uint32_t))); S->owned.push_back(p); S->d_refit_order = (uint32_t *) p;
    if (!hs.refit_order.empty()) { HIP_TRY(hipMemcpyAsync(S->d_refit_order, hs.refit_order.data(), hs.refit_order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s)); HIP_TRY(hipStreamSynchronize(s)); }
    HIP_TRY(dev_alloc(&p, (n_blas + 1) * sizeof(float))); S->owned.push_back(p); S->d_area = (float *) p;          /* + 1: the instance level's sum (not watched) */
    S->tri_box = tri_box;
    return 0;
}
static size_t blas_slot(const HostScene &hs, const BlasInfo *B) { return B == &hs.blas_top ? 0 : 1 + (size_t) (B - hs.blas_groups.data()); }
/* the launches of one refit pass of BLAS `B` on the device arrays as they are (triangle records + boxes, then the nodes level by level, deepest first); the node-area
 * sum accumulates in d_area[slot] */
static int enqueue_refit(HarSceneImpl *S, BlasInfo *B, hipStream_t s) {
    const size_t bi = blas_slot(S->hs, B);
    HIP_TRY(hipMemsetAsync(S->d_area + bi, 0, sizeof(float), s));
    launch_refit_triangles(s, S->ds, B->first_tri, B->tri_count, S->tri_box);
    for (size_t l = 0; l + 1 < B->level_begin.size(); ++l)
        launch_refit_nodes(s, S->ds, S->d_refit_order + B->order_first + B->level_begin[l], B->level_begin[l + 1] - B->level_begin[l], S->tri_box, S->node_box, S->d_area + bi);
    HIP_TRY(hipGetLastError());
    return 0;
}
static double refit_cost_figure(float area, const RefitBox &root) {
    const float dx = root.hi[0] - root.lo[0], dy = root.hi[1] - root.lo[1], dz = root.hi[2] - root.lo[2];
    const double root_area = 2.0 * ((double) dx * dy + (double) dy * dz + (double) dz * dx);
    return root_area > 0.0 ? (double) area / root_area : 0.0;           /* sum of the node areas over the root's area (the node term of the SAH) */
}
/* one refit pass + its cost figure, waited for */
static int refit_pass_sync(HarSceneImpl *S, BlasInfo *B, hipStream_t s, double &cost) {
    if (enqueue_refit(S, B, s)) return 1;
    float area = 0.f; RefitBox root{};
    HIP_TRY(hipMemcpyAsync(&area, S->d_area + blas_slot(S->hs, B), sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&root, S->node_box + B->root, sizeof(RefitBox), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    cost = refit_cost_figure(area, root);
    return 0;
}
static int refit_verdict(HarSceneImpl *S, const BlasInfo *B, double cost) {
    const double max_inflation = switches().refit_max_inflation;
    const uint32_t max_refits = switches().refit_max_steps;
    S->last_refit_cost = cost; S->last_refit_ratio = B->built_area > 0.0 ? cost / B->built_area : 1.0;
    if ((B->built_area > 0.0 && cost > max_inflation * B->built_area) || (max_refits && B->refits >= max_refits)) return HAR_UPDATE_REBUILD_ADVISED;
    return 0;
}
/* device -> host refresh of the vertex records of the meshes a device-resident update left stale on the host (hs.verts, hs.shade_tris): before anything on the host
 * reads positions again (group boxes, scene bounds, har_scene_get_vertices) */
extern "C++" int refresh_host_vertices(HarSceneImpl *S, hipStream_t s, int only_mesh) {
    HostScene &hs = S->hs; bool any = false;
    for (size_t k = 0; k < S->verts_host_stale.size(); ++k) {
        if (!S->verts_host_stale[k] || (only_mesh >= 0 && (size_t) only_mesh != k)) continue;
        const DMesh &m = hs.meshes[k];
        HIP_TRY(hipMemcpyAsync(hs.verts.data() + 8 * (size_t) m.voff, S->ds.verts + 8 * (size_t) m.voff, 32 * (size_t) m.vertex_count, hipMemcpyDeviceToHost, s));
        any = true;
    }
    if (!any) return 0;
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t k = 0; k < S->verts_host_stale.size(); ++k) {
        if (!S->verts_host_stale[k] || (only_mesh >= 0 && (size_t) only_mesh != k)) continue;
        const DMesh &m = hs.meshes[k];
#if HAR_SHADING_TRIS
        for (uint32_t f = 0; f < m.face_count; ++f)
            for (int c = 0; c < 3; ++c) std::memcpy(hs.shade_tris.data() + 24 * ((size_t) m.foff + f) + 8 * c, hs.verts.data() + 8 * ((size_t) m.voff + hs.faces[4 * ((size_t) m.foff + f) + c]), 32);
#endif
        S->verts_host_stale[k] = 0;
    }
    return 0;
}
/* ... and of the instance transforms a device-resident update left stale on the host (hs.insts; build_tlas re-derives the leaf records from them) */
static int refresh_host_instances(HarSceneImpl *S, hipStream_t s) {
    if (!S->insts_host_stale || S->hs.insts.empty()) { S->insts_host_stale = false; return 0; }
    HIP_TRY(hipMemcpyAsync(S->hs.insts.data(), S->ds.insts, S->hs.insts.size() * sizeof(DInst), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    S->insts_host_stale = false;
    return 0;
}
/* everything a HOST build of the instance level / the scene bounds reads, brought up to date after device-resident updates */
static int refresh_host_geometry(HarSceneImpl *S, hipStream_t s) {
    if (refresh_host_vertices(S, s, -1) || refresh_host_instances(S, s)) return 1;
    recompute_stale_group_boxes(S->hs);
    return 0;
}
/* the figures the LAST device-resident update left in the pinned record: 0, HAR_UPDATE_REBUILD_ADVISED, or 1 (a position was not finite) */
static int collect_pending_refit(HarSceneImpl *S) {
    if (!S->pend_active) return 0;
    HIP_TRY(hipEventSynchronize(S->pend_ev));          /* recorded one update (= at least one frame) ago, or just synchronised by the caller */
    S->pend_active = false;
    if (S->pend->bad) return fail("har_scene_update_vertices_device: a vertex position of the last update was not finite (the scene holds it: create a new scene)");
    return refit_verdict(S, S->pend_blas, refit_cost_figure(S->pend->area, S->pend->root));
}
int har_scene_update_vertices(HarScene S, uint32_t mesh, const float *vertices, void *stream) {
    if (!S || !vertices) return fail("null argument");
    HostScene &hs = S->hs; DScene &D = S->ds;
    hipStream_t s = (hipStream_t) stream;
    std::string e;
    if (!S->verts_host_stale.empty()) {         /* other meshes may have been updated on the device since: the host steps below read their positions */
        if (mesh < S->verts_host_stale.size()) S->verts_host_stale[mesh] = 0;          /* this one is overwritten */
        if (refresh_host_geometry(S, s)) return 1;
        if (collect_pending_refit(S) == 1) return 1;
    }
    if (refresh_host_instances(S, s)) return 1;
    BlasInfo *B = scene_set_vertices_host(hs, mesh, vertices, e);
    if (!B) { (void) fail(e); return HAR_UPDATE_NEEDS_NEW_SCENE; }
    if (mesh < S->normals_regenerated.size()) S->normals_regenerated[mesh] = 0;
    const DMesh &m = hs.meshes[mesh];
    if (ensure_refit_scratch(S, s)) return 1;
    /* the figure of the tree AS BUILT: the first update of a BLAS refits it once on the old vertices (which reproduces the built nodes bit for bit) */
    if (B->built_area == 0.0 && refit_pass_sync(S, B, s, B->built_area)) return 1;
    HIP_TRY(hipMemcpyAsync(const_cast<float *>(D.verts) + 8 * (size_t) m.voff, vertices, 32 * (size_t) m.vertex_count, hipMemcpyHostToDevice, s));
#if HAR_SHADING_TRIS
    HIP_TRY(hipMemcpyAsync(const_cast<float *>(D.shade_tris) + 24 * (size_t) m.foff, hs.shade_tris.data() + 24 * (size_t) m.foff, 96 * (size_t) m.face_count, hipMemcpyHostToDevice, s));
#endif
    double cost = 0.0;
    if (refit_pass_sync(S, B, s, cost)) return 1;
    if (!scene_after_refit_host(hs, B, e)) return fail(e);
    if (B != &hs.blas_top && upload_instance_level(S, s)) return 1;
    if (upload_scene_bounds(S, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return refit_verdict(S, B, cost);
}
static bool scene_needs_bounds(const HostScene &hs) {
    bool any = hs.env_emitter >= 0; for (const DEmitter &E : hs.emitters) any = any || E.type == 6u;
    return any;
}
/* corner list of a mesh (har_vertex_update.h), built on the host once and kept on the device */
static int ensure_corner_list(HarSceneImpl *S, uint32_t mesh, hipStream_t s) {
    HostScene &hs = S->hs;
    if (S->d_corner_begin.size() != hs.meshes.size()) { S->d_corner_begin.assign(hs.meshes.size(), nullptr); S->d_corners.assign(hs.meshes.size(), nullptr); }
    if (S->d_corner_begin[mesh]) return 0;
    const DMesh &m = hs.meshes[mesh];
    std::vector<uint32_t> begin((size_t) m.vertex_count + 1, 0u), corners(3 * (size_t) m.face_count);
    const uint32_t *F = hs.faces.data() + 4 * (size_t) m.foff;
    for (uint32_t f = 0; f < m.face_count; ++f) for (int k = 0; k < 3; ++k) ++begin[(size_t) F[4 * (size_t) f + k] + 1];
    for (uint32_t v = 0; v < m.vertex_count; ++v) begin[v + 1] += begin[v];
    std::vector<uint32_t> cursor(begin.begin(), begin.end() - 1);
    for (uint32_t f = 0; f < m.face_count; ++f) for (int k = 0; k < 3; ++k) corners[cursor[F[4 * (size_t) f + k]]++] = f | ((uint32_t) k << 30);      /* (face, corner) ascending per vertex */
    void *p = nullptr;
    HIP_TRY(dev_alloc(&p, begin.size() * sizeof(uint32_t))); S->owned.push_back(p); uint32_t *d_begin = (uint32_t *) p;
    HIP_TRY(dev_alloc(&p, std::max<size_t>(corners.size(), 1) * sizeof(uint32_t))); S->owned.push_back(p); uint32_t *d_corners = (uint32_t *) p;
    HIP_TRY(hipMemcpyAsync(d_begin, begin.data(), begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (!corners.empty()) HIP_TRY(hipMemcpyAsync(d_corners, corners.data(), corners.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                  /* once per mesh: the vectors die here */
    S->d_corners[mesh] = d_corners; S->d_corner_begin[mesh] = d_begin;
    return 0;
}
/* the device tables of the instance-level refit, for the TLAS as the host last built it (once per build_tlas: a small upload that waits) */
static int ensure_tlas_refit_tables(HarSceneImpl *S, hipStream_t s) {
    HostScene &hs = S->hs;
    if (S->d_tlas_serial == hs.tlas_serial && S->d_tlas_order) return 0;
    const size_t n_nodes = hs.tlas_order.size(), n_rec = hs.inst_recs.size();
    void *p = nullptr;
    if (n_nodes > S->d_tlas_cap) { HIP_TRY(dev_alloc(&p, n_nodes * sizeof(uint32_t))); S->owned.push_back(p); S->d_tlas_order = (uint32_t *) p; S->d_tlas_cap = n_nodes; }
    if (n_rec > S->d_inst_cap) {
        HIP_TRY(dev_alloc(&p, n_rec * sizeof(uint2))); S->owned.push_back(p); S->d_inst_vrange = (uint2 *) p;
        HIP_TRY(dev_alloc(&p, n_rec * sizeof(RefitBox))); S->owned.push_back(p); S->d_inst_box = (RefitBox *) p;
        S->d_inst_cap = n_rec;
    }
    const size_t n_inst = hs.insts.size();
    if (n_inst > S->d_rec_of_cap) { HIP_TRY(dev_alloc(&p, n_inst * sizeof(uint32_t))); S->owned.push_back(p); S->d_rec_of = (uint32_t *) p; S->d_rec_of_cap = n_inst; }
    std::vector<uint32_t> rec_of(n_inst, 0xffffffffu);
    for (size_t r = 0; r < n_rec; ++r) rec_of[hs.inst_recs[r].inst_index] = (uint32_t) r;
    if (n_inst) HIP_TRY(hipMemcpyAsync(S->d_rec_of, rec_of.data(), n_inst * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    std::vector<uint2> vr(n_rec);
    for (size_t r = 0; r < n_rec; ++r) {
        const HarShapeGroup &sg = hs.groups[hs.inst_group[hs.inst_recs[r].inst_index]];
        uint32_t cnt = 0; for (uint32_t m = sg.first_mesh; m < sg.first_mesh + sg.mesh_count; ++m) cnt += hs.meshes[m].vertex_count;
        vr[r] = make_uint2(hs.meshes[sg.first_mesh].voff, cnt);
    }
    if (n_nodes) HIP_TRY(hipMemcpyAsync(S->d_tlas_order, hs.tlas_order.data(), n_nodes * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_rec) HIP_TRY(hipMemcpyAsync(S->d_inst_vrange, vr.data(), n_rec * sizeof(uint2), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    S->d_tlas_serial = hs.tlas_serial;
    return 0;
}
int har_scene_update_vertices_device(HarScene S, uint32_t mesh, const float *positions, void *stream) {
    if (!S || !positions) return fail("null argument");
    HostScene &hs = S->hs; DScene &D = S->ds;
    hipStream_t s = (hipStream_t) stream;
    if (mesh >= hs.meshes.size()) { (void) fail("invalid mesh index"); return HAR_UPDATE_NEEDS_NEW_SCENE; }
    const DMesh &m = hs.meshes[mesh];
    if (m.emitter >= 0) { (void) fail("the mesh carries an area emitter (its sampling records are lowered from the positions): create a new scene"); return HAR_UPDATE_NEEDS_NEW_SCENE; }
    BlasInfo *B = nullptr;
    if (mesh < hs.top_mesh_count) B = &hs.blas_top;
    else for (size_t g = 0; g < hs.groups.size(); ++g) if (mesh >= hs.groups[g].first_mesh && mesh < hs.groups[g].first_mesh + hs.groups[g].mesh_count) B = &hs.blas_groups[g];
    if (!B) return fail("mesh belongs to no BLAS");
    /* what the PREVIOUS update's refit reported (its launches finished a frame ago): acted on one step late, so that this call waits for nothing */
    int verdict = collect_pending_refit(S);
    if (verdict == 1) return 1;
    if (S->verts_host_stale.size() != hs.meshes.size()) { S->verts_host_stale.assign(hs.meshes.size(), 0); S->normals_regenerated.assign(hs.meshes.size(), 0); }
    if (ensure_refit_scratch(S, s)) return 1;
    if (!S->pend) {
        HIP_TRY(hipHostMalloc((void **) &S->pend, sizeof(*S->pend), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&S->pend_ev, hipEventDisableTiming));
        void *p = nullptr; HIP_TRY(dev_alloc(&p, sizeof(uint32_t))); S->owned.push_back(p); S->d_bad = (uint32_t *) p;
    }
    if ((m.flags & 1u) && ensure_corner_list(S, mesh, s)) return 1;
    if (B->built_area == 0.0 && refit_pass_sync(S, B, s, B->built_area)) return 1;          /* once per BLAS: the figure of the tree as built */
    HIP_TRY(hipMemsetAsync(S->d_bad, 0, sizeof(uint32_t), s));
    launch_set_positions(s, D, m.voff, m.vertex_count, positions, S->d_bad);
    if (m.flags & 1u) { launch_vertex_normals(s, D, m.voff, m.foff, m.vertex_count, S->d_corner_begin[mesh], S->d_corners[mesh]); S->normals_regenerated[mesh] = 1; }
#if HAR_SHADING_TRIS
    launch_shading_triangles(s, D, m.voff, m.foff, m.face_count);
#endif
    if (enqueue_refit(S, B, s)) return 1;
    HIP_TRY(hipMemcpyAsync(&S->pend->area, S->d_area + blas_slot(hs, B), sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&S->pend->root, S->node_box + B->root, sizeof(RefitBox), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&S->pend->bad, S->d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(S->pend_ev, s));
    S->pend_active = true; S->pend_blas = B;
    S->verts_host_stale[mesh] = 1;
    if (B == &hs.blas_top && !scene_needs_bounds(hs)) { B->refits++; return verdict; }
    const bool host_tlas = switches().host_tlas_update;
    if (B != &hs.blas_top && !scene_needs_bounds(hs) && !host_tlas && hs.has_tlas && !hs.tlas_order.empty()) {
        /* an instanced mesh: the boxes of the group's instances move with its vertices.  The instance level keeps its topology and is REFITTED on the device like the
         * BLAS -- every leaf record's exact world-space bound (k_instance_boxes), then the TLAS nodes deepest level first -- so this update waits for nothing either.
         * (The host's cached instance boxes and the group's box are marked stale and re-derived from the refreshed vertices before the next HOST build of the TLAS.) */
        if (ensure_tlas_refit_tables(S, s)) return 1;
        launch_instance_boxes(s, D, (uint32_t) hs.inst_recs.size(), S->d_inst_vrange, S->d_inst_box);
        const size_t n_blas = 1 + hs.blas_groups.size();
        HIP_TRY(hipMemsetAsync(S->d_area + n_blas, 0, sizeof(float), s));
        for (size_t l = 0; l + 1 < hs.tlas_levels.size(); ++l)
            launch_refit_nodes(s, D, S->d_tlas_order + hs.tlas_levels[l], hs.tlas_levels[l + 1] - hs.tlas_levels[l], S->d_inst_box, S->node_box, S->d_area + n_blas);
        HIP_TRY(hipGetLastError());
        const size_t g = (size_t) (B - hs.blas_groups.data());
        if (hs.group_box_stale.size() != hs.groups.size()) hs.group_box_stale.assign(hs.groups.size(), 0);
        hs.group_box_stale[g] = 1;
        for (size_t i = 0; i < hs.insts.size(); ++i) if (hs.inst_group[i] == g) hs.inst_box_valid[i] = 0;
        B->refits++;
        return verdict;
    }
    /* environment / directional emitters follow the scene's bounding sphere (and HAR_HOST_TLAS_UPDATE keeps the instance level a host build): host builds over exact
     * vertex bounds, so these updates read the mesh back (32 B per vertex, device -> host) and wait -- still no host -> device copy of geometry */
    if (refresh_host_geometry(S, s)) return 1;
    const int now = collect_pending_refit(S);
    if (now == 1) return 1;
    std::string e;
    if (!scene_after_refit_host(hs, B, e)) return fail(e);
    if (B != &hs.blas_top && upload_instance_level(S, s)) return 1;
    if (upload_scene_bounds(S, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return now ? now : verdict;
}
int har_scene_update_instances_device(HarScene S, uint32_t first, uint32_t count, const float *to_world, void *stream) {
    if (!S || !to_world) return fail("null argument");
    if (count == 0) return 0;
    HostScene &hs = S->hs; DScene &D = S->ds;
    hipStream_t s = (hipStream_t) stream;
    if ((uint64_t) first + count > hs.insts.size()) return fail("instance range out of bounds");
    if (!hs.has_tlas) return fail("the scene has no instances");
    /* what the previous device-resident instance update reported (its launches finished a frame ago) */
    if (S->pend_inst_active) {
        HIP_TRY(hipEventSynchronize(S->pend_inst_ev)); S->pend_inst_active = false;
        if (*S->pend_inst) return fail("har_scene_update_instances_device: an instance transform of the last update was singular or not finite (that instance kept its old transform)");
    }
    const bool host_tlas = switches().host_tlas_update;
    if (scene_needs_bounds(hs) || host_tlas || hs.tlas_order.empty()) {
        /* emitters that follow the scene's bounding sphere: the host path (read the matrices back, invert, rebuild the instance level and the bounds) */
        std::vector<float> tw(12 * (size_t) count), to(12 * (size_t) count);
        HIP_TRY(hipMemcpyAsync(tw.data(), to_world, tw.size() * sizeof(float), hipMemcpyDeviceToHost, s)); HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < count; ++k) if (!affine_inverse(tw.data() + 12 * (size_t) k, to.data() + 12 * (size_t) k)) return fail("instance transform is singular or not finite");
        return har_scene_update_instances(S, first, count, tw.data(), to.data(), stream);
    }
    if (ensure_refit_scratch(S, s) || ensure_tlas_refit_tables(S, s)) return 1;
    if (!S->pend_inst) {
        HIP_TRY(hipHostMalloc((void **) &S->pend_inst, sizeof(uint32_t), hipHostMallocDefault)); *S->pend_inst = 0u;
        HIP_TRY(hipEventCreateWithFlags(&S->pend_inst_ev, hipEventDisableTiming));
        void *p = nullptr; HIP_TRY(dev_alloc(&p, sizeof(uint32_t))); S->owned.push_back(p); S->d_bad_inst = (uint32_t *) p;
    }
    /* transforms + inverses into the shading records and the TLAS leaf records, the instances' exact world-space bounds, the TLAS nodes deepest level first: the instance
     * level keeps the topology of its last host build (a refit, like the BLAS after a vertex update) */
    HIP_TRY(hipMemsetAsync(S->d_bad_inst, 0, sizeof(uint32_t), s));
    launch_set_instances(s, D, S->d_rec_of, first, count, to_world, S->d_bad_inst);
    launch_instance_boxes(s, D, (uint32_t) hs.inst_recs.size(), S->d_inst_vrange, S->d_inst_box);
    const size_t n_blas = 1 + hs.blas_groups.size();
    HIP_TRY(hipMemsetAsync(S->d_area + n_blas, 0, sizeof(float), s));
    for (size_t l = 0; l + 1 < hs.tlas_levels.size(); ++l)
        launch_refit_nodes(s, D, S->d_tlas_order + hs.tlas_levels[l], hs.tlas_levels[l + 1] - hs.tlas_levels[l], S->d_inst_box, S->node_box, S->d_area + n_blas);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S->pend_inst, S->d_bad_inst, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(S->pend_inst_ev, s));
    S->pend_inst_active = true; S->insts_host_stale = true;
    for (uint32_t k = 0; k < count; ++k) hs.inst_box_valid[first + k] = 0;
    return 0;
}
int har_scene_get_instances(HarScene S, uint32_t first, uint32_t count, float *to_world, float *to_object, void *stream) {
    if (!S || !to_world || !to_object) return fail("null argument");
    if ((uint64_t) first + count > S->hs.insts.size()) return fail("instance range out of bounds");
    if (refresh_host_instances(S, (hipStream_t) stream)) return 1;
    for (uint32_t k = 0; k < count; ++k) { std::memcpy(to_world + 12 * (size_t) k, S->hs.insts[first + k].to_world, 48); std::memcpy(to_object + 12 * (size_t) k, S->hs.insts[first + k].to_object, 48); }
    return 0;
}
int har_scene_get_vertices(HarScene S, uint32_t mesh, float *vertices, void *stream) {
    if (!S || !vertices) return fail("null argument");
    if (mesh >= S->hs.meshes.size()) return fail("invalid mesh index");
    if (refresh_host_vertices(S, (hipStream_t) stream, (int) mesh)) return 1;
    const DMesh &m = S->hs.meshes[mesh];
    std::memcpy(vertices, S->hs.verts.data() + 8 * (size_t) m.voff, 32 * (size_t) m.vertex_count);
    return 0;
}
int har_scene_refit_info(HarScene S, double info[4]) {
    if (!S || !info) return fail("null argument");
    uint32_t refits = S->hs.blas_top.refits; for (const BlasInfo &b : S->hs.blas_groups) refits += b.refits;
    info[0] = (double) refits; info[1] = S->last_refit_cost; info[2] = S->last_refit_ratio; info[3] = (double) S->hs.nodes.size();
    return 0;
}

extern "C++" int read_status(int *d_status, hipStream_t s) {
    int st = 0;
    HIP_TRY(hipMemcpyAsync(&st, d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st == HAR_STACK_OVERFLOW) return fail("BVH traversal stack overflow (scene too deep for the LDS stack)");
    return 0;
}

int har_ray_intersect_preliminary(HarScene S, uint32_t n, const float *o, const float *d, const float *maxt, const uint8_t *active, int naive, float *t, float *u,
                                  float *v, uint32_t *prim, uint32_t *shape, uint32_t *inst, void *stream) {
    if (!S) return fail("null scene");
    if (n == 0) return 0;
    int *st = nullptr; HIP_TRY(dev_alloc((void **) &st, sizeof(int))); HIP_TRY(hipMemsetAsync(st, 0, sizeof(int), (hipStream_t) stream));
    launch_api_intersect((hipStream_t) stream, S->ds, n, o, d, maxt, active, naive, t, u, v, prim, shape, inst, st);
    HIP_TRY(hipGetLastError());
    int rc = read_status(st, (hipStream_t) stream); dev_free(st);
    return rc;
}
int har_ray_test(HarScene S, uint32_t n, const float *o, const float *d, const float *maxt, const uint8_t *active, int naive, uint8_t *hit, void *stream) {
    if (!S) return fail("null scene");
    if (n == 0) return 0;
    int *st = nullptr; HIP_TRY(dev_alloc((void **) &st, sizeof(int))); HIP_TRY(hipMemsetAsync(st, 0, sizeof(int), (hipStream_t) stream));
    launch_api_ray_test((hipStream_t) stream, S->ds, n, o, d, maxt, active, naive, hit, st);
    HIP_TRY(hipGetLastError());
    int rc = read_status(st, (hipStream_t) stream); dev_free(st);
    return rc;
}
/* RayFlags the entry points accept (interaction.h:19-87): unknown bits and FollowShape together with DetachShape are refused, never ignored */
static int check_ray_flags(uint32_t ray_flags) {
    if (ray_flags & ~(uint32_t) RAY_KNOWN_FLAGS) return fail("ray_flags: unknown RayFlags bits (known: Minimal 0, Shading 1, NormalPartials 2, FollowShape 4, DetachShape 8)");
    if ((ray_flags & RAY_FOLLOW_SHAPE) && (ray_flags & RAY_DETACH_SHAPE)) return fail("ray_flags: at most one of FollowShape and DetachShape can be specified");
    return 0;
}
int har_compute_surface_interaction(HarScene S, uint32_t n, const float *o, const float *d, const float *t, const float *u, const float *v,
                                    const uint32_t *prim, const uint32_t *shape, const uint32_t *inst, uint32_t ray_flags, const uint8_t *active, float *out, void *stream) {
    if (!S) return fail("null scene");
    if (check_ray_flags(ray_flags)) return 1;
    if (n == 0) return 0;
    launch_api_si((hipStream_t) stream, S->ds, n, o, d, t, u, v, prim, shape, inst, ray_flags, active, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_ray_intersect(HarScene S, uint32_t n, const float *o, const float *d, const float *maxt, uint32_t ray_flags, const uint8_t *active, int naive, float *t, float *u,
                      float *v, uint32_t *prim, uint32_t *shape, uint32_t *inst, float *si, void *stream) {
    if (!S) return fail("null scene");
    if (check_ray_flags(ray_flags)) return 1;
    if (har_ray_intersect_preliminary(S, n, o, d, maxt, active, naive, t, u, v, prim, shape, inst, stream)) return 1;
    return har_compute_surface_interaction(S, n, o, d, t, u, v, prim, shape, inst, ray_flags, active, si, stream);
}
int har_sampler_seed(uint32_t seed, uint32_t lane_offset, uint32_t n, uint64_t *state, uint64_t *inc, void *stream) {
    if (n == 0) return 0;
    launch_api_sampler_seed((hipStream_t) stream, seed, lane_offset, n, state, inc);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_sampler_next_1d(uint32_t n, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out, void *stream) {
    if (n == 0) return 0;
    launch_api_sampler_next((hipStream_t) stream, n, state, inc, active, out, 1);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_sampler_next_2d(uint32_t n, uint64_t *state, const uint64_t *inc, const uint8_t *active, float *out, void *stream) {
    if (n == 0) return 0;
    launch_api_sampler_next((hipStream_t) stream, n, state, inc, active, out, 2);
    HIP_TRY(hipGetLastError());
    return 0;
}
/* HarBSDFContext -> BsdfCtx; NULL = BSDFContext() (Radiance, all lobes, all components) */
static int lower_ctx(const HarBSDFContext *ctx, BsdfCtx &out) {
    out = BsdfCtx();
    if (!ctx) return 0;
    if (ctx->mode > 1u) return fail("HarBSDFContext::mode must be 0 (TransportMode::Radiance) or 1 (TransportMode::Importance)");
    out.mode = ctx->mode; out.type_mask = ctx->type_mask; out.component = ctx->component;
    return 0;
}
/* is record `bsdf` a bumpmap (possibly under an outer one-BSDF `twosided`, which is a flag of the same record)?  Such a record needs the entries that carry the interaction */
static bool bsdf_reaches_bumpmap(HarScene S, uint32_t bsdf) { return S->hs.bsdfs[bsdf].type == BSDF_BUMPMAP; }
static int bsdf_eval_common(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo, const uint8_t *active,
                            float *value, float *pdf, void *stream) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (S->ds.bsdf_types & HAR_SCENE_ATTR) return fail("mesh_attribute: BSDF::eval / pdf see a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
    if (bsdf_reaches_bumpmap(S, bsdf)) return fail("bumpmap: BSDF::eval / pdf of a `bumpmap` record read si.n, si.sh_frame, si.dp_du and si.dp_dv: use har_bsdf_eval_pdf_si");
    BsdfCtx c; if (lower_ctx(ctx, c)) return 1;
    if (n == 0) return 0;
    if (!wi || !uv || !wo) return fail("null wi / uv / wo");
    launch_api_bsdf_eval_pdf((hipStream_t) stream, S->ds, bsdf, c, n, wi, uv, wo, active, value, pdf);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_bsdf_eval_pdf(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo, const uint8_t *active,
                      float *value, float *pdf, void *stream) {
    if (!value || !pdf) return fail("null value / pdf");
    return bsdf_eval_common(S, bsdf, ctx, n, wi, uv, wo, active, value, pdf, stream);
}
int har_bsdf_eval(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo, const uint8_t *active, float *value, void *stream) {
    if (!value) return fail("null value");
    return bsdf_eval_common(S, bsdf, ctx, n, wi, uv, wo, active, value, nullptr, stream);
}
int har_bsdf_pdf(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo, const uint8_t *active, float *pdf, void *stream) {
    if (!pdf) return fail("null pdf");
    return bsdf_eval_common(S, bsdf, ctx, n, wi, uv, wo, active, nullptr, pdf, stream);
}
int har_bsdf_sample(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *sample1, const float *sample2,
                    const uint8_t *active, float *wo, float *pdf, float *weight, float *eta, uint32_t *sampled_type, uint32_t *sampled_component, void *stream) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (S->ds.bsdf_types & HAR_SCENE_ATTR) return fail("mesh_attribute: BSDF::sample sees a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
    if (bsdf_reaches_bumpmap(S, bsdf)) return fail("bumpmap: BSDF::sample of a `bumpmap` record reads si.n, si.sh_frame, si.dp_du and si.dp_dv: use har_bsdf_sample_si");
    BsdfCtx c; if (lower_ctx(ctx, c)) return 1;
    if (n == 0) return 0;
    if (!wi || !uv || !sample2 || !wo || !pdf || !weight) return fail("null input / output arrays");
    launch_api_bsdf_sample((hipStream_t) stream, S->ds, bsdf, c, n, wi, uv, sample1, sample2, active, wo, pdf, weight, eta, sampled_type, sampled_component);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_emitter_sample_direction(HarScene S, uint32_t emitter, uint32_t n, const float *ref_p, const float *sample, const uint8_t *active,
                                 float *d, float *dist, float *pdf, float *p, float *nrm, float *uv, float *spec, void *stream) {
    if (!S || emitter >= S->hs.emitters.size()) return fail("invalid emitter index");
    if (S->hs.emitters[emitter].type != 8u) return fail("har_emitter_sample_direction: implemented for a `projector` (emitter type 8); the other emitters are sampled by the renders only");
    (void) sample;          /* Projector::sample_direction ignores its sample (projector.cpp:203) */
    if (n == 0) return 0;
    if (!ref_p || !d || !dist || !pdf || !p || !nrm || !uv || !spec) return fail("null input / output arrays");
    launch_api_emitter_sample_direction((hipStream_t) stream, S->ds, emitter, n, ref_p, active, d, dist, pdf, p, nrm, uv, spec);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_bsdf_eval_pdf_si(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *wo, const float *geom,
                         const uint8_t *active, float *value, float *pdf, void *stream) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (S->ds.bsdf_types & HAR_SCENE_ATTR) return fail("mesh_attribute: BSDF::eval / pdf see a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
    if (!value && !pdf) return fail("null value / pdf");
    BsdfCtx c; if (lower_ctx(ctx, c)) return 1;
    if (n == 0) return 0;
    if (!wi || !uv || !wo || !geom) return fail("null wi / uv / wo / geom");
    launch_api_bsdf_eval_pdf_si((hipStream_t) stream, S->ds, bsdf, c, n, wi, uv, wo, geom, active, value, pdf);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_bsdf_sample_si(HarScene S, uint32_t bsdf, const HarBSDFContext *ctx, uint32_t n, const float *wi, const float *uv, const float *sample1, const float *sample2, const float *geom,
                       const uint8_t *active, float *wo, float *pdf, float *weight, float *eta, uint32_t *sampled_type, uint32_t *sampled_component, void *stream) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (S->ds.bsdf_types & HAR_SCENE_ATTR) return fail("mesh_attribute: BSDF::sample sees a uv, not the shape that was hit; not available for a scene with a `mesh_attribute` texture");
    BsdfCtx c; if (lower_ctx(ctx, c)) return 1;
    if (n == 0) return 0;
    if (!wi || !uv || !sample2 || !geom || !wo || !pdf || !weight) return fail("null input / output arrays");
    launch_api_bsdf_sample_si((hipStream_t) stream, S->ds, bsdf, c, n, wi, uv, sample1, sample2, geom, active, wo, pdf, weight, eta, sampled_type, sampled_component);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_bsdf_alpha(HarScene S, uint32_t bsdf, uint32_t n, const float *uv, float *alpha_u, float *alpha_v, void *stream) {
    if (!S || bsdf >= S->hs.bsdfs.size()) return fail("invalid bsdf index");
    if (n == 0) return 0;
    if (!uv || !alpha_u || !alpha_v) return fail("null uv / alpha_u / alpha_v");
    launch_api_bsdf_alpha((hipStream_t) stream, S->ds, bsdf, n, uv, alpha_u, alpha_v);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_sensor_sample_ray_aperture(const HarSensor *sensor, uint32_t n, const float *px, const float *py, const float *ax, const float *ay, float *o, float *d, float *maxt, void *stream) {
    DSensor C; std::string e;
    if (!sensor || !lower_sensor(*sensor, C, e)) return fail(e.empty() ? "null sensor" : e);
    if (n == 0) return 0;
    if (!px || !py || !o || !d || !maxt || (!ax != !ay)) return fail("null input / output arrays");
    launch_api_sensor_ray((hipStream_t) stream, C, n, px, py, ax, ay, o, d, maxt);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_sensor_sample_ray(const HarSensor *sensor, uint32_t n, const float *px, const float *py, float *o, float *d, float *maxt, void *stream) {
    return har_sensor_sample_ray_aperture(sensor, n, px, py, nullptr, nullptr, o, d, maxt, stream);
}
static int lower_batch_children(const HarSensor *children, uint32_t n, std::vector<DCamera> &cams, uint32_t &aperture) {
    std::string e;
    return har::lower_batch_children(children, n, cams, aperture, e) ? 0 : fail(e);
}
int har_integrator_set_batch_sensors(HarIntegrator I, const HarSensor *children, uint32_t n, void *stream) {
    if (!I) return fail("null integrator");
    if (n == 0) { I->set.batch = DBatch{ nullptr, 0u, 0u }; return 0; }
    std::vector<DCamera> cams; uint32_t aperture = 0u;
    if (lower_batch_children(children, n, cams, aperture)) return 1;
    if (I->batch_cap < n) {
        (void) hipDeviceSynchronize();      /* renders in flight may still read the old table */
        dev_free(I->batch_cams, true); I->batch_cams = nullptr; I->batch_cap = 0; I->set.batch = DBatch{ nullptr, 0u, 0u };
        HIP_TRY(dev_alloc((void **) &I->batch_cams, (size_t) n * sizeof(DCamera)));
        I->batch_cap = n;
    }
    /* in stream order behind the renders that read the previous table; the host copy lives until the copy has run */
    HIP_TRY(hipMemcpyAsync(I->batch_cams, cams.data(), (size_t) n * sizeof(DCamera), hipMemcpyHostToDevice, (hipStream_t) stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t) stream));
    I->set.batch = DBatch{ I->batch_cams, n, aperture };
    return 0;
}
int har_batch_sample_ray(const HarSensor *children, uint32_t n_children, uint32_t n, const float *px, const float *py, float *o, float *d, float *maxt, void *stream) {
    return har_batch_sample_ray_aperture(children, n_children, n, px, py, nullptr, nullptr, o, d, maxt, stream);
}
int har_batch_sample_ray_aperture(const HarSensor *children, uint32_t n_children, uint32_t n, const float *px, const float *py, const float *ax, const float *ay,
                                  float *o, float *d, float *maxt, void *stream) {
    if (n_children == 0) return fail("BatchSensor: at least one child sensor must be specified!");
    std::vector<DCamera> cams; uint32_t aperture = 0u;
    if (lower_batch_children(children, n_children, cams, aperture)) return 1;
    if (n == 0) return 0;
    if (!px || !py || !o || !d || !maxt || (!ax != !ay)) return fail("null input / output arrays");
    DCamera *dc = nullptr;
    HIP_TRY(dev_alloc((void **) &dc, cams.size() * sizeof(DCamera)));
    hipError_t err = hipMemcpyAsync(dc, cams.data(), cams.size() * sizeof(DCamera), hipMemcpyHostToDevice, (hipStream_t) stream);
    if (err == hipSuccess) { launch_api_batch_ray((hipStream_t) stream, DBatch{ dc, n_children, aperture }, n, px, py, ax, ay, o, d, maxt); err = hipGetLastError(); }
    if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t) stream);
    dev_free(dc);
    HIP_TRY(err);
    return 0;
}
int har_film_put(const HarSensor *sensor, uint32_t n, const float *px, const float *py, const float *values4, float *film, void *stream) {
    DSensor C; std::string e;
    if (!sensor || !lower_sensor(*sensor, C, e)) return fail(e.empty() ? "null sensor" : e);
    if (n == 0) return 0;
    launch_api_film_put((hipStream_t) stream, C, n, px, py, values4, film);
    HIP_TRY(hipGetLastError());
    return 0;
}
int har_film_develop(const float *film, uint32_t width, uint32_t height, float *image, void *stream) {
    return har_film_develop_format(film, width, height, HAR_PIXEL_RGB, image, stream);
}
int har_film_develop_format(const float *film, uint32_t width, uint32_t height, int pixel_format, float *image, void *stream) {
    if (!film || !image) return fail("null film / image");
    if (pixel_format != HAR_PIXEL_RGB && pixel_format != HAR_PIXEL_Y && pixel_format != HAR_PIXEL_XYZ) return fail("har_film_develop_format: pixel_format must be HAR_PIXEL_RGB, _Y or _XYZ");
    launch_develop((hipStream_t) stream, film, width * height, image, pixel_format);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // extern "C"
