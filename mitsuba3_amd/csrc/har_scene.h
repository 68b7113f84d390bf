/*
 * har_scene.h -- device-side scene records and the per-vertex shading math of
 * the hip_ad_rgb path (surface interaction, diffuse BSDF, bitmap/srgb texture,
 * area emitter, perspective sensor, reconstruction filter).  HAR_HD so that the
 * same source runs in the HIP kernels and in the host test harness.
 * Each function cites the reference code it reproduces.
 */
#pragma once
#include "har_accel.h"
#include "har_bsdf.h"

namespace har {

struct DMesh    { uint32_t voff, foff, bsdf; int32_t emitter; uint32_t flags, face_count, vertex_count, pad1; };
/* mode: HarTexture::mode (bit 0 nearest, bit 1 mirror, bit 2 clamp), bit 31 (HAR_TEX_HAS_UV_XF): `uvm` is not the identity; uvm = BitmapTexture's `to_uv`
 * (bitmap.cpp:175), row-major 2 x 3 -- tex_taps applies it to the surface's uv before the lookup (bitmap.cpp:565,792,831,847) */
#define HAR_TEX_HAS_UV_XF 0x80000000u
/* bit 3 (HAR_TEX_ATTRIBUTE): not a bitmap but an attribute of ONE mesh (the `mesh_attribute` texture, src/textures/mesh_attribute.cpp): `data` = h rows of three floats
 * (w = 1; a one-channel attribute is stored three times), one row per vertex -- or, with bit 4 (HAR_TEX_ATTRIBUTE_FACE), per face -- of that mesh; pad = the mesh's first
 * face in DScene::faces, uvm[0] = `scale`.  Looked up by attr_taps / attr_fetch from an AttrAddr, never from a uv */
#define HAR_TEX_ATTRIBUTE 8u
#define HAR_TEX_ATTRIBUTE_FACE 16u
struct DTexture { const float *data; uint32_t w, h; uint32_t mode, pad; float uvm[6]; };
/* type 0: AreaLight on a rectangle (to_world, normal, inv_area, mesh); type 1: ConstantBackgroundEmitter
 * (src/emitters/constant.cpp): to_world[0..2] = bounding sphere centre, to_world[3] = radius, mesh = 0xffffffff; type 2: environment map
 * (DEnvmap); type 3: AreaLight on a triangle mesh: mesh, inv_area = 1 / surface area, to_world[0] / [1] = bit patterns of the offset of its
 * table in DScene::emitter_cdf and of its face count, to_world[2] = sum of the face areas; types 4 - 6 (point / spot / directional), 7 (bitmap area light) and 8
 * (projector): at their sample_direction functions below */
#ifndef HAR_SHADING_TRIS
/* 1 (default since round 5): compute_si reads ONE pre-gathered 96-byte block per face (its three vertex records, DScene::shade_tris) instead of face -> three scattered
 * vertices: one level of dependent loads less, one or two cache lines instead of three or four.  Bracketed A/B on one box (profiles/r05_ab_shading_tris.txt): k_shade
 * 10.5 -> 10.2 ms on instanced1m, 24.5 -> 23.85 ms on materials1m, flat1m unchanged; forward +0.5 %; GPU suite green on both builds.  Costs 96 B per face of HBM. */
#define HAR_SHADING_TRIS 1
#endif
struct DEmitter { float radiance[3]; float inv_area; float to_world[12]; float normal[3]; uint32_t mesh; uint32_t type; };
/* type 7 (area light on a rectangle with a BITMAP radiance): radiance[0] = bits of the texture index, radiance[1] = bits of the offset of its texel distribution in
 * DScene::emitter_cdf, radiance[2] = |dp_du x dp_dv| of the rectangle; the table: HAR_TEXEL_TABLE_HEADER floats { sum, 1 / sum, inverse to_uv (2 x 3) }, the marginal
 * running sums (h), the conditional ones (w * h) -- texel_table_fill in har_scene_host.cpp */
#define HAR_TEXEL_TABLE_HEADER 8u
struct DInst    { float to_world[12]; float to_object[12]; };
/* EnvironmentMapEmitter (src/emitters/envmap.cpp), emitter type 2.  `tex` = H x (W + 2) x 3 radiance with one halo column on each side
 * (:140-172), `warp` = storage of the Hierarchical2D<Float, 0> over the (W + 1) x H luminance * sin(theta) grid (distr_2d.h:405-560):
 * level 0 row-major, levels >= 1 in 2 x 2 blocks; lvl_offset / lvl_width index it. */
#define HAR_ENV_MAX_LEVELS 18
struct DEnvmap {
    const float *tex, *warp;
    uint32_t w, h, n_levels; float scale;
    float to_world[12], to_local[12];       /* column-major 3 x 4 */
    float center[3], radius;                /* scene bounding sphere (set_scene, :214-226) */
    uint32_t lvl_offset[HAR_ENV_MAX_LEVELS], lvl_width[HAR_ENV_MAX_LEVELS];
    uint32_t tex_index;                     /* the image's entry of the scene's texture table (where its gradient lives: grad_textures, envmap_taps) */
};

struct DScene {
    Accel accel;
    const uint32_t *blas_tri_ranges;   /* per TLAS record: first, count (brute-force kernel) */
    const float    *verts;             /* packed vertices, 8 f32 each (mesh_utils.h:19-34) */
#if HAR_SHADING_TRIS
    const float    *shade_tris;        /* the three vertex records of every face, 24 f32 per face in face order (see compute_si) */
#endif
    const uint32_t *faces;             /* packed faces, 4 u32 each */
    const DMesh    *meshes;
    const DBsdf    *bsdfs;
    const DTexture *textures;
    const DEmitter *emitters;
    const DInst    *insts;
    const float    *bsdf_tables;       /* roughplastic external transmittance tables, 64 floats each */
    uint32_t n_emitters, n_meshes, n_bsdfs, n_textures, n_insts;      /* n_insts: records of `insts` (the scene's instances) */
    int32_t  env_emitter;              /* index of the environment emitter (Scene::environment()), or -1 */
    uint32_t bsdf_types;               /* bit mask (1 << type) of the BSDF types present (+ bit 31: some record is twosided) */
    const DEnvmap *envmap;             /* device record of the environment map when emitters[env_emitter].type == 2 */
    const float   *emitter_cdf;        /* face-area tables of the mesh emitters (type 3): per emitter `count` unnormalised pmf values, then `count` cdf values */
    /* Scene::m_emitter_distr (scene.cpp:120-141): NULL = uniform emitter selection (every sampling_weight is 1); otherwise n_emitters unnormalised pmf values (the
     * weights), then n_emitters cdf values (running sums accumulated in double, distr_1d.h:236-266), with their sum, 1 / sum and the first / last bin of non-zero weight */
    const float   *emitter_distr;
    float    emitter_sum, emitter_norm;
    uint32_t emitter_valid_lo, emitter_valid_hi;
    /* copy of emitters[0] for scenes with exactly one emitter (kernel argument = scalar registers); emitter0_valid = 0: use the array; 2: the radiance was updated on the
     * device (har_scene_set_emitter_radiance_device) -- those three floats come from the array, everything else from this copy (round 6: an emitter-optimisation loop
     * keeps the scalar-register path) */
    DEmitter emitter0; uint32_t emitter0_valid;
};

struct DSensor {
    float s2c[16];
    float to_world[16];
    float near_clip, far_clip;
    uint32_t crop_x, crop_y, crop_w, crop_h;
    uint32_t samp_w, samp_h, border;   /* the sample grid of render(): the crop window + `border` pixels on every side (Film::sample_border, integrator.cpp:162-165); border = 0: the crop */
    uint32_t rfilter;            /* 0 box, 1 gaussian, 2 tent, 3 mitchell, 4 catmullrom, 5 lanczos */
    float rf_p0, rf_p1;          /* filter parameters (HarSensor::rfilter_stddev / rfilter_param1) */
    float radius;
    float coeff[10];             /* GaussianFilter::m_coeff (LLVM branch) */
    /* scaled principal point offset: film size * principal_point_offset / crop size (perspective.cpp:213-214); a thin lens has none and keeps its aperture radius and
     * focus distance there (thinlens.cpp:156-161, sensor.cpp:127), as HarSensor does: the record -- a kernel argument, and a member of ShadeParams -- keeps its size */
    union { float ppo_x; float aperture_radius; };
    union { float ppo_y; float focus_distance; };
    uint32_t projection;         /* 0 perspective, 1 orthographic, 2 thin lens (HarSensor::projection) */
};
/* One child of a `batch` sensor (src/sensors/batch.cpp): the camera part of a DSensor lowered for the child's sub-film (film width / child count, full crop).  The
 * table of children lives in device memory (DBatch); the film part of the render -- lane -> pixel map, filter, splat -- stays the batch sensor's own DSensor. */
struct DCamera {
    float s2c[16];
    float to_world[16];
    float near_clip, far_clip;
    float ppo_x, ppo_y;
    uint32_t projection;
    float aperture_radius, focus_distance;
    uint32_t pad;
};
HAR_HD DCamera batch_camera(const DSensor &C) {
    DCamera c;
    for (int i = 0; i < 16; ++i) { c.s2c[i] = C.s2c[i]; c.to_world[i] = C.to_world[i]; }
    const bool lens = C.projection == 2u;
    c.near_clip = C.near_clip; c.far_clip = C.far_clip; c.ppo_x = lens ? 0.f : C.ppo_x; c.ppo_y = lens ? 0.f : C.ppo_y; c.projection = C.projection;
    c.aperture_radius = lens ? C.aperture_radius : 0.f; c.focus_distance = lens ? C.focus_distance : 0.f; c.pad = 0u;
    return c;
}
struct DBatch { const DCamera *cams; uint32_t n; uint32_t aperture; };      /* n == 0: no batch, the DSensor is the camera; aperture != 0: a child is a thin lens -- every lane draws an aperture sample */

struct SurfInt {
    float t;
    Vec3 p, n, sn, ss, st, wi;
    float uv_x, uv_y;
    uint32_t mesh;
    HAR_HD bool valid() const { return t != HAR_INF; }
    HAR_HD Vec3 to_local(Vec3 v) const { return Vec3(dot3(v, ss), dot3(v, st), dot3(v, sn)); }   /* frame.h:34 */
    HAR_HD Vec3 to_world(Vec3 v) const { return fma3(sn, v.z, fma3(st, v.y, ss * v.x)); }         /* frame.h:39 */
};

/* PreliminaryIntersection::compute_surface_interaction (interaction.h:804-829) ->
 * Mesh::compute_surface_interaction (src/render/mesh.cpp:2255-2437) [+ Instance::
 * compute_surface_interaction, src/shapes/instance.cpp:150-266] ->
 * finalize_surface_interaction (interaction.h:559-605; `diffuse` packs no tangents so
 * the frame comes from coordinate_system(sh_frame.n)) */
HAR_HD SurfInt compute_si(const DScene &S, Vec3 ray_d, float t, float bu, float bv, uint32_t prim, uint32_t shape, uint32_t inst) {
    SurfInt si;
    si.t = t; si.uv_x = 0.f; si.uv_y = 0.f; si.mesh = 0;
    if (t == HAR_INF) { si.wi = -ray_d; return si; }
    const DMesh M = S.meshes[shape];
#if HAR_SHADING_TRIS
    /* the face's three vertex records pre-gathered into ONE 96-byte block -- hit -> mesh record -> block instead of hit -> mesh record -> face -> three scattered
     * vertices */
    const float *r0 = S.shade_tris + 24 * (size_t) (M.foff + prim), *r1 = r0 + 8, *r2 = r0 + 16;
#else
    const uint32_t *f = S.faces + 4 * (size_t) (M.foff + prim);
    const float *r0 = S.verts + 8 * (size_t) (M.voff + f[0]);
    const float *r1 = S.verts + 8 * (size_t) (M.voff + f[1]);
    const float *r2 = S.verts + 8 * (size_t) (M.voff + f[2]);
#endif
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 qa0 = reinterpret_cast<const float4 *>(r0)[0], qa1 = reinterpret_cast<const float4 *>(r0)[1];
    const float4 qb0 = reinterpret_cast<const float4 *>(r1)[0], qb1 = reinterpret_cast<const float4 *>(r1)[1];
    const float4 qc0 = reinterpret_cast<const float4 *>(r2)[0], qc1 = reinterpret_cast<const float4 *>(r2)[1];
    const float v0[8] = { qa0.x, qa0.y, qa0.z, qa0.w, qa1.x, qa1.y, qa1.z, qa1.w };
    const float v1[8] = { qb0.x, qb0.y, qb0.z, qb0.w, qb1.x, qb1.y, qb1.z, qb1.w };
    const float v2[8] = { qc0.x, qc0.y, qc0.z, qc0.w, qc1.x, qc1.y, qc1.z, qc1.w };
#else
    const float *v0 = r0, *v1 = r1, *v2 = r2;
#endif
    Vec3 p0(v0[0], v0[1], v0[2]), p1(v1[0], v1[1], v1[2]), p2(v2[0], v2[1], v2[2]);
    float b1 = bu, b2 = bv, b0 = 1.f - b1 - b2;
    Vec3 e1 = p1 - p0, e2 = p2 - p0;
    si.p = fma3(p0, b0, fma3(p1, b1, p2 * b2));
    si.n = normalize3(cross3(e1, e2));                       /* mesh.h:568-572 */
    if (M.flags & 1u) {
        Vec3 n0(v0[3], v0[4], v0[5]), dn1 = Vec3(v1[3], v1[4], v1[5]) - n0, dn2 = Vec3(v2[3], v2[4], v2[5]) - n0;
        Vec3 n = fma3(dn1, b1, fma3(dn2, b2, n0));
        si.sn = n * rsqrt_(dot3(n, n));
    } else si.sn = si.n;
    if (M.flags & 2u) {
        float u0 = v0[6], w0 = v0[7], du0 = v1[6] - u0, dv0 = v1[7] - w0, du1 = v2[6] - u0, dv1 = v2[7] - w0;
        si.uv_x = fma_(du0, b1, fma_(du1, b2, u0));
        si.uv_y = fma_(dv0, b1, fma_(dv1, b2, w0));
    } else { si.uv_x = b1; si.uv_y = b2; }
    si.mesh = shape;
    if (inst != 0xffffffffu) {                              /* instance.cpp:196-224 */
        const DInst &I = S.insts[inst];
        si.p = xf_point(I.to_world, si.p);
        si.n = normalize3(xf_normal(I.to_object, si.n));
        Vec3 n = xf_normal(I.to_object, si.sn);
        si.sn = n * rcp_(norm3(n));
    }
    coordinate_system(si.sn, si.ss, si.st);
    si.wi = si.to_local(-ray_d);
    return si;
}

/* the same interaction from a hit record that carries the face's index in the shading-triangle array and the mesh's flags (HAR_HIT_MATINFO): no load of the mesh record */
HAR_HD SurfInt compute_si_record(const DScene &S, Vec3 ray_d, float t, float bu, float bv, uint32_t gface, uint32_t mesh_flags, uint32_t shape, uint32_t inst) {
    SurfInt si;
    si.t = t; si.uv_x = 0.f; si.uv_y = 0.f; si.mesh = 0;
    if (t == HAR_INF) { si.wi = -ray_d; return si; }
#if HAR_SHADING_TRIS
    const float *r0 = S.shade_tris + 24 * (size_t) gface, *r1 = r0 + 8, *r2 = r0 + 16;
#else
    const uint32_t *f = S.faces + 4 * (size_t) gface; const uint32_t voff = S.meshes[shape].voff;
    const float *r0 = S.verts + 8 * (size_t) (voff + f[0]), *r1 = S.verts + 8 * (size_t) (voff + f[1]), *r2 = S.verts + 8 * (size_t) (voff + f[2]);
#endif
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 qa0 = reinterpret_cast<const float4 *>(r0)[0], qa1 = reinterpret_cast<const float4 *>(r0)[1];
    const float4 qb0 = reinterpret_cast<const float4 *>(r1)[0], qb1 = reinterpret_cast<const float4 *>(r1)[1];
    const float4 qc0 = reinterpret_cast<const float4 *>(r2)[0], qc1 = reinterpret_cast<const float4 *>(r2)[1];
    const float v0[8] = { qa0.x, qa0.y, qa0.z, qa0.w, qa1.x, qa1.y, qa1.z, qa1.w };
    const float v1[8] = { qb0.x, qb0.y, qb0.z, qb0.w, qb1.x, qb1.y, qb1.z, qb1.w };
    const float v2[8] = { qc0.x, qc0.y, qc0.z, qc0.w, qc1.x, qc1.y, qc1.z, qc1.w };
#else
    const float *v0 = r0, *v1 = r1, *v2 = r2;
#endif
    Vec3 p0(v0[0], v0[1], v0[2]), p1(v1[0], v1[1], v1[2]), p2(v2[0], v2[1], v2[2]);
    float b1 = bu, b2 = bv, b0 = 1.f - b1 - b2;
    Vec3 e1 = p1 - p0, e2 = p2 - p0;
    si.p = fma3(p0, b0, fma3(p1, b1, p2 * b2));
    si.n = normalize3(cross3(e1, e2));
    if (mesh_flags & 1u) {
        Vec3 n0(v0[3], v0[4], v0[5]), dn1 = Vec3(v1[3], v1[4], v1[5]) - n0, dn2 = Vec3(v2[3], v2[4], v2[5]) - n0;
        Vec3 n = fma3(dn1, b1, fma3(dn2, b2, n0));
        si.sn = n * rsqrt_(dot3(n, n));
    } else si.sn = si.n;
    if (mesh_flags & 2u) {
        float u0 = v0[6], w0 = v0[7], du0 = v1[6] - u0, dv0 = v1[7] - w0, du1 = v2[6] - u0, dv1 = v2[7] - w0;
        si.uv_x = fma_(du0, b1, fma_(du1, b2, u0));
        si.uv_y = fma_(dv0, b1, fma_(dv1, b2, w0));
    } else { si.uv_x = b1; si.uv_y = b2; }
    si.mesh = shape;
    if (inst != 0xffffffffu) {
        const DInst &I = S.insts[inst];
        si.p = xf_point(I.to_world, si.p);
        si.n = normalize3(xf_normal(I.to_object, si.n));
        Vec3 n = xf_normal(I.to_object, si.sn);
        si.sn = n * rcp_(norm3(n));
    }
    coordinate_system(si.sn, si.ss, si.st);
    si.wi = si.to_local(-ray_d);
    return si;
}

/* RayFlags (include/mitsuba/render/interaction.h:19-87).  The wavefront kernels compute what RayFlags::Default asks for (compute_si above); the array-valued
 * Scene::ray_intersect / PreliminaryIntersection::compute_surface_interaction entry points honour the caller's flags through compute_si_flags.  FollowShape /
 * DetachShape only choose which AD dependence the reference tracks through the hit; the primal values are the same (the C ABI carries no AD graph). */
enum { RAY_MINIMAL = 0u, RAY_SHADING = 1u, RAY_NORMAL_PARTIALS = 2u, RAY_FOLLOW_SHAPE = 4u, RAY_DETACH_SHAPE = 8u, RAY_KNOWN_FLAGS = 15u };
struct SurfPartials { Vec3 dp_du, dp_dv, dn_du, dn_dv; };
/* Position / normal partials of Mesh::compute_surface_interaction (src/render/mesh.cpp:2334-2395: dn / d barycentric of the normalised interpolated normal,
 * change of variables to the texture parameterisation) and their transport through an instance (src/shapes/instance.cpp:206-212,250-253) */
HAR_HD void compute_si_partials(const DScene &S, float bu, float bv, uint32_t prim, uint32_t shape, uint32_t inst, bool normal_partials, SurfPartials &P) {
    const DMesh M = S.meshes[shape];
    const uint32_t *f = S.faces + 4 * (size_t) (M.foff + prim);
    const float *v0 = S.verts + 8 * (size_t) (M.voff + f[0]), *v1 = S.verts + 8 * (size_t) (M.voff + f[1]), *v2 = S.verts + 8 * (size_t) (M.voff + f[2]);
    const Vec3 p0(v0[0], v0[1], v0[2]), e1 = Vec3(v1[0], v1[1], v1[2]) - p0, e2 = Vec3(v2[0], v2[1], v2[2]) - p0;
    const float b1 = bu, b2 = bv;
    const bool need_dn = (M.flags & 1u) && normal_partials;
    Vec3 dn_db1(0.f), dn_db2(0.f), sn(0.f);
    if (M.flags & 1u) {
        Vec3 n0(v0[3], v0[4], v0[5]), dn1 = Vec3(v1[3], v1[4], v1[5]) - n0, dn2 = Vec3(v2[3], v2[4], v2[5]) - n0;
        Vec3 n = fma3(dn1, b1, fma3(dn2, b2, n0));
        const float il = rsqrt_(dot3(n, n));
        n = n * il; sn = n;
        if (need_dn) {
            dn1 = dn1 * il; dn2 = dn2 * il;
            dn_db1 = fma3(n, -dot3(n, dn1), dn1); dn_db2 = fma3(n, -dot3(n, dn2), dn2);        /* dr::fnmadd(n, dot(n, dn), dn) */
        }
    }
    P.dn_du = Vec3(0.f); P.dn_dv = Vec3(0.f);
    if (M.flags & 2u) {
        const float u0 = v0[6], w0 = v0[7], du0x = v1[6] - u0, du0y = v1[7] - w0, du1x = v2[6] - u0, du1y = v2[7] - w0;
        const float det = fms_(du0x, du1y, du0y * du1x), inv_det = det != 0.f ? rcp_(det) : 0.f;
        /* to_uv_basis(d1, d2) = ( fmsub(duv1.y, d1, duv0.y * d2), fnmadd(duv1.x, d1, duv0.x * d2) ) * inv_det */
        P.dp_du = Vec3(fms_(du1y, e1.x, du0y * e2.x), fms_(du1y, e1.y, du0y * e2.y), fms_(du1y, e1.z, du0y * e2.z)) * inv_det;
        P.dp_dv = Vec3(fnma_(du1x, e1.x, du0x * e2.x), fnma_(du1x, e1.y, du0x * e2.y), fnma_(du1x, e1.z, du0x * e2.z)) * inv_det;
        if (need_dn) {
            P.dn_du = Vec3(fms_(du1y, dn_db1.x, du0y * dn_db2.x), fms_(du1y, dn_db1.y, du0y * dn_db2.y), fms_(du1y, dn_db1.z, du0y * dn_db2.z)) * inv_det;
            P.dn_dv = Vec3(fnma_(du1x, dn_db1.x, du0x * dn_db2.x), fnma_(du1x, dn_db1.y, du0x * dn_db2.y), fnma_(du1x, dn_db1.z, du0x * dn_db2.z)) * inv_det;
        }
    } else {
        P.dp_du = e1; P.dp_dv = e2;
        if (need_dn) { P.dn_du = dn_db1; P.dn_dv = dn_db2; }
    }
    if (inst != 0xffffffffu) {
        const DInst &I = S.insts[inst];
        if (need_dn) {                  /* instance.cpp:206-212 (meshes without vertex normals: the partials are zero and stay zero) */
            Vec3 n = xf_normal(I.to_object, sn);
            const float inv_len = rcp_(norm3(n));
            n = n * inv_len;
            const Vec3 du = xf_normal(I.to_object, P.dn_du) * inv_len, dv = xf_normal(I.to_object, P.dn_dv) * inv_len;
            P.dn_du = fma3(n, -dot3(n, du), du); P.dn_dv = fma3(n, -dot3(n, dv), dv);
        }
        P.dp_du = xf_vector(I.to_world, P.dp_du); P.dp_dv = xf_vector(I.to_world, P.dp_dv);
    }
}

/* The shading frame of a shape that packs a tangent for a BSDFFlags::NormalMapped material (kernels of scenes with a `normalmap` record only).  The reference packs
 * per-vertex tangents (mesh.cpp:612-623, 2417-2429); here only shapes whose tangent IS the direction of the face's dp_du carry MESH_TANGENT_FRAME -- a rectangle, whose four
 * vertices share normalize(to_world * (1, 0, 0)) (rectangle.cpp:131-153) -- and every other mesh with normals and texcoords under a normalmap is refused at load.
 * finalize_surface_interaction (interaction.h:570-598): s = fnmadd(n, dot(n, s), s), normalised (coordinate_system(n) -- what compute_si left -- when it vanishes),
 * t = cross(n, s), negated where frame_flipped: the shape's bit (MESH_FRAME_FLIPPED: a mirroring to_world, flip_normals included, mesh.cpp:1160-1215) xor a mirroring
 * instance transform (instance.cpp:218-222).  Leaves every other mesh's interaction as it is. */
enum { MESH_TANGENT_FRAME = 4u, MESH_FRAME_FLIPPED = 8u };
HAR_HD void si_tangent_frame(const DScene &S, SurfInt &si, Vec3 ray_d, float bu, float bv, uint32_t prim, uint32_t shape, uint32_t inst) {
    if (si.t == HAR_INF) return;
    const uint32_t mf = S.meshes[shape].flags;
    if (!(mf & MESH_TANGENT_FRAME)) return;
    SurfPartials P; compute_si_partials(S, bu, bv, prim, shape, inst, false, P);
    bool flipped = (mf & MESH_FRAME_FLIPPED) != 0u;
    if (inst != 0xffffffffu) {
        const DInst &I = S.insts[inst];
        const Vec3 c0 = xf_vector(I.to_world, Vec3(1.f, 0.f, 0.f)), c1 = xf_vector(I.to_world, Vec3(0.f, 1.f, 0.f)), c2 = xf_vector(I.to_world, Vec3(0.f, 0.f, 1.f));
        if (dot3(c0, cross3(c1, c2)) < 0.f) flipped = !flipped;
    }
    const Vec3 s0 = normalize3(P.dp_du);
    const Vec3 s = fma3(si.sn, -dot3(si.sn, s0), s0);
    const float sqr_norm = dot3(s, s);
    if (sqr_norm > 0.f) { si.ss = s * rsqrt_(sqr_norm); si.st = cross3(si.sn, si.ss); }
    if (flipped) si.st = -si.st;
    si.wi = si.to_local(-ray_d);
}

/* One lane of the array-valued PreliminaryIntersection::compute_surface_interaction in a scene with a `normalmap` record (k_api_si_nmap and its host twin,
 * har_surface_interaction_host): the 33 rows of k_api_si (har_kernels.hip) with the tangent frame above in sh_frame.s / .t and wi */
HAR_HD void si_rows_tangent(const DScene &S, uint32_t n, uint32_t i, Vec3 D, float t, float u, float v, uint32_t prim, uint32_t shape, uint32_t inst, uint32_t ray_flags, bool active, float *out) {
    const bool shading = (ray_flags & RAY_SHADING) != 0u, valid = active && t != HAR_INF;
    Vec3 vs[6] = { Vec3(0.f), Vec3(0.f), Vec3(0.f), Vec3(0.f), Vec3(0.f), Vec3(0.f) };
    float uvx = 0.f, uvy = 0.f;
    SurfPartials P; P.dp_du = Vec3(0.f); P.dp_dv = Vec3(0.f); P.dn_du = Vec3(0.f); P.dn_dv = Vec3(0.f);
    if (valid) {
        SurfInt si = compute_si(S, D, t, u, v, prim, shape, inst);
        vs[0] = si.p; vs[1] = si.n;
        if (shading) {
            si_tangent_frame(S, si, D, u, v, prim, shape, inst);
            vs[2] = si.sn; vs[3] = si.ss; vs[4] = si.st; vs[5] = si.wi; uvx = si.uv_x; uvy = si.uv_y;
            compute_si_partials(S, u, v, prim, shape, inst, (ray_flags & RAY_NORMAL_PARTIALS) != 0u, P);
        }
    } else if (shading) { coordinate_system(Vec3(0.f), vs[3], vs[4]); vs[5] = -D; }
    for (int k = 0; k < 6; ++k) { out[(3 * k) * (size_t) n + i] = vs[k].x; out[(3 * k + 1) * (size_t) n + i] = vs[k].y; out[(3 * k + 2) * (size_t) n + i] = vs[k].z; }
    out[18 * (size_t) n + i] = uvx; out[19 * (size_t) n + i] = uvy; out[20 * (size_t) n + i] = valid ? t : HAR_INF;
    const Vec3 ps[4] = { P.dp_du, P.dp_dv, P.dn_du, P.dn_dv };
    for (int k = 0; k < 4; ++k) { out[(21 + 3 * k) * (size_t) n + i] = ps[k].x; out[(22 + 3 * k) * (size_t) n + i] = ps[k].y; out[(23 + 3 * k) * (size_t) n + i] = ps[k].z; }
}

/* Interaction::offset_p / spawn_ray / spawn_ray_to (interaction.h:161-191) */
HAR_HD Vec3 offset_p(const SurfInt &si, Vec3 d) {
    float mag = (1.f + hmax3(abs3(si.p))) * HAR_RAY_EPS;
    mag = mulsign_(mag, dot3(si.n, d));
    return fma3(si.n, mag, si.p);
}
HAR_HD void spawn_ray_to(const SurfInt &si, Vec3 target, Vec3 &o, Vec3 &d, float &maxt) {
    o = offset_p(si, target - si.p);
    Vec3 dd = target - o;
    float dist = norm3(dd);
    d = div3(dd, dist);
    maxt = dist * (1.f - HAR_SHADOW_EPS);
}

/* dr::Texture<Float, 2>::eval (call site bitmap.cpp:842-850; Dr.Jit's texture.h is NOT IN TREE -- parity unpinned): texel centres at (i + 1/2) / res; the integer
 * texel index is wrapped by WrapMode Repeat (i mod res), Clamp (clip to [0, res - 1]) or Mirror (the image flipped every other repetition, so that index -1 is
 * texel 0 and index res is texel res - 1); FilterMode::Nearest takes the texel under floor(uv * res), Linear blends the four around uv * res - 1/2. */
struct TexTaps { uint32_t idx[4]; float w0x, w1x, w0y, w1y; };
HAR_HD int32_t tex_wrap(int32_t i, int32_t n, uint32_t mode) {
    if (mode & 4u) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);                       /* clamp */
    const int32_t shifted = i < 0 ? i + 1 : i, div = shifted / n;                     /* truncating division, as the reference's integer divisor */
    int32_t mod = i - div * n;
    if (mod < 0) mod += n;
    if ((mode & 2u) && (((div & 1) == 0) == (i < 0))) mod = n - 1 - mod;              /* mirror: flip unless (even repetition) xor (negative side) */
    return mod;
}
HAR_HD void tex_taps(const DTexture &T, float u, float v, TexTaps &l) {
    const int32_t W = (int32_t) T.w, H = (int32_t) T.h;
    if (T.mode & HAR_TEX_HAS_UV_XF) {                                                    /* uv = m_transform * si.uv (bitmap.cpp:847; AffineTransform * Point, transform.h:322-335) */
        const float tu = fma_(T.uvm[1], v, fma_(T.uvm[0], u, T.uvm[2])), tv = fma_(T.uvm[4], v, fma_(T.uvm[3], u, T.uvm[5]));
        u = tu; v = tv;
    }
    if (T.mode & 1u) {                                                                 /* nearest: one texel, written as four coincident taps of weight (1, 0) */
        const int32_t x = tex_wrap((int32_t) floorf(u * (float) T.w), W, T.mode), y = tex_wrap((int32_t) floorf(v * (float) T.h), H, T.mode);
        l.w1x = 0.f; l.w1y = 0.f; l.w0x = 1.f; l.w0y = 1.f;
        l.idx[0] = l.idx[1] = l.idx[2] = l.idx[3] = (uint32_t) (y * W + x);
        return;
    }
    float px = fma_(u, (float) T.w, -0.5f), py = fma_(v, (float) T.h, -0.5f);
    float fx = floorf(px), fy = floorf(py);
    int32_t ix = (int32_t) fx, iy = (int32_t) fy;
    l.w1x = px - fx; l.w1y = py - fy; l.w0x = 1.f - l.w1x; l.w0y = 1.f - l.w1y;
    int32_t x0, x1, y0, y1;
    if ((T.mode & 7u) == 0u) {                                                         /* bilinear + repeat, the defaults: the round-1 code path */
        x0 = ix % W; if (x0 < 0) x0 += W;
        x1 = (ix + 1) % W; if (x1 < 0) x1 += W;
        y0 = iy % H; if (y0 < 0) y0 += H;
        y1 = (iy + 1) % H; if (y1 < 0) y1 += H;
    } else { x0 = tex_wrap(ix, W, T.mode); x1 = tex_wrap(ix + 1, W, T.mode); y0 = tex_wrap(iy, H, T.mode); y1 = tex_wrap(iy + 1, H, T.mode); }
    l.idx[0] = (uint32_t) (y0 * W + x0); l.idx[1] = (uint32_t) (y0 * W + x1);
    l.idx[2] = (uint32_t) (y1 * W + x0); l.idx[3] = (uint32_t) (y1 * W + x1);
}
HAR_HD Vec3 tex_fetch(const DTexture &T, const TexTaps &l) {
    float out[3];
    if (T.mode & 1u) { for (int c = 0; c < 3; ++c) out[c] = T.data[3 * (size_t) l.idx[0] + c]; return Vec3(out[0], out[1], out[2]); }
    for (int c = 0; c < 3; ++c) {
        float v00 = T.data[3 * (size_t) l.idx[0] + c], v10 = T.data[3 * (size_t) l.idx[1] + c];
        float v01 = T.data[3 * (size_t) l.idx[2] + c], v11 = T.data[3 * (size_t) l.idx[3] + c];
        float v0 = fma_(l.w0x, v00, l.w1x * v10), v1 = fma_(l.w0x, v01, l.w1x * v11);
        out[c] = fma_(l.w0y, v0, l.w1y * v1);
    }
    return Vec3(out[0], out[1], out[2]);
}
/* BitmapTexture::eval_1_grad (bitmap.cpp:543-599), in its order of operations: uv' = to_uv * uv, the four texels of eval_fetch (the taps of tex_taps: f00, f10, f01, f11),
 * each reduced to one number -- the channel of a one-channel bitmap (`mono`: stored three times, channel 0 is read), luminance() of a three-channel texel --,
 * df_x = fmadd(w0.y, f10 - f00, w1.y * (f11 - f01)), df_y = fmadd(w0.x, f01 - f00, w1.x * (f11 - f10)), then the TRANSPOSE of to_uv's 2 x 2 block and the resolution
 * (w, h), component by component.  A nearest-filtered bitmap returns (0, 0) (:558-560).  One difference in rounding: the reference writes each row of the transposed
 * product as two multiplies and an add (:594-597); here it is fmadd(m0, df_x, m1 * df_y), one rounding less -- inside every bar (docs/parity.md). */
HAR_HD float tex_value_1(const DTexture &T, uint32_t idx, bool mono) {
    const float *p = T.data + 3 * (size_t) idx;
    return mono ? p[0] : p[0] * 0.212671f + p[1] * 0.715160f + p[2] * 0.072169f;           /* luminance(), spectrum.h:439-442 */
}
HAR_HD void tex_eval_1_grad(const DTexture &T, bool mono, float u, float v, float &gu, float &gv) {
    gu = 0.f; gv = 0.f;
    if (T.mode & 1u) return;
    TexTaps l; tex_taps(T, u, v, l);
    const float f00 = tex_value_1(T, l.idx[0], mono), f10 = tex_value_1(T, l.idx[1], mono), f01 = tex_value_1(T, l.idx[2], mono), f11 = tex_value_1(T, l.idx[3], mono);
    const float dfx = fma_(l.w0y, f10 - f00, l.w1y * (f11 - f01)), dfy = fma_(l.w0x, f01 - f00, l.w1x * (f11 - f10));
    const bool xf = (T.mode & HAR_TEX_HAS_UV_XF) != 0u;
    const float m00 = xf ? T.uvm[0] : 1.f, m01 = xf ? T.uvm[1] : 0.f, m10 = xf ? T.uvm[3] : 0.f, m11 = xf ? T.uvm[4] : 1.f;
    gu = (float) T.w * fma_(m00, dfx, m10 * dfy);
    gv = (float) T.h * fma_(m01, dfx, m11 * dfy);
}
/* ... and its transpose: eval_1_grad is linear in the texels, so for an adjoint (gu, gv) of the gradient the deposit into tap k (texel l.idx[k]) is
 * w[k] = `scale` * (ax * d df_x / d f_k + ay * d df_y / d f_k), (ax, ay) = the adjoint pushed through the same matrix and the resolution,
 * d df_x / d f = (-w0.y, +w0.y, -w1.y, +w1.y), d df_y / d f = (-w0.x, -w1.x, +w0.x, +w1.x) over (f00, f10, f01, f11).  A three-channel map multiplies w[k] by the luminance
 * coefficient of the channel; a one-channel map receives it in channel 0 (tex_eval_1_grad_channels).  A nearest map: zero weights. */
HAR_HD void tex_eval_1_grad_transpose(const DTexture &T, float u, float v, float gu, float gv, float scale, TexTaps &l, float w[4]) {
    tex_taps(T, u, v, l);
    w[0] = w[1] = w[2] = w[3] = 0.f;
    if (T.mode & 1u) return;
    const bool xf = (T.mode & HAR_TEX_HAS_UV_XF) != 0u;
    const float m00 = xf ? T.uvm[0] : 1.f, m01 = xf ? T.uvm[1] : 0.f, m10 = xf ? T.uvm[3] : 0.f, m11 = xf ? T.uvm[4] : 1.f;
    const float hu = (float) T.w * gu, hv = (float) T.h * gv;
    const float ax = scale * fma_(m00, hu, m01 * hv), ay = scale * fma_(m10, hu, m11 * hv);
    w[0] = fma_(-l.w0y, ax, -l.w0x * ay); w[1] = fma_(l.w0y, ax, -l.w1x * ay);
    w[2] = fma_(-l.w1y, ax, l.w0x * ay);  w[3] = fma_(l.w1y, ax, l.w1x * ay);
}
HAR_HD Vec3 tex_eval_1_grad_channels(bool mono) { return mono ? Vec3(1.f, 0.f, 0.f) : Vec3(0.212671f, 0.715160f, 0.072169f); }

/* ---- the `mesh_attribute` texture (src/textures/mesh_attribute.cpp -> Mesh::eval_attribute*, src/render/mesh.cpp:2464-2631).  Where a hit looks an attribute up:
 * `face` = the face's index in DScene::faces (the mesh's first face + si.prim_index), (b1, b2) = Mesh::barycentric_coordinates(si) (mesh.cpp:2227-2251): the
 * least-squares solve of si.p against the face's vertex positions, NOT the hit's prim_uv.  Filled by attr_addr in the kernels of scenes with such a texture only. */
struct AttrAddr { uint32_t face; float b1, b2; };
HAR_HD uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }       /* (rows are clamped to the record: no lookup or deposit leaves it, whatever the caller bound) */
HAR_HD AttrAddr attr_addr(const DScene &S, Vec3 p, uint32_t prim, uint32_t shape) {
    AttrAddr a; a.face = S.meshes[shape].foff + prim;
    const uint32_t *f = S.faces + 4 * (size_t) a.face; const uint32_t voff = S.meshes[shape].voff;
    const float *v0 = S.verts + 8 * (size_t) (voff + f[0]), *v1 = S.verts + 8 * (size_t) (voff + f[1]), *v2 = S.verts + 8 * (size_t) (voff + f[2]);
    const Vec3 p0(v0[0], v0[1], v0[2]), rel = p - p0, du = Vec3(v1[0], v1[1], v1[2]) - p0, dv = Vec3(v2[0], v2[1], v2[2]) - p0;
    const float b1 = dot3(du, rel), b2 = dot3(dv, rel), a11 = dot3(du, du), a12 = dot3(du, dv), a22 = dot3(dv, dv);
    const float inv_det = rcp_(fms_(a11, a22, a12 * a12));
    a.b1 = fms_(a22, b1, a12 * b2) * inv_det; a.b2 = fnma_(a12, b1, a11 * b2) * inv_det;
    return a;
}
/* the rows and weights of Mesh::interpolate_attribute (mesh.cpp:2470-2515) in a TexTaps: idx[0..2] = the three rows (a face attribute: its row three times, weights
 * 1, 0, 0), w0x / w1x / w0y = b0 / b1 / b2, w1y = `scale`; idx[3] repeats row 0 and carries no weight (tap_weights) */
HAR_HD void attr_taps(const DScene &S, const DTexture &T, const AttrAddr &a, TexTaps &l) {
    l.w1y = T.uvm[0];
    if (T.mode & HAR_TEX_ATTRIBUTE_FACE) {
        const uint32_t row = min_u32(a.face - T.pad, T.h - 1u);
        l.idx[0] = l.idx[1] = l.idx[2] = l.idx[3] = row; l.w0x = 1.f; l.w1x = 0.f; l.w0y = 0.f;
        return;
    }
    const uint32_t *f = S.faces + 4 * (size_t) a.face;
    l.idx[0] = min_u32(f[0], T.h - 1u); l.idx[1] = min_u32(f[1], T.h - 1u); l.idx[2] = min_u32(f[2], T.h - 1u); l.idx[3] = l.idx[0];
    l.w0x = 1.f - a.b1 - a.b2; l.w1x = a.b1; l.w0y = a.b2;
}
/* fmadd(a0, b0, fmadd(a1, b1, a2 * b2)) (mesh.cpp:2495-2497) times `scale` (mesh_attribute.cpp eval) */
HAR_HD Vec3 attr_fetch(const DTexture &T, const TexTaps &l) {
    float out[3];
    for (int c = 0; c < 3; ++c) {
        const float a0 = T.data[3 * (size_t) l.idx[0] + c], a1 = T.data[3 * (size_t) l.idx[1] + c], a2 = T.data[3 * (size_t) l.idx[2] + c];
        out[c] = fma_(a0, l.w0x, fma_(a1, l.w1x, a2 * l.w0y)) * l.w1y;
    }
    return Vec3(out[0], out[1], out[2]);
}
/* d value / d (row idx[k]) of a lookup: the four bilinear products, or -- `attribute` -- the three barycentric weights times `scale` */
HAR_HD void tap_weights(const TexTaps &l, bool attribute, float w[4]) {
    if (attribute) { w[0] = l.w0x * l.w1y; w[1] = l.w1x * l.w1y; w[2] = l.w0y * l.w1y; w[3] = 0.f; return; }
    w[0] = l.w0x * l.w0y; w[1] = l.w1x * l.w0y; w[2] = l.w0x * l.w1y; w[3] = l.w1x * l.w1y;
}
/* the taps of texture record T at a vertex: an attribute record from `aa` (null in every kernel of a scene without one: the branch folds away), a bitmap from (u, v) */
HAR_HD bool tex_taps_at(const DScene &S, const DTexture &T, float u, float v, const AttrAddr *aa, TexTaps &l) {
    if (aa && (T.mode & HAR_TEX_ATTRIBUTE)) { attr_taps(S, T, *aa, l); return true; }
    tex_taps(T, u, v, l);
    return false;
}
/* Texture::eval for `reflectance`: srgb constant (src/spectra/srgb.cpp), bitmap or mesh attribute */
HAR_HD Vec3 bsdf_reflectance(const DScene &S, const DBsdf &B, float u, float v, TexTaps &taps, const AttrAddr *aa = nullptr) {
    if (B.texture < 0) return Vec3(B.r, B.g, B.b);
    const DTexture T = S.textures[B.texture];
    if (tex_taps_at(S, T, u, v, aa, taps)) return attr_fetch(T, taps);
    return tex_fetch(T, taps);
}
/* Texture::eval_1 of bitmap `tex` at (u, v) (bitmap.cpp:523-541): the channel of a one-channel bitmap (`mono`: stored three times, channel 0 is read), luminance() of the
 * interpolated texel of a three-channel one -- the arithmetic of blend_weight below, without its clip.  `l`: the taps of the lookup (the adjoint scatters through them) */
HAR_HD float tex_eval_1(const DScene &S, int32_t tex, bool mono, float u, float v, TexTaps &l) {
    const DTexture T = S.textures[tex];
    tex_taps(T, u, v, l);
    const Vec3 c = tex_fetch(T, l);
    return mono ? c.x : c.x * 0.212671f + c.y * 0.715160f + c.z * 0.072169f;
}
/* the roughness of a record at (u, v), before Microfacet's max(., 1e-4) (roughconductor.cpp:244-245: m_alpha_u->eval_1(si), m_alpha_v->eval_1(si)): the constants of the
 * record, or -- a roughconductor with BF_ALPHA_TEX -- the lookup of the map(s) DBsdf::table / ::pad name; ONE lookup for an isotropic map (the same index twice) */
HAR_HD void bsdf_alpha(const DScene &S, const DBsdf &B, float u, float v, float &au, float &av) {
    au = B.alpha_u; av = B.alpha_v;
    if (B.type != BSDF_ROUGHCONDUCTOR || !(B.flags & BF_ALPHA_TEX)) return;
    const int32_t tu = B.table, tv = (int32_t) B.pad;
    TexTaps l;
    if (tu >= 0) au = tex_eval_1(S, tu, (B.flags & BF_ALPHA_MONO_U) != 0u, u, v, l);
    if (tv >= 0) av = tv == tu ? au : tex_eval_1(S, tv, (B.flags & BF_ALPHA_MONO_V) != 0u, u, v, l);
}
/* evaluated colour parameters of a BSDF record at (u, v); TYPES: only the HAR_SCENE_ALPHAMAP bit is read -- the kernels of scenes with a roughness map look the roughness up
 * here, once per vertex, for sample / eval / pdf alike */
template <uint32_t TYPES = 0u>
HAR_HD BsdfInputs bsdf_inputs(const DScene &S, const DBsdf &B, float u, float v, TexTaps &taps, const AttrAddr *aa = nullptr) {
    BsdfInputs in;
    in.slot0 = bsdf_reflectance(S, B, u, v, taps, aa);
    in.slot1 = Vec3(B.r2, B.g2, B.b2);
    in.table = B.table >= 0 ? S.bsdf_tables + B.table : nullptr;      /* (a blend record keeps a record index there: its `table` is never read) */
    if ((TYPES & HAR_SCENE_ALPHAMAP) != 0u) {
        if (B.type == BSDF_ROUGHCONDUCTOR) in.table = nullptr;         /* (... and a roughconductor with a roughness map a texture index) */
        bsdf_alpha(S, B, u, v, in.alpha_u, in.alpha_v);
    }
    return in;
}

/* TwoSidedBRDF (src/bsdfs/twosided.cpp:112-270): which record serves this side, and how wi / wo are mirrored.
 * Returns false when the BSDF is zero on this side (two different nested BSDFs and wi.z == 0). */
struct BsdfSide { uint32_t index; Vec3 wi; float wo_sign; };
HAR_HD bool bsdf_side(const DScene &S, uint32_t index, Vec3 wi, BsdfSide &side) {
    const DBsdf &B = S.bsdfs[index];
    side.index = index; side.wi = wi; side.wo_sign = 1.f;
    if (!(B.flags & BF_TWOSIDED)) return true;
    if (B.back < 0) {                      /* m_brdf[0] == m_brdf[1]: wo.z = mulsign(wo.z, wi.z); wi.z = abs(wi.z) */
        side.wo_sign = sign_(wi.z); side.wi.z = fabsf(wi.z);
        return true;
    }
    if (wi.z > 0.f) return true;
    if (wi.z < 0.f) { side.index = (uint32_t) B.back; side.wi.z = -wi.z; side.wo_sign = -1.f; return true; }
    return false;
}
/* BSDF::component_count() of a record: the model's, or for a blend the two nested records' (blendbsdf.cpp:94-97) */
template <uint32_t TYPES = 0u>          /* (only the HAR_SCENE_THIN bit is read) */
HAR_HD uint32_t bsdf_record_component_count(const DScene &S, const DBsdf &B) {
    if (B.type == BSDF_BLEND) return bsdf_component_count<TYPES>(S.bsdfs[B.table].type) + bsdf_component_count<TYPES>(S.bsdfs[B.pad].type);
    return bsdf_component_count<TYPES>(B.type);
}
/* The context a nested BSDF of a `twosided` record sees (twosided.cpp:129-146, 164-180): the front side and a one-BSDF `twosided` get the caller's context as it
 * is; the back side of a two-BSDF pair gets `component - component_count(front)` (uint32 arithmetic, as in the reference) unless the component is "all" */
template <bool BLEND = false>         /* BLEND: the front record may be a blend (scenes with such a record) */
HAR_HD BsdfCtx bsdf_side_ctx(const DScene &S, uint32_t index, const BsdfSide &side, BsdfCtx ctx) {
    const DBsdf &B = S.bsdfs[index];
    if ((B.flags & BF_TWOSIDED) && B.back >= 0 && side.wo_sign < 0.f && ctx.component != 0xffffffffu) ctx.component -= BLEND ? bsdf_record_component_count(S, B) : bsdf_component_count(B.type);
    return ctx;
}

/* ---- BlendBSDF (src/bsdfs/blendbsdf.cpp), record type 6: slot 0 is the weight, DBsdf::table / ::pad name the two nested (leaf, not twosided) records.  Everything it
 * returns is an affine combination of eval / pdf / sample of the two nested BSDFs, evaluated at the vertex's uv with their own colour inputs.  Only the kernels of scenes
 * that hold such a record carry this code (TYPES & HAR_SCENE_BLEND); the nested models run with that bit cleared.
 * eval_weight (:224-226) = clip(weight->eval_1(si), 0, 1); eval_1 of a bitmap (bitmap.cpp:523-541): the channel of a one-channel bitmap (BF_MONO; stored three times, channel
 * 0 is read), luminance (spectrum.h:439-442) of the interpolated texel of a three-channel one; a constant is stored (w, w, w).  `inside`: the unclipped weight lies strictly
 * inside (0, 1), where d clip / d weight = 1 (0 outside; the derivative AT 0 and 1 is unpinned, docs/parity.md) */
HAR_HD float blend_weight(const DBsdf &B, const BsdfInputs &in, bool &inside) {
    const float raw = (B.texture < 0 || (B.flags & BF_MONO)) ? in.slot0.x : in.slot0.x * 0.212671f + in.slot0.y * 0.715160f + in.slot0.z * 0.072169f;
    inside = raw > 0.f && raw < 1.f;
    return fminf(fmaxf(raw, 0.f), 1.f);
}
/* d value / d (slot 0 of nested BSDF k), factor included: (1 - w) * d_slot0 of BSDF 0, w * d_slot0 of BSDF 1 (the adjoint files them under the nested records) */
struct BlendChildGrad { Vec3 d[2]; };
/* eval / pdf / eval_pdf (:162-222).  e.d_slot0 = d value / d weight = v1 - v0 where the weight is not clipped (with a component selected: +/- the nested value) */
template <uint32_t TYPES, bool CTX>
HAR_HD void blend_eval_pdf(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, Vec3 wo, float u, float v, BsdfEval &e, const BsdfCtx &ctx, BlendChildGrad *cg = nullptr, const AttrAddr *aa = nullptr) {
    constexpr uint32_t LEAF = TYPES & ~HAR_SCENE_COMPOSITE;
    bool inside; const float w = blend_weight(B, in, inside);
    const uint32_t child[2] = { (uint32_t) B.table, B.pad };
    if (cg) { cg->d[0] = Vec3(0.f); cg->d[1] = Vec3(0.f); }
    if (CTX && ctx.component != 0xffffffffu) {                   /* :167-175, :185-191, :205-215: one nested BSDF, its value scaled, its pdf as it is */
        const uint32_t n0 = bsdf_component_count<TYPES>(S.bsdfs[child[0]].type);
        const bool first = ctx.component < n0;
        BsdfCtx ctx2 = ctx; if (!first) ctx2.component -= n0;
        const float k = first ? 1.f - w : w;
        const DBsdf &N = S.bsdfs[child[first ? 0 : 1]];
        TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps, aa);
        bsdf_eval_pdf_one<LEAF, CTX>(N, nin, wi, wo, e, ctx2);
        const Vec3 nv = e.value;
        if (cg) cg->d[first ? 0 : 1] = e.d_slot0 * k;
        e.value = nv * k; e.d_slot1 = Vec3(0.f);
        e.d_slot0 = inside ? (first ? -nv : nv) : Vec3(0.f);
        return;
    }
    Vec3 val[2]; float pdf[2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1          /* one copy of the model switch, run twice: two copies side by side cost the shading kernels their registers */
#endif
    for (int k = 0; k < 2; ++k) {
        const DBsdf &N = S.bsdfs[child[k]];
        TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps, aa);
        BsdfEval ne; bsdf_eval_pdf_one<LEAF, CTX>(N, nin, wi, wo, ne, ctx);
        val[k] = ne.value; pdf[k] = ne.pdf;
        if (cg) cg->d[k] = ne.d_slot0 * (k == 0 ? 1.f - w : w);
    }
    e.value = val[0] * (1.f - w) + val[1] * w;                   /* :220-221 */
    e.pdf = pdf[0] * (1.f - w) + pdf[1] * w;
    e.d_slot0 = inside ? val[1] - val[0] : Vec3(0.f); e.d_slot1 = Vec3(0.f);
}
/* sample (:108-160): sample1 > w takes nested BSDF 0 with (sample1 - w) / (1 - w), otherwise BSDF 1 with sample1 / w; the other one is evaluated at the sampled direction.
 * eta, sampled_type and sampled_component are the sampled BSDF's own (not offset, as in the reference); delta lobes go through the same arithmetic. */
template <uint32_t TYPES, bool CTX>
HAR_HD void blend_sample(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, float u, float v, float s1, float s2x, float s2y, BsdfSample &bs, const BsdfCtx &ctx, const AttrAddr *aa = nullptr) {
    constexpr uint32_t LEAF = TYPES & ~HAR_SCENE_COMPOSITE;
    bool inside; const float w = blend_weight(B, in, inside);
    const uint32_t child[2] = { (uint32_t) B.table, B.pad };
    if (CTX && ctx.component != 0xffffffffu) {                   /* :116-126 */
        const uint32_t n0 = bsdf_component_count<TYPES>(S.bsdfs[child[0]].type);
        const bool first = ctx.component < n0;
        BsdfCtx ctx2 = ctx; if (!first) ctx2.component -= n0;
        const DBsdf &N = S.bsdfs[child[first ? 0 : 1]];
        TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps, aa);
        bsdf_sample_one<LEAF, CTX>(N, nin, wi, s1, s2x, s2y, bs, ctx2);
        bs.weight = bs.weight * (first ? 1.f - w : w);
        return;
    }
    bs.wo = Vec3(0.f); bs.pdf = 0.f; bs.weight = Vec3(0.f); bs.eta = 0.f; bs.delta = false; bs.type = 0u; bs.comp = 0u;
    const bool m0 = s1 > w, m1 = s1 <= w;
    if (!m0 && !m1) return;
    const DBsdf &Ns = S.bsdfs[child[m0 ? 0 : 1]], &No = S.bsdfs[child[m0 ? 1 : 0]];
    TexTaps taps;
    const BsdfInputs sin = bsdf_inputs<TYPES>(S, Ns, u, v, taps, aa);
    bsdf_sample_one<LEAF, CTX>(Ns, sin, wi, m0 ? (s1 - w) / (1.f - w) : s1 / w, s2x, s2y, bs, ctx);
    const BsdfInputs oin = bsdf_inputs<TYPES>(S, No, u, v, taps, aa);
    BsdfEval eo; bsdf_eval_pdf_one<LEAF, CTX>(No, oin, wi, bs.wo, eo, ctx);
    /* :138-141 / :150-153: weight is nested BSDF 1's share in both branches */
    const float pdf_weighted = m0 ? w * eo.pdf + (1.f - w) * bs.pdf : w * bs.pdf + (1.f - w) * eo.pdf;
    const Vec3 sum = m0 ? eo.value * w + (bs.weight * (1.f - w)) * bs.pdf : (bs.weight * w) * bs.pdf + eo.value * (1.f - w);
    bs.weight = sum * (pdf_weighted > 0.f ? rcp_(pdf_weighted) : 0.f);
    bs.pdf = pdf_weighted;
}

/* ---- MaskBSDF (src/bsdfs/mask.cpp), record type 7: slot 0 is the opacity, DBsdf::pad names the nested record -- a leaf model that may carry the twosided flag (one
 * BSDF or a pair): bsdf_side is applied to IT, with the vertex's unmirrored wi, and the leaf it returns is evaluated with its own colour inputs at the vertex's uv.  Only
 * the kernels of scenes that hold such a record carry this code (TYPES & HAR_SCENE_MASK).  eval_opacity (:225-227) = clip(opacity->eval_1(si), 0, 1): the blend weight's
 * arithmetic, `inside` included.  Components: the nested BSDF's, then the null lobe at the last index (:107-113). */
HAR_HD float mask_opacity(const DBsdf &B, const BsdfInputs &in, bool &inside) { return blend_weight(B, in, inside); }
template <uint32_t TYPES = 0u>          /* (only the HAR_SCENE_THIN bit is read: a nested thin dielectric has two components) */
HAR_HD uint32_t mask_null_index(const DScene &S, const DBsdf &B) {
    const DBsdf &N = S.bsdfs[B.pad];
    uint32_t c = bsdf_component_count<TYPES>(N.type);
    if (N.flags & BF_TWOSIDED) c += N.back >= 0 ? bsdf_component_count(S.bsdfs[N.back].type) : c;        /* twosided.cpp:86-100: the front BSDF's components, then the back's -- also when both are ONE BSDF */
    return c;
}
/* eval / pdf / eval_pdf (:169-217): the nested value times the opacity; the pdf is 0 when the context leaves the nested components out and is scaled by the opacity only
 * when the null lobe is enabled.  e.d_slot0 = d value / d opacity = the nested value where the opacity is not clipped; cg->d[0] = d value / d (slot 0 of the nested LEAF) */
template <uint32_t TYPES, bool CTX>
HAR_HD void mask_eval_pdf(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, Vec3 wo, float u, float v, BsdfEval &e, const BsdfCtx &ctx, BlendChildGrad *cg = nullptr, const AttrAddr *aa = nullptr) {
    constexpr uint32_t LEAF = TYPES & ~HAR_SCENE_COMPOSITE;
    bool inside; const float o = mask_opacity(B, in, inside);
    bool transmission = true, nested = true;
    if (CTX) {
        const uint32_t null_index = mask_null_index<TYPES>(S, B);
        transmission = ctx.is_enabled(LOBE_NULL, null_index);
        nested = ctx.component == 0xffffffffu || ctx.component < null_index;
    }
    BsdfEval ne; ne.value = Vec3(0.f); ne.pdf = 0.f; ne.d_slot0 = Vec3(0.f); ne.d_slot1 = Vec3(0.f);
    BsdfSide ns;
    if (bsdf_side(S, B.pad, wi, ns)) {
        const DBsdf &N = S.bsdfs[ns.index];
        TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps, aa);
        bsdf_eval_pdf_one<LEAF, CTX>(N, nin, ns.wi, Vec3(wo.x, wo.y, wo.z * ns.wo_sign), ne, CTX ? bsdf_side_ctx(S, B.pad, ns, ctx) : ctx);
    }
    e.value = ne.value * o;
    e.pdf = !nested ? 0.f : (transmission ? ne.pdf * o : ne.pdf);
    e.d_slot0 = inside ? ne.value : Vec3(0.f); e.d_slot1 = Vec3(0.f);
    if (cg) { cg->d[0] = ne.d_slot0 * o; cg->d[1] = Vec3(0.f); }
}
/* sample (:121-167): sample1 < o takes the nested BSDF with sample1 / o -- its weight, type, component and eta as they are, its pdf times o --, otherwise the null lobe:
 * wo = -wi (the vertex's own wi, not the mirrored one), pdf = 1 - o, weight = 1, eta = 1.  A context that enables only one of the two makes o 1 or 0. */
template <uint32_t TYPES, bool CTX>
HAR_HD void mask_sample(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, float u, float v, float s1, float s2x, float s2y, BsdfSample &bs, const BsdfCtx &ctx, const AttrAddr *aa = nullptr) {
    constexpr uint32_t LEAF = TYPES & ~HAR_SCENE_COMPOSITE;
    bs.wo = Vec3(0.f); bs.pdf = 0.f; bs.weight = Vec3(0.f); bs.eta = 0.f; bs.delta = false; bs.type = 0u; bs.comp = 0u;
    bool inside; float o = mask_opacity(B, in, inside);
    const uint32_t null_index = mask_null_index<TYPES>(S, B);
    if (CTX) {
        const bool transmission = ctx.is_enabled(LOBE_NULL, null_index), nested = ctx.component == 0xffffffffu || ctx.component < null_index;
        if (!transmission && !nested) return;
        if (transmission != nested) o = transmission ? 1.f : 0.f;
    }
    if (s1 < o) {
        BsdfSide ns;
        if (!bsdf_side(S, B.pad, wi, ns)) return;
        const DBsdf &N = S.bsdfs[ns.index];
        TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps, aa);
        bsdf_sample_one<LEAF, CTX>(N, nin, ns.wi, s1 / o, s2x, s2y, bs, CTX ? bsdf_side_ctx(S, B.pad, ns, ctx) : ctx);
        bs.wo.z *= ns.wo_sign; bs.pdf *= o;
        return;
    }
    bs.wo = Vec3(-wi.x, -wi.y, -wi.z); bs.pdf = 1.f - o; bs.weight = Vec3(1.f); bs.eta = 1.f; bs.delta = true; bs.type = LOBE_NULL; bs.comp = null_index;
}

/* Kernels of scenes with a thin dielectric (HAR_SCENE_THIN): would bsdf_sample<TYPES>, default context, return the NULL lobe for `sample1` at the record B that serves
 * this side?  The decision alone, in the arithmetic of the sample functions -- a thin leaf (sample1 <= r' reflects), a mask record (sample1 < opacity takes the nested
 * BSDF with sample1 / opacity, which may be a thin leaf), a blend record whose sampled child is a thin leaf.  What `path` needs at the LAST vertex of a path, where the
 * JIT variants draw the sample and valid_ray takes its type (path.cpp:263-267, 307-308) but nothing else of it is used. */
template <uint32_t TYPES>
HAR_HD bool sample_takes_null_lobe(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, float s1) {
    if (B.type == BSDF_THINDIELECTRIC) return !(s1 <= thin_reflectance(B.eta, wi.z));
    if (B.type == BSDF_MASK) {
        bool inside; const float o = mask_opacity(B, in, inside);
        if (!(s1 < o)) return true;
        BsdfSide ns;
        if (bsdf_side(S, B.pad, wi, ns) && S.bsdfs[ns.index].type == BSDF_THINDIELECTRIC) return !(s1 / o <= thin_reflectance(S.bsdfs[ns.index].eta, ns.wi.z));
        return false;
    }
    if (B.type == BSDF_BLEND) {
        bool inside; const float w = blend_weight(B, in, inside);
        const bool m0 = s1 > w, m1 = s1 <= w;
        if (!m0 && !m1) return false;
        const DBsdf &N = S.bsdfs[m0 ? (uint32_t) B.table : B.pad];
        if (N.type == BSDF_THINDIELECTRIC) return !((m0 ? (s1 - w) / (1.f - w) : s1 / w) <= thin_reflectance(N.eta, wi.z));
    }
    return false;
}

/* ---- NormalMap (src/bsdfs/normalmap.cpp), record type 8: slot 0 is the normal-map colour (Texture::eval_3: a constant rgb or a three-channel bitmap), DBsdf::pad names
 * the nested record -- a leaf model that may carry the twosided flag: bsdf_side is applied to it with the PERTURBED wi', as twosided.cpp sees perturbed_si.  Only the kernels
 * of scenes that hold such a record carry this code (TYPES & HAR_SCENE_NORMALMAP).  Components and flags are the nested BSDF's (:117-122): the context passes through.
 * frame() (:224-244), in the reference's order of operations: n = fmadd(c, 2, -1); with flip_invalid_normals n <- (-n.x, -n.y, n.z) where cos_theta(wi) * dot(wi, n) <= 0;
 * n = normalize(n); s = normalize(fnmadd(n, n.x, (1, 0, 0))); t = cross(n, s) -- the frame relative to si.sh_frame, which is all eval / pdf / sample read. */
struct NormalFrame {
    Vec3 s, t, n;
    HAR_HD Vec3 to_local(Vec3 v) const { return Vec3(dot3(v, s), dot3(v, t), dot3(v, n)); }       /* frame.h:34 */
    HAR_HD Vec3 to_world(Vec3 v) const { return fma3(n, v.z, fma3(t, v.y, s * v.x)); }             /* frame.h:39 */
};
HAR_HD NormalFrame normalmap_frame(const DBsdf &B, Vec3 c, Vec3 wi) {
    Vec3 n(fma_(c.x, 2.f, -1.f), fma_(c.y, 2.f, -1.f), fma_(c.z, 2.f, -1.f));
    if ((B.flags & BF_NM_FLIP) && wi.z * dot3(wi, n) <= 0.f) n = Vec3(-n.x, -n.y, n.z);
    NormalFrame F;
    F.n = normalize3(n);
    F.s = normalize3(Vec3(fnma_(F.n.x, F.n.x, 1.f), fnma_(F.n.y, F.n.x, 0.f), fnma_(F.n.z, F.n.x, 0.f)));
    F.t = cross3(F.n, F.s);
    return F;
}
/* Frame::tan_theta_2 (frame.h:80-83) and eval_shadow_terminator (normalmap_helpers.h:20-25) */
HAR_HD float frame_tan_theta_2(Vec3 v) { return fmaxf(fnma_(v.z, v.z, 1.f), 0.f) / sqr_(v.z); }
HAR_HD float normalmap_shadow_terminator(Vec3 perturbed_n, Vec3 wo) {
    const float alpha2 = fminf(0.125f * frame_tan_theta_2(perturbed_n), 1.f);
    return 2.f / (1.f + sqrtf(1.f + alpha2 * frame_tan_theta_2(wo)));
}
/* eval / pdf / eval_pdf (:163-219): the nested BSDF at wi' = frame.to_local(wi), wo' = frame.to_local(wo); zero unless cos_theta(wo) * cos_theta(wo') > 0; the value -- not
 * the pdf -- times the shadow terminator of (frame.n, wo).  d_slot0 stays zero (the record's slot 0 is the normal map: its derivative is not a per-channel scale; it
 * comes from normalmap_weighted_value_grad, har_normalmap_grad.h); cg->d[0] = d value / d (slot 0 of the nested LEAF). */
/* (the part behind the frame, shared with the bumpmap record: both hand it their NormalFrame) */
template <uint32_t TYPES, bool CTX>
HAR_HD void perturbed_eval_pdf(const DScene &S, const DBsdf &B, const NormalFrame &F, Vec3 wi, Vec3 wo, float u, float v, BsdfEval &e, const BsdfCtx &ctx, BlendChildGrad *cg = nullptr) {
    constexpr uint32_t LEAF = TYPES & ~HAR_SCENE_RECORD_BITS;
    const Vec3 pwi = F.to_local(wi), pwo = F.to_local(wo);
    if (!(wo.z * pwo.z > 0.f)) return;
    BsdfSide ns;
    if (!bsdf_side(S, B.pad, pwi, ns)) return;
    const DBsdf &N = S.bsdfs[ns.index];
    TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps);
    BsdfEval ne; bsdf_eval_pdf_one<LEAF, CTX>(N, nin, ns.wi, Vec3(pwo.x, pwo.y, pwo.z * ns.wo_sign), ne, CTX ? bsdf_side_ctx(S, B.pad, ns, ctx) : ctx);
    const float shadow = (B.flags & BF_NM_SHADOW) ? normalmap_shadow_terminator(F.n, wo) : 1.f;
    e.value = (B.flags & BF_NM_SHADOW) ? ne.value * shadow : ne.value;
    e.pdf = ne.pdf;
    if (cg) cg->d[0] = ne.d_slot0 * shadow;          /* d value / d (slot 0 of the nested LEAF): the leaf receives shadow * d_slot0(nested at wi', wo') */
}
template <uint32_t TYPES, bool CTX>
HAR_HD void normalmap_eval_pdf(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, Vec3 wo, float u, float v, BsdfEval &e, const BsdfCtx &ctx, BlendChildGrad *cg = nullptr) {
    e.value = Vec3(0.f); e.pdf = 0.f; e.d_slot0 = Vec3(0.f); e.d_slot1 = Vec3(0.f);
    const NormalFrame F = normalmap_frame(B, in.slot0, wi);
    perturbed_eval_pdf<TYPES, CTX>(S, B, F, wi, wo, u, v, e, ctx, cg);
}
/* sample (:134-160): the nested sample at wi'; nothing when its weight is zero; wo = frame.to_world(wo') -- back in the UNPERTURBED frame --, pdf and weight zero unless
 * cos_theta(wo') * cos_theta(wo) > 0 (wo, eta, sampled_type and sampled_component stay what the nested BSDF returned), the weight times the shadow terminator */
template <uint32_t TYPES, bool CTX>
HAR_HD void perturbed_sample(const DScene &S, const DBsdf &B, const NormalFrame &F, Vec3 wi, float u, float v, float s1, float s2x, float s2y, BsdfSample &bs, const BsdfCtx &ctx) {
    constexpr uint32_t LEAF = TYPES & ~HAR_SCENE_RECORD_BITS;
    const Vec3 pwi = F.to_local(wi);
    BsdfSide ns;
    if (!bsdf_side(S, B.pad, pwi, ns)) return;
    const DBsdf &N = S.bsdfs[ns.index];
    TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps);
    bsdf_sample_one<LEAF, CTX>(N, nin, ns.wi, s1, s2x, s2y, bs, CTX ? bsdf_side_ctx(S, B.pad, ns, ctx) : ctx);
    bs.wo.z *= ns.wo_sign;
    const bool nonzero = bs.weight.x != 0.f || bs.weight.y != 0.f || bs.weight.z != 0.f;                             /* :146 (a lane of a wavefront: the rest still runs, masked) */
    const Vec3 pwo = bs.wo, wo = F.to_world(pwo);
    const bool active = nonzero && pwo.z * wo.z > 0.f;
    bs.wo = wo;
    if (!active) { bs.pdf = 0.f; bs.weight = Vec3(0.f); return; }
    if (B.flags & BF_NM_SHADOW) bs.weight = bs.weight * normalmap_shadow_terminator(F.n, wo);
}
template <uint32_t TYPES, bool CTX>
HAR_HD void normalmap_sample(const DScene &S, const DBsdf &B, const BsdfInputs &in, Vec3 wi, float u, float v, float s1, float s2x, float s2y, BsdfSample &bs, const BsdfCtx &ctx) {
    bs.wo = Vec3(0.f); bs.pdf = 0.f; bs.weight = Vec3(0.f); bs.eta = 0.f; bs.delta = false; bs.type = 0u; bs.comp = 0u;
    const NormalFrame F = normalmap_frame(B, in.slot0, wi);
    perturbed_sample<TYPES, CTX>(S, B, F, wi, u, v, s1, s2x, s2y, bs, ctx);
}

/* ---- BumpMap (src/bsdfs/bumpmap.cpp), record type 9: DBsdf::texture is the height bitmap (Texture::eval_1_grad: one channel -- BF_MONO -- or the luminance of three),
 * DBsdf::alpha_u holds `scale`, DBsdf::pad names the nested record (a leaf model that may carry the twosided flag), BF_NM_FLIP / BF_NM_SHADOW are the two switches.
 * Components and flags are the nested BSDF's (:124-128: no BSDFFlags::NormalMapped, so the shape's frame stays what it is).  Only the kernels of scenes that hold such a
 * record carry this code (TYPES & HAR_SCENE_BUMPMAP).  The frame needs more of the interaction than wi and uv: BumpGeom, filled for vertices on a bumpmap record only.
 * frame() (:224-253), line for line:
 *   grad_uv = scale * eval_1_grad;  dp_du' = fmadd(sh_n, grad_uv.x - dot(sh_n, dp_du), dp_du), likewise dp_dv';  n = normalize(cross(dp_du', dp_dv'));
 *   n = -n where dot(si.n, n) < 0;  n = si.to_local(n);  with flip_invalid_normals n <- (-n.x, -n.y, n.z) where cos_theta(wi) * dot(wi, n) <= 0;
 *   s = normalize(fnmadd(n, dot(n, si.dp_du), si.dp_du));  t = cross(n, s).
 * The `s` line dots the LOCAL n with the WORLD-space dp_du and subtracts a local vector from a world one -- that is what the reference computes (:249), and parity is
 * with the reference, so it is implemented literally (docs/parity.md). */
struct BumpGeom { Vec3 n, sn, ss, st, dp_du, dp_dv; float gx, gy; /* grad_uv = scale * eval_1_grad at the vertex's uv */ };
HAR_HD NormalFrame bumpmap_frame_grad(const DBsdf &B, const BumpGeom &G, float gx, float gy, Vec3 wi) {
    const Vec3 dpu = fma3(G.sn, gx - dot3(G.sn, G.dp_du), G.dp_du), dpv = fma3(G.sn, gy - dot3(G.sn, G.dp_dv), G.dp_dv);
    Vec3 n = normalize3(cross3(dpu, dpv));
    if (dot3(G.n, n) < 0.f) n = -n;
    n = Vec3(dot3(n, G.ss), dot3(n, G.st), dot3(n, G.sn));
    if ((B.flags & BF_NM_FLIP) && wi.z * dot3(wi, n) <= 0.f) n = Vec3(-n.x, -n.y, n.z);
    NormalFrame F;
    F.n = n;
    F.s = normalize3(fma3(n, -dot3(n, G.dp_du), G.dp_du));
    F.t = cross3(F.n, F.s);
    return F;
}
HAR_HD NormalFrame bumpmap_frame(const DBsdf &B, const BumpGeom &G, Vec3 wi) { return bumpmap_frame_grad(B, G, G.gx, G.gy, wi); }
/* the interaction fields frame() reads, and the height gradient at (u, v) */
HAR_HD BumpGeom bump_geom(const DScene &S, const DBsdf &B, Vec3 n, Vec3 sn, Vec3 ss, Vec3 st, Vec3 dp_du, Vec3 dp_dv, float u, float v) {
    BumpGeom G; G.n = n; G.sn = sn; G.ss = ss; G.st = st; G.dp_du = dp_du; G.dp_dv = dp_dv;
    float gx, gy; tex_eval_1_grad(S.textures[B.texture], (B.flags & BF_MONO) != 0u, u, v, gx, gy);
    G.gx = B.alpha_u * gx; G.gy = B.alpha_u * gy;
    return G;
}
/* eval / pdf / eval_pdf / sample (:137-222) behind the frame are the normalmap's code */
template <uint32_t TYPES, bool CTX>
HAR_HD void bumpmap_eval_pdf(const DScene &S, const DBsdf &B, const BumpGeom *G, Vec3 wi, Vec3 wo, float u, float v, BsdfEval &e, const BsdfCtx &ctx, BlendChildGrad *cg = nullptr) {
    e.value = Vec3(0.f); e.pdf = 0.f; e.d_slot0 = Vec3(0.f); e.d_slot1 = Vec3(0.f);
    if (!G) return;
    const NormalFrame F = bumpmap_frame(B, *G, wi);
    perturbed_eval_pdf<TYPES, CTX>(S, B, F, wi, wo, u, v, e, ctx, cg);
}
template <uint32_t TYPES, bool CTX>
HAR_HD void bumpmap_sample(const DScene &S, const DBsdf &B, const BumpGeom *G, Vec3 wi, float u, float v, float s1, float s2x, float s2y, BsdfSample &bs, const BsdfCtx &ctx) {
    bs.wo = Vec3(0.f); bs.pdf = 0.f; bs.weight = Vec3(0.f); bs.eta = 0.f; bs.delta = false; bs.type = 0u; bs.comp = 0u;
    if (!G) return;
    const NormalFrame F = bumpmap_frame(B, *G, wi);
    perturbed_sample<TYPES, CTX>(S, B, F, wi, u, v, s1, s2x, s2y, bs, ctx);
}

/* (u, v): the vertex's texture coordinates -- read only by the kernels of blend / mask scenes, whose nested records look up their own colour inputs there */
template <uint32_t TYPES = HAR_BSDF_ALL_TYPES, bool CTX = false>
HAR_HD void bsdf_eval_pdf(const DScene &S, const BsdfSide &side, const BsdfInputs &in, bool side_ok, Vec3 wo, BsdfEval &e, const BsdfCtx &ctx = BsdfCtx(), float u = 0.f, float v = 0.f,
                          BlendChildGrad *cg = nullptr, const AttrAddr *aa = nullptr, const BumpGeom *bg = nullptr /* kernels of bump scenes: the interaction of a vertex on a bumpmap record */) {
    if (!side_ok) { e.value = Vec3(0.f); e.pdf = 0.f; e.d_slot0 = Vec3(0.f); e.d_slot1 = Vec3(0.f); if ((TYPES & HAR_SCENE_BLEND) != 0u && cg) { cg->d[0] = Vec3(0.f); cg->d[1] = Vec3(0.f); } return; }
    if ((TYPES & HAR_SCENE_BLEND) != 0u && S.bsdfs[side.index].type == BSDF_BLEND) {
        blend_eval_pdf<TYPES, CTX>(S, S.bsdfs[side.index], in, side.wi, Vec3(wo.x, wo.y, wo.z * side.wo_sign), u, v, e, ctx, cg, aa);
        return;
    }
    if ((TYPES & HAR_SCENE_MASK) != 0u && S.bsdfs[side.index].type == BSDF_MASK) {
        mask_eval_pdf<TYPES, CTX>(S, S.bsdfs[side.index], in, side.wi, Vec3(wo.x, wo.y, wo.z * side.wo_sign), u, v, e, ctx, cg, aa);
        return;
    }
    if ((TYPES & HAR_SCENE_BLEND) != 0u && cg) { cg->d[0] = Vec3(0.f); cg->d[1] = Vec3(0.f); }
    if ((TYPES & HAR_SCENE_NORMALMAP) != 0u && S.bsdfs[side.index].type == BSDF_NORMALMAP) {
        normalmap_eval_pdf<TYPES, CTX>(S, S.bsdfs[side.index], in, side.wi, Vec3(wo.x, wo.y, wo.z * side.wo_sign), u, v, e, ctx, cg);
        return;
    }
    if ((TYPES & HAR_SCENE_BUMPMAP) != 0u && S.bsdfs[side.index].type == BSDF_BUMPMAP) {
        bumpmap_eval_pdf<TYPES, CTX>(S, S.bsdfs[side.index], bg, side.wi, Vec3(wo.x, wo.y, wo.z * side.wo_sign), u, v, e, ctx, cg);
        return;
    }
    bsdf_eval_pdf_one<(TYPES & ~HAR_SCENE_RECORD_BITS), CTX>(S.bsdfs[side.index], in, side.wi, Vec3(wo.x, wo.y, wo.z * side.wo_sign), e, ctx);
}
/* d value / d {alpha, eta, k} of the record serving this side (see bsdf_eval_extra_one) */
template <uint32_t TYPES = HAR_BSDF_ALL_TYPES>
HAR_HD void bsdf_eval_extra(const DScene &S, const BsdfSide &side, const BsdfInputs &in, bool side_ok, Vec3 wo, BsdfEvalExtra &x) {
    if (!side_ok) { x.d_alpha_u = Vec3(0.f); x.d_alpha_v = Vec3(0.f); x.d_eta = Vec3(0.f); x.d_k = Vec3(0.f); return; }
    bsdf_eval_extra_one<TYPES>(S.bsdfs[side.index], in, side.wi, Vec3(wo.x, wo.y, wo.z * side.wo_sign), x);
}
template <uint32_t TYPES = HAR_BSDF_ALL_TYPES, bool CTX = false>
HAR_HD void bsdf_sample(const DScene &S, const BsdfSide &side, const BsdfInputs &in, bool side_ok, float s1, float s2x, float s2y, BsdfSample &bs, const BsdfCtx &ctx = BsdfCtx(),
                        float u = 0.f, float v = 0.f, const AttrAddr *aa = nullptr, const BumpGeom *bg = nullptr) {
    if (!side_ok) { bs.wo = Vec3(0.f); bs.pdf = 0.f; bs.weight = Vec3(0.f); bs.eta = 0.f; bs.delta = false; bs.type = 0u; bs.comp = 0u; return; }
    if ((TYPES & HAR_SCENE_BLEND) != 0u && S.bsdfs[side.index].type == BSDF_BLEND) blend_sample<TYPES, CTX>(S, S.bsdfs[side.index], in, side.wi, u, v, s1, s2x, s2y, bs, ctx, aa);
    else if ((TYPES & HAR_SCENE_MASK) != 0u && S.bsdfs[side.index].type == BSDF_MASK) mask_sample<TYPES, CTX>(S, S.bsdfs[side.index], in, side.wi, u, v, s1, s2x, s2y, bs, ctx, aa);
    else if ((TYPES & HAR_SCENE_NORMALMAP) != 0u && S.bsdfs[side.index].type == BSDF_NORMALMAP) normalmap_sample<TYPES, CTX>(S, S.bsdfs[side.index], in, side.wi, u, v, s1, s2x, s2y, bs, ctx);
    else if ((TYPES & HAR_SCENE_BUMPMAP) != 0u && S.bsdfs[side.index].type == BSDF_BUMPMAP) bumpmap_sample<TYPES, CTX>(S, S.bsdfs[side.index], bg, side.wi, u, v, s1, s2x, s2y, bs, ctx);
    else bsdf_sample_one<(TYPES & ~HAR_SCENE_RECORD_BITS), CTX>(S.bsdfs[side.index], in, side.wi, s1, s2x, s2y, bs, ctx);
    bs.wo.z *= side.wo_sign;
}

/* One lane of the array-valued BSDF::eval_pdf / sample that carry the interaction (har_bsdf_eval_pdf_si / har_bsdf_sample_si, their kernels and host twins): `geom` is
 * 18 x n -- si.n, sh_frame.n, sh_frame.s, sh_frame.t, dp_du, dp_dv, three rows each --, read for a bumpmap record (an outer `twosided` folds wi in front of the frame);
 * every other record is evaluated as by har_bsdf_eval_pdf / har_bsdf_sample */
HAR_HD BumpGeom bump_geom_rows(const DScene &S, const DBsdf &B, uint32_t n, uint32_t i, const float *geom, float u, float v) {
    Vec3 r[6];
    for (int k = 0; k < 6; ++k) r[k] = Vec3(geom[(3 * k) * (size_t) n + i], geom[(3 * k + 1) * (size_t) n + i], geom[(3 * k + 2) * (size_t) n + i]);
    return bump_geom(S, B, r[0], r[1], r[2], r[3], r[4], r[5], u, v);
}
template <uint32_t AMAP = 0u>          /* AMAP = HAR_SCENE_ALPHAMAP: the entries of a scene with a roughness map (kernels of their own; the host twins always) */
HAR_HD void bsdf_eval_pdf_si_lane(const DScene &S, uint32_t bsdf, const BsdfCtx &ctx, uint32_t n, uint32_t i, const float *wi, const float *uv, const float *wo, const float *geom,
                                  bool active, float *value, float *pdf) {
    BsdfEval e; e.value = Vec3(0.f); e.pdf = 0.f;
    if (active) {
        BsdfSide side; const bool ok = bsdf_side(S, bsdf, Vec3(wi[i], wi[n + i], wi[2 * (size_t) n + i]), side);
        const DBsdf &B = S.bsdfs[side.index];
        TexTaps taps; const BsdfInputs in = bsdf_inputs<AMAP>(S, B, uv[i], uv[n + i], taps);
        BumpGeom G; const bool bump = B.type == BSDF_BUMPMAP;
        if (bump) G = bump_geom_rows(S, B, n, i, geom, uv[i], uv[n + i]);
        bsdf_eval_pdf<HAR_BSDF_ALL_TYPES | HAR_SCENE_RECORD_BITS | AMAP, true>(S, side, in, ok, Vec3(wo[i], wo[n + i], wo[2 * (size_t) n + i]), e, bsdf_side_ctx<true>(S, bsdf, side, ctx), uv[i], uv[n + i],
                                                                          nullptr, nullptr, bump ? &G : nullptr);
    }
    if (value) { value[i] = e.value.x; value[n + i] = e.value.y; value[2 * (size_t) n + i] = e.value.z; }
    if (pdf) pdf[i] = e.pdf;
}
template <uint32_t AMAP = 0u>
HAR_HD void bsdf_sample_si_lane(const DScene &S, uint32_t bsdf, const BsdfCtx &ctx, uint32_t n, uint32_t i, const float *wi, const float *uv, const float *s1, const float *s2,
                                const float *geom, bool active, float *wo, float *pdf, float *weight, float *eta, uint32_t *stype, uint32_t *scomp) {
    BsdfSample b; b.wo = Vec3(0.f); b.pdf = 0.f; b.weight = Vec3(0.f); b.eta = 0.f; b.delta = false; b.type = 0u; b.comp = 0u;
    if (active) {
        BsdfSide side; const bool ok = bsdf_side(S, bsdf, Vec3(wi[i], wi[n + i], wi[2 * (size_t) n + i]), side);
        const DBsdf &B = S.bsdfs[side.index];
        TexTaps taps; const BsdfInputs in = bsdf_inputs<AMAP>(S, B, uv[i], uv[n + i], taps);
        BumpGeom G; const bool bump = B.type == BSDF_BUMPMAP;
        if (bump) G = bump_geom_rows(S, B, n, i, geom, uv[i], uv[n + i]);
        bsdf_sample<HAR_BSDF_ALL_TYPES | HAR_SCENE_RECORD_BITS | AMAP, true>(S, side, in, ok, s1 ? s1[i] : 0.f, s2[i], s2[n + i], b, bsdf_side_ctx<true>(S, bsdf, side, ctx), uv[i], uv[n + i], nullptr, bump ? &G : nullptr);
    }
    wo[i] = b.wo.x; wo[n + i] = b.wo.y; wo[2 * (size_t) n + i] = b.wo.z; pdf[i] = b.pdf;
    weight[i] = b.weight.x; weight[n + i] = b.weight.y; weight[2 * (size_t) n + i] = b.weight.z;
    if (eta) eta[i] = b.eta;
    if (stype) stype[i] = b.type;
    if (scomp) scomp[i] = b.comp;
}

/* One lane of har_bsdf_alpha / har_bsdf_alpha_host: the roughness record `bsdf` itself (no `twosided` side is chosen) evaluates at uv point i, before max(., 1e-4) */
HAR_HD void bsdf_alpha_lane(const DScene &S, uint32_t bsdf, uint32_t n, uint32_t i, const float *uv, float *alpha_u, float *alpha_v) {
    float au, av; bsdf_alpha(S, S.bsdfs[bsdf], uv[i], uv[n + i], au, av);
    alpha_u[i] = au; alpha_v[i] = av;
}

/* SmoothDiffuse::eval_pdf / sample (src/bsdfs/diffuse.cpp:159-179, 100-124) */
HAR_HD void diffuse_eval_pdf(Vec3 refl, Vec3 wi, Vec3 wo, Vec3 &value, float &pdf) {
    bool active = wi.z > 0.f && wo.z > 0.f;
    value = active ? (refl * HAR_INV_PI) * wo.z : Vec3(0.f);
    pdf = active ? HAR_INV_PI * wo.z : 0.f;
}
HAR_HD void diffuse_sample(Vec3 refl, Vec3 wi, float s2x, float s2y, Vec3 &wo, float &pdf, Vec3 &weight) {
    wo = square_to_cosine_hemisphere(s2x, s2y);
    pdf = HAR_INV_PI * wo.z;
    weight = (wi.z > 0.f && pdf > 0.f) ? refl : Vec3(0.f);
}

/* AreaLight::sample_direction (src/emitters/area.cpp:118-168), Shape::sample_direction
 * (src/render/shape.cpp:93-110), Rectangle::sample_position (src/shapes/rectangle.cpp:159-173) */
struct DirSample { Vec3 p, n, d; float dist, pdf; };
#define HAR_INV_FOUR_PI 0.07957747154594766788f
/* warp::square_to_uniform_sphere (include/mitsuba/core/warp.h:250-255) */
HAR_HD Vec3 square_to_uniform_sphere(float sx, float sy) {
    float z = fnma_(2.f, sy, 1.f), r = sqrtf(fmaxf(fnma_(z, z, 1.f), 0.f));
    float s, c; sincos_(2.f * HAR_PI * sx, s, c);
    return Vec3(r * c, r * s, z);
}
/* ---- environment map (src/emitters/envmap.cpp) ------------------------------------------------------------------------- */
HAR_HD float clip01_(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
/* warp::interval_to_linear (include/mitsuba/core/warp.h:446-453) */
HAR_HD float interval_to_linear(float v0, float v1, float sample) {
    if (fabsf(v0 - v1) > 1e-4f * (v0 + v1))
        return (v0 - sqrtf(fmaxf(lerp_(v0 * v0, v1 * v1, sample), 0.f))) / (v0 - v1);
    return sample;
}
HAR_HD uint32_t hier_index(uint32_t x, uint32_t y, uint32_t width) { return ((x & 1u) | (((x & ~1u) | (y & 1u)) << 1)) + ((y & ~1u) * width); }
/* Hierarchical2D<Float, 0>::sample (distr_2d.h:520-600) + warp::square_to_bilinear (warp.h:478-494) */
HAR_HD void hier2d_sample(const DEnvmap &E, float sx, float sy, float &u, float &v, float &pdf) {
    sx = clip01_(sx); sy = clip01_(sy);
    uint32_t ox = 0, oy = 0;
    for (int l = (int) E.n_levels - 1; l > 0; --l) {
        ox <<= 1; oy <<= 1;
        const float *q = E.warp + (((E.lvl_offset[l] + hier_index(ox, oy, E.lvl_width[l])) >> 2) << 2);
        const float v00 = q[0], v10 = q[1], v01 = q[2], v11 = q[3];
        sx = clip01_(sx); sy = clip01_(sy);
        const float r0 = v00 + v10, r1 = v01 + v11;
        sy *= r0 + r1;
        const bool ym = sy > r0;
        if (ym) { oy += 1u; sy -= r0; }
        const float dy = ym ? r1 : r0, c0 = ym ? v01 : v00, c1 = ym ? v11 : v10;
        sx *= dy;
        const bool xm = sx > c0;
        if (xm) { sx -= c0; ox += 1u; }
        const float dx = xm ? c1 : c0;
        const float inv = rcp_(dy * dx);
        sy *= dx * inv; sx *= dy * inv;
    }
    const uint32_t W0 = E.lvl_width[0];
    const float *d = E.warp + E.lvl_offset[0] + ox + oy * W0;
    const float v00 = d[0], v10 = d[1], v01 = d[W0], v11 = d[W0 + 1];
    const float r0 = v00 + v10, r1 = v01 + v11;
    sy = interval_to_linear(r0, r1, sy);
    const float c0 = lerp_(v00, v01, sy), c1 = lerp_(v10, v11, sy);
    sx = interval_to_linear(c0, c1, sx);
    pdf = lerp_(c0, c1, sx);
    u = ((float) (int32_t) ox + sx) * (1.f / (float) E.w);                  /* m_patch_size = 1 / (size - 1), size = (W + 1, H) */
    v = ((float) (int32_t) oy + sy) * (1.f / (float) (E.h - 1u));
}
/* Hierarchical2D::eval (distr_2d.h:700-725) */
HAR_HD float hier2d_eval(const DEnvmap &E, float px, float py) {
    px = clip01_(px) * (float) E.w; py = clip01_(py) * (float) (E.h - 1u);
    uint32_t ox = (uint32_t) (int32_t) px, oy = (uint32_t) (int32_t) py;
    if (ox > E.w - 1u) ox = E.w - 1u;
    if (oy > E.h - 2u) oy = E.h - 2u;
    px -= (float) (int32_t) ox; py -= (float) (int32_t) oy;
    const uint32_t W0 = E.lvl_width[0];
    const float *d = E.warp + E.lvl_offset[0] + ox + oy * W0;
    return lerp_(lerp_(d[0], d[1], px), lerp_(d[W0], d[W0 + 1], px), py);
}
/* eval_spectrum, RGB branch (envmap.cpp:531-548,589-597): dr::Texture bilinear lookup with WrapMode::Clamp on the halo'ed storage */
HAR_HD Vec3 envmap_eval_uv(const DEnvmap &E, float u_, float v_) {
    const float rx = (float) E.w, ry = (float) E.h;
    const float u = u_ - floorf(u_), v = clip01_(v_);
    const float pos_x = fma_(u, rx, 1.f) / (rx + 2.f), pos_y = fma_(v, ry - 1.f, 0.5f) / ry;
    const int32_t sw = (int32_t) E.w + 2, H = (int32_t) E.h;
    const float px = fma_(pos_x, (float) sw, -0.5f), py = fma_(pos_y, ry, -0.5f);
    const float fx = floorf(px), fy = floorf(py);
    const int32_t ix = (int32_t) fx, iy = (int32_t) fy;
    const float w1x = px - fx, w1y = py - fy, w0x = 1.f - w1x, w0y = 1.f - w1y;
    const int32_t x0 = ix < 0 ? 0 : (ix > sw - 1 ? sw - 1 : ix), x1 = ix + 1 < 0 ? 0 : (ix + 1 > sw - 1 ? sw - 1 : ix + 1),
                  y0 = iy < 0 ? 0 : (iy > H - 1 ? H - 1 : iy), y1 = iy + 1 < 0 ? 0 : (iy + 1 > H - 1 ? H - 1 : iy + 1);
    const float *p00 = E.tex + 3 * ((size_t) y0 * sw + x0), *p10 = E.tex + 3 * ((size_t) y0 * sw + x1),
                *p01 = E.tex + 3 * ((size_t) y1 * sw + x0), *p11 = E.tex + 3 * ((size_t) y1 * sw + x1);
    float out[3];
    for (int c = 0; c < 3; ++c) {
        const float a = fma_(w0x, p00[c], w1x * p10[c]), b = fma_(w0x, p01[c], w1x * p11[c]);
        out[c] = fma_(w0y, a, w1y * b) * E.scale;
    }
    return Vec3(out[0], out[1], out[2]);
}
/* The transpose of envmap_eval_uv: the four taps of that lookup as indices into the REAL image (H x W texels, row-major) and their weights, with the same arithmetic --
 * envmap_eval_uv(u, v) = scale * sum_k w[k] * image[idx[k]].  The halo columns of the storage are copies of the opposite edge (refresh_halo, envmap.cpp:229-246): storage
 * column 0 is real column W - 1, storage column W + 1 is real column 0, storage column x is real column x - 1 otherwise; rows clamp as the lookup clamps them. */
struct EnvTaps { uint32_t idx[4]; float w[4]; };
HAR_HD void envmap_taps(const DEnvmap &E, float u_, float v_, EnvTaps &T) {
    const float rx = (float) E.w, ry = (float) E.h;
    const float u = u_ - floorf(u_), v = clip01_(v_);
    const float pos_x = fma_(u, rx, 1.f) / (rx + 2.f), pos_y = fma_(v, ry - 1.f, 0.5f) / ry;
    const int32_t sw = (int32_t) E.w + 2, H = (int32_t) E.h, W = (int32_t) E.w;
    const float px = fma_(pos_x, (float) sw, -0.5f), py = fma_(pos_y, ry, -0.5f);
    const float fx = floorf(px), fy = floorf(py);
    const int32_t ix = (int32_t) fx, iy = (int32_t) fy;
    const float w1x = px - fx, w1y = py - fy, w0x = 1.f - w1x, w0y = 1.f - w1y;
    const int32_t x0 = ix < 0 ? 0 : (ix > sw - 1 ? sw - 1 : ix), x1 = ix + 1 < 0 ? 0 : (ix + 1 > sw - 1 ? sw - 1 : ix + 1),
                  y0 = iy < 0 ? 0 : (iy > H - 1 ? H - 1 : iy), y1 = iy + 1 < 0 ? 0 : (iy + 1 > H - 1 ? H - 1 : iy + 1);
    const int32_t r0 = x0 == 0 ? W - 1 : (x0 == W + 1 ? 0 : x0 - 1), r1 = x1 == 0 ? W - 1 : (x1 == W + 1 ? 0 : x1 - 1);
    T.idx[0] = (uint32_t) (y0 * W + r0); T.idx[1] = (uint32_t) (y0 * W + r1); T.idx[2] = (uint32_t) (y1 * W + r0); T.idx[3] = (uint32_t) (y1 * W + r1);
    T.w[0] = w0x * w0y; T.w[1] = w1x * w0y; T.w[2] = w0x * w1y; T.w[3] = w1x * w1y;
}
HAR_HD void envmap_direction_to_uv(Vec3 d, float &u, float &v) {                                   /* envmap.cpp:454-459 */
    u = atan2_(d.x, -d.z) * (0.5f * HAR_INV_PI);
    v = acos_(fminf(fmaxf(d.y, -1.f), 1.f)) * HAR_INV_PI;
}
/* EnvironmentMapEmitter::eval (envmap.cpp:228-236): radiance arriving along world direction d (= -si.wi of the escaping ray) */
HAR_HD Vec3 envmap_eval(const DEnvmap &E, Vec3 d_world) {
    float u, v; envmap_direction_to_uv(xf_vector(E.to_local, d_world), u, v);
    return envmap_eval_uv(E, u, v);
}
/* EnvironmentMapEmitter::pdf_direction (envmap.cpp:325-339) */
HAR_HD float envmap_pdf_direction(const DEnvmap &E, Vec3 d_world) {
    const Vec3 d = xf_vector(E.to_local, d_world);
    float u, v; envmap_direction_to_uv(d, u, v);
    u -= .5f / (float) E.w;
    u -= floorf(u); v -= floorf(v);
    const float inv_sin_theta = rsqrt_(fmaxf(d.x * d.x + d.z * d.z, 0x1p-24f * 0x1p-24f));
    return hier2d_eval(E, u, v) * inv_sin_theta * (1.f / (2.f * (HAR_PI * HAR_PI)));
}
/* EnvironmentMapEmitter::sample_direction (envmap.cpp:284-323) */
/* `unit` (optional): the weight the sample would carry for a unit radiance LOOKUP, 1 / pdf (the map's `scale` is part of the lookup); `uv_out`: where the map is looked up,
 * i.e. after the half-texel shift */
HAR_HD void envmap_sample_direction(const DEnvmap &E, Vec3 ref_p, float sx, float sy, struct DirSample &ds, Vec3 &spec, float *unit = nullptr, float *uv_out = nullptr);

/* PointLight::sample_direction (src/emitters/point.cpp:119-148): emitter type 4, position in to_world[9..11], `radiance` = radiant intensity; pdf 1, delta */
HAR_HD void point_sample_direction(const DEmitter &E, Vec3 ref_p, DirSample &ds, Vec3 &spec, float *unit = nullptr) {
    ds.p = Vec3(E.to_world[9], E.to_world[10], E.to_world[11]); ds.n = Vec3(0.f); ds.pdf = 1.f;
    ds.d = ds.p - ref_p;
    const float dist2 = dot3(ds.d, ds.d), inv_dist = rsqrt_(dist2);
    ds.dist = sqrtf(dist2);
    ds.d = ds.d * inv_dist;
    const float w = inv_dist * inv_dist;
    spec = Vec3(E.radiance[0], E.radiance[1], E.radiance[2]) * w;
    if (unit) *unit = w;
}
/* SpotLight::sample_direction (src/emitters/spot.cpp:177-211) with falloff_curve (:143-151): emitter type 5; the record holds the linear part of to_world^-1 in
 * to_world[0..8], the position in [9..11], normal = (cutoff angle in radians, its cosine, the beam width's cosine), inv_area = 1 / transition width */
HAR_HD void spot_sample_direction(const DEmitter &E, Vec3 ref_p, DirSample &ds, Vec3 &spec, float *unit = nullptr) {
    ds.p = Vec3(E.to_world[9], E.to_world[10], E.to_world[11]); ds.n = Vec3(0.f); ds.pdf = 1.f;
    ds.d = ds.p - ref_p;
    ds.dist = norm3(ds.d);
    const float inv_dist = rcp_(ds.dist);
    ds.d = ds.d * inv_dist;
    const Vec3 local_dir = normalize3(xf_vector(E.to_world, -ds.d));            /* to_world[0..8] = the inverse's linear part: a vector needs no more */
    const float cos_theta = local_dir.z;
    const float beam_res = cos_theta >= E.normal[2] ? 1.f : (E.normal[0] - acos_(cos_theta)) * E.inv_area;
    const float falloff = cos_theta > E.normal[1] ? beam_res : 0.f;
    const bool active = falloff > 0.f;
    const float w = falloff * (inv_dist * inv_dist);
    spec = active ? Vec3(E.radiance[0], E.radiance[1], E.radiance[2]) * w : Vec3(0.f);
    if (unit) *unit = active ? w : 0.f;
}
/* DirectionalEmitter::sample_direction (src/emitters/directional.cpp:149-176): emitter type 6; the record holds the direction of travel in to_world[0..2], the scene's
 * bounding sphere (set_scene, :99-109) in [3..5] (centre) and [6] (radius); `radiance` = the irradiance */
HAR_HD void directional_sample_direction(const DEmitter &E, Vec3 ref_p, DirSample &ds, Vec3 &spec, float *unit = nullptr) {
    const Vec3 d(E.to_world[0], E.to_world[1], E.to_world[2]);
    const float radius = fmaxf(E.to_world[6], norm3(ref_p - Vec3(E.to_world[3], E.to_world[4], E.to_world[5])));
    const float dist = 2.f * radius;
    ds.p = ref_p - d * dist; ds.n = d; ds.pdf = 1.f; ds.d = -d; ds.dist = dist;
    spec = Vec3(E.radiance[0], E.radiance[1], E.radiance[2]);
    if (unit) *unit = 1.f;
}
/* `unit` (optional): the weight the sample would carry for a unit radiance, i.e. d spec / d radiance */
HAR_HD void emitter_sample_direction(const DEmitter &E, Vec3 ref_p, float sx, float sy, DirSample &ds, Vec3 &spec, float *unit = nullptr) {
    if (E.type == 1u) {                                     /* ConstantBackgroundEmitter::sample_direction, constant.cpp:127-153 */
        Vec3 d = square_to_uniform_sphere(sx, sy);
        Vec3 c(E.to_world[0], E.to_world[1], E.to_world[2]);
        float radius = fmaxf(E.to_world[3], norm3(ref_p - c)), dist = 2.f * radius;
        ds.p = fma3(d, dist, ref_p); ds.n = -d; ds.pdf = HAR_INV_FOUR_PI; ds.d = d; ds.dist = dist;
        spec = div3(Vec3(E.radiance[0], E.radiance[1], E.radiance[2]), ds.pdf);
        if (unit) *unit = rcp_(ds.pdf);
        return;
    }
    ds.p = xf_point(E.to_world, Vec3(fma_(sx, 2.f, -1.f), fma_(sy, 2.f, -1.f), 0.f));
    ds.n = Vec3(E.normal[0], E.normal[1], E.normal[2]);
    ds.pdf = E.inv_area;
    ds.d = ds.p - ref_p;
    float dist2 = dot3(ds.d, ds.d);
    ds.dist = sqrtf(dist2);
    ds.d = div3(ds.d, ds.dist);
    float dp = fabsf(dot3(ds.d, ds.n));
    float x = dist2 / dp;
    ds.pdf *= finite_(x) ? x : 0.f;
    bool active = dot3(ds.d, ds.n) < 0.f && ds.pdf != 0.f;
    spec = active ? div3(Vec3(E.radiance[0], E.radiance[1], E.radiance[2]), ds.pdf) : Vec3(0.f);
    if (unit) *unit = active ? rcp_(ds.pdf) : 0.f;
}
HAR_HD void envmap_sample_direction(const DEnvmap &E, Vec3 ref_p, float sx, float sy, DirSample &ds, Vec3 &spec, float *unit, float *uv_out) {
    float u, v, pdf; hier2d_sample(E, sx, sy, u, v, pdf);
    u += .5f / (float) E.w;
    if (uv_out) { uv_out[0] = u; uv_out[1] = v; }
    const bool active = pdf > 0.f;
    float st, ct, sp, cp; sincos_(v * HAR_PI, st, ct); sincos_(u * (2.f * HAR_PI), sp, cp);
    const float inv_sin_theta = rcp_(fmaxf(st, 0x1p-24f));
    const Vec3 dl(sp * st, ct, -cp * st);
    const Vec3 c(E.center[0], E.center[1], E.center[2]);
    const float radius = fmaxf(E.radius, norm3(ref_p - c)), dist = 2.f * radius;
    const Vec3 d = xf_vector(E.to_world, dl);
    ds.p = fma3(d, dist, ref_p); ds.n = -d; ds.d = d; ds.dist = dist;
    ds.pdf = active ? pdf * inv_sin_theta * (1.f / (2.f * (HAR_PI * HAR_PI))) : 0.f;
    spec = active ? div3(envmap_eval_uv(E, u, v), ds.pdf) : Vec3(0.f);
    if (unit) *unit = active ? rcp_(ds.pdf) : 0.f;
}
/* DiscreteDistribution::sample / sample_reuse_pmf (include/mitsuba/core/distr_1d.h:117-140,205-219): value *= sum; dr::binary_search over [lo, hi] (m_valid) with the
 * predicate of the variant -- JIT: (cdf[i] < value || cdf[i] == 0) && cdf[i] != sum, scalar: cdf[i] < value -- then the index, the re-used sample
 * (value - cdf_normalized[index - 1]) / pmf_normalized[index] and the normalised pmf */
HAR_HD uint32_t discrete_sample_reuse_pmf(const float *pmf, const float *cdf, uint32_t lo, uint32_t hi, float sum, float normalization, float value01, bool jit,
                                          float &reused, float &pmf_out) {
    const float value = value01 * sum;
    uint32_t start = lo, end = hi, iterations = 0;
    if (start < end) { uint32_t span = end - start; iterations = 1; while (span >>= 1) ++iterations; }
    for (uint32_t i = 0; i < iterations; ++i) {
        const uint32_t middle = (start + end) >> 1;
        const float c = cdf[middle];
        const bool cond = jit ? (((c < value) || c == 0.f) && c != sum) : (c < value);
        if (cond) start = middle + 1u < end ? middle + 1u : end; else end = middle;
    }
    const float pmf_n = pmf[start] * normalization, cdf_n = start > 0u ? cdf[start - 1u] * normalization : 0.f;
    reused = (value01 - cdf_n) / pmf_n; pmf_out = pmf_n;
    return start;
}
/* Scene::sample_emitter (src/render/scene.cpp:248-271) and Scene::pdf_emitter (:273-279): the emitter a uniform sample picks, the weight 1 / probability and the re-used
 * sample.  Uniform choice unless the scene holds a distribution over the emitters' sampling weights (DScene::emitter_distr).  `jit`: the variant's predicate of
 * DiscreteDistribution::sample.  No emitters: index 0xffffffff, weight 0 (:251-256). */
HAR_HD uint32_t scene_sample_emitter(const DScene &S, float sample, bool jit, float &weight, float &reused) {
    weight = 1.f; reused = sample;
    if (S.n_emitters < 2u) { if (S.n_emitters == 0u) weight = 0.f; return S.n_emitters ? 0u : 0xffffffffu; }
    if (S.emitter_distr != nullptr) {
        float p;
        const uint32_t index = discrete_sample_reuse_pmf(S.emitter_distr, S.emitter_distr + S.n_emitters, S.emitter_valid_lo, S.emitter_valid_hi, S.emitter_sum, S.emitter_norm,
                                                         sample, jit, reused, p);
        weight = rcp_(p);
        return index;
    }
    const float scaled = sample * (float) S.n_emitters;
    uint32_t index = (uint32_t) scaled; if (index > S.n_emitters - 1u) index = S.n_emitters - 1u;
    weight = (float) S.n_emitters; reused = scaled - (float) index;
    return index;
}
HAR_HD float scene_pdf_emitter(const DScene &S, uint32_t index) {
    if (S.emitter_distr == nullptr) return S.n_emitters ? 1.f / (float) S.n_emitters : 0.f;      /* m_emitter_pmf, scene.cpp:139 */
    return S.emitter_distr[index] * S.emitter_norm;                                             /* eval_pmf_normalized */
}
/* AreaLight::sample_direction on a triangle mesh: Mesh::sample_position (src/render/mesh.cpp:1662-1712) -- DiscreteDistribution::sample_reuse over the
 * face areas (distr_1d.h:117-183, JIT predicate, dr::binary_search over [0, n - 1]), warp::square_to_uniform_triangle (warp.h:153-156), interpolated
 * vertex normals when the mesh has them -- then Shape::sample_direction (shape.cpp:93-110) and the one-sided test of area.cpp:118-168 */
HAR_HD void mesh_emitter_sample_direction(const DScene &S, const DEmitter &E, Vec3 ref_p, float sx, float sy, DirSample &ds, Vec3 &spec, float *unit = nullptr) {
    const uint32_t off = as_u32(E.to_world[0]), nf = as_u32(E.to_world[1]);
    const float sum = E.to_world[2], normalization = E.inv_area;
    const float *pmf = S.emitter_cdf + off, *cdf = pmf + nf;
    const float value = sy * sum;
    uint32_t start = 0, end = nf - 1u, iterations = 0;
    if (start < end) { uint32_t span = end - start; iterations = 1; while (span >>= 1) ++iterations; }
    for (uint32_t i = 0; i < iterations; ++i) {
        const uint32_t middle = (start + end) >> 1;
        const float c = cdf[middle];
        const bool cond = ((c < value) || c == 0.f) && c != sum;
        if (cond) start = middle + 1u < end ? middle + 1u : end; else end = middle;
    }
    const uint32_t idx = start;
    const float pmf_n = pmf[idx] * normalization, cdf_n = idx > 0 ? cdf[idx - 1u] * normalization : 0.f;
    sy = (sy - cdf_n) / pmf_n;
    const DMesh M = S.meshes[E.mesh];
    const uint32_t *f = S.faces + 4 * ((size_t) M.foff + idx);
    const float *v0 = S.verts + 8 * ((size_t) M.voff + f[0]), *v1 = S.verts + 8 * ((size_t) M.voff + f[1]), *v2 = S.verts + 8 * ((size_t) M.voff + f[2]);
    const Vec3 p0(v0[0], v0[1], v0[2]), e0 = Vec3(v1[0], v1[1], v1[2]) - p0, e1 = Vec3(v2[0], v2[1], v2[2]) - p0;
    const float t = sqrtf(fmaxf(1.f - sx, 0.f)), bx = 1.f - t, by = t * sy;
    ds.p = fma3(e0, bx, fma3(e1, by, p0));
    Vec3 n;
    if (M.flags & 1u) n = fma3(Vec3(v0[3], v0[4], v0[5]), 1.f - bx - by, fma3(Vec3(v1[3], v1[4], v1[5]), bx, Vec3(v2[3], v2[4], v2[5]) * by));
    else n = cross3(e0, e1);
    ds.n = normalize3(n);
    ds.pdf = normalization;
    ds.d = ds.p - ref_p;
    const float dist2 = dot3(ds.d, ds.d);
    ds.dist = sqrtf(dist2);
    ds.d = div3(ds.d, ds.dist);
    const float dp = fabsf(dot3(ds.d, ds.n));
    const float x = dist2 / dp;
    ds.pdf *= finite_(x) ? x : 0.f;
    const bool active = dot3(ds.d, ds.n) < 0.f && ds.pdf != 0.f;
    spec = active ? div3(Vec3(E.radiance[0], E.radiance[1], E.radiance[2]), ds.pdf) : Vec3(0.f);
    if (unit) *unit = active ? rcp_(ds.pdf) : 0.f;
}
/* AreaLight::pdf_direction (area.cpp:170-197) / Shape::pdf_direction (shape.cpp:112-124) */
HAR_HD float emitter_pdf_direction(const DEmitter &E, Vec3 d, Vec3 n, float dist) {
    float dp = dot3(d, n);
    if (!(dp < 0.f)) return 0.f;
    float adp = fabsf(dp);
    float pdf = E.inv_area;
    pdf *= (adp != 0.f) ? (dist * dist) / adp : 0.f;
    return pdf;
}

/* ---- AreaLight with a spatially varying radiance (emitter type 7; area.cpp:133-165, 185-191) */
/* dr::binary_search(0, last, cdf[i] < value) */
HAR_HD uint32_t cdf_search(const float *cdf, uint32_t last, float value) {
    uint32_t start = 0, end = last, iterations = 0;
    if (start < end) { uint32_t span = end - start; iterations = 1; while (span >>= 1) ++iterations; }
    for (uint32_t i = 0; i < iterations; ++i) {
        const uint32_t middle = (start + end) >> 1;
        if (cdf[middle] < value) start = middle + 1u < end ? middle + 1u : end; else end = middle;
    }
    return start;
}
/* DiscreteDistribution2D::pdf (distr_2d.h:121-131) of texel (x, y): difference of neighbouring conditional sums * normalization */
HAR_HD float texel_pdf(const float *cond, uint32_t w, float normalization, uint32_t x, uint32_t y) {
    const size_t i = (size_t) y * w + x;
    return (cond[i] - (x > 0u ? cond[i - 1u] : 0.f)) * normalization;
}
/* BitmapTexture::pdf_texture (bitmap.cpp:673-703), position in the TEXTURE's parameterisation */
HAR_HD float bitmap_pdf_texture(const DTexture &T, const float *tab, float u, float v) {
    const float *cond = tab + HAR_TEXEL_TABLE_HEADER + T.h;
    const float texels = (float) ((int32_t) T.w * (int32_t) T.h);
    const int32_t W = (int32_t) T.w, H = (int32_t) T.h;
    if (T.mode & 1u) {
        const int32_t x = tex_wrap((int32_t) floorf(u * (float) T.w), W, T.mode), y = tex_wrap((int32_t) floorf(v * (float) T.h), H, T.mode);
        return texel_pdf(cond, T.w, tab[1], (uint32_t) x, (uint32_t) y) * texels;
    }
    const float px = fma_(u, (float) T.w, -0.5f), py = fma_(v, (float) T.h, -0.5f), fx = floorf(px), fy = floorf(py);
    const int32_t ix = (int32_t) fx, iy = (int32_t) fy;
    const float w1x = px - fx, w1y = py - fy, w0x = 1.f - w1x, w0y = 1.f - w1y;
    const uint32_t x0 = (uint32_t) tex_wrap(ix, W, T.mode), x1 = (uint32_t) tex_wrap(ix + 1, W, T.mode), y0 = (uint32_t) tex_wrap(iy, H, T.mode), y1 = (uint32_t) tex_wrap(iy + 1, H, T.mode);
    const float v00 = texel_pdf(cond, T.w, tab[1], x0, y0), v10 = texel_pdf(cond, T.w, tab[1], x1, y0), v01 = texel_pdf(cond, T.w, tab[1], x0, y1), v11 = texel_pdf(cond, T.w, tab[1], x1, y1);
    const float v0 = fma_(w0x, v00, w1x * v10), v1 = fma_(w0x, v01, w1x * v11);
    return fma_(w0y, v0, w1y * v1) * texels;
}
/* warp::interval_to_tent (warp.h:196-200) */
HAR_HD float interval_to_tent(float s) {
    s -= 0.5f;
    return mulsign_(1.f - sqrtf(fmaxf(fma_(fabsf(s), -2.f, 1.f), 0.f)), s);
}
/* BitmapTexture::sample_position (bitmap.cpp:622-660) over DiscreteDistribution2D::sample (distr_2d.h:141-180): surface uv + its density */
HAR_HD void bitmap_sample_position(const DTexture &T, const float *tab, float sx, float sy, float &u, float &v, float &pdf) {
    const float *marg = tab + HAR_TEXEL_TABLE_HEADER, *cond_all = marg + T.h;
    sx = fminf(fmaxf(sx, 1.17549435e-38f), 0x1.fffffep-1f); sy = fminf(fmaxf(sy, 1.17549435e-38f), 0x1.fffffep-1f);
    sy *= tab[0];
    const uint32_t row = cdf_search(marg, T.h - 1u, sy);
    const float *cond = cond_all + (size_t) row * T.w;
    sx *= cond[T.w - 1u];
    const uint32_t col = cdf_search(cond, T.w - 1u, sx);
    const float c0 = col > 0u ? cond[col - 1u] : 0.f, c1 = cond[col], r0 = row > 0u ? marg[row - 1u] : 0.f, r1 = marg[row];
    sx -= c0; sy -= r0;
    if (c1 != c0) sx = sx / (c1 - c0);
    if (r1 != r0) sy = sy / (r1 - r0);
    const float inv_w = 1.f / (float) T.w, inv_h = 1.f / (float) T.h;
    float qx, qy;
    if (T.mode & 1u) { qx = ((float) col + sx) * inv_w; qy = ((float) row + sy) * inv_h; }
    else {
        qx = ((float) col + 0.5f + interval_to_tent(sx)) * inv_w; qy = ((float) row + 0.5f + interval_to_tent(sy)) * inv_h;
        if (!(T.mode & 6u)) { if (qx < 0.f) qx += 1.f; if (qx > 1.f) qx -= 1.f; if (qy < 0.f) qy += 1.f; if (qy > 1.f) qy -= 1.f; }
        else { if (qx < 0.f) qx = -qx; if (qx > 1.f) qx = 2.f - qx; if (qy < 0.f) qy = -qy; if (qy > 1.f) qy = 2.f - qy; }
    }
    u = fma_(tab[3], qy, fma_(tab[2], qx, tab[4])); v = fma_(tab[6], qy, fma_(tab[5], qx, tab[7]));
    pdf = bitmap_pdf_texture(T, tab, qx, qy);
}
HAR_HD Vec3 texture_eval_uv(const DTexture &T, float u, float v) { TexTaps taps; tex_taps(T, u, v, taps); return tex_fetch(T, taps); }
/* AreaLight::sample_direction, spatially varying branch (area.cpp:133-165) with Rectangle::eval_parameterization (rectangle.cpp:215-237) */
/* `unit` / `uv_out` (optional, prb adjoint w.r.t. the bitmap's texels -- `radiance` is a differentiable traverse entry, area.cpp:64-70): the weight the sample carries per unit of
 * radiance(ds.uv), and ds.uv itself; the texel distribution the sample was drawn from stays detached (prb.py:174-175) */
HAR_HD void textured_area_sample_direction(const DScene &S, const DEmitter &E, Vec3 ref_p, float sx, float sy, DirSample &ds, Vec3 &spec, float *unit = nullptr, float *uv_out = nullptr) {
    const DTexture T = S.textures[as_u32(E.radiance[0])];
    const float *tab = S.emitter_cdf + as_u32(E.radiance[1]);
    float u, v, pdf;
    bitmap_sample_position(T, tab, sx, sy, u, v, pdf);
    if (uv_out) { uv_out[0] = u; uv_out[1] = v; }
    bool active = pdf != 0.f;
    ds.p = xf_point(E.to_world, Vec3(fma_(u, 2.f, -1.f), fma_(v, 2.f, -1.f), 0.f));
    ds.n = Vec3(E.normal[0], E.normal[1], E.normal[2]);
    ds.d = ds.p - ref_p;
    const float dist2 = dot3(ds.d, ds.d);
    ds.dist = sqrtf(dist2);
    ds.d = div3(ds.d, ds.dist);
    const float dp = dot3(ds.d, ds.n);
    active = active && dp < 0.f;
    ds.pdf = active ? pdf / E.radiance[2] * dist2 / -dp : 0.f;
    spec = active ? div3(texture_eval_uv(T, u, v), ds.pdf) : Vec3(0.f);
    if (unit) *unit = active ? rcp_(ds.pdf) : 0.f;
}
/* AreaLight::pdf_direction, spatially varying branch (area.cpp:185-191): pdf_position(ds.uv) * dist^2 / (|dp_du x dp_dv| * -dp) */
HAR_HD float textured_area_pdf_direction(const DScene &S, const DEmitter &E, Vec3 d, Vec3 n, float dist, float u, float v) {
    const float dp = dot3(d, n);
    if (!(dp < 0.f)) return 0.f;
    const DTexture T = S.textures[as_u32(E.radiance[0])];
    float tu = u, tv = v;
    if (T.mode & HAR_TEX_HAS_UV_XF) { tu = fma_(T.uvm[1], v, fma_(T.uvm[0], u, T.uvm[2])); tv = fma_(T.uvm[4], v, fma_(T.uvm[3], u, T.uvm[5])); }
    return bitmap_pdf_texture(T, S.emitter_cdf + as_u32(E.radiance[1]), tu, tv) * (dist * dist) / (E.radiance[2] * -dp);
}

/* ---- Projector (src/emitters/projector.cpp), emitter type 8: the reciprocal of the perspective camera.  The record (DEmitter keeps its size: DScene::emitter0 passes
 * one as kernel arguments) holds to_world^-1 in to_world[0..11], `mesh` = the irradiance bitmap's index in DScene::textures (0xffffffff: a constant irradiance),
 * radiance = the bits of that index in [0] (where light_texel_commit reads it) or, for a constant, irradiance * scale; inv_area = the bits of the offset of its block in
 * DScene::emitter_cdf, normal = (scale, x_fov in degrees, -) as the host handed them in.  The block, HAR_PROJECTOR_TABLE floats (projector_table_fill in
 * har_scene_host.cpp): [0..3] the live coefficients m00, m02, m11, m12 of the two uv rows of camera_to_sample (perspective_projection(size, size, 0, x_fov, 1e-4, 1e4),
 * sensor.h:234-269: u = (m00 x + m02 z) / z, v = (m11 y + m12 z) / z), [4..6] the translation of to_world, [7..9] to_world * (0, 0, 1), [10] scale, [11] x_fov */
#define HAR_PROJECTOR_TABLE 12u
/* Projector::sample_direction (projector.cpp:202-244).  `unit` (optional): the weight the sample carries per unit of the irradiance LOOKUP, pi / (z^2 * -dot(n, d)) --
 * `scale` left out, as for the environment map: spec = lookup * scale * unit for a bitmap, (irradiance * scale) * unit for a constant; `uv_out`: ds.uv.  A lane outside
 * the frustum never touches the bitmap (its uv may be anything, NaN included). */
HAR_HD void projector_sample_direction(const DScene &S, const DEmitter &E, Vec3 ref_p, DirSample &ds, Vec3 &spec, float *unit = nullptr, float *uv_out = nullptr) {
    const float *tab = S.emitter_cdf + as_u32(E.inv_area);
    const Vec3 it_local = xf_point(E.to_world, ref_p);                                      /* :208 */
    const float inv_w = rcp_(it_local.z);                                                    /* :211, the homogeneous divide (w = z) */
    const float u = fma_(tab[0], it_local.x, tab[1] * it_local.z) * inv_w, v = fma_(tab[2], it_local.y, tab[3] * it_local.z) * inv_w;
    const bool active = u >= 0.f && u <= 1.f && v >= 0.f && v <= 1.f && it_local.z > 0.f;   /* :212 */
    ds.p = Vec3(tab[4], tab[5], tab[6]); ds.n = Vec3(tab[7], tab[8], tab[9]);                /* :222-223 */
    if (uv_out) { uv_out[0] = u; uv_out[1] = v; }
    ds.pdf = active ? 1.f : 0.f;
    ds.d = ds.p - ref_p;
    const float dist_squared = dot3(ds.d, ds.d);
    ds.dist = sqrtf(dist_squared);
    ds.d = ds.d * rcp_(ds.dist);                                                             /* :229-232 */
    const float denom = (it_local.z * it_local.z) * -dot3(ds.n, ds.d);                       /* :240-241 */
    spec = Vec3(0.f);
    if (active) {
        if (E.mesh != 0xffffffffu) spec = texture_eval_uv(S.textures[E.mesh], u, v) * (HAR_PI * tab[10] / denom);
        else spec = Vec3(E.radiance[0], E.radiance[1], E.radiance[2]) * (HAR_PI / denom);    /* (`scale` is in the record's colour) */
    }
    if (unit) *unit = active ? HAR_PI / denom : 0.f;
}

/* One lane of the array-valued Emitter::sample_direction of a projector (k_api_emitter_sample_direction and its host twin, har_emitter_sample_direction_host): rows
 * d (3), dist, pdf, p (3), n (3), uv (2), spec (3) of n lanes each; a lane whose `active` byte is 0 writes zeros.  The record is the one the renders sample (for a
 * constant irradiance `scale` is in its colour). */
HAR_HD void projector_sample_direction_lane(const DScene &S, uint32_t emitter, uint32_t n, uint32_t i, const float *ref_p, bool active,
                                            float *d, float *dist, float *pdf, float *p, float *nrm, float *uv, float *spec) {
    const size_t i1 = (size_t) n + i, i2 = 2 * (size_t) n + i;
    DirSample ds; ds.p = Vec3(0.f); ds.n = Vec3(0.f); ds.d = Vec3(0.f); ds.dist = 0.f; ds.pdf = 0.f;
    Vec3 w(0.f); float q[2] = { 0.f, 0.f };
    if (active) projector_sample_direction(S, S.emitters[emitter], Vec3(ref_p[i], ref_p[i1], ref_p[i2]), ds, w, nullptr, q);
    d[i] = ds.d.x; d[i1] = ds.d.y; d[i2] = ds.d.z; dist[i] = ds.dist; pdf[i] = ds.pdf;
    p[i] = ds.p.x; p[i1] = ds.p.y; p[i2] = ds.p.z; nrm[i] = ds.n.x; nrm[i1] = ds.n.y; nrm[i2] = ds.n.z;
    uv[i] = q[0]; uv[i1] = q[1]; spec[i] = w.x; spec[i1] = w.y; spec[i2] = w.z;
}

/* PerspectiveCamera::sample_ray (src/sensors/perspective.cpp:200-237); CAM: DSensor, or DCamera (a child of a batch sensor).  For projection 0 and 1 ONLY: in a
 * DSensor of projection 2 the words of ppo_x / ppo_y hold the lens parameters.  Callers that may meet a thin lens go through camera_sample_ray<true>; the others
 * (k_raygen, k_shade's first-vertex rebuild, the scalar driver) are never handed one: launch_raygen, run_chunk and har_render_scalar send it elsewhere or refuse it. */
template <class CAM>
HAR_HD void sensor_sample_ray(const CAM &C, float px, float py, Vec3 &o, Vec3 &d, float &maxt) {
    const float *M = C.s2c;
    float r0 = M[3], r1 = M[7], r2 = M[11], r3 = M[15];
    px = px + C.ppo_x; py = py + C.ppo_y;                              /* perspective.cpp:216-221 */
    r0 = fma_(M[0], px, r0); r1 = fma_(M[4], px, r1); r2 = fma_(M[8], px, r2);  r3 = fma_(M[12], px, r3);
    r0 = fma_(M[1], py, r0); r1 = fma_(M[5], py, r1); r2 = fma_(M[9], py, r2);  r3 = fma_(M[13], py, r3);
    r0 = fma_(M[2], 0.f, r0); r1 = fma_(M[6], 0.f, r1); r2 = fma_(M[10], 0.f, r2); r3 = fma_(M[14], 0.f, r3);
    if (C.projection == 1u) {            /* OrthographicCamera::sample_ray (orthographic.cpp:131-157): near_p = sample_to_camera * p (affine), o = to_world * near_p, d = normalize(to_world * +z) */
        const float *T = C.to_world;
        Vec3 ow(fma_(T[0], r0, T[3]), fma_(T[4], r0, T[7]), fma_(T[8], r0, T[11]));
        ow = Vec3(fma_(T[1], r1, ow.x), fma_(T[5], r1, ow.y), fma_(T[9], r1, ow.z));
        o = Vec3(fma_(T[2], r2, ow.x), fma_(T[6], r2, ow.y), fma_(T[10], r2, ow.z));
        d = normalize3(Vec3(T[2], T[6], T[10]));
        maxt = C.far_clip - C.near_clip;
        return;
    }
    float iw = rcp_(r3);
    Vec3 dl = normalize3(Vec3(r0 * iw, r1 * iw, r2 * iw));
    const float *T = C.to_world;
    Vec3 dw(T[0] * dl.x, T[4] * dl.x, T[8] * dl.x);
    dw = Vec3(fma_(T[1], dl.y, dw.x), fma_(T[5], dl.y, dw.y), fma_(T[9], dl.y, dw.z));
    dw = Vec3(fma_(T[2], dl.z, dw.x), fma_(T[6], dl.z, dw.y), fma_(T[10], dl.z, dw.z));
    float inv_z = rcp_(dl.z);
    float near_t = C.near_clip * inv_z, far_t = C.far_clip * inv_z;
    d = dw;
    o = Vec3(T[3], T[7], T[11]) + dw * near_t;
    maxt = far_t - near_t;
}

/* ThinLensCamera::sample_ray (src/sensors/thinlens.cpp:219-257): the film position goes to the near plane, from there to the plane of focus; the ray leaves the point
 * (ax, ay) -> concentric disk * aperture_radius of the lens towards that point.  Unlike the pinhole models the origins of a pixel's rays differ. */
template <class CAM>
HAR_HD void thinlens_sample_ray(const CAM &C, float px, float py, float ax, float ay, Vec3 &o, Vec3 &d, float &maxt) {
    const float *M = C.s2c;
    float r0 = M[3], r1 = M[7], r2 = M[11], r3 = M[15];
    r0 = fma_(M[0], px, r0); r1 = fma_(M[4], px, r1); r2 = fma_(M[8], px, r2);  r3 = fma_(M[12], px, r3);
    r0 = fma_(M[1], py, r0); r1 = fma_(M[5], py, r1); r2 = fma_(M[9], py, r2);  r3 = fma_(M[13], py, r3);
    r0 = fma_(M[2], 0.f, r0); r1 = fma_(M[6], 0.f, r1); r2 = fma_(M[10], 0.f, r2); r3 = fma_(M[14], 0.f, r3);
    const float iw = rcp_(r3);
    const Vec3 near_p(r0 * iw, r1 * iw, r2 * iw);
    float lx, ly; square_to_uniform_disk_concentric(ax, ay, lx, ly);
    lx = C.aperture_radius * lx; ly = C.aperture_radius * ly;                       /* aperture_p = (lx, ly, 0) */
    const float fs = C.focus_distance / near_p.z;
    const Vec3 focus_p(near_p.x * fs, near_p.y * fs, near_p.z * fs);
    const Vec3 dl = normalize3(Vec3(focus_p.x - lx, focus_p.y - ly, focus_p.z - 0.f));
    const float *T = C.to_world;
    Vec3 ow(fma_(T[0], lx, T[3]), fma_(T[4], lx, T[7]), fma_(T[8], lx, T[11]));
    ow = Vec3(fma_(T[1], ly, ow.x), fma_(T[5], ly, ow.y), fma_(T[9], ly, ow.z));
    ow = Vec3(fma_(T[2], 0.f, ow.x), fma_(T[6], 0.f, ow.y), fma_(T[10], 0.f, ow.z));
    Vec3 dw(T[0] * dl.x, T[4] * dl.x, T[8] * dl.x);
    dw = Vec3(fma_(T[1], dl.y, dw.x), fma_(T[5], dl.y, dw.y), fma_(T[9], dl.y, dw.z));
    dw = Vec3(fma_(T[2], dl.z, dw.x), fma_(T[6], dl.z, dw.y), fma_(T[10], dl.z, dw.z));
    const float inv_z = rcp_(dl.z);
    const float near_t = C.near_clip * inv_z, far_t = C.far_clip * inv_z;
    d = dw;
    o = ow + dw * near_t;
    maxt = far_t - near_t;
}
/* sample_ray of any camera model; LENS = false leaves the thin lens out of kernels that never see one (they keep their registers) */
template <bool LENS, class CAM>
HAR_HD void camera_sample_ray(const CAM &C, float px, float py, float ax, float ay, Vec3 &o, Vec3 &d, float &maxt) {
    if (LENS && C.projection == 2u) { thinlens_sample_ray(C, px, py, ax, ay, o, d, maxt); return; }
    sensor_sample_ray(C, px, py, o, d, maxt);
}

/* GaussianFilter::eval, LLVM branch: max(estrin(x^2, coeff), 0) (src/rfilters/gaussian.cpp:57-101) */
HAR_HD float estrin10(float x, const float *c) {
    float x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    float a0 = fma_(x, c[1], c[0]), a1 = fma_(x, c[3], c[2]), a2 = fma_(x, c[5], c[4]), a3 = fma_(x, c[7], c[6]), a4 = fma_(x, c[9], c[8]);
    float b0 = fma_(x2, a1, a0), b1 = fma_(x2, a3, a2);
    float c0 = fma_(x4, b1, b0);
    return fma_(x8, a4, c0);
}
/* ... and the other reconstruction filters: tent.cpp:54-56, mitchell.cpp:60-79, catmullrom.cpp:39-54, lanczos.cpp:57-67 */
HAR_HD float rfilter_eval(const DSensor &C, float x) {
    switch (C.rfilter) {
    case 2: return fmaxf(0.f, 1.f - fabsf(x * (1.f / C.radius)));
    case 3: {
        x = fabsf(x); const float x2 = x * x, x3 = x2 * x, B = C.rf_p0, Cc = C.rf_p1;
        const float a3 = (12.f - 9.f * B - 6.f * Cc), a2 = (-18.f + 12.f * B + 6.f * Cc), a0 = (6.f - 2.f * B),
                    b3 = (-B - 6.f * Cc), b2 = (6.f * B + 30.f * Cc), b1 = (-12.f * B - 48.f * Cc), b0 = (8.f * B + 24.f * Cc);
        const float r = (1.f / 6.f) * (x < 1.f ? fma_(a3, x3, fma_(a2, x2, a0)) : fma_(b3, x3, fma_(b2, x2, fma_(b1, x, b0))));
        return x < 2.f ? r : 0.f;
    }
    case 4: {
        x = fabsf(x); const float x2 = x * x, x3 = x2 * x, B = 0.f, Cc = .5f;
        const float r = (1.f / 6.f) * (x < 1.f ? (12.f - 9.f * B - 6.f * Cc) * x3 + (-18.f + 12.f * B + 6.f * Cc) * x2 + (6.f - 2.f * B)
                                               : (-B - 6.f * Cc) * x3 + (6.f * B + 30.f * Cc) * x2 + (-12.f * B - 48.f * Cc) * x + (8.f * B + 24.f * Cc));
        return x < 2.f ? r : 0.f;
    }
    case 5: {
        x = fabsf(x);
        const float x1 = HAR_PI * x, x2 = x1 / C.radius;
        float s1, c1, s2, c2; sincos_(x1, s1, c1); sincos_(x2, s2, c2);
        const float r = (s1 * s2) / (x1 * x2);
        return x < HAR_EPSILON ? 1.f : (x > C.radius ? 0.f : r);
    }
    default: return fmaxf(estrin10(x * x, C.coeff), 0.f);
    }
}

/* lane -> pixel/sample mapping of SamplingIntegrator::render (integrator.cpp:322-339) and
 * render_sample (:448-466): returns integer pixel (crop-relative) and jittered film position */
struct LaneSample { float pos_x, pos_y, ipos_x, ipos_y; };
HAR_HD LaneSample lane_sample(const DSensor &C, uint32_t idx, uint32_t spp, uint32_t log_spp, float jx, float jy) {
    uint32_t p = (log_spp != 0xffffffffu) ? (idx >> log_spp) : (idx / spp);
    uint32_t y = p / C.samp_w, x = p - C.samp_w * y;                 /* integrator.cpp:330-331 over film_size = crop_size + 2 * border_size */
    LaneSample L;
    /* pos -= border_size; pos += crop_offset (integrator.cpp:333-336): a Vector2i, negative in the border of a crop window at the film's origin */
    L.ipos_x = (float) ((int32_t) (x + C.crop_x) - (int32_t) C.border); L.ipos_y = (float) ((int32_t) (y + C.crop_y) - (int32_t) C.border);
    L.pos_x = L.ipos_x + jx; L.pos_y = L.ipos_y + jy;
    return L;
}
/* BatchSensor::sample_ray (src/sensors/batch.cpp:138-145): the child a film position falls on and the position on that child's film.  The product and the difference
 * are two rounded fp32 operations, as in the reference (the build keeps -ffp-contract=off); a position of 1 or beyond lands on the last child with px2 >= 1 */
HAR_HD uint32_t batch_select(float px, uint32_t n, float &px2) {
    const float idx_f = px * (float) n;
    const uint32_t idx_u = (uint32_t) idx_f;
    px2 = idx_f - (float) idx_u;
    return idx_u < n - 1u ? idx_u : n - 1u;
}
/* the ray of child `batch_select(px)` of the table.  Device: the lanes of a wave are consecutive samples of consecutive pixels of a row, so all of them pick the
 * same child except where the wave crosses a seam (or a row's end) -- the uniform wave reads the record through an index it holds in a scalar register (scalar loads,
 * one copy of the 160-byte record per wave), the others read theirs per lane. */
template <bool LENS = false>      /* LENS: children may be thin lenses, (ax, ay) is the aperture sample (pinhole children ignore it) */
HAR_HD void batch_sample_ray(const DBatch &B, float px, float py, Vec3 &o, Vec3 &d, float &maxt, float ax = .5f, float ay = .5f) {
    float px2;
    const uint32_t index = batch_select(px, B.n, px2);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t first = (uint32_t) __builtin_amdgcn_readfirstlane((int) index);
    if (__builtin_amdgcn_ballot_w64(index != first) == 0ull) { camera_sample_ray<LENS>(B.cams[first], px2, py, ax, ay, o, d, maxt); return; }
#endif
    camera_sample_ray<LENS>(B.cams[index], px2, py, ax, ay, o, d, maxt);
}
/* `batch` (optional): the children of a batch sensor -- C is then the batch sensor's wide film, whose crop window is the full film */
template <bool LENS = false>
HAR_HD void lane_camera_ray(const DSensor &C, const LaneSample &L, Vec3 &o, Vec3 &d, float &maxt, const DBatch *batch = nullptr, float ax = .5f, float ay = .5f) {
    float sx = 1.f / (float) C.crop_w, sy = 1.f / (float) C.crop_h;
    float ox = -(float) C.crop_x * sx, oy = -(float) C.crop_y * sy;
    if (batch) { batch_sample_ray<LENS>(*batch, fma_(L.pos_x, sx, ox), fma_(L.pos_y, sy, oy), o, d, maxt, ax, ay); return; }
    camera_sample_ray<LENS>(C, fma_(L.pos_x, sx, ox), fma_(L.pos_y, sy, oy), ax, ay, o, d, maxt);
}

} // namespace har
