/*
 * har_aov.h -- AOVIntegratorImpl::sample (src/integrators/aov.cpp:175-306) for ONE lane, HAR_HD: the same source runs in the
 * HIP kernels of har_aov.hip and in the host twin (har_aov_sample_host, har_scalar.cpp), so that the two can be compared bit for bit.
 *
 * An AOV is a function of the camera ray's closest surface interaction.  On a miss the whole interaction is zero (aov.cpp:186), so every
 * channel is zero.  The albedo goes through the BSDF code of har_bsdf.h / har_scene.h (bsdf_side, bsdf_inputs, bsdf_eval_pdf_one): there is
 * no second BSDF implementation here.
 */
#pragma once
#include "har_scene.h"

namespace har {

/* AOV types (the values of HAR_AOV_* in hip_ad_rgb.h) and their channel counts (aov.cpp:117-168) */
enum { AOV_ALBEDO = 0, AOV_DEPTH = 1, AOV_POSITION = 2, AOV_UV = 3, AOV_GEO_NORMAL = 4, AOV_SH_NORMAL = 5, AOV_DP_DU = 6, AOV_DP_DV = 7, AOV_PRIM_INDEX = 8,
       AOV_SHAPE_INDEX = 9, AOV_TYPE_COUNT = 10 };
#define HAR_AOV_MAX_TYPES 32         /* entries of one `aovs` specification */
#define HAR_AOV_MAX_CHANNELS 96
HAR_HD uint32_t aov_type_channels(uint32_t type) {
    return (type == AOV_DEPTH || type == AOV_PRIM_INDEX || type == AOV_SHAPE_INDEX) ? 1u : type == AOV_UV ? 2u : 3u;
}

/* the AOV list of a pass, by value in the kernel arguments */
struct AovSpec { uint32_t n, channels; uint8_t type[HAR_AOV_MAX_TYPES]; };

/* types[0 .. n) -> spec; returns nullptr, or what is wrong with the list */
inline const char *aov_spec_lower(uint32_t n, const uint32_t *types, AovSpec &spec) {
    spec.n = 0; spec.channels = 0;
    for (uint32_t k = 0; k < HAR_AOV_MAX_TYPES; ++k) spec.type[k] = 0;
    if (n && !types) return "null AOV type list";
    if (n > HAR_AOV_MAX_TYPES) return "too many AOVs in one integrator (at most 32)";
    for (uint32_t k = 0; k < n; ++k) {
        if (types[k] >= (uint32_t) AOV_TYPE_COUNT) return "Invalid AOV type (not one of HAR_AOV_*)!";
        spec.type[k] = (uint8_t) types[k]; spec.channels += aov_type_channels(types[k]);
    }
    spec.n = n;
    return nullptr;
}

/* BSDF::eval_diffuse_reflectance(si) of the BSDF of mesh `si.mesh` (aov.cpp:206-222):
 *  - `twosided` picks the record of the side the ray arrives on, with wi.z made positive, and is zero at wi.z == 0 for a pair of two BSDFs
 *    (twosided.cpp:284-307) -- what bsdf_side() does for eval / sample;
 *  - `diffuse`: the reflectance texture at si.uv (diffuse.cpp:181); `plastic` / `roughplastic`: `diffuse_reflectance` (plastic.cpp:362, roughplastic.cpp:504);
 *    both are colour slot 0 of the record;
 *  - every other model: the base class, eval(BSDFContext(), si, wo = (0, 0, 1)) * pi (src/render/bsdf.cpp:38-43). */
template <uint32_t COMP = 0u>        /* COMP: the HAR_SCENE_BLEND / HAR_SCENE_MASK / HAR_SCENE_ATTR / HAR_SCENE_NORMALMAP / HAR_SCENE_BUMPMAP bits of the records the scene may hold (the kernels of other scenes compile those branches out) */
HAR_HD Vec3 aov_albedo(const DScene &S, const SurfInt &si, const AttrAddr *aa = nullptr) {
    constexpr bool BLEND = (COMP & HAR_SCENE_BLEND) != 0u;
    BsdfSide side;
    if (!bsdf_side(S, S.meshes[si.mesh].bsdf, si.wi, side)) return Vec3(0.f);
    if ((COMP & HAR_SCENE_MASK) != 0u && S.bsdfs[side.index].type == BSDF_MASK) {
        /* MaskBSDF::eval_diffuse_reflectance (mask.cpp:229-232): the nested BSDF's own answer -- through its `twosided`, if it has one (twosided.cpp:243-259) */
        const uint32_t nested = S.bsdfs[side.index].pad;
        if (!bsdf_side(S, nested, si.wi, side)) return Vec3(0.f);
    }
    if ((COMP & HAR_SCENE_NORMALMAP) != 0u && S.bsdfs[side.index].type == BSDF_NORMALMAP) {
        /* NormalMap::eval_diffuse_reflectance (normalmap.cpp:250-253): the nested BSDF's answer for the UNPERTURBED si (the side an outer `twosided` mirrored) */
        const uint32_t nested = S.bsdfs[side.index].pad;
        if (!bsdf_side(S, nested, side.wi, side)) return Vec3(0.f);
    }
    if ((COMP & HAR_SCENE_BUMPMAP) != 0u && S.bsdfs[side.index].type == BSDF_BUMPMAP) {
        /* BumpMap::eval_diffuse_reflectance (bumpmap.cpp:259-262): the nested BSDF's answer for the UNPERTURBED si */
        const uint32_t nested = S.bsdfs[side.index].pad;
        if (!bsdf_side(S, nested, side.wi, side)) return Vec3(0.f);
    }
    const DBsdf &B = S.bsdfs[side.index];
    TexTaps taps;
    const BsdfInputs in = bsdf_inputs(S, B, si.uv_x, si.uv_y, taps, aa);
    if (BLEND && B.type == BSDF_BLEND) {       /* BlendBSDF::eval_diffuse_reflectance (blendbsdf.cpp:228-233): rho_0 * (1 - w) + rho_1 * w of the nested BSDFs' own answers */
        bool inside; const float w = blend_weight(B, in, inside);
        const uint32_t child[2] = { (uint32_t) B.table, B.pad };
        Vec3 rho[2];
        for (int k = 0; k < 2; ++k) {
            const DBsdf &N = S.bsdfs[child[k]];
            TexTaps nt; const BsdfInputs nin = bsdf_inputs(S, N, si.uv_x, si.uv_y, nt, aa);
            if (N.type == BSDF_DIFFUSE || N.type == BSDF_ROUGHPLASTIC || N.type == BSDF_PLASTIC) rho[k] = nin.slot0;
            else { BsdfEval ne; bsdf_eval_pdf_one<HAR_BSDF_ALL_TYPES, false>(N, nin, side.wi, Vec3(0.f, 0.f, 1.f), ne); rho[k] = ne.value * HAR_PI; }
        }
        return rho[0] * (1.f - w) + rho[1] * w;
    }
    if (B.type == BSDF_DIFFUSE || B.type == BSDF_ROUGHPLASTIC || B.type == BSDF_PLASTIC) return in.slot0;
    BsdfEval e;
    bsdf_eval_pdf_one<HAR_BSDF_ALL_TYPES, false>(B, in, side.wi, Vec3(0.f, 0.f, 1.f), e);
    return e.value * HAR_PI;
}

/* Writes the channels of `spec` for one lane: channel c goes to out[c * stride].  `hit` is the closest intersection of the ray (o is not needed:
 * si.p comes from the triangle), `top_meshes` = number of top-level meshes of the scene.
 * shape_index (aov.cpp:288-297, the scalar branch): the 1-based position of the hit instance -- or, without one, of the hit shape -- in the
 * scene's shape list, which here is { top-level meshes, instances }; 0 on a miss. */
/* BSDF::sh_frame(si).n (aov.cpp:245-256) of a hit in a scene with a `normalmap` record: frame().second.n = si.to_world(frame.n) (normalmap.cpp:224-248), the flip
 * decided by the camera ray's wi.  Every other record returns si.sh_frame (bsdf.h:602-604) -- and so does a `twosided` OVER a normalmap, which does not forward
 * sh_frame() to its nested BSDF (twosided.cpp has no override) */
HAR_HD Vec3 aov_sh_normal_nmap(const DScene &S, const SurfInt &si) {
    const DBsdf &B = S.bsdfs[S.meshes[si.mesh].bsdf];
    if (B.type != BSDF_NORMALMAP || (B.flags & BF_TWOSIDED)) return si.sn;
    TexTaps taps;
    const BsdfInputs in = bsdf_inputs(S, B, si.uv_x, si.uv_y, taps);
    const NormalFrame F = normalmap_frame(B, in.slot0, si.wi);
    return si.to_world(F.n);
}

/* ... and in a scene with a `bumpmap` record: BumpMap::sh_frame = frame(si) (bumpmap.cpp:255-257), n = si.to_world(frame.n); plain si.sh_frame under an outer
 * `twosided`, as above.  P = the hit's position partials */
HAR_HD Vec3 aov_sh_normal_bump(const DScene &S, const SurfInt &si, const SurfPartials &P) {
    const DBsdf &B = S.bsdfs[S.meshes[si.mesh].bsdf];
    if (B.type != BSDF_BUMPMAP) return aov_sh_normal_nmap(S, si);
    if (B.flags & BF_TWOSIDED) return si.sn;
    const BumpGeom G = bump_geom(S, B, si.n, si.sn, si.ss, si.st, P.dp_du, P.dp_dv, si.uv_x, si.uv_y);
    const NormalFrame F = bumpmap_frame(B, G, si.wi);
    return si.to_world(F.n);
}

template <uint32_t COMP = 0u>
HAR_HD void aov_lane(const DScene &S, const AovSpec &spec, uint32_t top_meshes, Vec3 ray_d, const Hit &hit, bool active, float *out, size_t stride) {
    const bool valid = active && hit.t != HAR_INF;
    SurfInt si; SurfPartials P;
    bool need_partials = false, need_albedo = false;
    for (uint32_t k = 0; k < spec.n; ++k) { need_partials |= spec.type[k] == AOV_DP_DU || spec.type[k] == AOV_DP_DV; need_albedo |= spec.type[k] == AOV_ALBEDO; }
    Vec3 albedo(0.f);
    if (valid) {
        si = compute_si(S, ray_d, hit.t, hit.u, hit.v, hit.prim, hit.shape, hit.inst);
        if ((COMP & HAR_SCENE_NORMALMAP) != 0u) si_tangent_frame(S, si, ray_d, hit.u, hit.v, hit.prim, hit.shape, hit.inst);
        if (need_partials || (COMP & HAR_SCENE_BUMPMAP) != 0u) compute_si_partials(S, hit.u, hit.v, hit.prim, hit.shape, hit.inst, false, P);
        if (need_albedo && (COMP & HAR_SCENE_ATTR) != 0u) {       /* scenes with a `mesh_attribute` texture: the albedo is looked up at the face and the barycentrics of si.p */
            AttrAddr addr; addr.face = 0u; addr.b1 = 0.f; addr.b2 = 0.f;
            if (hit.inst == 0xffffffffu) addr = attr_addr(S, si.p, hit.prim, hit.shape);
            albedo = aov_albedo<COMP>(S, si, &addr);
        } else if (need_albedo) albedo = aov_albedo<COMP>(S, si);
    }
    size_t c = 0;
    for (uint32_t k = 0; k < spec.n; ++k) {
        Vec3 v(0.f);
        const uint32_t type = spec.type[k];
        if (valid) {
            switch (type) {
                case AOV_ALBEDO: v = albedo; break;
                case AOV_DEPTH: v.x = si.t; break;
                case AOV_POSITION: v = si.p; break;
                case AOV_UV: v.x = si.uv_x; v.y = si.uv_y; break;
                case AOV_GEO_NORMAL: v = si.n; break;
                case AOV_SH_NORMAL: v = (COMP & HAR_SCENE_BUMPMAP) != 0u ? aov_sh_normal_bump(S, si, P) : (COMP & HAR_SCENE_NORMALMAP) != 0u ? aov_sh_normal_nmap(S, si) : si.sn; break;          /* BSDF::sh_frame(si): si.sh_frame unless a `normalmap` perturbs it */
                case AOV_DP_DU: v = P.dp_du; break;
                case AOV_DP_DV: v = P.dp_dv; break;
                case AOV_PRIM_INDEX: v.x = (float) hit.prim; break;
                default: v.x = (float) (hit.inst != 0xffffffffu ? top_meshes + hit.inst + 1u : hit.shape + 1u); break;
            }
        }
        const uint32_t nc = aov_type_channels(type);
        out[c * stride] = v.x; ++c;
        if (nc > 1) { out[c * stride] = v.y; ++c; }
        if (nc > 2) { out[c * stride] = v.z; ++c; }
    }
}

} // namespace har
