/*
 * har_normalmap_grad.h -- the derivative of a `normalmap` record's value with respect to the looked-up normal-map colour (HAR_HD: the adjoint
 * shading kernel of normalmap scenes, shade_lane in har_path.h, and the host entry har_normalmap_grad_host run it).
 *
 * prb re-evaluates bsdf.eval(ctx, si, wo) attached (prb.py), and NormalMap::traverse registers the map as differentiable (normalmap.cpp:131): for the scalar
 * F = sum_c A_c value_c of one term the adjoint with respect to the colour c is the chain through
 *   n_raw = 2 c - 1;  the flip (the branch taken; no derivative of the select);  n = normalize(n_raw);  s = normalize((1, 0, 0) - n n.x);  t = cross(n, s);
 *   wi' = to_local(wi), wo' = to_local(wo);  the nested value's six directional partials (har_bsdf_dir.h);  the shadow term, whose min(., 1) takes the branch the value
 *   takes.  The orientation test carries no derivative.
 * Hand-derived reverse sweep over that chain: the nested model contributes dF / d wi', dF / d wo' (bsdf_weighted_value_dir), everything in front of it is a handful of
 * vector products.  value depends on c only through normalize(2 c - 1), so sum_k dF/dc_k (c_k - 0.5) = 0: the sweep ends in the projection (g - n (n . g)) / |n_raw|,
 * which has that property by construction.  Delta models nested in a normal map evaluate to zero and give a zero gradient.
 */
#pragma once
#include "har_scene.h"
#include "har_bsdf_dir.h"

namespace har {

/* F = sum_c A_c value_c(wi, wo) of normalmap record B for the looked-up colour c, and dc[k] = dF / d c_k.  wi, wo: local directions of the vertex as the record sees
 * them (an outer `twosided` has folded them already: the fold does not depend on c).  (u, v): the vertex's texture coordinates, for the nested record's own colours. */
template <uint32_t TYPES = 0u>          /* (only the HAR_SCENE_ALPHAMAP bit is read: the nested record may carry a roughness map) */
HAR_HD float normalmap_weighted_value_grad(const DScene &S, const DBsdf &B, Vec3 c, Vec3 wi, Vec3 wo, float u, float v, Vec3 A, float dc[3]) {
    dc[0] = dc[1] = dc[2] = 0.f;
    /* forward, as normalmap_frame (har_scene.h) */
    Vec3 r(fma_(c.x, 2.f, -1.f), fma_(c.y, 2.f, -1.f), fma_(c.z, 2.f, -1.f));
    const bool flip = (B.flags & BF_NM_FLIP) && wi.z * dot3(wi, r) <= 0.f;
    if (flip) r = Vec3(-r.x, -r.y, r.z);
    const float inv_l = rsqrt_(dot3(r, r));
    const Vec3 n = r * inv_l;
    const Vec3 a(fnma_(n.x, n.x, 1.f), fnma_(n.y, n.x, 0.f), fnma_(n.z, n.x, 0.f));
    const float inv_la = rsqrt_(dot3(a, a));
    const Vec3 s = a * inv_la, t = cross3(n, s);
    const Vec3 pwi(dot3(wi, s), dot3(wi, t), dot3(wi, n)), pwo(dot3(wo, s), dot3(wo, t), dot3(wo, n));
    if (!(wo.z * pwo.z > 0.f)) return 0.f;
    BsdfSide ns;
    if (!bsdf_side(S, B.pad, pwi, ns)) return 0.f;
    const DBsdf &N = S.bsdfs[ns.index];
    TexTaps taps; const BsdfInputs nin = bsdf_inputs<TYPES>(S, N, u, v, taps);
    float g[6];
    const float fn = bsdf_weighted_value_dir<TYPES>(N, nin, ns.wi, Vec3(pwo.x, pwo.y, pwo.z * ns.wo_sign), A, g);
    g[2] *= ns.wo_sign; g[5] *= ns.wo_sign;          /* a nested `twosided` mirrored wi'.z and wo'.z by the same sign */
    /* the shadow term 2 / (1 + sqrt(1 + alpha2 tan^2(wo))), alpha2 = min(tan^2(n) / 8, 1), tan^2(v) = max(1 - v.z^2, 0) / v.z^2: it depends on c through n.z alone */
    float sh = 1.f, dsh_dnz = 0.f;
    if (B.flags & BF_NM_SHADOW) {
        const float tn = frame_tan_theta_2(n), two = frame_tan_theta_2(wo), raw = 0.125f * tn, alpha2 = fminf(raw, 1.f);
        const float q = sqrtf(1.f + alpha2 * two);
        sh = 2.f / (1.f + q);
        if (raw < 1.f && fnma_(n.z, n.z, 1.f) > 0.f && q > 0.f) {
            const float dtn_dnz = -2.f / (n.z * n.z * n.z);                                   /* d / dz (1 - z^2) / z^2 */
            dsh_dnz = -2.f / ((1.f + q) * (1.f + q)) * (0.5f / q) * two * 0.125f * dtn_dnz;
        }
    }
    /* reverse sweep: F = sh * fn(wi'(s, t, n), wo'(s, t, n)) */
    Vec3 gs = (wi * g[0] + wo * g[3]) * sh, gt = (wi * g[1] + wo * g[4]) * sh, gn = (wi * g[2] + wo * g[5]) * sh;
    gn.z += fn * dsh_dnz;
    gn = gn + cross3(s, gt); gs = gs + cross3(gt, n);                                             /* t = cross(n, s) */
    const Vec3 ga = (gs - s * dot3(s, gs)) * inv_la;                                              /* s = a / |a| */
    gn = gn - ga * n.x; gn.x -= dot3(ga, n);                                                      /* a = (1, 0, 0) - n n.x */
    Vec3 gr = (gn - n * (dot3(n, gn) / dot3(n, n))) * inv_l;                                      /* n = r / |r| (|n|^2 as computed: the projection is exact for THIS n) */
    if (flip) gr = Vec3(-gr.x, -gr.y, gr.z);
    dc[0] = 2.f * gr.x; dc[1] = 2.f * gr.y; dc[2] = 2.f * gr.z;                                   /* r = 2 c - 1 */
    return sh * fn;
}

} // namespace har
