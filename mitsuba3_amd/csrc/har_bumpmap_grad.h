/*
 * har_bumpmap_grad.h -- the derivative of a `bumpmap` record's value with respect to the (scaled) uv-gradient of its height map (HAR_HD: the adjoint shading
 * kernel of bump scenes, shade_lane in har_path.h, and the host entry har_bumpmap_grad_host run it).
 *
 * prb re-evaluates bsdf.eval(ctx, si, wo) attached (prb.py), and BumpMap::traverse registers the height texture as differentiable (bumpmap.cpp:131-135).  The value
 * depends on the texels only through grad_uv = scale * eval_1_grad, two numbers that are LINEAR in the texels (har_scene.h, tex_eval_1_grad): for the scalar
 * F = sum_c A_c value_c of one term this header gives dF / d grad_uv, and the in-place commit pushes it through the transpose of eval_1_grad into the texels.
 * Hand-derived reverse sweep over frame() (bumpmap.cpp:224-253) and eval() (:164-183), from the value back to grad_uv:
 *   the nested model's six directional partials (bsdf_weighted_value_dir) at wi' = to_local(wi), wo' = to_local(wo);  the shadow term, whose min(., 1) takes the branch
 *   the value takes;  t = cross(n, s);  s = normalize(dp_du - n dot(n, dp_du));  the second flip (-x, -y, z);  n = si.to_local(n);  the geometric flip;
 *   n = normalize(cross(dp_du', dp_dv'));  dp_du' = fmadd(sh_n, grad_uv.x - dot(sh_n, dp_du), dp_du), likewise dp_dv'.
 * The selects (both flips, the orientation test) carry no derivative.  Delta models nested in a bump map evaluate to zero and give a zero gradient.
 */
#pragma once
#include "har_scene.h"
#include "har_bsdf_dir.h"

namespace har {

/* F = sum_c A_c value_c(wi, wo) of bumpmap record B at the scaled height gradient (gx, gy), and dg[0] = dF / d gx, dg[1] = dF / d gy.  wi, wo: local directions of the
 * vertex as the record sees them (an outer `twosided` has folded them already: the fold does not depend on the texels).  (u, v): the vertex's texture coordinates,
 * for the nested record's own colours. */
template <uint32_t TYPES = 0u>          /* (only the HAR_SCENE_ALPHAMAP bit is read: the nested record may carry a roughness map) */
HAR_HD float bumpmap_weighted_value_grad(const DScene &S, const DBsdf &B, const BumpGeom &G, float gx, float gy, Vec3 wi, Vec3 wo, float u, float v, Vec3 A, float dg[2]) {
    dg[0] = dg[1] = 0.f;
    /* forward, as bumpmap_frame_grad (har_scene.h) */
    const Vec3 dpu = fma3(G.sn, gx - dot3(G.sn, G.dp_du), G.dp_du), dpv = fma3(G.sn, gy - dot3(G.sn, G.dp_dv), G.dp_dv);
    const Vec3 c = cross3(dpu, dpv);
    const float inv_lc = rsqrt_(dot3(c, c));
    Vec3 nw = c * inv_lc;
    const bool geo_flip = dot3(G.n, nw) < 0.f;
    if (geo_flip) nw = -nw;
    Vec3 n(dot3(nw, G.ss), dot3(nw, G.st), dot3(nw, G.sn));
    const bool flip = (B.flags & BF_NM_FLIP) && wi.z * dot3(wi, n) <= 0.f;
    if (flip) n = Vec3(-n.x, -n.y, n.z);
    const float q = dot3(n, G.dp_du);
    const Vec3 a = fma3(n, -q, G.dp_du);
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
    /* the shadow term 2 / (1 + sqrt(1 + alpha2 tan^2(wo))), alpha2 = min(tan^2(n) / 8, 1): it depends on the height map through n.z alone */
    float sh = 1.f, dsh_dnz = 0.f;
    if (B.flags & BF_NM_SHADOW) {
        const float tn = frame_tan_theta_2(n), two = frame_tan_theta_2(wo), raw = 0.125f * tn, alpha2 = fminf(raw, 1.f);
        const float r = sqrtf(1.f + alpha2 * two);
        sh = 2.f / (1.f + r);
        if (raw < 1.f && fnma_(n.z, n.z, 1.f) > 0.f && r > 0.f) {
            const float dtn_dnz = -2.f / (n.z * n.z * n.z);                                       /* d / dz (1 - z^2) / z^2 */
            dsh_dnz = -2.f / ((1.f + r) * (1.f + r)) * (0.5f / r) * two * 0.125f * dtn_dnz;
        }
    }
    /* reverse sweep: F = sh * fn(wi'(s, t, n), wo'(s, t, n)) */
    Vec3 gs = (wi * g[0] + wo * g[3]) * sh, gt = (wi * g[1] + wo * g[4]) * sh, gn = (wi * g[2] + wo * g[5]) * sh;
    gn.z += fn * dsh_dnz;
    gn = gn + cross3(s, gt); gs = gs + cross3(gt, n);                                             /* t = cross(n, s) */
    const Vec3 ga = (gs - s * dot3(s, gs)) * inv_la;                                              /* s = a / |a| */
    gn = gn - ga * q + G.dp_du * (-dot3(ga, n));                                                  /* a = dp_du - n q, q = dot(n, dp_du) (the literal line :249) */
    if (flip) gn = Vec3(-gn.x, -gn.y, gn.z);                                                      /* the second flip */
    Vec3 gw = fma3(G.sn, gn.z, fma3(G.st, gn.y, G.ss * gn.x));                                    /* n = si.to_local(n_world) */
    if (geo_flip) gw = -gw;                                                                       /* the geometric flip */
    const Vec3 n0 = c * inv_lc;
    const Vec3 gc = (gw - n0 * (dot3(n0, gw) / dot3(n0, n0))) * inv_lc;                           /* n_world = c / |c| */
    const Vec3 gdpu = cross3(dpv, gc), gdpv = cross3(gc, dpu);                                    /* c = cross(dp_du', dp_dv') */
    dg[0] = dot3(G.sn, gdpu); dg[1] = dot3(G.sn, gdpv);                                           /* dp_du' = sh_n (gx - ...) + dp_du */
    return sh * fn;
}

} // namespace har
