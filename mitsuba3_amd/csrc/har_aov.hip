/*
 * har_aov.hip -- gfx950 kernels of the `aov` integrator (src/integrators/aov.cpp): per-pixel depth, position, normals, albedo, uv, partials and ids.
 *
 *   k_aov_trace -> k_aov_fill -> k_splat_channels
 *
 * The pass is self-contained: the camera rays are regenerated per lane (raygen_lane: the sampler stream and film position of har_render's lane) and
 * traced with the per-lane traversal of the array-valued ray queries (k_api_intersect: Traversal<>::step over an LDS stack), so this translation
 * unit shares no kernel and no workspace with the path tracer.  All AOV logic is aov_lane() of har_aov.h (shared with the host twin); the kernels
 * only move data.  64-lane waves, 256-thread blocks.
 */
#include "har_aov_launch.h"
#include "har_kernels.h"

namespace har {

static constexpr int kBlock = 256;
#define HAR_SPLAT_TILE_PIXELS_AOV 512          /* LDS tile of the gather (float4 per pixel: 8 KB), as k_splat's */
#define HAR_SPLAT_GATHER_MAX_SPLIT_AOV 8
static inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

template <int CAP> struct AovStack {
    static constexpr int Capacity = CAP;
    static constexpr bool kSelectRefill = true;
    uint2 *col;   /* &lds[threadIdx.x]; entry l lives at col[l * kBlock] */
    __device__ __forceinline__ void push(int l, uint32_t x, uint32_t y) { col[l * kBlock] = make_uint2(x, y); }
    __device__ __forceinline__ void pop(int l, uint32_t &x, uint32_t &y) { uint2 v = col[l * kBlock]; x = v.x; y = v.y; }
};

/* closest hit of one ray per lane; LANES: the ray is the camera ray of lane lane_base + i, otherwise ray i of the SoA arrays (masked lanes trace nothing) */
template <int CAP, bool LANES>
__global__ __launch_bounds__(kBlock) void k_aov_trace(DScene S, DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                                                      const float *o, const float *d, const float *maxt, const uint8_t *active, float4 *h0, uint2 *h1, int *status) {
    __shared__ uint2 lds[CAP * kBlock];
    AovStack<CAP> stack{ lds + threadIdx.x };
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Vec3 O, D; float tmax; bool act = true;
    if (LANES) { LaneSample ls; const PathState st = raygen_lane(C, seed, spp, log_spp, lane_base + i, ls); O = st.o; D = st.d; tmax = st.maxt; }
    else { O = Vec3(o[i], o[n + i], o[2 * (size_t) n + i]); D = Vec3(d[i], d[n + i], d[2 * (size_t) n + i]); tmax = maxt[i]; act = !(active && !active[i]); }
    Hit hit; hit.t = HAR_INF; hit.u = 0.f; hit.v = 0.f; hit.prim = 0; hit.shape = 0; hit.inst = 0xffffffffu;
    int st = 0;
    if (act) {
        Traversal<HAR_TRAV_POLICY> T; T.begin(S.accel, O, D, tmax, (S.accel.top_last & 2u) != 0u);
        while (!T.template step<false, AovStack<CAP>, NoProbe, 1>(S.accel, stack, st)) { }
        hit = T.hit;
    }
    if (st) atomicMax(status, st);
    h0[i] = make_float4(hit.t, hit.u, hit.v, __uint_as_float(hit.prim));
    h1[i] = make_uint2(hit.shape, hit.inst);
}

/* camera rays of the lanes of a BATCH sensor's render (k_raygen_batch's rays) or of a render through a thin lens (k_raygen_lens's; batch.n == 0: C is the lens), SoA with
 * stride n: the AOV pass of such a sensor then runs the _rays flavours of the kernels below on them, which keeps the single-sensor flavours as they are */
__global__ __launch_bounds__(kBlock) void k_aov_batch_rays(DSensor C, DBatch batch, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                                                           float *o, float *d, float *maxt) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    LaneSample ls; PathState st;
    if (batch.n) st = raygen_lane<true>(C, seed, spp, log_spp, lane_base + i, ls, nullptr, nullptr, &batch);
    else st = raygen_lane<true>(C, seed, spp, log_spp, lane_base + i, ls);
    o[i] = st.o.x; o[n + i] = st.o.y; o[2 * (size_t) n + i] = st.o.z; d[i] = st.d.x; d[n + i] = st.d.y; d[2 * (size_t) n + i] = st.d.z; maxt[i] = st.maxt;
}

/* AOVIntegratorImpl::sample per lane: the channels of `spec`, channel-major (aov[c * stride + i]) so that these stores and the splat's loads coalesce */
template <bool LANES, bool BLEND = false>
__global__ __launch_bounds__(kBlock) void k_aov_fill(DScene S, AovSpec spec, uint32_t top_meshes, DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base,
                                                     uint32_t n, const float *d, const uint8_t *active, const float4 *h0, const uint2 *h1, float *aov, size_t stride) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Vec3 D; bool act = true;
    if (LANES) { LaneSample ls; D = raygen_lane(C, seed, spp, log_spp, lane_base + i, ls).d; }
    else { D = Vec3(d[i], d[n + i], d[2 * (size_t) n + i]); act = !(active && !active[i]); }
    const float4 a = h0[i]; const uint2 b = h1[i];
    Hit hit; hit.t = a.x; hit.u = a.y; hit.v = a.z; hit.prim = __float_as_uint(a.w); hit.shape = b.x; hit.inst = b.y;
    aov_lane<(BLEND ? HAR_SCENE_BLEND : 0u)>(S, spec, top_meshes, D, hit, act, aov + i, stride);
}
/* ... of a scene that holds a `mask` record (blend and mask records resolved); a kernel of its own, so that the ones above keep their code and names */
template <bool LANES>
__global__ __launch_bounds__(kBlock) void k_aov_fill_mask(DScene S, AovSpec spec, uint32_t top_meshes, DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base,
                                                          uint32_t n, const float *d, const uint8_t *active, const float4 *h0, const uint2 *h1, float *aov, size_t stride) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Vec3 D; bool act = true;
    if (LANES) { LaneSample ls; D = raygen_lane(C, seed, spp, log_spp, lane_base + i, ls).d; }
    else { D = Vec3(d[i], d[n + i], d[2 * (size_t) n + i]); act = !(active && !active[i]); }
    const float4 a = h0[i]; const uint2 b = h1[i];
    Hit hit; hit.t = a.x; hit.u = a.y; hit.v = a.z; hit.prim = __float_as_uint(a.w); hit.shape = b.x; hit.inst = b.y;
    aov_lane<HAR_SCENE_COMPOSITE>(S, spec, top_meshes, D, hit, act, aov + i, stride);
}

/* ... of a scene that holds a `mesh_attribute` texture: the albedo is looked up at the face and the barycentrics of si.p (aov_lane); a kernel of its own again */
template <bool LANES>
__global__ __launch_bounds__(kBlock) void k_aov_fill_attr(DScene S, AovSpec spec, uint32_t top_meshes, DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base,
                                                          uint32_t n, const float *d, const uint8_t *active, const float4 *h0, const uint2 *h1, float *aov, size_t stride) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Vec3 D; bool act = true;
    if (LANES) { LaneSample ls; D = raygen_lane(C, seed, spp, log_spp, lane_base + i, ls).d; }
    else { D = Vec3(d[i], d[n + i], d[2 * (size_t) n + i]); act = !(active && !active[i]); }
    const float4 a = h0[i]; const uint2 b = h1[i];
    Hit hit; hit.t = a.x; hit.u = a.y; hit.v = a.z; hit.prim = __float_as_uint(a.w); hit.shape = b.x; hit.inst = b.y;
    aov_lane<HAR_SCENE_WIDEST>(S, spec, top_meshes, D, hit, act, aov + i, stride);
}

/* ... of a scene that holds a `normalmap` record: the tangent frame of the shapes that pack one, the perturbed shading normal, the nested albedo; a kernel of its own again */
template <bool LANES>
__global__ __launch_bounds__(kBlock) void k_aov_fill_nmap(DScene S, AovSpec spec, uint32_t top_meshes, DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base,
                                                          uint32_t n, const float *d, const uint8_t *active, const float4 *h0, const uint2 *h1, float *aov, size_t stride) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Vec3 D; bool act = true;
    if (LANES) { LaneSample ls; D = raygen_lane(C, seed, spp, log_spp, lane_base + i, ls).d; }
    else { D = Vec3(d[i], d[n + i], d[2 * (size_t) n + i]); act = !(active && !active[i]); }
    const float4 a = h0[i]; const uint2 b = h1[i];
    Hit hit; hit.t = a.x; hit.u = a.y; hit.v = a.z; hit.prim = __float_as_uint(a.w); hit.shape = b.x; hit.inst = b.y;
    aov_lane<HAR_SCENE_NMAP_RECORD_BITS>(S, spec, top_meshes, D, hit, act, aov + i, stride);
}

/* ... of a scene that holds a `bumpmap` record: the bump frame's shading normal (it reads the hit's position partials) and the nested albedo; a kernel of its own again */
template <bool LANES>
__global__ __launch_bounds__(kBlock) void k_aov_fill_bump(DScene S, AovSpec spec, uint32_t top_meshes, DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base,
                                                          uint32_t n, const float *d, const uint8_t *active, const float4 *h0, const uint2 *h1, float *aov, size_t stride) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Vec3 D; bool act = true;
    if (LANES) { LaneSample ls; D = raygen_lane(C, seed, spp, log_spp, lane_base + i, ls).d; }
    else { D = Vec3(d[i], d[n + i], d[2 * (size_t) n + i]); act = !(active && !active[i]); }
    const float4 a = h0[i]; const uint2 b = h1[i];
    Hit hit; hit.t = a.x; hit.u = a.y; hit.v = a.z; hit.prim = __float_as_uint(a.w); hit.shape = b.x; hit.inst = b.y;
    aov_lane<HAR_SCENE_RECORD_BITS>(S, spec, top_meshes, D, hit, act, aov + i, stride);
}

/* ImageBlock::put (coalesced JIT branch, imageblock.cpp:444-520) of `channels` values + the weight per lane: the LDS gather of k_splat (har_kernels.hip) for an
 * arbitrary channel count.  The lanes' film positions, separable filter weights and the block's footprint are computed and staged in LDS ONCE; the channels then go
 * through the value array and the tile in groups of four (float4), channel `channels` being the weight (value 1), the slots behind it zero.  Blocks whose lanes span
 * two image rows and lanes with a shifted footprint (see k_splat) scatter their taps themselves. */
template <int TAPS>
__global__ __launch_bounds__(kBlock) void k_splat_channels(DSensor C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                                                           const float *aov, size_t stride, uint32_t channels, float *film) {
    __shared__ float tile[4 * HAR_SPLAT_TILE_PIXELS_AOV];
    __shared__ float4 s_val[kBlock];
    __shared__ float s_wx[TAPS][kBlock + 1], s_wy[TAPS][kBlock + 1];
    __shared__ int ext[6];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool act = i < n;
    const uint32_t n_act_u = min((uint32_t) kBlock, n - blockIdx.x * kBlock);
    const uint32_t fstride = channels + 1u;
    Footprint F; F.count = 0; F.x0 = 0; F.y0 = 0;
    for (int k = 0; k < HAR_MAX_FILTER_TAPS; ++k) { F.wx[k] = 0.f; F.wy[k] = 0.f; }
    bool shifted = false;
    if (act) {
        const LaneSample ls = lane_film_pos(C, seed, spp, log_spp, lane_base + i);
        film_footprint(C, ls, F);
        const uint32_t nh = (F.count - 1u) / 2u;
        const uint32_t px0 = (uint32_t) ((int32_t) ls.ipos_x - (int32_t) nh - (int32_t) C.crop_x), py0 = (uint32_t) ((int32_t) ls.ipos_y - (int32_t) nh - (int32_t) C.crop_y);
        shifted = F.x0 != px0 || F.y0 != py0;
        if (threadIdx.x == 0) { ext[0] = (int) px0; ext[1] = (int) py0; ext[4] = (int) F.count; }
        if (threadIdx.x == n_act_u - 1u) { ext[2] = (int) px0; ext[3] = (int) py0; }
    }
    const bool gathered = act && !shifted;
#pragma unroll
    for (int k = 0; k < TAPS; ++k) { s_wx[k][threadIdx.x] = gathered ? F.wx[k] : 0.f; s_wy[k][threadIdx.x] = gathered ? F.wy[k] : 0.f; }
    __syncthreads();
    const int ox = ext[0], oy = ext[1], tw = ext[2] + ext[4] - ext[0], th = ext[4];
    const bool one_row = tw > 0 && ext[1] == ext[3] && th <= TAPS;
    if (one_row) {
        const int count = th, nhalf = (count - 1) / 2, y_pix = oy + nhalf;
        const int64_t g0 = (int64_t) lane_base + (int64_t) blockIdx.x * kBlock;
        const int n_act = (int) n_act_u;
        const int slab_w = HAR_SPLAT_TILE_PIXELS_AOV / th;
        for (uint32_t cg = 0; cg < fstride; cg += 4u) {
            /* the group's four values of every lane; the previous group's readers are past the barrier that ends its last slab */
            float v4[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t c = cg + k;
                v4[k] = !gathered ? 0.f : c < channels ? aov[(size_t) c * stride + i] : c == channels ? 1.f : 0.f;
            }
            s_val[threadIdx.x] = make_float4(v4[0], v4[1], v4[2], v4[3]);
            __syncthreads();
            for (int c0 = 0; c0 < tw; c0 += slab_w) {
                const int sw = min(slab_w, tw - c0), E = sw * th;
                int G = 1; while (G < HAR_SPLAT_GATHER_MAX_SPLIT_AOV && E * G * 2 <= kBlock) G *= 2;
                for (int idx = threadIdx.x; idx < E * G; idx += kBlock) {
                    const int e = idx % E, g = idx / E, tx = e % sw, ty = e / sw, col = ox + c0 + tx;
                    float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
                    const int x_first = ox + nhalf, x_last = ext[2] + nhalf;
                    const int t_lo = max(0, col + nhalf - x_last), t_hi = min(count - 1, col + nhalf - x_first);
                    for (int t = t_lo; t <= t_hi; ++t) {
                        const int x = col - t + nhalf;
                        if (x < -(int) C.border || x >= (int) (C.crop_w + C.border)) continue;
                        const int64_t first = ((int64_t) (y_pix + (int) C.border) * C.samp_w + (x + (int) C.border)) * spp - g0;
                        int la = (int) max((int64_t) 0, first), lb = (int) min((int64_t) n_act, first + spp);
                        if (la >= lb) continue;
                        const int len = lb - la; lb = la + (len * (g + 1)) / G; la = la + (len * g) / G;
                        const float *wxp = s_wx[t], *wyp = s_wy[ty];
#pragma unroll 4
                        for (int l = la; l < lb; ++l) {
                            const float w = wxp[l] * wyp[l];
                            const float4 v = s_val[l]; ax += v.x * w; ay += v.y * w; az += v.z * w; aw += v.w * w;
                        }
                    }
                    reinterpret_cast<float4 *>(tile)[idx] = make_float4(ax, ay, az, aw);
                }
                __syncthreads();
                for (int k = threadIdx.x; k < E * 4; k += kBlock) {
                    float v = tile[k];
                    for (int g = 1; g < G; ++g) v += tile[k + 4 * E * g];
                    const int px = k >> 2, x = ox + c0 + px % sw, y = oy + px / sw;
                    const uint32_t c = cg + (uint32_t) (k & 3);
                    if (v != 0.f && c < fstride && (uint32_t) x < C.crop_w && (uint32_t) y < C.crop_h)
                        atomicAdd(film + (size_t) fstride * ((size_t) y * C.crop_w + x) + c, v);
                }
                __syncthreads();
            }
        }
    }
    if (act && (!one_row || shifted)) {
        for (uint32_t c = 0; c < fstride; ++c) {
            const float val = c < channels ? aov[(size_t) c * stride + i] : 1.f;
            if (val == 0.f) continue;
#pragma unroll
            for (int ys = 0; ys < TAPS; ++ys)
#pragma unroll
                for (int xs = 0; xs < TAPS; ++xs) {
                    const uint32_t x = F.x0 + (uint32_t) xs, y = F.y0 + (uint32_t) ys;
                    if ((uint32_t) xs < F.count && (uint32_t) ys < F.count && x < C.crop_w && y < C.crop_h)
                        atomicAdd(film + (size_t) fstride * ((size_t) y * C.crop_w + x) + c, val * (F.wx[xs] * F.wy[ys]));
                }
        }
    }
}

void launch_aov_trace_lanes(hipStream_t s, const DScene &S, bool deep, const DSensor &C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                            float4 *h0, uint2 *h1, int *status) {
    if (deep) hipLaunchKernelGGL((k_aov_trace<HAR_LDS_STACK_DEPTH, true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, nullptr, nullptr, h0, h1, status);
    else hipLaunchKernelGGL((k_aov_trace<HAR_LDS_STACK_SMALL, true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, nullptr, nullptr, h0, h1, status);
}
void launch_aov_batch_rays(hipStream_t s, const DSensor &C, const DBatch &batch, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                           float *o, float *d, float *maxt) {
    hipLaunchKernelGGL(k_aov_batch_rays, dim3(blocks_for(n)), dim3(kBlock), 0, s, C, batch, seed, spp, log_spp, lane_base, n, o, d, maxt);
}
void launch_aov_trace_rays(hipStream_t s, const DScene &S, bool deep, uint32_t n, const float *o, const float *d, const float *maxt, const uint8_t *active,
                           float4 *h0, uint2 *h1, int *status) {
    const DSensor C{};
    if (deep) hipLaunchKernelGGL((k_aov_trace<HAR_LDS_STACK_DEPTH, false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, C, 0u, 1u, 0u, 0u, n, o, d, maxt, active, h0, h1, status);
    else hipLaunchKernelGGL((k_aov_trace<HAR_LDS_STACK_SMALL, false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, C, 0u, 1u, 0u, 0u, n, o, d, maxt, active, h0, h1, status);
}
void launch_aov_fill_lanes(hipStream_t s, const DScene &S, const AovSpec &spec, uint32_t top_meshes, const DSensor &C, uint32_t seed, uint32_t spp, uint32_t log_spp,
                           uint32_t lane_base, uint32_t n, const float4 *h0, const uint2 *h1, float *aov, size_t stride) {
    if (S.bsdf_types & HAR_SCENE_BUMPMAP) { hipLaunchKernelGGL((k_aov_fill_bump<true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, h0, h1, aov, stride); return; }
    if (S.bsdf_types & HAR_SCENE_NORMALMAP) { hipLaunchKernelGGL((k_aov_fill_nmap<true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, h0, h1, aov, stride); return; }
    if (S.bsdf_types & HAR_SCENE_ATTR) { hipLaunchKernelGGL((k_aov_fill_attr<true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, h0, h1, aov, stride); return; }
    if (S.bsdf_types & HAR_SCENE_MASK) { hipLaunchKernelGGL((k_aov_fill_mask<true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, h0, h1, aov, stride); return; }
    if (S.bsdf_types & HAR_SCENE_BLEND) { hipLaunchKernelGGL((k_aov_fill<true, true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, h0, h1, aov, stride); return; }
    hipLaunchKernelGGL((k_aov_fill<true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, seed, spp, log_spp, lane_base, n, nullptr, nullptr, h0, h1, aov, stride);
}
void launch_aov_fill_rays(hipStream_t s, const DScene &S, const AovSpec &spec, uint32_t top_meshes, uint32_t n, const float *d, const uint8_t *active,
                          const float4 *h0, const uint2 *h1, float *aov) {
    const DSensor C{};
    if (S.bsdf_types & HAR_SCENE_BUMPMAP) { hipLaunchKernelGGL((k_aov_fill_bump<false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, 0u, 1u, 0u, 0u, n, d, active, h0, h1, aov, (size_t) n); return; }
    if (S.bsdf_types & HAR_SCENE_NORMALMAP) { hipLaunchKernelGGL((k_aov_fill_nmap<false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, 0u, 1u, 0u, 0u, n, d, active, h0, h1, aov, (size_t) n); return; }
    if (S.bsdf_types & HAR_SCENE_ATTR) { hipLaunchKernelGGL((k_aov_fill_attr<false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, 0u, 1u, 0u, 0u, n, d, active, h0, h1, aov, (size_t) n); return; }
    if (S.bsdf_types & HAR_SCENE_MASK) { hipLaunchKernelGGL((k_aov_fill_mask<false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, 0u, 1u, 0u, 0u, n, d, active, h0, h1, aov, (size_t) n); return; }
    if (S.bsdf_types & HAR_SCENE_BLEND) { hipLaunchKernelGGL((k_aov_fill<false, true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, 0u, 1u, 0u, 0u, n, d, active, h0, h1, aov, (size_t) n); return; }
    hipLaunchKernelGGL((k_aov_fill<false>), dim3(blocks_for(n)), dim3(kBlock), 0, s, S, spec, top_meshes, C, 0u, 1u, 0u, 0u, n, d, active, h0, h1, aov, (size_t) n);
}
void launch_splat_channels(hipStream_t s, const DSensor &C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n, const float *aov, size_t stride,
                           uint32_t channels, float *film) {
    const uint32_t taps = C.rfilter == 0 ? 1u : 2u * (uint32_t) ceilf(C.radius - .5f) + 1u;
    if (taps <= 5) hipLaunchKernelGGL((k_splat_channels<5>), dim3(blocks_for(n)), dim3(kBlock), 0, s, C, seed, spp, log_spp, lane_base, n, aov, stride, channels, film);
    else hipLaunchKernelGGL((k_splat_channels<HAR_MAX_FILTER_TAPS>), dim3(blocks_for(n)), dim3(kBlock), 0, s, C, seed, spp, log_spp, lane_base, n, aov, stride, channels, film);
}

} // namespace har
