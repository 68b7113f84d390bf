/* har_aov_launch.h -- launch wrappers of the AOV kernels (har_aov.hip) */
#pragma once
#include <hip/hip_runtime.h>
#include "har_aov.h"
#include "har_path.h"

namespace har {

/* Closest hits of the AOV pass, one record per lane IN LANE ORDER: h0 = { t, u, v, prim }, h1 = { shape, instance }.
 * `deep`: the scene's depth-first bound exceeds HAR_LDS_STACK_SMALL entries (the kernel with the HAR_LDS_STACK_DEPTH-entry LDS stack runs).
 * _lanes: the camera rays of lanes [lane_base, lane_base + n) of render() at `seed` (raygen_lane);  _rays: n caller-supplied rays (SoA) under a mask */
void launch_aov_trace_lanes(hipStream_t s, const DScene &S, bool deep, const DSensor &C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                            float4 *h0, uint2 *h1, int *status);
void launch_aov_trace_rays(hipStream_t s, const DScene &S, bool deep, uint32_t n, const float *o, const float *d, const float *maxt, const uint8_t *active,
                           float4 *h0, uint2 *h1, int *status);
/* the camera rays of lanes [lane_base, lane_base + n) of a batch sensor's render, SoA with stride n (for the _rays launches) */
void launch_aov_batch_rays(hipStream_t s, const DSensor &C, const DBatch &batch, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n,
                           float *o, float *d, float *maxt);
/* k_aov_fill: aov_lane() per lane, channel-major: aov[c * stride + i] */
void launch_aov_fill_lanes(hipStream_t s, const DScene &S, const AovSpec &spec, uint32_t top_meshes, const DSensor &C, uint32_t seed, uint32_t spp, uint32_t log_spp,
                           uint32_t lane_base, uint32_t n, const float4 *h0, const uint2 *h1, float *aov, size_t stride);
void launch_aov_fill_rays(hipStream_t s, const DScene &S, const AovSpec &spec, uint32_t top_meshes, uint32_t n, const float *d, const uint8_t *active,
                          const float4 *h0, const uint2 *h1, float *aov);
/* k_splat_channels: ImageBlock::put of `channels` values + the weight per lane into film (H x W x (channels + 1)) */
void launch_splat_channels(hipStream_t s, const DSensor &C, uint32_t seed, uint32_t spp, uint32_t log_spp, uint32_t lane_base, uint32_t n, const float *aov, size_t stride,
                           uint32_t channels, float *film);

} // namespace har
