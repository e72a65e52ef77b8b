/*
 * hrcore_aov.h — feature buffers (AOVs) of libhrcore: per-pixel sums that accumulate with the frame, for a denoiser, adaptive
 * sampling, compositing or a convergence check.
 *
 * First visible surface of a pass at a pixel: the first hit of that pass's camera path at which the shader reaches its visualizer
 * switch (physicallyBased, glass).  A pass-through does not count — an alpha-masked texel, the back face of a single-sided
 * material — the surface behind it does.  These are exactly the hits a render with enable_visualizer records.  Camera rays that
 * miss, and hits on materials of no class, record nothing.
 *
 * Planes (W x H float4 each, row 0 = bottom, like the frame):
 *   HR_AOV_PLANE_ALBEDO        rgb = sum over passes of baseColor at that surface, as HR_VIS_BASE_COLOR computes it (texture x
 *                              vertex colours, glass included); a = passes that recorded a surface.
 *   HR_AOV_PLANE_NORMAL_DEPTH  xyz = sum of the world-space shading normal N as HR_VIS_FINAL_NORMALS sees it (after the normal map
 *                              and the double-sided flip; not remapped to [0,1]); w = sum of the surface point's camera-space depth:
 *                              dot(P - eye, forward), eye = view_matrix column 3, forward = -normalize(view_matrix column 2).
 *   HR_AOV_PLANE_MOMENTS       rgb = sum over passes of s * s per channel, s = the pass's complete sample (the one added to the
 *                              frame; HR_ESTIMATOR_ALL_LIGHTS: after its partial sums are combined); a = sum of the sample's alpha
 *                              (bit-identical to the frame's alpha).
 * Every plane is summed in pass order, in the same launch that adds the pass to the frame (a = a + v, one pass after the other): the
 * frame and the planes always hold the same passes, counted from the pass after the planes were last zeroed.  AOVs never change
 * the frame: it is bit-identical with them on or off.
 *
 * Not part of hrcore.h: that header's ABI version does not change with these calls; this one has its own.  A context group
 * (hrcore_group.h) takes every call: enabling goes to every member, read-backs and copies assemble the members' tiles.
 */
#ifndef HRCORE_AOV_H
#define HRCORE_AOV_H

#include "hrcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_AOV_API_VERSION 1u
uint32_t hr_aov_api_version(void);

#define HR_AOV_SURFACE 1u /* planes ALBEDO + NORMAL_DEPTH: two more float4 frames per pass slot */
#define HR_AOV_MOMENTS 2u /* plane MOMENTS */

#define HR_AOV_PLANE_ALBEDO 0
#define HR_AOV_PLANE_NORMAL_DEPTH 1
#define HR_AOV_PLANE_MOMENTS 2

/* Completes the passes in flight; a changed mask (re)allocates and zeroes the planes it names (and frees the others), 0 frees
 * them all; an unchanged mask does nothing.  Unknown bits: HR_ERR_INVALID.  hr_clear and hr_frame_resize zero the enabled planes. */
int hr_aov_enable(hr_ctx *ctx, uint32_t mask);
/* The enabled mask (0 when none). */
int hr_aov_mask(hr_ctx *ctx, uint32_t *mask);
/* Like hr_readback: completes the enqueued passes, copies one plane to a pinned host buffer owned by the ctx (W x H float4, row
 * 0 = bottom; valid until the next hr_aov_readback / hr_aov_enable / hr_frame_resize / hr_ctx_destroy); passes (may be NULL) =
 * passes summed into the plane since it was last zeroed.  A plane that is not enabled, or a bad plane id: HR_ERR_INVALID.  In a
 * tile-sharded context (world > 1) the pixels other ranks own read as 0. */
int hr_aov_readback(hr_ctx *ctx, int32_t plane, const float **rgba, int32_t *width, int32_t *height, uint64_t *passes);
/* Asynchronous device-to-device copy of one plane (W x H float4) to device_out (e.g. a torch tensor), ordered like hr_display:
 * after every enqueued pass.  stream: where the copy runs (NULL: the ctx stream); the ctx's next resolve waits for it. */
int hr_aov_copy(hr_ctx *ctx, int32_t plane, void *device_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_AOV_H */
