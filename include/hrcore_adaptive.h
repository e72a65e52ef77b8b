/*
 * hrcore_adaptive.h — adaptive sampling: a per-pixel sample mask the ray generators honour, and device kernels that build it from the
 * frame and the sample moments of hrcore_aov.h (HR_AOV_MOMENTS).
 *
 * THE SAMPLE MASK.  One bit per pixel of the frame.  While a mask is installed, a pass samples a pixel only when its bit is set (AND
 * whatever the pass itself decides: interactive mode's blocks).  A pixel that is not sampled is what interactive mode's unrendered block
 * pixels already are: its pass sample is 0 0 0 0, it sends no ray, records no AOV and is not counted in hr_pass_stats::paths.  The
 * frame's alpha and MOMENTS.a therefore stay per-pixel sample counts, and everything that divides by them (the display resolve, the
 * denoiser) works on an adaptively sampled frame unchanged.  Without a mask every pixel is sampled: the state of a new context, and the
 * bits of every frame, plane and counter are those of a library without this header.
 *
 * THE ESTIMATE.  Every operation is one binary32 operation in the order written, no contraction, sqrt_ / fmax_ of hr_math.h, correctly
 * rounded division, lum(v) = (0.2126 v.r + 0.7152 v.g) + 0.0722 v.b as in hrcore_denoise.h.  The per-pixel
 * function is heatray_amd/csrc/hr_adaptive.h; heatray_amd/adaptive.py restates it in numpy float32, bit for bit.
 * Per pixel, F = frame, M = MOMENTS:
 *   n = F.a
 *   not n > 0               : err = +inf              (no sample yet: always sampled)
 *   n < (float)min_samples  : err = +inf
 *   else  c = F.rgb / n
 *         e = M.rgb - (n * c) * c,  e = e > 0 ? e : 0
 *         v = lum((e / (n - 1)) / n)                  the variance of the mean (the denoiser's, without the albedo)
 *         err = sqrt_(v) / fmax_(lum(c), floor)
 *   unconverged(p) = err_p > threshold                (+inf > threshold; a NaN error — a pixel that holds NaN — is not)
 *   mask(p) = any unconverged q with |qx - px| <= radius and |qy - py| <= radius, q inside the image
 *
 * THE KNOWN LIMIT.  Deciding from the same samples one is about to average is biased: a pixel whose variance is UNDER-estimated stops
 * early.  min_samples and the dilation are the guards, not a proof.  In a point-lit closed room (cornell_box at 128 x 128) 55 % of the
 * pixels pass the rule after 16 passes, 35 % after 32, 24 % after 48 and 18 % after 64: the share of "converged" pixels FALLS as
 * samples arrive, so most of them had simply not seen their variance yet (many early samples are equal).  With radius = 2 all but
 * 1-2 % of them stay sampled because a neighbour is unconverged.  With radius = 0 they would be switched off for good: a pixel that is
 * no longer sampled never changes its estimate, only a neighbour can bring it back.  Keep radius >= 1.
 *
 * Memory: the mask costs W x H / 8 bytes on every context that holds one (plus W x H bytes of staging for the byte form);
 * hr_adaptive_update adds 4 bytes per pixel for the error map and a second set of mask words, on the context's device (a group's: its
 * first).  Not counted against hr_ctx_desc::memory_budget.  hr_frame_resize and hr_ctx_destroy free them.
 *
 * Not part of hrcore.h, hrcore_aov.h or hrcore_denoise.h: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_ADAPTIVE_H
#define HRCORE_ADAPTIVE_H

#include "hrcore_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_ADAPTIVE_API_VERSION 1u
uint32_t hr_adaptive_api_version(void);

#define HR_ADAPTIVE_MIN_SAMPLES_LOWEST 2
#define HR_ADAPTIVE_MIN_SAMPLES_HIGHEST 65536
#define HR_ADAPTIVE_MAX_RADIUS 4

/* ---- the sample mask: which pixels a pass samples */

/* mask: W x H bytes, row 0 = bottom like the frame, non-zero = the pixel is sampled by the passes rendered from now on.  Completes the
 * enqueued passes first (a batch never sees two masks).  NULL removes the mask (every pixel is sampled).  hr_clear and hr_frame_resize
 * remove it too.  A tile-sharded context takes the whole-frame mask and consults its own pixels; a context group hands it to every
 * member. */
int hr_sample_mask_set(hr_ctx *ctx, const uint8_t *mask);
/* the mask in force -> out (W x H bytes, 0 / 1); *installed (may be NULL) = 0 when there is none (out is then all 1); synchronous */
int hr_sample_mask_get(hr_ctx *ctx, uint8_t *out, int32_t *installed);

/* ---- the error estimate and the mask made from it, on the device */

typedef struct hr_adaptive_params {
    float threshold;      /* a pixel is converged when its error <= threshold; finite, > 0; default 0.02 */
    float floor;          /* luminance below which the error is no longer relative; finite, > 0; default 0.05 */
    int32_t min_samples;  /* a pixel with fewer samples is never converged; 2 .. 65536; default 16 */
    int32_t radius;       /* an unconverged pixel keeps the (2 radius + 1)^2 pixels around it sampled; 0 .. 4; default 2 */
    uint32_t reserved[4]; /* 0 */
} hr_adaptive_params;

void hr_adaptive_default_params(hr_adaptive_params *p);

typedef struct hr_adaptive_result {
    uint64_t unconverged_pixels; /* before the dilation: error > threshold (which includes n < min_samples) */
    uint64_t active_pixels;      /* after it: bits set in the mask that was built */
    float max_error;             /* largest finite error of a pixel with n >= min_samples (0: none) */
    uint32_t passes;             /* complete passes in the frame the estimate was made from */
} hr_adaptive_result;

/* Completes the enqueued passes, computes the error map from the frame and HR_AOV_PLANE_MOMENTS, builds the mask and installs it (as
 * hr_sample_mask_set would); synchronous (the result comes back).  params == NULL: the defaults.  out may be NULL.  install == 0:
 * compute and report only, the mask in force stays.  HR_ERR_INVALID (hr_last_error says which): parameters out of range or not finite;
 * HR_AOV_MOMENTS not enabled, or enabled after the frame's first pass (the plane does not hold the frame's passes: hr_clear, or enable
 * it first); a tile-sharded context outside a group (world > 1: it holds only its own tiles and the dilation reads across them).  A
 * context group assembles the frame and the plane on its first device, runs there and sends the mask to every member: the result is
 * the plain context's, bit for bit. */
int hr_adaptive_update(hr_ctx *ctx, const hr_adaptive_params *params, int32_t install, hr_adaptive_result *out);
/* the error map of the last hr_adaptive_update: W x H floats -> device_out, asynchronously, ordered like hr_aov_copy (HR_ERR_INVALID
 * when there has been none since the last hr_frame_resize) */
int hr_adaptive_error_copy(hr_ctx *ctx, void *device_out, void *stream);
/* ... -> host_out (W x H floats of the caller's), synchronous */
int hr_adaptive_error_readback(hr_ctx *ctx, float *host_out);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_ADAPTIVE_H */
