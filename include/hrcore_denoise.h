/*
 * hrcore_denoise.h — a variance-guided edge-avoiding a-trous denoiser over the frame and the AOV planes of hrcore_aov.h.
 *
 * A post-process: it reads the accumulation buffer and the three planes (ALBEDO, NORMAL_DEPTH, MOMENTS) and writes a denoised image
 * elsewhere.  It never changes the frame, the planes or what a later pass adds to them.  The output is a ONE-SAMPLE accumulation buffer
 * (W x H float4, row 0 = bottom, rgb = the denoised mean colour, a = 1; a pixel without samples is 0 0 0 0), so the display resolve
 * applies to it unchanged.
 *
 * The contract.  Every operation is one binary32 operation in the order written, no contraction, sqrt_ / exp_ / fmax_ of hr_math.h,
 * correctly rounded division.  lum(v) = (0.2126 v.r + 0.7152 v.g) + 0.0722 v.b.  The per-pixel functions are
 * heatray_amd/csrc/hr_denoise.h; heatray_amd/denoise.py restates them in numpy float32, bit for bit.
 *
 * Prepare, per pixel (F = frame, A = ALBEDO, G = NORMAL_DEPTH, M = MOMENTS):
 *   n = F.a.  Not n > 0: the pixel is INVALID (interactive mode's unrendered block pixels): it is nobody's tap and comes out as 0 0 0 0.
 *   c = F.rgb / n;  hits = A.a;  a = fmax_((A.rgb + (n - hits)) / n, 0.01)      a pass that met no surface counts as albedo 1
 *   d = c / a                                                                   the demodulated colour the filter works on
 *   n >= 2:  e = M.rgb - (n * c) * c, e = e > 0 ? e : 0;  v = lum(((e / (n - 1)) / n) / (a * a))      variance of the mean
 *   n <  2:  v = 0: ONE sample has no variance estimate; the pixel passes through unfiltered (and still is its neighbours' tap).
 *            The filter starts working at two passes; interactive mode's one-sample blocks pass through.
 *            (hrcore_denoise_spatial.h has calls that give such pixels a variance borrowed from their neighbours first.)
 *   l2 = (G.x G.x + G.y G.y) + G.z G.z;  N = G.xyz / sqrt_(l2) where hits > 0 and l2 > 0, else 0 0 0
 *   z = G.w / hits where hits > 0, else 0;   cov = hits / n
 *   facing(p, q) = (cov_p == 0 and cov_q == 0) or dot(N_p, N_q) > 0, dot = (x x + y y) + z z: only then does q lend p its variance or depth
 *   g (a second launch, from the prepared z): the largest |z - z_q| over the four direct neighbours q (left, right, below, above) that
 *   are inside the image, have cov_q > 0 and dot(N_p, N_q) > 0; 0 where there is none or cov_p is not > 0.
 *
 * Iterate, i = 0 .. iterations - 1, step = 1 << i, per valid pixel p:
 *   vbar = sum(g3 v_q) / sum(g3) over the 3 x 3 neighbours q at distance ONE (rows dy = -1, 0, 1, in each dx = -1, 0, 1) that are
 *          inside, valid and (but for p itself) facing p, g3 = (1/16 1/8 1/16; 1/8 1/4 1/8; 1/16 1/8 1/16);   sl = sigma_l * sqrt_(vbar) + 1e-6
 *   zs = sigma_z * (g_p * (float)step) + 1e-3 * |z_p| + 1e-30
 *   taps q = p + step * (dx, dy), rows dy = -2 .. 2, in each dx = -2 .. 2, with k = K[|dy|] * K[|dx|], K = (3/8, 1/4, 1/16).  A tap outside
 *   the image or invalid weighs 0.  The centre tap weighs k.  Any other:
 *       wn = 1 where cov_p == 0 and cov_q == 0, else fmax_(dot(N_p, N_q), 0) squared normal_power times
 *       wc = fmax_(1 - 4 |cov_p - cov_q|, 0)
 *       we = exp_(-(|z_p - z_q| / zs + |lum(d_p) - lum(d_q)| / sl))          the depth and the luminance term, one exponential
 *       w  = ((k * wn) * wc) * we
 *   Taps with w > 0 are summed in tap order: S += w d_q, V += (w w) v_q, W += w.   d_p' = S / W,  v_p' = V / (W W).
 * Finish: rgb = d * a, a = 1.  iterations == 0 gives the remodulated mean (c up to the rounding of c / a * a).
 *
 * What the guides cannot see: they describe the FIRST visible surface.  Behind glass, in a mirror and on geometry smaller than a pixel
 * they say little, and the filter then leans on the luminance term alone (DESIGN.md has the measured errors).
 *
 * Memory: the first call allocates working planes on the context's device (a group's: on its first device): 68 bytes per pixel
 * (two colour + variance planes, normal + depth, albedo + coverage, depth gradient) and, for hr_denoise_readback / _display / a foreign
 * stream, a result image of 16 more, plus the pinned host copy hr_denoise_readback hands out.  They are NOT counted against
 * hr_ctx_desc::memory_budget.  hr_frame_resize, hr_aov_enable with another mask and hr_ctx_destroy free them.
 *
 * Not part of hrcore.h or hrcore_aov.h: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_DENOISE_H
#define HRCORE_DENOISE_H

#include "hrcore_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_DENOISE_API_VERSION 1u
uint32_t hr_denoise_api_version(void);

#define HR_DENOISE_MAX_ITERATIONS 8
#define HR_DENOISE_MAX_NORMAL_POWER 16

/* which a-trous kernel runs an iteration: the same bits either way */
#define HR_DENOISE_KERNEL_AUTO 0  /* what measured fastest for the step */
#define HR_DENOISE_KERNEL_PLAIN 1 /* every tap a global load */
#define HR_DENOISE_KERNEL_TILED 2 /* a workgroup stages its tile and halo in LDS (steps 1 and 2; larger steps run plain) */

typedef struct hr_denoise_params {
    int32_t iterations;   /* 0 .. HR_DENOISE_MAX_ITERATIONS, default 5 */
    int32_t normal_power; /* the normal weight is squared this many times: 0 .. HR_DENOISE_MAX_NORMAL_POWER, default 7 (the 128th power) */
    float sigma_l;        /* luminance, in standard deviations of the mean: finite, >= 0, default 4 */
    float sigma_z;        /* depth, in multiples of the centre's depth gradient times the step: finite, >= 0, default 4 */
    int32_t kernel;       /* HR_DENOISE_KERNEL_* */
    uint32_t reserved[3]; /* 0 */
} hr_denoise_params;

void hr_denoise_default_params(hr_denoise_params *p);

/* All three complete the enqueued passes first (like hr_aov_copy), take params == NULL as the defaults and fail with HR_ERR_INVALID
 * (hr_last_error says which) for: parameters out of range or not finite; a context without both HR_AOV_SURFACE and HR_AOV_MOMENTS
 * enabled (hr_aov_enable); planes that do not hold the same passes as the frame because they were enabled after the frame's first
 * pass (hr_clear, or enable them first); a tile-sharded context outside a group (world > 1: it holds only its own tiles).  A context
 * group assembles the frame and the planes on its first device and filters there: the result is the plain context's, bit for bit.
 * passes (may be NULL): complete passes in the frame that was filtered. */

/* The denoised image -> device_out (W x H float4), asynchronously.  The filter runs on the ctx stream; with another `stream` the result
 * is copied out there, ordered after the filter, and the ctx's next work waits for the copy (like hr_aov_copy). */
int hr_denoise(hr_ctx *ctx, const hr_denoise_params *params, void *device_out, void *stream, uint32_t *passes);
/* ... -> a pinned host buffer owned by the ctx (valid until the next hr_denoise_readback / hr_frame_resize / hr_aov_enable /
 * hr_ctx_destroy); synchronous. */
int hr_denoise_readback(hr_ctx *ctx, const hr_denoise_params *params, const float **rgba, int32_t *width, int32_t *height, uint32_t *passes);
/* hr_display's fragment applied to the denoised image -> device_out, asynchronously on the ctx stream.  format: HR_DISPLAY_RGBA8,
 * HR_DISPLAY_RGBA32F or HR_DISPLAY_HDR_RGBA32F (no HR_DISPLAY_PROGRESSIVE: the filter needs complete passes). */
int hr_denoise_display(hr_ctx *ctx, const hr_denoise_params *params, const hr_display_params *display, int32_t format, void *device_out,
                       uint32_t *passes_shown);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_DENOISE_H */
