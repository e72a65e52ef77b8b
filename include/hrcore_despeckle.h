/*
 * hrcore_despeckle.h — firefly suppression: an outlier clamp over the frame and its MOMENTS plane, run on the device ahead of the
 * denoiser.
 *
 * hr_denoise takes a pixel's luminance tolerance from the pixel's own variance, so a firefly (one sample many times brighter than
 * its neighbourhood) has the widest tolerance around and the iterations spread it into a blotch.  The calls here clamp such a pixel
 * to a multiple of what its neighbours show, and write a frame and a moments plane the rest of the chain takes as they are:
 *
 *     hr_despeckle(ctx, 0, 0, 0, out, moments_out, 0, 0, &r);       the frame and its MOMENTS plane -> out, moments_out
 *     hr_despeckle_denoise(ctx, 0, 0, 1, 0, out, 0, 0, &r);          ... and hr_denoise_spatial run from them instead of the raw pair
 *
 * Unlike a blind neighbourhood clamp it has the MOMENTS plane: a bright pixel whose own samples agree with each other (a small lamp,
 * a highlight that has converged) is left alone, so a converged frame comes back untouched, bit for bit.
 *
 * Opt-in, a pure post-process: the frame, the planes, the pass pipeline and later passes are untouched.
 *
 * IMAGES are W x H float4 in accumulation format (rgb sums, a = sample count n, row 0 = bottom) on the context's device; the moments
 * plane holds the sums of the samples' squares (HR_AOV_PLANE_MOMENTS).  The outputs have the same format and keep every pixel's
 * sample count: hr_exposure_meter / hr_exposure_display, hr_metric_compare and the denoiser's Prepare take them as they are.
 *
 * ARITHMETIC.  The rules are hrcore_denoise.h's: every operation is one binary32 operation in the order written, no contraction,
 * correctly rounded division, lum(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z, fmax_(x, y) = x < y ? y : x.  The per-pixel functions
 * are heatray_amd/csrc/hr_despeckle.h; heatray_amd/despeckle.py restates them in numpy float32, bit for bit.
 *
 * CLASSES.  For pixel p of the frame F, n = F.a:
 *   EMPTY      !(n > 0).  Both output pixels are copies of the inputs, bit for bit.  It is nobody's tap.
 *   otherwise  c_k = F_k / n,  l = lum(c)
 *   NONFINITE  l or n is NaN or +-Inf.  Both output pixels are 0 0 0 0: a hole the denoiser skips.  It is nobody's tap.
 *   VALID      every other pixel.
 *
 * NEIGHBOURHOOD of a VALID pixel p: taps q = p + (dx, dy), rows dy = -2 .. 2, in each dx = -2 .. 2, the centre left out (24 taps, in
 * that order).  A tap counts when it is inside the image and VALID.  K = the number of counting taps.
 *   R = the rank-th largest l_q among them (rank 1: the maximum), found by comparisons only: the four largest so far are kept in
 *   order, and a tap's l_q takes the place of the first of them it is greater than (>), the displaced ones moving down.
 *   K < min_taps:  p is STARVED and is copied.
 *
 * THRESHOLD.  T = fmax_(ratio * R + floor, 0)      two operations in that order, then the fmax_
 *   ex = l - T.  p is OVER when ex > 0; a pixel that is not OVER is copied.
 *
 * THE CERTAINTY GUARD: Prepare's variance of the mean, without the albedo.  M = the moments plane's pixel:
 *   e_k = M_k - (n * c_k) * c_k;  e_k = e_k > 0 ? e_k : 0;  vc_k = (e_k / (n - 1)) / n;  v = lum(vc)
 *   an OVER pixel is KEPT (copied) iff n >= 2 and ex * ex > (sigmas * sigmas) * v: its own samples put it that far above T.
 *   A comparison with a NaN is false: a pixel with non-finite moments is clamped.
 *
 * THE CLAMP.  Every other OVER pixel is CLAMPED:
 *   s = T / l;  out = (F.x * s, F.y * s, F.z * s, F.a);  moments_out = (M.x * (s * s), M.y * (s * s), M.z * (s * s), M.a)
 *
 * A flat frame, and a frame whose bright pixels are certain of themselves, come back byte for byte.  One sample's firefly (n = 1 has
 * no variance of its own) is clamped to `ratio` times its second-brightest neighbour.
 *
 * Limits.  The taps are not tested against the surface guides: a one-sample pixel on a thin bright feature (a lamp one pixel wide)
 * is clamped to its surroundings until it has two samples that agree.  A cluster of more than `rank` - 1 fireflies inside one 5 x 5
 * window raises R and survives.  The clamp removes energy: the output is biased low by what the clamped samples carried.
 * There is no display entry: the output goes to hr_exposure_display as an image.
 *
 * Memory: two context-owned planes (32 bytes per pixel) for the despeckled pair when it does not go straight to the caller's memory
 * (a foreign stream, the read-backs, the _denoise entries), made by the first call that needs them; 8 KB of counters.  They are
 * freed with the denoiser's buffers (hr_frame_resize, hr_aov_enable, hr_ctx_destroy).
 *
 * A context group is served: its frame and MOMENTS plane are assembled on its first device, as for hr_denoise.  A tile-sharded
 * context (world > 1) outside a group is refused.
 *
 * Not part of any other header: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_DESPECKLE_H
#define HRCORE_DESPECKLE_H

#include "hrcore_denoise_spatial.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_DESPECKLE_API_VERSION 1u
uint32_t hr_despeckle_api_version(void);

#define HR_DESPECKLE_RANK_HIGHEST 4
#define HR_DESPECKLE_TAPS 24

typedef struct hr_despeckle_params {
    int32_t rank;         /* R is the rank-th largest neighbour luminance; 1 .. 4; default 2 */
    int32_t min_taps;     /* counting taps a pixel needs, else it is STARVED; rank .. 24; default 8 (what an image corner has) */
    float ratio;          /* finite, >= 1; default 2 */
    float sigmas;         /* the certainty guard's width in standard deviations of the pixel's mean; finite, >= 0; default 3 */
    float floor;          /* added to ratio * R; finite, >= 0; default 0 */
    uint32_t reserved[3]; /* 0 */
} hr_despeckle_params;

typedef struct hr_despeckle_result {
    uint64_t valid_pixels;     /* VALID pixels: the four below (but nonfinite) are among them */
    uint64_t clamped_pixels;   /* OVER and not sure of themselves: scaled down to T */
    uint64_t kept_pixels;      /* OVER, and their own samples say so: copied */
    uint64_t starved_pixels;   /* fewer than min_taps counting taps: copied */
    uint64_t nonfinite_pixels; /* NaN or +-Inf in the mean's luminance or the sample count: zeroed */
    uint64_t reserved[3];
} hr_despeckle_result;

void hr_despeckle_default_params(hr_despeckle_params *p);

/* device_frame / device_moments: both NULL (the ctx's frame and its MOMENTS plane, after completing the enqueued passes) or both given
 * (W x H float4 each, on the ctx's device, complete on the ctx's stream; then no AOV plane is asked about, as hr_exposure_meter with an
 * image).  device_out: required.  device_moments_out: may be NULL.  `stream` behaves as in hr_denoise.  passes (may be NULL): the
 * frame's complete passes, 0 for a caller's images.  result (may be NULL): with a result the call waits for the kernel and returns the
 * counters; without one it does not wait.
 * HR_ERR_INVALID (hr_last_error names the field), in this order: a null device_out; only one of the two inputs; an output that is one of
 * the inputs or the other output (the same pointer: the kernel reads neighbours); a parameter out of range or a non-zero reserved word;
 * a tile-sharded context; no frame; with the ctx's own frame, HR_AOV_MOMENTS not enabled or enabled after the frame's first pass.  The
 * context stays usable after every refusal. */
int hr_despeckle(hr_ctx *ctx, const hr_despeckle_params *params, const void *device_frame, const void *device_moments, void *device_out,
                 void *device_moments_out, void *stream, uint32_t *passes, hr_despeckle_result *result);
/* The despeckled frame, and where `moments` is not NULL the despeckled moments, of the ctx's own frame in host memory the ctx owns
 * (valid until the next read-back of this header).  Waits. */
int hr_despeckle_readback(hr_ctx *ctx, const hr_despeckle_params *params, const float **rgba, const float **moments, int32_t *width,
                          int32_t *height, uint32_t *passes, hr_despeckle_result *result);
/* hr_denoise (spatial == 0) or hr_denoise_spatial (spatial != 0; sparams NULL = its defaults) run from the despeckled frame and
 * moments of the ctx's own frame; ALBEDO and NORMAL_DEPTH are the ctx's planes.  The denoiser's kernels and their order are those of
 * hr_denoise / hr_denoise_spatial.  They need HR_AOV_SURFACE | HR_AOV_MOMENTS, and also refuse whatever hr_denoise /
 * hr_denoise_spatial refuse.  result: the despeckle's counters. */
int hr_despeckle_denoise(hr_ctx *ctx, const hr_despeckle_params *params, const hr_denoise_params *dparams, int32_t spatial,
                         const hr_denoise_spatial_params *sparams, void *device_out, void *stream, uint32_t *passes, hr_despeckle_result *result);
int hr_despeckle_denoise_readback(hr_ctx *ctx, const hr_despeckle_params *params, const hr_denoise_params *dparams, int32_t spatial,
                                  const hr_denoise_spatial_params *sparams, const float **rgba, int32_t *width, int32_t *height,
                                  uint32_t *passes, hr_despeckle_result *result);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_DESPECKLE_H */
