// hr_exposure.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_exposure.h.  The kernels are in
// hr_exposure.hip, the arithmetic in hr_exposure.h.
//
// Ordering: everything runs on the context's stream — the words' zeroing, the histogram, the reduce, the display that reads the scale
// word the reduce wrote — behind the resolves (or a group's gather) enqueued there; the host sees a number only where a call is
// documented to wait.  The adaptation state lives on the device: a metering enqueued behind another adapts from it without the host.
#include "hr_exposure.h"

static int exposureCheckParams(hr_ctx *c, const hr_exposure_params *in, hr_exposure_params *p)
{
    if (in)
        *p = *in;
    else
        hr_exposure_default_params(p);
    if (!std::isfinite(p->key) || !(p->key > 0.0f)) FAIL(c, HR_ERR_INVALID, "exposure: key must be finite and greater than 0");
    if (p->low_permille < 0 || p->high_permille > 1000 || p->low_permille >= p->high_permille)
        FAIL(c, HR_ERR_INVALID, "exposure: low_permille = " + std::to_string(p->low_permille) + ", high_permille = " + std::to_string(p->high_permille) +
                                    " are not 0 <= low < high <= 1000");
    if (!std::isfinite(p->min_scale) || !std::isfinite(p->max_scale) || !(p->min_scale > 0.0f) || !(p->min_scale <= p->max_scale))
        FAIL(c, HR_ERR_INVALID, "exposure: min_scale and max_scale must be finite with 0 < min_scale <= max_scale");
    if (!(p->adapt >= 0.0f && p->adapt <= 1.0f)) FAIL(c, HR_ERR_INVALID, "exposure: adapt must lie in 0 .. 1");
    for (uint32_t r : p->reserved)
        if (r) FAIL(c, HR_ERR_INVALID, "exposure: the reserved words of hr_exposure_params must be 0");
    return HR_OK;
}

// the window of the parameters within W x H (0 0 0 0: all of it)
static int exposureWindow(hr_ctx *c, const hr_exposure_params &p, ExWindow *win)
{
    const int32_t *w = p.window;
    if (w[0] == 0 && w[1] == 0 && w[2] == 0 && w[3] == 0) {
        *win = ExWindow{0, 0, c->W, c->H};
        return HR_OK;
    }
    if (!(0 <= w[0] && w[0] < w[2] && w[2] <= c->W && 0 <= w[1] && w[1] < w[3] && w[3] <= c->H))
        FAIL(c, HR_ERR_INVALID, "exposure: the window " + std::to_string(w[0]) + " " + std::to_string(w[1]) + " " + std::to_string(w[2]) + " " + std::to_string(w[3]) +
                                    " is not 0 <= x0 < x1 <= " + std::to_string(c->W) + ", 0 <= y0 < y1 <= " + std::to_string(c->H));
    *win = ExWindow{w[0], w[1], w[2], w[3]};
    return HR_OK;
}

// the one place that reads the host words: the last fetched metering -> the result (and the bins)
static void exposureFill(const hr_ctx *c, hr_exposure_result *out, uint64_t *bins)
{
    const unsigned long long *h = c->exposure.bins.host;
    const auto f = [h](int word) {
        const uint32_t b = (uint32_t)h[word];
        float v;
        std::memcpy(&v, &b, 4);
        return v;
    };
    *out = hr_exposure_result{};
    out->scale = f(kExWordScale), out->target = f(kExWordTarget), out->key_luminance = f(kExWordLavg);
    out->position = (uint32_t)h[kExWordPosition];
    out->counted = h[kExWordCounted], out->used = h[kExWordUsed];
    out->below = h[kExBelow], out->above = h[kExAbove], out->nonfinite = h[kExNonfinite], out->invalid = h[kExInvalid];
    out->flags = (uint32_t)h[kExWordFlags];
    if (bins)
        for (int k = 0; k < kExBins; ++k) bins[k] = h[k];
}

// Checks, finds the image (device_image, or the frame: complete, or with `progressive` as far as it is resolved), and enqueues the
// metering on the ctx stream.  *image: what was metered; *passes: the frame's passes in it (0 for a device_image).
static int exposureRun(hr_ctx *c, const hr_exposure_params *params, const void *device_image, bool progressive, const float **image, uint32_t *passes)
{
    hr_exposure_params p;
    int rc = exposureCheckParams(c, params, &p);
    if (rc) return rc;
    const FrameNeed need{0, "exposure", "the meter", true, false, "", ""};
    *passes = 0;
    if (device_image) {
        rc = frameKindReady(c, need);
        *image = (const float *)device_image;
    } else if (!progressive) {
        rc = frameReady(c, need, image, passes);
        if (rc == HR_OK && !c->grp) *passes = (uint32_t)(c->nextResolveOrder - c->resolvedAtClear); // (as hr_display counts them)
    } else { // what is resolved already, as hr_display shows it
        rc = frameKindReady(c, need);
        if (rc == HR_OK && c->grp) rc = groupAssemble(c, false, passes, nullptr);
        if (rc == HR_OK && !c->grp) *passes = (uint32_t)(c->nextResolveOrder - c->resolvedAtClear);
        *image = c->grp ? c->fbInternal : c->fb();
    }
    if (rc) return rc;
    ExWindow win;
    rc = exposureWindow(c, p, &win);
    if (rc) return rc;
    HIP_TRY(c, c->exposure.bins.ensure(kExWords));
    if (!c->exposure.state) {
        HIP_TRY(c, c->exposure.state.alloc(2));
        HIP_TRY(c, hipMemsetAsync(c->exposure.state, 0, 2 * sizeof(uint32_t), c->stream));
    }
    HIP_TRY(c, c->exposure.bins.zero(c->stream));
    launchExposureMeter(c->stream, c->numCUs, c->W, c->H, *image, win, ExParams{p.key, p.low_permille, p.high_permille, p.min_scale, p.max_scale, p.adapt}, c->exposure.bins.dev,
                        c->exposure.state);
    HIP_TRY(c, hipGetLastError());
    c->exposure.metered = true;
    return HR_OK;
}

// the last metering, fetched and waited for, -> out
static int exposureFetch(hr_ctx *c, hr_exposure_result *out, uint64_t *bins)
{
    HIP_TRY(c, c->exposure.bins.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    exposureFill(c, out, bins);
    return HR_OK;
}

extern "C" {

uint32_t hr_exposure_api_version(void) { return HR_EXPOSURE_API_VERSION; }

void hr_exposure_default_params(hr_exposure_params *p)
{
    if (!p) return;
    *p = hr_exposure_params{};
    p->key = 0.18f, p->low_permille = 100, p->high_permille = 950;
    p->min_scale = 1.0f / 256.0f, p->max_scale = 256.0f, p->adapt = 1.0f;
}

int hr_exposure_meter(hr_ctx *c, const hr_exposure_params *params, const void *device_image, hr_exposure_result *out)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    const float *image = nullptr;
    uint32_t n = 0;
    const int rc = exposureRun(c, params, device_image, false, &image, &n);
    if (rc) return rc;
    return exposureFetch(c, out, nullptr);
}

int hr_exposure_display(hr_ctx *c, const hr_exposure_params *params, const hr_display_params *display, int32_t format, const void *device_image, void *device_out,
                        uint32_t *passes_shown)
{
    ENTER(c);
    if (!display || !device_out) FAIL(c, HR_ERR_INVALID, "null argument");
    const bool progressive = (format & HR_DISPLAY_PROGRESSIVE) != 0;
    format &= ~HR_DISPLAY_PROGRESSIVE;
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format");
    const float *image = nullptr;
    uint32_t n = 0;
    const int rc = exposureRun(c, params, device_image, progressive, &image, &n);
    if (rc) return rc;
    FrameDev fr = c->frame; // (exposureRun has refused world > 1: every pixel is this context's; a group's frame is rank 0 of 1)
    fr.fb = const_cast<float *>(image);
    launchExposureDisplay(c->stream, fr, *display, format, c->exposure.bins.dev, device_out);
    HIP_TRY(c, hipGetLastError());
    if (passes_shown) *passes_shown = n;
    return HR_OK;
}

int hr_exposure_last(hr_ctx *c, hr_exposure_result *out, uint64_t *bins)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    if (!c->exposure.metered) FAIL(c, HR_ERR_INVALID, "exposure: nothing has been metered yet (hr_exposure_meter, hr_exposure_display)");
    return exposureFetch(c, out, bins);
}

int hr_exposure_reset(hr_ctx *c)
{
    ENTER(c);
    if (c->exposure.state) HIP_TRY(c, hipMemsetAsync(c->exposure.state, 0, 2 * sizeof(uint32_t), c->stream));
    return HR_OK;
}

} // extern "C"
