// hr_metric.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_metric.h.  The kernel is in
// hr_metric.hip, the arithmetic (the fold among it) in hr_metric.h.
//
// Ordering: everything runs on the context's stream — the words' zeroing, the kernel, the fetch — behind the resolves (or a group's
// gather) enqueued there; every call waits for its result.
#include "hr_metric.h"

static int metricCheckParams(hr_ctx *c, const hr_metric_params *in, hr_metric_params *p)
{
    if (in)
        *p = *in;
    else
        hr_metric_default_params(p);
    for (uint32_t r : p->reserved)
        if (r) FAIL(c, HR_ERR_INVALID, "metric: the reserved words of hr_metric_params must be 0");
    return HR_OK;
}

// the window of the parameters within W x H (0 0 0 0: all of it)
static int metricWindow(hr_ctx *c, const hr_metric_params &p, MtWindow *win)
{
    const int32_t *w = p.window;
    if (w[0] == 0 && w[1] == 0 && w[2] == 0 && w[3] == 0) {
        *win = MtWindow{0, 0, c->W, c->H};
        return HR_OK;
    }
    if (!(0 <= w[0] && w[0] < w[2] && w[2] <= c->W && 0 <= w[1] && w[1] < w[3] && w[3] <= c->H))
        FAIL(c, HR_ERR_INVALID, "metric: the window " + std::to_string(w[0]) + " " + std::to_string(w[1]) + " " + std::to_string(w[2]) + " " + std::to_string(w[3]) +
                                    " is not 0 <= x0 < x1 <= " + std::to_string(c->W) + ", 0 <= y0 < y1 <= " + std::to_string(c->H));
    *win = MtWindow{w[0], w[1], w[2], w[3]};
    return HR_OK;
}

// the one place that reads the host words: the last fetched measurement -> the result (and the bins), through hr_metric.h's fold (mtFinish)
static void metricFill(const hr_ctx *c, hr_metric_result *out, uint64_t *numBins, uint64_t *denBins)
{
    const unsigned long long *h = c->metric.bins.host;
    *out = hr_metric_result{};
    const MtFolded f = mtFinish(h, c->metric.kind);
    out->num = f.num, out->den = f.den, out->value = f.value, out->mse = f.mse, out->flags = f.flags;
    out->counted = h[kMtWordCounted], out->differing = h[kMtWordDiffering], out->nonfinite = h[kMtWordNonfinite], out->skipped = h[kMtWordSkipped];
    const uint32_t maxBits = (uint32_t)h[kMtWordMaxAbs];
    std::memcpy(&out->max_abs, &maxBits, 4);
    out->passes = c->metric.passes, out->kind = c->metric.kind;
    for (int k = 0; k < kMtBins; ++k) {
        if (numBins) numBins[k] = h[kMtWordNum + k];
        if (denBins) denBins[k] = h[kMtWordDen + k];
    }
}

// the last measurement, fetched and waited for, -> out
static int metricFetch(hr_ctx *c, hr_metric_result *out, uint64_t *numBins, uint64_t *denBins)
{
    HIP_TRY(c, c->metric.bins.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    metricFill(c, out, numBins, denBins);
    return HR_OK;
}

// Checks, finds the two images (compare: device_image or the frame, and the reference; estimate: the frame and its MOMENTS plane),
// measures and waits
static int metricRun(hr_ctx *c, uint32_t kind, const hr_metric_params *params, const void *device_image, const void *device_reference, hr_metric_result *out)
{
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    hr_metric_params p;
    int rc = metricCheckParams(c, params, &p);
    if (rc) return rc;
    if (kind == HR_METRIC_COMPARE && !device_reference) FAIL(c, HR_ERR_INVALID, "metric: null reference");
    const float *image = nullptr, *other = (const float *)device_reference;
    uint32_t passes = 0;
    if (kind == HR_METRIC_ESTIMATE) {
        const FrameNeed need{HR_AOV_MOMENTS, "metric", "the sum", true, true, "metric: the estimate needs the sample moments: hr_aov_enable(HR_AOV_MOMENTS)",
                             "metric: the MOMENTS plane was enabled after the frame's first pass and does not hold"};
        rc = frameReady(c, need, &image, &passes);
        other = c->aov.plane[HR_AOV_PLANE_MOMENTS];
    } else {
        const FrameNeed need{0, "metric", "the sum", true, false, "", ""};
        if (device_image) {
            rc = frameKindReady(c, need);
            image = (const float *)device_image;
        } else {
            rc = frameReady(c, need, &image, &passes);
        }
    }
    if (rc) return rc;
    MtWindow win;
    rc = metricWindow(c, p, &win);
    if (rc) return rc;
    HIP_TRY(c, c->metric.bins.ensure(kMtWords));
    HIP_TRY(c, c->metric.bins.zero(c->stream));
    launchMetricAccumulate(c->stream, c->numCUs, c->W, c->H, (int)kind, image, other, win, c->metric.bins.dev);
    HIP_TRY(c, hipGetLastError());
    c->metric.measured = true, c->metric.kind = kind, c->metric.passes = passes;
    return metricFetch(c, out, nullptr, nullptr);
}

extern "C" {

uint32_t hr_metric_api_version(void) { return HR_METRIC_API_VERSION; }

void hr_metric_default_params(hr_metric_params *p)
{
    if (!p) return;
    *p = hr_metric_params{};
}

int hr_metric_compare(hr_ctx *c, const hr_metric_params *params, const void *device_image, const void *device_reference, hr_metric_result *out)
{
    ENTER(c);
    return metricRun(c, HR_METRIC_COMPARE, params, device_image, device_reference, out);
}

int hr_metric_estimate(hr_ctx *c, const hr_metric_params *params, hr_metric_result *out)
{
    ENTER(c);
    return metricRun(c, HR_METRIC_ESTIMATE, params, nullptr, nullptr, out);
}

int hr_metric_last(hr_ctx *c, hr_metric_result *out, uint64_t *num_bins, uint64_t *den_bins)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    if (!c->metric.measured) FAIL(c, HR_ERR_INVALID, "metric: nothing has been measured yet (hr_metric_compare, hr_metric_estimate)");
    return metricFetch(c, out, num_bins, den_bins);
}

} // extern "C"
