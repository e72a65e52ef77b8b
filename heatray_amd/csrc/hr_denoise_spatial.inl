// hr_denoise_spatial.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_denoise_spatial.h.  The
// kernel is in hr_denoise_spatial.hip; the checks, the buffers and the launches around it are denoiseRun's (hr_denoise.inl), which takes
// the estimate's parameters as its optional last argument.

static int denoiseSpatialCheckParams(hr_ctx *c, const hr_denoise_spatial_params *in, hr_denoise_spatial_params *p)
{
    if (in)
        *p = *in;
    else
        hr_denoise_spatial_default_params(p);
    if (p->below < HR_DENOISE_SPATIAL_BELOW_LOWEST || p->below > HR_DENOISE_SPATIAL_BELOW_HIGHEST)
        FAIL(c, HR_ERR_INVALID, "denoise spatial: below = " + std::to_string(p->below) + " is outside " + std::to_string(HR_DENOISE_SPATIAL_BELOW_LOWEST) + " .. " +
                                    std::to_string(HR_DENOISE_SPATIAL_BELOW_HIGHEST));
    if (p->min_taps < HR_DENOISE_SPATIAL_MIN_TAPS_LOWEST || p->min_taps > HR_DENOISE_SPATIAL_MIN_TAPS_HIGHEST)
        FAIL(c, HR_ERR_INVALID, "denoise spatial: min_taps = " + std::to_string(p->min_taps) + " is outside " + std::to_string(HR_DENOISE_SPATIAL_MIN_TAPS_LOWEST) + " .. " +
                                    std::to_string(HR_DENOISE_SPATIAL_MIN_TAPS_HIGHEST));
    for (int k = 0; k < 6; ++k)
        if (p->reserved[k]) FAIL(c, HR_ERR_INVALID, "denoise spatial: reserved[" + std::to_string(k) + "] must be 0");
    return HR_OK;
}

// denoiseRun with the estimate; with `out` it waits for the kernels and returns the counters
static int denoiseSpatialRun(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, float *dst, uint32_t *passes, bool varianceOnly,
                             hr_denoise_spatial_result *out)
{
    DenoiseSpatialRun run;
    run.varianceOnly = varianceOnly;
    int rc = denoiseSpatialCheckParams(c, sparams, &run.p);
    if (rc == HR_OK) rc = denoiseRun(c, dparams, dst, passes, &run);
    if (rc) return rc;
    if (out) {
        HIP_TRY(c, hipMemcpyAsync(c->dnSpatialResultHost, c->dnSpatialResult, kDenoiseSpatialResultWords * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        *out = hr_denoise_spatial_result{};
        out->spatial_pixels = c->dnSpatialResultHost[0], out->estimated_pixels = c->dnSpatialResultHost[1], out->starved_pixels = c->dnSpatialResultHost[2];
    }
    return HR_OK;
}

extern "C" {

uint32_t hr_denoise_spatial_api_version(void) { return HR_DENOISE_SPATIAL_API_VERSION; }

void hr_denoise_spatial_default_params(hr_denoise_spatial_params *p)
{
    if (!p) return;
    *p = hr_denoise_spatial_params{};
    p->below = 4, p->min_taps = 6;
}

int hr_denoise_spatial(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, void *device_out, void *stream, uint32_t *passes,
                       hr_denoise_spatial_result *result)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "null output");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (st == c->stream) return denoiseSpatialRun(c, dparams, sparams, (float *)device_out, passes, false, result);
    // a foreign stream: as in hr_denoise
    int rc = denoiseSpatialRun(c, dparams, sparams, nullptr, passes, false, result);
    if (rc) return rc;
    if (!c->evAov) HIP_TRY(c, hipEventCreateWithFlags(&c->evAov, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->evAov, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(st, c->evAov, 0));
    HIP_TRY(c, hipMemcpyAsync(device_out, c->dnOut, (size_t)c->W * c->H * 16, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipEventRecord(c->evAov, st));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evAov, 0));
    return HR_OK;
}

int hr_denoise_spatial_readback(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, const float **rgba, int32_t *w, int32_t *h,
                                uint32_t *passes, hr_denoise_spatial_result *result)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "null output");
    int rc = denoiseSpatialRun(c, dparams, sparams, nullptr, passes, false, nullptr);
    if (rc) return rc;
    const size_t bytes = (size_t)c->W * c->H * 16;
    if (c->dnPinnedBytes < bytes) {
        if (c->dnPinned) hipHostFree(c->dnPinned);
        c->dnPinned = nullptr, c->dnPinnedBytes = 0;
        HIP_TRY(c, hipHostMalloc((void **)&c->dnPinned, bytes, hipHostMallocDefault));
        c->dnPinnedBytes = bytes;
    }
    HIP_TRY(c, hipMemcpyAsync(c->dnPinned, c->dnOut, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->dnSpatialResultHost, c->dnSpatialResult, kDenoiseSpatialResultWords * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (result) {
        *result = hr_denoise_spatial_result{};
        result->spatial_pixels = c->dnSpatialResultHost[0], result->estimated_pixels = c->dnSpatialResultHost[1], result->starved_pixels = c->dnSpatialResultHost[2];
    }
    *rgba = c->dnPinned;
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

int hr_denoise_spatial_display(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, const hr_display_params *display, int32_t format,
                               void *device_out, uint32_t *passes_shown)
{
    ENTER(c);
    if (!display || !device_out) FAIL(c, HR_ERR_INVALID, "null argument");
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format (the denoised display has no progressive form)");
    int rc = denoiseSpatialRun(c, dparams, sparams, nullptr, passes_shown, false, nullptr);
    if (rc) return rc;
    FrameDev fr = c->frame; // (as in hr_denoise_display)
    fr.fb = c->dnOut;
    launchDisplay(c->cfg(c->stream), fr, *display, format, device_out);
    HIP_TRY(c, hipGetLastError());
    return HR_OK;
}

int hr_denoise_spatial_variance(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, float *host_out, hr_denoise_spatial_result *result)
{
    ENTER(c);
    if (!host_out) FAIL(c, HR_ERR_INVALID, "null output");
    int rc = denoiseSpatialRun(c, dparams, sparams, nullptr, nullptr, true, nullptr);
    if (rc) return rc;
    const size_t px = (size_t)c->W * c->H;
    std::vector<float> cv(px * 4); // (cv[1]: colour + variance; a call for inspection, not a hot path)
    HIP_TRY(c, hipMemcpyAsync(cv.data(), c->dnWork + 4 * px, px * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->dnSpatialResultHost, c->dnSpatialResult, kDenoiseSpatialResultWords * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < px; ++i) host_out[i] = cv[4 * i + 3];
    if (result) {
        *result = hr_denoise_spatial_result{};
        result->spatial_pixels = c->dnSpatialResultHost[0], result->estimated_pixels = c->dnSpatialResultHost[1], result->starved_pixels = c->dnSpatialResultHost[2];
    }
    return HR_OK;
}

} // extern "C"
