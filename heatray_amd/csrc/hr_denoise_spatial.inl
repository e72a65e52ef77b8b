// hr_denoise_spatial.inl — a section of hr_core.hip (included at its end, after hr_denoise.inl): the entry points of
// include/hrcore_denoise_spatial.h.  The kernel is in hr_denoise_spatial.hip; the checks, the buffers and the launches around it are
// denoiseRun's, and the calls are hr_denoise.inl's three (denoiseToDevice, denoiseReadback, denoiseDisplay) with the estimate's
// parameters in a DenoiseSpatialRun.  What is left here: the parameter check, the defaults, hr_denoise_spatial_variance.

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
    DenoiseSpatialRun run{{}, false};
    const int rc = denoiseSpatialCheckParams(c, sparams, &run.p);
    return rc ? rc : denoiseToDevice(c, dparams, &run, device_out, stream, passes, result);
}

int hr_denoise_spatial_readback(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, const float **rgba, int32_t *w, int32_t *h,
                                uint32_t *passes, hr_denoise_spatial_result *result)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "null output");
    DenoiseSpatialRun run{{}, false};
    const int rc = denoiseSpatialCheckParams(c, sparams, &run.p);
    return rc ? rc : denoiseReadback(c, dparams, &run, rgba, w, h, passes, result);
}

int hr_denoise_spatial_display(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, const hr_display_params *display, int32_t format,
                               void *device_out, uint32_t *passes_shown)
{
    ENTER(c);
    if (!display || !device_out) FAIL(c, HR_ERR_INVALID, "null argument");
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format (the denoised display has no progressive form)");
    DenoiseSpatialRun run{{}, false};
    const int rc = denoiseSpatialCheckParams(c, sparams, &run.p);
    return rc ? rc : denoiseDisplay(c, dparams, &run, display, format, device_out, passes_shown);
}

int hr_denoise_spatial_variance(hr_ctx *c, const hr_denoise_params *dparams, const hr_denoise_spatial_params *sparams, float *host_out, hr_denoise_spatial_result *result)
{
    ENTER(c);
    if (!host_out) FAIL(c, HR_ERR_INVALID, "null output");
    DenoiseSpatialRun run{{}, true};
    int rc = denoiseSpatialCheckParams(c, sparams, &run.p);
    if (rc == HR_OK) rc = denoiseRun(c, dparams, nullptr, nullptr, &run);
    if (rc) return rc;
    const size_t px = (size_t)c->W * c->H;
    std::vector<float> cv(px * 4); // (cv[1]: colour + variance; a call for inspection, not a hot path)
    HIP_TRY(c, hipMemcpyAsync(cv.data(), c->denoise.work + 4 * px, px * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, c->denoise.spatial.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < px; ++i) host_out[i] = cv[4 * i + 3];
    denoiseSpatialFill(c, result);
    return HR_OK;
}

} // extern "C"
