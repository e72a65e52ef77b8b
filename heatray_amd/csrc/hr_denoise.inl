// hr_denoise.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_denoise.h.  The kernels are in
// hr_denoise.hip; the buffers' life follows the AOV planes' (aovFreePlanes).

// Which kernel runs an iteration when the caller leaves the choice to the library: the LDS-tiled kernel for the steps it exists for
// (1 and 2), the plain one beyond (profiles/denoise_time.txt has the measurement).
static bool denoiseUseTiled(const hr_denoise_params &p, int step)
{
    if (p.kernel == HR_DENOISE_KERNEL_PLAIN) return false;
    return denoiseTiledHasStep(step);
}

static int denoiseCheckParams(hr_ctx *c, const hr_denoise_params *in, hr_denoise_params *p)
{
    if (in)
        *p = *in;
    else
        hr_denoise_default_params(p);
    if (p->iterations < 0 || p->iterations > HR_DENOISE_MAX_ITERATIONS)
        FAIL(c, HR_ERR_INVALID, "denoise: iterations = " + std::to_string(p->iterations) + " is outside 0 .. " + std::to_string(HR_DENOISE_MAX_ITERATIONS));
    if (p->normal_power < 0 || p->normal_power > HR_DENOISE_MAX_NORMAL_POWER)
        FAIL(c, HR_ERR_INVALID, "denoise: normal_power = " + std::to_string(p->normal_power) + " is outside 0 .. " + std::to_string(HR_DENOISE_MAX_NORMAL_POWER));
    if (!std::isfinite(p->sigma_l) || p->sigma_l < 0.0f) FAIL(c, HR_ERR_INVALID, "denoise: sigma_l must be finite and not negative");
    if (!std::isfinite(p->sigma_z) || p->sigma_z < 0.0f) FAIL(c, HR_ERR_INVALID, "denoise: sigma_z must be finite and not negative");
    if (p->kernel < HR_DENOISE_KERNEL_AUTO || p->kernel > HR_DENOISE_KERNEL_TILED) FAIL(c, HR_ERR_INVALID, "denoise: unknown kernel " + std::to_string(p->kernel));
    return HR_OK;
}

// both masks on, and the planes zeroed when the frame was: they hold the frame's passes
static int denoiseCheckPlanes(hr_ctx *c)
{
    const uint32_t both = HR_AOV_SURFACE | HR_AOV_MOMENTS;
    if ((c->aovMask & both) != both)
        FAIL(c, HR_ERR_INVALID, "denoise needs the AOV planes: hr_aov_enable(HR_AOV_SURFACE | HR_AOV_MOMENTS) before the frame's first pass (enabled mask: " +
                                    std::to_string(c->aovMask) + ")");
    if (c->aovZeroedAt != c->frameZeroedAt)
        FAIL(c, HR_ERR_INVALID, "denoise: the AOV planes were enabled after the frame's first pass and do not hold the frame's passes: hr_clear, or hr_aov_enable before rendering");
    return HR_OK;
}

static int denoiseEnsureBuffers(hr_ctx *c, bool needOut)
{
    const size_t px = (size_t)c->W * c->H;
    if (!c->dnWork) HIP_TRY(c, hipMalloc((void **)&c->dnWork, px * kDenoiseBytesPerPixel));
    if (needOut && !c->dnOut) HIP_TRY(c, hipMalloc((void **)&c->dnOut, px * 16));
    return HR_OK;
}

// hr_denoise_spatial.inl's calls: the spatial variance estimate of include/hrcore_denoise_spatial.h between Prepare and the first iteration
struct DenoiseSpatialRun {
    hr_denoise_spatial_params p; // checked by the caller
    bool varianceOnly;           // stop after the estimate: cv[1] holds its variance, no image is written
};

// Completes the passes, checks, and enqueues the filter on the ctx stream; the image goes to `out`, or to c->dnOut when out is null.
// Without `spatial` every launch is hr_denoise's.
static int denoiseRun(hr_ctx *c, const hr_denoise_params *params, float *out, uint32_t *passes, const DenoiseSpatialRun *spatial = nullptr)
{
    hr_denoise_params p;
    int rc = denoiseCheckParams(c, params, &p);
    if (rc) return rc;
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    uint32_t n = 0;
    const float *frame = nullptr;
    if (c->grp) {
        rc = denoiseCheckPlanes(c); // (the group's own mask: hr_aov_enable on the handle)
        if (rc == HR_OK) rc = groupAll(c, [](hr_ctx *m, int) { return denoiseCheckPlanes(m); });
        if (rc == HR_OK) rc = groupAssemble(c, true, &n, nullptr);
        for (int plane = 0; plane < 3 && rc == HR_OK; ++plane) rc = groupAovAssemble(c, plane, nullptr);
        if (rc) return rc;
        frame = c->fbInternal;
    } else {
        if (c->world > 1)
            FAIL(c, HR_ERR_INVALID, "denoise: a tile-sharded context (world > 1) holds only its own tiles and the filter reads across them: use a context group, which assembles the frame");
        rc = denoiseCheckPlanes(c);
        if (rc == HR_OK) rc = drainPipeline(c);
        if (rc == HR_OK) rc = overflowCheck(c);
        if (rc) return rc;
        n = (uint32_t)(c->nextResolveOrder - c->frameZeroedAt);
        frame = c->fb();
    }
    rc = denoiseEnsureBuffers(c, out == nullptr && !(spatial && spatial->varianceOnly));
    if (rc) return rc;
    if (spatial && !c->dnSpatialResult) HIP_TRY(c, hipMalloc((void **)&c->dnSpatialResult, kDenoiseSpatialResultWords * 8));
    if (spatial && !c->dnSpatialResultHost) HIP_TRY(c, hipHostMalloc((void **)&c->dnSpatialResultHost, kDenoiseSpatialResultWords * 8, hipHostMallocDefault));
    if (!out) out = c->dnOut;
    const size_t px = (size_t)c->W * c->H;
    DenoiseBufs b;
    b.cv[0] = c->dnWork, b.cv[1] = b.cv[0] + 4 * px, b.nd = b.cv[1] + 4 * px, b.ac = b.nd + 4 * px, b.grad = b.ac + 4 * px;
    launchDenoisePrepare(c->stream, c->W, c->H, frame, c->aovPlane[HR_AOV_PLANE_ALBEDO], c->aovPlane[HR_AOV_PLANE_NORMAL_DEPTH], c->aovPlane[HR_AOV_PLANE_MOMENTS], b);
    int first = 0; // the half of the ping-pong the iterations start from
    if (spatial) {
        HIP_TRY(c, hipMemsetAsync(c->dnSpatialResult, 0, kDenoiseSpatialResultWords * 8, c->stream));
        launchDenoiseSpatial(c->stream, c->W, c->H, frame, b, p, spatial->p, c->dnSpatialResult); // cv[0] -> cv[1]: the same colour, the estimated variance
        first = 1;
    }
    const int iterations = (spatial && spatial->varianceOnly) ? -1 : p.iterations;
    if (iterations == 0) launchDenoiseFinish(c->stream, c->W, c->H, b, out); // (reads cv[0]: the colour the estimate left as it was)
    for (int it = 0; it < iterations; ++it)
        launchDenoiseAtrous(c->stream, c->W, c->H, b, (it & 1) ^ first, 1 << it, p, denoiseUseTiled(p, 1 << it), it == iterations - 1 ? out : nullptr);
    HIP_TRY(c, hipGetLastError());
    if (passes) *passes = n;
    return HR_OK;
}

extern "C" {

uint32_t hr_denoise_api_version(void) { return HR_DENOISE_API_VERSION; }

void hr_denoise_default_params(hr_denoise_params *p)
{
    if (!p) return;
    *p = hr_denoise_params{};
    p->iterations = 5, p->normal_power = 7, p->sigma_l = 4.0f, p->sigma_z = 4.0f, p->kernel = HR_DENOISE_KERNEL_AUTO;
}

int hr_denoise(hr_ctx *c, const hr_denoise_params *params, void *device_out, void *stream, uint32_t *passes)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "null output");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (st == c->stream) return denoiseRun(c, params, (float *)device_out, passes);
    // a foreign stream: filter on the ctx stream into the ctx's image, copy out over there, and the ctx's next work behind the copy
    int rc = denoiseRun(c, params, nullptr, passes);
    if (rc) return rc;
    if (!c->evAov) HIP_TRY(c, hipEventCreateWithFlags(&c->evAov, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->evAov, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(st, c->evAov, 0));
    HIP_TRY(c, hipMemcpyAsync(device_out, c->dnOut, (size_t)c->W * c->H * 16, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipEventRecord(c->evAov, st));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evAov, 0));
    return HR_OK;
}

int hr_denoise_readback(hr_ctx *c, const hr_denoise_params *params, const float **rgba, int32_t *w, int32_t *h, uint32_t *passes)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "null output");
    int rc = denoiseRun(c, params, nullptr, passes);
    if (rc) return rc;
    const size_t bytes = (size_t)c->W * c->H * 16;
    if (c->dnPinnedBytes < bytes) {
        if (c->dnPinned) hipHostFree(c->dnPinned);
        c->dnPinned = nullptr, c->dnPinnedBytes = 0;
        HIP_TRY(c, hipHostMalloc((void **)&c->dnPinned, bytes, hipHostMallocDefault));
        c->dnPinnedBytes = bytes;
    }
    HIP_TRY(c, hipMemcpyAsync(c->dnPinned, c->dnOut, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *rgba = c->dnPinned;
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

int hr_denoise_display(hr_ctx *c, const hr_denoise_params *params, const hr_display_params *display, int32_t format, void *device_out, uint32_t *passes_shown)
{
    ENTER(c);
    if (!display || !device_out) FAIL(c, HR_ERR_INVALID, "null argument");
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format (the denoised display has no progressive form)");
    int rc = denoiseRun(c, params, nullptr, passes_shown);
    if (rc) return rc;
    FrameDev fr = c->frame; // (denoiseRun has refused world > 1: every pixel is this context's; a group's frame is rank 0 of 1)
    fr.fb = c->dnOut;
    launchDisplay(c->cfg(c->stream), fr, *display, format, device_out);
    HIP_TRY(c, hipGetLastError());
    return HR_OK;
}

} // extern "C"
