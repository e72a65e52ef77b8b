// hr_denoise.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_denoise.h.  The kernels are in
// hr_denoise.hip; the buffers' life follows the AOV planes' (featuresPlanesGone).  The calls of include/hrcore_denoise_spatial.h run through
// the same three functions (denoiseToDevice, denoiseReadback, denoiseDisplay) with a DenoiseSpatialRun.

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

static int denoiseEnsureBuffers(hr_ctx *c, bool needOut)
{
    const size_t px = (size_t)c->W * c->H;
    if (!c->denoise.work) HIP_TRY(c, c->denoise.work.alloc(px * kDenoiseBytesPerPixel / sizeof(float)));
    if (needOut && !c->denoise.out) HIP_TRY(c, c->denoise.out.alloc(px * 4));
    return HR_OK;
}

// hr_denoise_spatial.inl's calls: the spatial variance estimate of include/hrcore_denoise_spatial.h between Prepare and the first iteration
struct DenoiseSpatialRun {
    hr_denoise_spatial_params p; // checked by the caller
    bool varianceOnly;           // stop after the estimate: cv[1] holds its variance, no image is written
};

// hr_despeckle.inl's calls: a pair that stands in for the frame and its MOMENTS plane, made on the ctx stream from the frame that the
// caller's own frameReady (with the denoiser's need) has completed; ALBEDO and NORMAL_DEPTH stay the ctx's planes
struct DenoiseSource {
    const float *frame, *moments; // W x H float4 each, accumulation format, the frame's sample counts
    uint32_t passes;              // what that frameReady gave
};

// Completes the passes, checks, and enqueues the filter on the ctx stream; the image goes to `out`, or to c->denoise.out when out is null.
// Without `spatial` every launch is hr_denoise's.  With `source` the two launches that read the frame and the MOMENTS plane (Prepare
// and the spatial estimate) read the pair instead; without it every launch and their order are as they were.
static int denoiseRun(hr_ctx *c, const hr_denoise_params *params, float *out, uint32_t *passes, const DenoiseSpatialRun *spatial = nullptr,
                      const DenoiseSource *source = nullptr)
{
    hr_denoise_params p;
    int rc = denoiseCheckParams(c, params, &p);
    if (rc) return rc;
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame"); // (asked first: a sharded context without a frame hears this, not frameReady's refusal)
    uint32_t n = 0;
    const float *frame = nullptr, *moments = nullptr;
    if (source) {
        frame = source->frame, moments = source->moments, n = source->passes;
    } else {
        const FrameNeed need{HR_AOV_SURFACE | HR_AOV_MOMENTS, "denoise", "the filter", true, false, std::string("denoise") + kNeedsAovPlanes, std::string("denoise") + kAovPlanesLate};
        rc = frameReady(c, need, &frame, &n);
        if (rc) return rc;
        moments = c->aov.plane[HR_AOV_PLANE_MOMENTS];
    }
    rc = denoiseEnsureBuffers(c, out == nullptr && !(spatial && spatial->varianceOnly));
    if (rc) return rc;
    if (spatial) HIP_TRY(c, c->denoise.spatial.ensure(kDenoiseSpatialResultWords));
    if (!out) out = c->denoise.out;
    const size_t px = (size_t)c->W * c->H;
    DenoiseBufs b;
    b.cv[0] = c->denoise.work, b.cv[1] = b.cv[0] + 4 * px, b.nd = b.cv[1] + 4 * px, b.ac = b.nd + 4 * px, b.grad = b.ac + 4 * px;
    launchDenoisePrepare(c->stream, c->W, c->H, frame, c->aov.plane[HR_AOV_PLANE_ALBEDO], c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH], moments, b);
    int first = 0; // the half of the ping-pong the iterations start from
    if (spatial) {
        HIP_TRY(c, c->denoise.spatial.zero(c->stream));
        launchDenoiseSpatial(c->stream, c->W, c->H, frame, b, p, spatial->p, c->denoise.spatial.dev); // cv[0] -> cv[1]: the same colour, the estimated variance
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

// the estimate's counters, fetched and waited for, -> its result (null: nobody asked)
static void denoiseSpatialFill(const hr_ctx *c, hr_denoise_spatial_result *out)
{
    if (!out) return;
    *out = hr_denoise_spatial_result{};
    out->spatial_pixels = c->denoise.spatial.host[0], out->estimated_pixels = c->denoise.spatial.host[1], out->starved_pixels = c->denoise.spatial.host[2];
}

// The three calls of include/hrcore_denoise.h behind their argument checks.  hr_denoise_spatial.inl's calls are the same with `spatial`
// (and a `result` to fetch); without it every launch, and their order, is the plain call's.  hr_despeckle.inl's calls bring a `source`.
static int denoiseToDevice(hr_ctx *c, const hr_denoise_params *params, const DenoiseSpatialRun *spatial, void *device_out, void *stream, uint32_t *passes,
                           hr_denoise_spatial_result *result, const DenoiseSource *source = nullptr)
{
    // a foreign stream: filter on the ctx stream into the ctx's image, and copy out over there
    const bool foreign = stream && (hipStream_t)stream != c->stream;
    int rc = denoiseRun(c, params, foreign ? nullptr : (float *)device_out, passes, spatial, source);
    if (rc == HR_OK && result) { // (a result asked for: the call waits for the kernels)
        HIP_TRY(c, c->denoise.spatial.fetch(c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        denoiseSpatialFill(c, result);
    }
    if (rc || !foreign) return rc;
    return copyOutOnStream(c, device_out, c->denoise.out, (size_t)c->W * c->H * 16, stream);
}

static int denoiseReadback(hr_ctx *c, const hr_denoise_params *params, const DenoiseSpatialRun *spatial, const float **rgba, int32_t *w, int32_t *h, uint32_t *passes,
                           hr_denoise_spatial_result *result, const DenoiseSource *source = nullptr)
{
    int rc = denoiseRun(c, params, nullptr, passes, spatial, source);
    const size_t bytes = (size_t)c->W * c->H * 16;
    if (rc == HR_OK) rc = growPinned(c, c->denoise.pinned, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->denoise.pinned.get(), c->denoise.out, bytes, hipMemcpyDeviceToHost, c->stream));
    if (spatial) HIP_TRY(c, c->denoise.spatial.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (one wait for the image and the counters)
    denoiseSpatialFill(c, result);
    *rgba = c->denoise.pinned.get();
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

static int denoiseDisplay(hr_ctx *c, const hr_denoise_params *params, const DenoiseSpatialRun *spatial, const hr_display_params *display, int32_t format, void *device_out,
                          uint32_t *passes_shown)
{
    int rc = denoiseRun(c, params, nullptr, passes_shown, spatial);
    if (rc) return rc;
    FrameDev fr = c->frame; // (denoiseRun has refused world > 1: every pixel is this context's; a group's frame is rank 0 of 1)
    fr.fb = c->denoise.out;
    launchDisplay(c->cfg(c->stream), fr, *display, format, device_out);
    HIP_TRY(c, hipGetLastError());
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
    return denoiseToDevice(c, params, nullptr, device_out, stream, passes, nullptr);
}

int hr_denoise_readback(hr_ctx *c, const hr_denoise_params *params, const float **rgba, int32_t *w, int32_t *h, uint32_t *passes)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "null output");
    return denoiseReadback(c, params, nullptr, rgba, w, h, passes, nullptr);
}

int hr_denoise_display(hr_ctx *c, const hr_denoise_params *params, const hr_display_params *display, int32_t format, void *device_out, uint32_t *passes_shown)
{
    ENTER(c);
    if (!display || !device_out) FAIL(c, HR_ERR_INVALID, "null argument");
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format (the denoised display has no progressive form)");
    return denoiseDisplay(c, params, nullptr, display, format, device_out, passes_shown);
}

} // extern "C"
