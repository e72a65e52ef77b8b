// hr_despeckle.inl — a section of hr_core.hip (included at its end, after hr_denoise_spatial.inl): the entry points of
// include/hrcore_despeckle.h.  The kernel is in hr_despeckle.hip, the arithmetic in hr_despeckle.h.  The _denoise entries hand the
// despeckled pair to hr_denoise.inl's calls as a DenoiseSource: the denoiser's launches are its own.
//
// Ordering: the counters' zeroing, the kernel and every launch behind it run on the context's stream, behind the resolves (or a group's
// gather) enqueued there; a caller's stream only ever sees copies of the context's planes (copyOutOnStream).

static int despeckleCheckParams(hr_ctx *c, const hr_despeckle_params *in, hr_despeckle_params *p)
{
    if (in)
        *p = *in;
    else
        hr_despeckle_default_params(p);
    if (p->rank < 1 || p->rank > HR_DESPECKLE_RANK_HIGHEST)
        FAIL(c, HR_ERR_INVALID, "despeckle: rank = " + std::to_string(p->rank) + " is outside 1 .. " + std::to_string(HR_DESPECKLE_RANK_HIGHEST));
    if (p->min_taps < p->rank || p->min_taps > HR_DESPECKLE_TAPS)
        FAIL(c, HR_ERR_INVALID, "despeckle: min_taps = " + std::to_string(p->min_taps) + " is outside rank .. " + std::to_string(HR_DESPECKLE_TAPS));
    if (!std::isfinite(p->ratio) || p->ratio < 1.0f) FAIL(c, HR_ERR_INVALID, "despeckle: ratio must be finite and at least 1");
    if (!std::isfinite(p->sigmas) || p->sigmas < 0.0f) FAIL(c, HR_ERR_INVALID, "despeckle: sigmas must be finite and not negative");
    if (!std::isfinite(p->floor) || p->floor < 0.0f) FAIL(c, HR_ERR_INVALID, "despeckle: floor must be finite and not negative");
    for (int k = 0; k < 3; ++k)
        if (p->reserved[k]) FAIL(c, HR_ERR_INVALID, "despeckle: reserved[" + std::to_string(k) + "] must be 0");
    return HR_OK;
}

// the one place that reads the host words: the counters, fetched and waited for, -> the result (null: nobody asked)
static void despeckleFill(const hr_ctx *c, hr_despeckle_result *out)
{
    if (!out) return;
    *out = hr_despeckle_result{};
    for (int s = 0; s < kDespeckleSlots; ++s) { // (the workgroups' adds are spread over copies of the counters: hr_kernels.h)
        const unsigned long long *h = c->despeckle.result.host + (size_t)s * kDespeckleSlotStride;
        out->valid_pixels += h[0], out->clamped_pixels += h[1], out->kept_pixels += h[2], out->starved_pixels += h[3], out->nonfinite_pixels += h[4];
    }
}

static int despeckleEnsurePlanes(hr_ctx *c)
{
    if (!c->despeckle.planes) HIP_TRY(c, c->despeckle.planes.alloc((size_t)c->W * c->H * 8));
    return HR_OK;
}
static float *despeckleMomentsPlane(const hr_ctx *c) { return c->despeckle.planes + (size_t)c->W * c->H * 4; }

// the kernel over a ready pair, on the ctx stream; with `fetch` the counters' copy to the host is enqueued behind it (the caller waits)
static int despeckleLaunch(hr_ctx *c, const hr_despeckle_params &p, const float *frame, const float *moments, float *out, float *momentsOut, bool fetch)
{
    HIP_TRY(c, c->despeckle.result.ensure(kDespeckleResultWords));
    HIP_TRY(c, c->despeckle.result.zero(c->stream));
    launchDespeckle(c->stream, c->W, c->H, frame, moments, p, out, momentsOut, c->despeckle.result.dev);
    HIP_TRY(c, hipGetLastError());
    if (fetch) HIP_TRY(c, c->despeckle.result.fetch(c->stream));
    return HR_OK;
}

// The ctx's own frame and MOMENTS plane (and, for the _denoise entries, the surface planes: `aov`) -> out and momentsOut, or, with out
// null, the ctx's despeckled planes.  (hr_despeckle has refused a caller's output that is the frame or the plane itself.)
static int despeckleOwnFrame(hr_ctx *c, const hr_despeckle_params &p, uint32_t aov, bool fetch, float *out, float *momentsOut, uint32_t *passes)
{
    const bool surface = (aov & HR_AOV_SURFACE) != 0;
    const FrameNeed need{aov, "despeckle", "the clamp", true, false,
                         surface ? std::string("despeckle") + kNeedsAovPlanes : std::string("despeckle needs the sample moments: hr_aov_enable(HR_AOV_MOMENTS)"),
                         surface ? std::string("despeckle") + kAovPlanesLate : std::string("despeckle: the MOMENTS plane was enabled after the frame's first pass and does not hold")};
    const float *frame = nullptr;
    int rc = frameReady(c, need, &frame, passes);
    if (rc) return rc;
    const float *moments = c->aov.plane[HR_AOV_PLANE_MOMENTS];
    if (!out) {
        rc = despeckleEnsurePlanes(c);
        if (rc) return rc;
        out = c->despeckle.planes, momentsOut = despeckleMomentsPlane(c);
    }
    return despeckleLaunch(c, p, frame, moments, out, momentsOut, fetch);
}

// the checks the two _denoise entries share, then the despeckled pair of the ctx's frame as the denoiser's source
static int despeckleDenoiseSource(hr_ctx *c, const hr_despeckle_params *params, const hr_denoise_params *dparams, int32_t spatial, const hr_denoise_spatial_params *sparams,
                                  bool fetch, DenoiseSpatialRun *run, DenoiseSource *source)
{
    hr_despeckle_params p;
    hr_denoise_params dp;
    int rc = despeckleCheckParams(c, params, &p);
    if (rc == HR_OK) rc = denoiseCheckParams(c, dparams, &dp); // (denoiseRun asks again: here so that every parameter is judged before the context is)
    if (rc == HR_OK && spatial) rc = denoiseSpatialCheckParams(c, sparams, &run->p);
    if (rc) return rc;
    run->varianceOnly = false;
    uint32_t n = 0;
    rc = despeckleOwnFrame(c, p, HR_AOV_SURFACE | HR_AOV_MOMENTS, fetch, nullptr, nullptr, &n);
    if (rc) return rc;
    *source = DenoiseSource{c->despeckle.planes, despeckleMomentsPlane(c), n};
    return HR_OK;
}

extern "C" {

uint32_t hr_despeckle_api_version(void) { return HR_DESPECKLE_API_VERSION; }

void hr_despeckle_default_params(hr_despeckle_params *p)
{
    if (!p) return;
    *p = hr_despeckle_params{};
    p->rank = 2, p->min_taps = 8, p->ratio = 2.0f, p->sigmas = 3.0f, p->floor = 0.0f;
}

int hr_despeckle(hr_ctx *c, const hr_despeckle_params *params, const void *device_frame, const void *device_moments, void *device_out, void *device_moments_out,
                 void *stream, uint32_t *passes, hr_despeckle_result *result)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "despeckle: null output");
    if ((device_frame == nullptr) != (device_moments == nullptr))
        FAIL(c, HR_ERR_INVALID, std::string("despeckle: device_frame and device_moments go together, and ") + (device_frame ? "device_moments" : "device_frame") + " is null");
    if (device_out == device_moments_out) FAIL(c, HR_ERR_INVALID, "despeckle: device_out and device_moments_out are the same memory");
    // the inputs as the kernel will read them (the ctx's own: null while there is no frame or no plane, which no output equals)
    const void *inFrame = device_frame ? device_frame : (c->grp ? c->fbInternal : c->fb()), *inMoments = device_frame ? device_moments : c->aov.plane[HR_AOV_PLANE_MOMENTS];
    if (device_out == inFrame || device_out == inMoments) FAIL(c, HR_ERR_INVALID, "despeckle: device_out is one of the inputs (the kernel reads neighbours)");
    if (device_moments_out && (device_moments_out == inFrame || device_moments_out == inMoments))
        FAIL(c, HR_ERR_INVALID, "despeckle: device_moments_out is one of the inputs (the kernel reads neighbours)");
    hr_despeckle_params p;
    int rc = despeckleCheckParams(c, params, &p);
    if (rc) return rc;
    // a foreign stream: the kernel runs on the ctx stream into the ctx's planes, and they are copied out over there
    const bool foreign = stream && (hipStream_t)stream != c->stream;
    float *out = foreign ? nullptr : (float *)device_out, *momentsOut = foreign ? nullptr : (float *)device_moments_out;
    uint32_t n = 0;
    if (device_frame) {
        const FrameNeed need{0, "despeckle", "the clamp", true, false, "", ""};
        rc = frameKindReady(c, need);
        if (rc == HR_OK && foreign) rc = despeckleEnsurePlanes(c);
        if (rc) return rc;
        if (foreign) out = c->despeckle.planes, momentsOut = despeckleMomentsPlane(c);
        rc = despeckleLaunch(c, p, (const float *)device_frame, (const float *)device_moments, out, momentsOut, result != nullptr);
    } else {
        rc = despeckleOwnFrame(c, p, HR_AOV_MOMENTS, result != nullptr, out, momentsOut, &n);
    }
    if (rc) return rc;
    if (foreign) {
        const size_t bytes = (size_t)c->W * c->H * 16;
        rc = copyOutOnStream(c, device_out, c->despeckle.planes, bytes, stream);
        if (rc == HR_OK && device_moments_out) rc = copyOutOnStream(c, device_moments_out, despeckleMomentsPlane(c), bytes, stream);
        if (rc) return rc;
    }
    if (result) { // (a result asked for: the call waits for the kernel)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        despeckleFill(c, result);
    }
    if (passes) *passes = n;
    return HR_OK;
}

int hr_despeckle_readback(hr_ctx *c, const hr_despeckle_params *params, const float **rgba, const float **moments, int32_t *w, int32_t *h, uint32_t *passes,
                          hr_despeckle_result *result)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "despeckle: null output");
    hr_despeckle_params p;
    int rc = despeckleCheckParams(c, params, &p);
    uint32_t n = 0;
    if (rc == HR_OK) rc = despeckleOwnFrame(c, p, HR_AOV_MOMENTS, true, nullptr, nullptr, &n);
    const size_t bytes = (size_t)c->W * c->H * 16;
    if (rc == HR_OK) rc = growPinned(c, c->despeckle.pinned, 2 * bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->despeckle.pinned.get(), c->despeckle.planes, moments ? 2 * bytes : bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (one wait for the images and the counters)
    despeckleFill(c, result);
    *rgba = c->despeckle.pinned.get();
    if (moments) *moments = c->despeckle.pinned.get() + bytes / sizeof(float);
    if (w) *w = c->W;
    if (h) *h = c->H;
    if (passes) *passes = n;
    return HR_OK;
}

int hr_despeckle_denoise(hr_ctx *c, const hr_despeckle_params *params, const hr_denoise_params *dparams, int32_t spatial, const hr_denoise_spatial_params *sparams,
                         void *device_out, void *stream, uint32_t *passes, hr_despeckle_result *result)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "despeckle: null output");
    DenoiseSpatialRun run{{}, false};
    DenoiseSource source{};
    int rc = despeckleDenoiseSource(c, params, dparams, spatial, sparams, result != nullptr, &run, &source);
    if (rc == HR_OK) rc = denoiseToDevice(c, dparams, spatial ? &run : nullptr, device_out, stream, passes, nullptr, &source);
    if (rc || !result) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a result asked for: the call waits for the kernels)
    despeckleFill(c, result);
    return HR_OK;
}

int hr_despeckle_denoise_readback(hr_ctx *c, const hr_despeckle_params *params, const hr_denoise_params *dparams, int32_t spatial, const hr_denoise_spatial_params *sparams,
                                  const float **rgba, int32_t *w, int32_t *h, uint32_t *passes, hr_despeckle_result *result)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "despeckle: null output");
    DenoiseSpatialRun run{{}, false};
    DenoiseSource source{};
    int rc = despeckleDenoiseSource(c, params, dparams, spatial, sparams, true, &run, &source);
    if (rc == HR_OK) rc = denoiseReadback(c, dparams, spatial ? &run : nullptr, rgba, w, h, passes, nullptr, &source); // (its wait covers the counters' copy)
    if (rc) return rc;
    despeckleFill(c, result);
    return HR_OK;
}

} // extern "C"
