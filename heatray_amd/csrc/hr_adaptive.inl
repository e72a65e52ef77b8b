// hr_adaptive.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_adaptive.h.  The kernels are in
// hr_adaptive.hip; cameraLane (hr_raygen.hip) reads the mask through FrameDev::mask.
//
// Ordering.  The mask words are rewritten in place on the context's stream after drainPipeline: every enqueued pass has been given its
// resolve there by then, and a resolve waits for its pass's last stage, so the write comes after every ray generation that read the
// old words; drainPipeline also makes each pipeline group's next step wait for the context's stream (needUserSync), so the next ray
// generation comes after the write.  The calls below do wait for the stream — the caller's bytes are pageable host memory, an update's
// result goes back to the host — but the mask's ordering against the passes does not rest on that.

static int adaptiveCheckParams(hr_ctx *c, const hr_adaptive_params *in, hr_adaptive_params *p)
{
    if (in)
        *p = *in;
    else
        hr_adaptive_default_params(p);
    if (!std::isfinite(p->threshold) || !(p->threshold > 0.0f)) FAIL(c, HR_ERR_INVALID, "adaptive: threshold must be finite and greater than 0");
    if (!std::isfinite(p->floor) || !(p->floor > 0.0f)) FAIL(c, HR_ERR_INVALID, "adaptive: floor must be finite and greater than 0");
    if (p->min_samples < HR_ADAPTIVE_MIN_SAMPLES_LOWEST || p->min_samples > HR_ADAPTIVE_MIN_SAMPLES_HIGHEST)
        FAIL(c, HR_ERR_INVALID, "adaptive: min_samples = " + std::to_string(p->min_samples) + " is outside " + std::to_string(HR_ADAPTIVE_MIN_SAMPLES_LOWEST) + " .. " +
                                    std::to_string(HR_ADAPTIVE_MIN_SAMPLES_HIGHEST));
    if (p->radius < 0 || p->radius > HR_ADAPTIVE_MAX_RADIUS)
        FAIL(c, HR_ERR_INVALID, "adaptive: radius = " + std::to_string(p->radius) + " is outside 0 .. " + std::to_string(HR_ADAPTIVE_MAX_RADIUS));
    return HR_OK;
}

static int sampleMaskEnsure(hr_ctx *c, bool bytesToo)
{
    if (!c->adaptive.maskWords) HIP_TRY(c, c->adaptive.maskWords.alloc(sampleMaskWords(c->W, c->H)));
    if (bytesToo && !c->adaptive.maskBytes) HIP_TRY(c, c->adaptive.maskBytes.alloc((size_t)c->W * c->H));
    return HR_OK;
}

// a plain context: the byte mask (host memory) -> its words, installed; null removes the mask
static int sampleMaskSetPlain(hr_ctx *c, const uint8_t *mask)
{
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    int rc = drainPipeline(c);
    if (rc) return rc;
    if (!mask) {
        c->frame.mask = nullptr;
        return HR_OK;
    }
    rc = sampleMaskEnsure(c, true);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->adaptive.maskBytes, mask, (size_t)c->W * c->H, hipMemcpyHostToDevice, c->stream));
    launchMaskPack(c->stream, c->W, c->H, c->adaptive.maskBytes, c->adaptive.maskWords);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the caller's bytes are pageable host memory: read before the call returns)
    c->frame.mask = c->adaptive.maskWords;
    return HR_OK;
}

// a context group: the words on the group's first device (complete: its stream was synchronised) -> every member, installed there
static int groupSampleMaskDistribute(hr_ctx *c)
{
    const uint32_t *src = c->adaptive.maskWords;
    const int dev0 = c->device;
    const size_t bytes = sampleMaskWords(c->W, c->H) * 4;
    return groupAll(c, [=](hr_ctx *m, int) {
        int rc = drainPipeline(m);
        if (rc == HR_OK) rc = sampleMaskEnsure(m, false);
        if (rc) return rc;
        HIP_TRY(m, hipMemcpyPeerAsync(m->adaptive.maskWords, m->device, src, dev0, bytes, m->stream));
        HIP_TRY(m, hipStreamSynchronize(m->stream)); // (the source is the group's buffer, which its next call may rewrite)
        m->frame.mask = m->adaptive.maskWords;
        return HR_OK;
    });
}

static int groupSampleMaskSet(hr_ctx *c, const uint8_t *mask)
{
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    if (!mask) {
        const int rc = groupAll(c, [](hr_ctx *m, int) { return sampleMaskSetPlain(m, nullptr); });
        if (rc) return rc;
        c->frame.mask = nullptr;
        return HR_OK;
    }
    int rc = sampleMaskEnsure(c, true);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->adaptive.maskBytes, mask, (size_t)c->W * c->H, hipMemcpyHostToDevice, c->stream));
    launchMaskPack(c->stream, c->W, c->H, c->adaptive.maskBytes, c->adaptive.maskWords);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = groupSampleMaskDistribute(c);
    if (rc) return rc;
    c->frame.mask = c->adaptive.maskWords;
    return HR_OK;
}

extern "C" {

uint32_t hr_adaptive_api_version(void) { return HR_ADAPTIVE_API_VERSION; }

void hr_adaptive_default_params(hr_adaptive_params *p)
{
    if (!p) return;
    *p = hr_adaptive_params{};
    p->threshold = 0.02f, p->floor = 0.05f, p->min_samples = 16, p->radius = 2;
}

int hr_sample_mask_set(hr_ctx *c, const uint8_t *mask)
{
    ENTER(c);
    return c->grp ? groupSampleMaskSet(c, mask) : sampleMaskSetPlain(c, mask);
}

int hr_sample_mask_get(hr_ctx *c, uint8_t *out, int32_t *installed)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    if (installed) *installed = c->frame.mask ? 1 : 0;
    const size_t px = (size_t)c->W * c->H;
    if (!c->frame.mask) {
        std::memset(out, 1, px);
        return HR_OK;
    }
    const int rc = sampleMaskEnsure(c, true);
    if (rc) return rc;
    launchMaskUnpack(c->stream, c->W, c->H, c->frame.mask, c->adaptive.maskBytes); // (a group's handle holds the copy its members were sent)
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, c->adaptive.maskBytes, px, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HR_OK;
}

int hr_adaptive_update(hr_ctx *c, const hr_adaptive_params *params, int32_t install, hr_adaptive_result *out)
{
    ENTER(c);
    hr_adaptive_params p;
    int rc = adaptiveCheckParams(c, params, &p);
    if (rc) return rc;
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame"); // (asked first: a sharded context without a frame hears this, not frameReady's refusal)
    uint32_t n = 0;
    const float *frame = nullptr;
    const FrameNeed need{HR_AOV_MOMENTS, "adaptive", "the mask's dilation", true, false, "adaptive sampling needs the sample moments: hr_aov_enable(HR_AOV_MOMENTS)",
                         "adaptive: the MOMENTS plane was enabled after the frame's first pass and does not hold"};
    rc = frameReady(c, need, &frame, &n);
    if (rc) return rc;
    const size_t px = (size_t)c->W * c->H, maskBytes = sampleMaskWords(c->W, c->H) * 4;
    if (!c->adaptive.error) HIP_TRY(c, c->adaptive.error.alloc(px));
    if (!c->adaptive.builtWords) HIP_TRY(c, c->adaptive.builtWords.alloc(maskBytes / 4));
    HIP_TRY(c, c->adaptive.result.ensure(kAdaptiveResultWords));
    if (install) {
        rc = sampleMaskEnsure(c, false);
        if (rc) return rc;
    }
    HIP_TRY(c, c->adaptive.result.zero(c->stream));
    launchAdaptiveError(c->stream, c->W, c->H, frame, c->aov.plane[HR_AOV_PLANE_MOMENTS], p, c->adaptive.error);
    launchAdaptiveMask(c->stream, c->W, c->H, c->adaptive.error, p, c->adaptive.builtWords, c->adaptive.result.dev);
    HIP_TRY(c, hipGetLastError());
    c->adaptive.errorValid = true;
    if (install) HIP_TRY(c, hipMemcpyAsync(c->adaptive.maskWords, c->adaptive.builtWords, maskBytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, c->adaptive.result.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (install) {
        if (c->grp) {
            rc = groupSampleMaskDistribute(c);
            if (rc) return rc;
        }
        c->frame.mask = c->adaptive.maskWords;
    }
    if (out) {
        *out = hr_adaptive_result{};
        out->unconverged_pixels = c->adaptive.result.host[0], out->active_pixels = c->adaptive.result.host[1];
        std::memcpy(&out->max_error, &c->adaptive.result.host[2], 4);
        out->passes = n;
    }
    return HR_OK;
}

int hr_adaptive_error_copy(hr_ctx *c, void *device_out, void *stream)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    if (!c->adaptive.errorValid) FAIL(c, HR_ERR_INVALID, "adaptive: no error map: hr_adaptive_update has not run since the frame was last resized");
    return copyOutOnStream(c, device_out, c->adaptive.error, (size_t)c->W * c->H * sizeof(float), stream); // (the next update rewrites the map: behind the copy)
}

int hr_adaptive_error_readback(hr_ctx *c, float *host_out)
{
    ENTER(c);
    if (!host_out) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    if (!c->adaptive.errorValid) FAIL(c, HR_ERR_INVALID, "adaptive: no error map: hr_adaptive_update has not run since the frame was last resized");
    HIP_TRY(c, hipMemcpyAsync(host_out, c->adaptive.error, (size_t)c->W * c->H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HR_OK;
}

} // extern "C"
