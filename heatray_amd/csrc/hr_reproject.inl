// hr_reproject.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_reproject.h.  The kernels are in
// hr_reproject.hip, the per-pixel arithmetic in hr_reproject.h; the parameter, camera and frame checks are hr_history.inl's.
//
// Ordering: as in hr_history.inl.  Both kernels run on the context's stream after drainPipeline, which also makes each pipeline group's
// next step wait for that stream; the next resolve is enqueued behind them there.
#include "hr_reproject.h"

// what merge and preview ask before they launch: parameters, camera, frame (drains the pipeline), a history; the buffers of the counters
static int reprojectPrepare(hr_ctx *c, const char *what, const hr_pass_params *camera, const hr_history_params *params, hr_history_params *p, uint32_t *passes)
{
    int rc = historyCheckParams(c, params, p);
    if (rc == HR_OK) rc = historyCheckCamera(c, camera);
    if (rc) return rc;
    rc = historyCheckFrame(c, what, passes);
    if (rc) return rc;
    if (!c->history.captured) FAIL(c, HR_ERR_INVALID, std::string(what) + ": no captured history (hr_history_capture; hr_frame_resize and hr_history_drop remove it)");
    HIP_TRY(c, c->reproject.result.ensure(kReprojectResultWords));
    return HR_OK;
}

// the preview's counters, fetched and waited for, -> its result (null: nobody asked)
static void previewFill(const hr_ctx *c, hr_reproject_preview_result *out)
{
    if (!out) return;
    *out = hr_reproject_preview_result{};
    out->own_pixels = c->reproject.result.host[0], out->previewed_pixels = c->reproject.result.host[1], out->empty_pixels = c->reproject.result.host[2];
}

// Checks, and enqueues the preview on the ctx stream; the image goes to `dst`, or to c->reproject.out when dst is null.  With `out` it waits.
static int previewRun(hr_ctx *c, const hr_pass_params *camera, const hr_history_params *params, float *dst, hr_reproject_preview_result *out)
{
    hr_history_params p;
    uint32_t n = 0;
    int rc = reprojectPrepare(c, "reproject preview", camera, params, &p, &n);
    if (rc) return rc;
    if (!dst) {
        if (!c->reproject.out) HIP_TRY(c, c->reproject.out.alloc((size_t)c->W * c->H * 4));
        dst = c->reproject.out;
    }
    const HsLaunch l = historyLaunch(c, camera, p);
    HIP_TRY(c, c->reproject.result.zero(c->stream));
    launchReprojectPreview(c->stream, c->W, c->H, l.cam, l.P, c->history.hist, c->fb(), c->aov.plane[HR_AOV_PLANE_ALBEDO], c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH], dst, c->reproject.result.dev);
    HIP_TRY(c, hipGetLastError());
    if (out) {
        HIP_TRY(c, c->reproject.result.fetch(c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        previewFill(c, out);
    }
    return HR_OK;
}

extern "C" {

uint32_t hr_reproject_api_version(void) { return HR_REPROJECT_API_VERSION; }

int hr_reproject_merge(hr_ctx *c, const hr_pass_params *camera, const hr_history_params *params, hr_reproject_result *out)
{
    ENTER(c);
    hr_history_params p;
    uint32_t n = 0;
    int rc = reprojectPrepare(c, "reproject merge", camera, params, &p, &n);
    if (rc) return rc;
    if (c->history.merged && !c->reproject.merged)
        FAIL(c, HR_ERR_INVALID, "reproject merge: hr_history_merge has already merged the history into this frame (a progressive merge would count it twice): hr_clear first");
    const size_t words = rpExaminedWords(c->W, c->H);
    if (!c->reproject.examined) {
        HIP_TRY(c, c->reproject.examined.alloc(words));
        c->reproject.stale = true;
    }
    if (c->reproject.stale) HIP_TRY(c, hipMemsetAsync(c->reproject.examined, 0, words * 8, c->stream));
    c->reproject.stale = false;
    const HsLaunch l = historyLaunch(c, camera, p);
    HIP_TRY(c, c->reproject.result.zero(c->stream));
    launchReprojectMerge(c->stream, c->W, c->H, l.cam, l.P, c->history.hist, c->fb(), c->aov.plane[HR_AOV_PLANE_ALBEDO], c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH],
                         c->aov.plane[HR_AOV_PLANE_MOMENTS], c->reproject.examined, c->reproject.result.dev);
    HIP_TRY(c, hipGetLastError());
    c->history.merged = c->reproject.merged = true;
    c->snapshotEpoch++; // (progressive snapshots taken before the merge are not handed out any more)
    HIP_TRY(c, c->reproject.result.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out) {
        *out = hr_reproject_result{};
        out->reused_pixels = c->reproject.result.host[0], out->rejected_pixels = c->reproject.result.host[1], out->history_samples = c->reproject.result.host[2];
        out->pending_pixels = c->reproject.result.host[3], out->examined_pixels = c->reproject.result.host[4];
        out->history_passes = c->history.passes, out->passes = n;
    }
    return HR_OK;
}

int hr_reproject_examined_get(hr_ctx *c, uint8_t *host_out)
{
    ENTER(c);
    if (!host_out) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->grp) FAIL(c, HR_ERR_INVALID, "reproject: a context group is not supported");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    const size_t px = (size_t)c->W * c->H;
    std::memset(host_out, 0, px);
    if (!c->reproject.examined || c->reproject.stale) return HR_OK; // (no pixel of this frame has been examined)
    std::vector<unsigned long long> words(rpExaminedWords(c->W, c->H));
    HIP_TRY(c, hipMemcpyAsync(words.data(), c->reproject.examined, words.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int blocksX = (c->W + 7) / 8;
    for (int y = 0; y < c->H; ++y)
        for (int x = 0; x < c->W; ++x) host_out[(size_t)y * c->W + x] = (uint8_t)((words[(size_t)(y >> 3) * blocksX + (x >> 3)] >> ((y & 7) * 8 + (x & 7))) & 1ull);
    return HR_OK;
}

int hr_reproject_preview(hr_ctx *c, const hr_pass_params *camera, const hr_history_params *params, void *device_out, void *stream, hr_reproject_preview_result *out)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "null output");
    if (!stream || (hipStream_t)stream == c->stream) return previewRun(c, camera, params, (float *)device_out, out);
    // a foreign stream: the kernel on the ctx stream into the ctx's image, and the copy out over there
    int rc = previewRun(c, camera, params, nullptr, out);
    if (rc) return rc;
    return copyOutOnStream(c, device_out, c->reproject.out, (size_t)c->W * c->H * 16, stream);
}

int hr_reproject_preview_readback(hr_ctx *c, const hr_pass_params *camera, const hr_history_params *params, const float **rgba, int32_t *w, int32_t *h,
                                  hr_reproject_preview_result *out)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "null output");
    int rc = previewRun(c, camera, params, nullptr, nullptr);
    if (rc) return rc;
    const size_t bytes = (size_t)c->W * c->H * 16;
    rc = growPinned(c, c->reproject.pinned, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->reproject.pinned.get(), c->reproject.out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, c->reproject.result.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (one wait for the image and the counters)
    previewFill(c, out);
    *rgba = c->reproject.pinned.get();
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

} // extern "C"
