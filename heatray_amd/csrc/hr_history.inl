// hr_history.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_history.h.  The kernels are in
// hr_history.hip, the per-pixel arithmetic and the two cameras' arithmetic (hsCameras) in hr_history.h.
//
// Ordering.  Both kernels run on the context's stream after drainPipeline: every enqueued pass has been given its resolve there by then,
// so a capture reads and a merge rewrites a frame and planes that hold exactly the passes requested so far; drainPipeline also makes
// each pipeline group's next step wait for the context's stream (needUserSync), and the next resolve is enqueued behind the merge on
// that same stream.  A merge waits for the stream because its result goes back to the host.
#include "hr_history.h"

static int historyCheckParams(hr_ctx *c, const hr_history_params *in, hr_history_params *p)
{
    if (in)
        *p = *in;
    else
        hr_history_default_params(p);
    if (p->max_history < HR_HISTORY_MAX_HISTORY_LOWEST || p->max_history > HR_HISTORY_MAX_HISTORY_HIGHEST)
        FAIL(c, HR_ERR_INVALID, "history: max_history = " + std::to_string(p->max_history) + " is outside " + std::to_string(HR_HISTORY_MAX_HISTORY_LOWEST) + " .. " +
                                    std::to_string(HR_HISTORY_MAX_HISTORY_HIGHEST));
    if (!std::isfinite(p->normal_cos) || p->normal_cos < -1.0f || p->normal_cos > 1.0f) FAIL(c, HR_ERR_INVALID, "history: normal_cos must lie in -1 .. 1");
    if (!std::isfinite(p->plane_tol) || !(p->plane_tol > 0.0f)) FAIL(c, HR_ERR_INVALID, "history: plane_tol must be finite and greater than 0");
    if (!std::isfinite(p->min_weight) || !(p->min_weight > 0.0f) || p->min_weight > 1.0f) FAIL(c, HR_ERR_INVALID, "history: min_weight must be greater than 0 and at most 1");
    return HR_OK;
}

static int historyCheckCamera(hr_ctx *c, const hr_pass_params *cam)
{
    if (!cam) FAIL(c, HR_ERR_INVALID, "history: null camera");
    bool finite = std::isfinite(cam->fov_tan) && std::isfinite(cam->aspect_ratio);
    for (float v : cam->view_matrix) finite = finite && std::isfinite(v);
    if (!finite) FAIL(c, HR_ERR_INVALID, "history: the camera (view_matrix, fov_tan, aspect_ratio) is not finite");
    return HR_OK;
}

// what capture, merge and hr_reproject.inl's calls all ask of the context: a plain one, whose frame (c->fb()) holds at least one pass
static int historyCheckFrame(hr_ctx *c, const char *what, uint32_t *passes)
{
    const float *frame = nullptr;
    const FrameNeed need{HR_AOV_SURFACE | HR_AOV_MOMENTS, what, "the gather", false, true, std::string(what) + kNeedsAovPlanes, std::string(what) + kAovPlanesLate};
    return frameReady(c, need, &frame, passes);
}

// what every gather from the captured history is launched with (the merges here, in hr_reproject.inl and hr_motion.inl, and the preview):
// the captured camera against the new one, and the checked parameters as the kernels take them
struct HsLaunch {
    HsCam cam;
    HsParams P;
};

static HsLaunch historyLaunch(const hr_ctx *c, const hr_pass_params *camera, const hr_history_params &p)
{
    return HsLaunch{hsCameras(c->history.view, c->history.aspect, c->history.fovTan, camera->view_matrix, camera->aspect_ratio, camera->fov_tan),
                    HsParams{(float)p.max_history, p.normal_cos, p.plane_tol, p.min_weight}};
}

extern "C" {

uint32_t hr_history_api_version(void) { return HR_HISTORY_API_VERSION; }

void hr_history_default_params(hr_history_params *p)
{
    if (!p) return;
    *p = hr_history_params{};
    p->max_history = 32, p->normal_cos = 0.9f, p->plane_tol = 0.02f, p->min_weight = 0.25f;
}

int hr_history_capture(hr_ctx *c, const hr_pass_params *camera)
{
    ENTER(c);
    int rc = historyCheckCamera(c, camera);
    if (rc) return rc;
    uint32_t n = 0;
    rc = historyCheckFrame(c, "history capture", &n);
    if (rc) return rc;
    if (!c->history.hist) HIP_TRY(c, c->history.hist.alloc((size_t)c->W * c->H * kHistoryBytesPerPixel / sizeof(float)));
    c->history.captured = false;
    launchHistoryCapture(c->stream, c->W, c->H, c->fb(), c->aov.plane[HR_AOV_PLANE_ALBEDO], c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH], c->aov.plane[HR_AOV_PLANE_MOMENTS], c->history.hist);
    HIP_TRY(c, hipGetLastError());
    std::memcpy(c->history.view, camera->view_matrix, sizeof(c->history.view));
    c->history.fovTan = camera->fov_tan, c->history.aspect = camera->aspect_ratio;
    c->history.passes = n, c->history.captured = true;
    return HR_OK;
}

int hr_history_merge(hr_ctx *c, const hr_pass_params *camera, const hr_history_params *params, hr_history_result *out)
{
    ENTER(c);
    hr_history_params p;
    int rc = historyCheckParams(c, params, &p);
    if (rc == HR_OK) rc = historyCheckCamera(c, camera);
    if (rc) return rc;
    uint32_t n = 0;
    rc = historyCheckFrame(c, "history merge", &n);
    if (rc) return rc;
    if (!c->history.captured) FAIL(c, HR_ERR_INVALID, "history merge: no captured history (hr_history_capture; hr_frame_resize and hr_history_drop remove it)");
    if (c->history.merged) FAIL(c, HR_ERR_INVALID, "history merge: the history has already been merged into this frame (one merge per hr_clear: a second would count it twice)");
    HIP_TRY(c, c->history.result.ensure(kHistoryResultWords));
    HIP_TRY(c, c->history.result.zero(c->stream));
    const HsLaunch l = historyLaunch(c, camera, p);
    launchHistoryMerge(c->stream, c->W, c->H, l.cam, l.P, c->history.hist, c->fb(), c->aov.plane[HR_AOV_PLANE_ALBEDO], c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH],
                       c->aov.plane[HR_AOV_PLANE_MOMENTS], c->history.result.dev);
    HIP_TRY(c, hipGetLastError());
    c->history.merged = true;
    c->snapshotEpoch++; // (progressive snapshots taken before the merge are not handed out any more)
    HIP_TRY(c, c->history.result.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out) {
        *out = hr_history_result{};
        out->reused_pixels = c->history.result.host[0], out->rejected_pixels = c->history.result.host[1], out->history_samples = c->history.result.host[2];
        out->history_passes = c->history.passes, out->passes = n;
    }
    return HR_OK;
}

int hr_history_drop(hr_ctx *c)
{
    ENTER(c);
    if (c->grp) return HR_OK; // (a group never holds one)
    const int rc = c->history.hist ? quiesce(c) : HR_OK;
    if (rc) return rc;
    const bool merged = c->history.merged; // (the frame has still been merged into: dropping the history does not allow a second merge of a new one)
    c->history.release();
    c->history.merged = merged;
    return HR_OK;
}

int hr_history_info(hr_ctx *c, int32_t *captured, uint32_t *passes)
{
    ENTER(c);
    const bool have = !c->grp && c->history.captured;
    if (captured) *captured = have ? 1 : 0;
    if (passes) *passes = have ? c->history.passes : 0u;
    return HR_OK;
}

int hr_history_readback(hr_ctx *c, float *host_out)
{
    ENTER(c);
    if (!host_out) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->grp || !c->history.captured) FAIL(c, HR_ERR_INVALID, "history: no captured history");
    HIP_TRY(c, hipMemcpyAsync(host_out, c->history.hist, (size_t)c->W * c->H * kHistoryBytesPerPixel, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HR_OK;
}

} // extern "C"
