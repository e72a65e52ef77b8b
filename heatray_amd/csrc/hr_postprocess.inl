// hr_postprocess.inl — a section of hr_core.hip (included before the feature sections): the host plumbing that the AOV planes, the
// denoiser, adaptive sampling, history reprojection, the progressive merge, auto-exposure, the convergence metric and firefly suppression share ("Adding a post-process feature"), and
// the one table of when each feature's state goes; the state itself, with ResultCounters, is in hr_features.h.

// `bytes` of device memory that is complete on the ctx stream -> dst, on `stream` (null: the ctx stream).  On a foreign stream the copy
// waits for everything enqueued on the ctx stream so far, and the ctx's next work goes behind the copy: the next resolve, filter or update
// may rewrite `src` at once.  (One event serves every such copy: each wait is enqueued right behind its record.)
static int copyOutOnStream(hr_ctx *c, void *dst, const void *src, size_t bytes, void *stream)
{
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (st == c->stream) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return HR_OK;
    }
    if (!c->evCopyOut) HIP_TRY(c, c->evCopyOut.create(hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->evCopyOut, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(st, c->evCopyOut, 0));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipEventRecord(c->evCopyOut, st));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evCopyOut, 0));
    return HR_OK;
}

// ---- when the features' state goes.  These four are the only callers of a feature's release() (hr_history_drop and hr_motion_drop apart; the context's
// destructor would free what is left, but hr_ctx_destroy and groupDestroy come through featuresDestroyed first) and the only
// code that resets a feature's flags; a plain context, a group's handle and its members all come through them.  Every caller has
// drained or synchronised what could still use the memory.
// The AOV planes are going (aovAllocPlanes: hr_frame_resize, hr_aov_enable): so does what was computed from them at their size.
static void featuresPlanesGone(hr_ctx *c)
{
    c->denoise.release();   // (the denoiser's buffers live and die with the planes it reads)
    c->despeckle.release(); // (... and so do the despeckled frame and moments the denoiser can be run from)
    c->aov.pinned.reset();
}
// The frame has another size (hr_frame_resize, groupResize): what was made for the old one goes, an installed sample mask included.
static void featuresFrameResized(hr_ctx *c)
{
    c->adaptive.release();
    c->frame.mask = nullptr;
    c->history.release();
    c->reproject.release();
    c->motion.releaseFrame(); // (include/hrcore_motion.h: the planes go, the snapshot stays)
}
// The frame starts afresh (hr_clear, groupClear).
static void featuresFrameCleared(hr_ctx *c)
{
    c->frame.mask = nullptr;       // (include/hrcore_adaptive.h: a new frame starts without a sample mask)
    c->history.merged = false;     // (include/hrcore_history.h: ... and may take over a captured history once)
    c->reproject.merged = false, c->reproject.stale = true; // (include/hrcore_reproject.h: ... or progressively: no pixel of the new frame has been examined)
}
// The context goes (hr_ctx_destroy, groupDestroy).
static void featuresDestroyed(hr_ctx *c)
{
    featuresPlanesGone(c);
    featuresFrameResized(c);
    c->aov.release();
    c->exposure.release();
    c->metric.release();
    c->meshPrep.release();
    c->deform.release();
    c->query.release();
    c->motion.release();
}

// ---- "a full-frame post-process wants this frame"
struct FrameNeed {
    uint32_t aov;       // the AOV planes it reads (HR_AOV_*): enabled, and zeroed when the frame was, so they hold the frame's passes; 0: none, the planes are not asked about
    const char *name;   // starts its messages: "denoise", "history merge"
    const char *reader; // what reads across the tiles, for the refusals of a sharded frame: "the filter"
    bool group;         // a context group is served: its frame and the planes of `aov` are assembled on its first device
    bool nonEmpty;      // a frame of 0 passes is an error
    std::string needs;  // a plane of `aov` is off: the message up to " before the frame's first pass" (name + kNeedsAovPlanes)
    std::string late;   // the planes were enabled after the first pass: the message up to " the frame's passes" (name + kAovPlanesLate)
};
static const char kNeedsAovPlanes[] = " needs the AOV planes: hr_aov_enable(HR_AOV_SURFACE | HR_AOV_MOMENTS)";
static const char kAovPlanesLate[] = ": the AOV planes were enabled after the frame's first pass and do not hold";

static int groupAovAssemble(hr_ctx *c, int32_t plane, uint64_t *passes); // hr_aov.inl

// one context's planes (a group's handle, each of its members, a plain context)
static int framePlanesReady(hr_ctx *c, const FrameNeed &need)
{
    if (need.aov == 0) return HR_OK; // (it reads no plane: whether and when they were enabled is not its business)
    if ((c->aov.mask & need.aov) != need.aov)
        FAIL(c, HR_ERR_INVALID, need.needs + " before the frame's first pass (enabled mask: " + std::to_string(c->aov.mask) + ")");
    if (c->aov.zeroedAt != c->frameZeroedAt) FAIL(c, HR_ERR_INVALID, need.late + " the frame's passes: hr_clear, or hr_aov_enable before rendering");
    return HR_OK;
}

// the kind of context, then a frame: what frameReady asks first (and all a caller that brings its own image asks)
static int frameKindReady(hr_ctx *c, const FrameNeed &need)
{
    if (c->grp && !need.group)
        FAIL(c, HR_ERR_INVALID, std::string(need.name) + ": a context group is not supported (" + need.reader + " reads across the members' tiles): capture and merge on a plain context");
    if (!c->grp && c->world > 1)
        FAIL(c, HR_ERR_INVALID, std::string(need.name) + ": a tile-sharded context (world > 1) holds only its own tiles and " + need.reader + " reads across them" +
                                    (need.group ? ": use a context group, which assembles the frame" : ""));
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    return HR_OK;
}

// Checks in this order: the kind of context, a frame, the planes; then completes the enqueued passes (a group: assembles its frame and
// planes) and reports a ray queue overflow.  *frame: the complete frame on the ctx's device; *passes: the complete passes in it.
static int frameReady(hr_ctx *c, const FrameNeed &need, const float **frame, uint32_t *passes)
{
    int rc = frameKindReady(c, need);
    if (rc == HR_OK) rc = framePlanesReady(c, need); // (a group: its own mask, hr_aov_enable on the handle)
    if (rc == HR_OK && c->grp) rc = groupAll(c, [&need](hr_ctx *m, int) { return framePlanesReady(m, need); });
    if (rc) return rc;
    if (c->grp) {
        rc = groupAssemble(c, true, passes, nullptr);
        for (int plane = 0; plane < 3 && rc == HR_OK; ++plane)
            if (need.aov & (plane == HR_AOV_PLANE_MOMENTS ? HR_AOV_MOMENTS : HR_AOV_SURFACE)) rc = groupAovAssemble(c, plane, nullptr);
        if (rc) return rc;
        *frame = c->fbInternal;
    } else {
        rc = drainPipeline(c);
        if (rc == HR_OK) rc = overflowCheck(c);
        if (rc) return rc;
        *passes = (uint32_t)(c->nextResolveOrder - c->frameZeroedAt);
        *frame = c->fb();
    }
    if (need.nonEmpty && *passes == 0) FAIL(c, HR_ERR_INVALID, std::string(need.name) + ": the frame is empty (0 passes)");
    return HR_OK;
}
