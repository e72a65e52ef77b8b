// hr_aov.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_aov.h.  The device side is in
// hr_shade.hip and hr_frame.hip (k_shade_hit<MODE | 4, CLS> records a pass's first visible surface in the pass slot's AOV record, k_resolve_aov folds
// the records and the samples' squares into the frame's planes); the planes' life follows the frame's (hr_clear, hr_frame_resize).

static const char *const kAovPlaneNames[3] = {"ALBEDO", "NORMAL_DEPTH", "MOMENTS"};

static int aovCheckPlane(hr_ctx *c, int32_t plane)
{
    if (plane < 0 || plane > HR_AOV_PLANE_MOMENTS) FAIL(c, HR_ERR_INVALID, "bad AOV plane id " + std::to_string(plane));
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    if (!c->aov.plane[plane])
        FAIL(c, HR_ERR_INVALID, std::string("AOV plane ") + kAovPlaneNames[plane] + " is not enabled (hr_aov_enable with " +
                                    (plane == HR_AOV_PLANE_MOMENTS ? "HR_AOV_MOMENTS" : "HR_AOV_SURFACE") + ")");
    return HR_OK;
}

// ---- context groups: every member holds its own planes (its tiles); the group's planes on the first device are assembled like the frame
static int groupAovEnable(hr_ctx *c, uint32_t mask)
{
    int rc = groupAll(c, [mask](hr_ctx *m, int) { return hr_aov_enable(m, mask); });
    if (rc) return rc;
    if (mask == c->aov.mask) return HR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a gather in flight writes the planes about to go)
    c->aov.mask = mask;
    return aovAllocPlanes(c);
}

// the plane of every member packed, copied to the first device and gathered into the group's plane; *passes: the fewest passes a member
// that owns pixels has summed into it
static int groupAovAssemble(hr_ctx *c, int32_t plane, uint64_t *passes)
{
    GroupState *g = c->grp;
    const int dev0 = c->device;
    const bool afterGather = g->gathered;
    const hipEvent_t evGathered = g->evGathered;
    int rc = groupAll(c, [&](hr_ctx *m, int i) {
        GroupState::Member &M = g->m[i];
        int rc = drainPipeline(m);
        if (rc == HR_OK) rc = overflowCheck(m);
        if (rc == HR_OK) rc = aovCheckPlane(m, plane);
        if (rc) return rc;
        if (M.slots) {
            if (afterGather) HIP_TRY(m, hipStreamWaitEvent(m->stream, evGathered, 0)); // the last gather has read the buffer
            FrameDev fr = m->frame;
            fr.fb = m->aov.plane[plane];
            launchPackOwned(m->cfg(m->stream), fr, m->aov.plane[plane], M.packed, 0, nullptr);
            HIP_TRY(m, hipGetLastError());
            if (M.staging) HIP_TRY(m, hipMemcpyPeerAsync(M.staging, dev0, M.packed, M.device, M.slots * 16, m->stream));
        }
        HIP_TRY(m, hipEventRecord(M.evPacked, m->stream));
        M.passes = (uint32_t)(m->nextResolveOrder - m->aov.zeroedAt);
        return HR_OK;
    });
    if (rc) return rc;
    GatherList list{};
    list.n = g->n;
    uint32_t blocks = 0;
    uint64_t fewest = 0;
    bool any = false;
    for (int i = 0; i < g->n; ++i) {
        const GroupState::Member &M = g->m[i];
        list.blockStart[i] = blocks;
        list.packed[i] = M.staging ? M.staging : M.packed;
        blocks += (uint32_t)((M.slots + (uint64_t)gatherBlock() - 1) / (uint64_t)gatherBlock());
        HIP_TRY(c, hipStreamWaitEvent(c->stream, M.evPacked, 0));
        if (M.slots) fewest = any ? std::min<uint64_t>(fewest, M.passes) : M.passes, any = true;
    }
    list.blockStart[g->n] = blocks;
    launchGatherMembers(c->cfg(c->stream), c->frame, list, c->aov.plane[plane]);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(g->evGathered, c->stream));
    g->gathered = true;
    if (passes) *passes = fewest;
    return HR_OK;
}

extern "C" {

uint32_t hr_aov_api_version(void) { return HR_AOV_API_VERSION; }

int hr_aov_enable(hr_ctx *c, uint32_t mask)
{
    ENTER(c);
    if (mask & ~(HR_AOV_SURFACE | HR_AOV_MOMENTS)) FAIL(c, HR_ERR_INVALID, "unknown AOV mask bits " + std::to_string(mask & ~(HR_AOV_SURFACE | HR_AOV_MOMENTS)));
    if (c->grp) return groupAovEnable(c, mask);
    if (mask == c->aov.mask) return HR_OK;
    QUIESCE(c);
    // HR_AOV_SURFACE changes what a pass slot holds: the slots are released and re-allocated with the new size (as when
    // HR_ESTIMATOR_ALL_LIGHTS is first used)
    const bool slotsChange = ((mask ^ c->aov.mask) & HR_AOV_SURFACE) != 0;
    if (slotsChange) {
        const uint32_t keepCap = c->queueCapacity;
        freeQueues(c);
        c->queueCapacity = keepCap;
    }
    c->aov.mask = mask;
    const int rc = aovAllocPlanes(c);
    if (rc) return rc;
    if (slotsChange) slotBudget(c);
    return HR_OK;
}

int hr_aov_mask(hr_ctx *c, uint32_t *mask)
{
    ENTER(c);
    if (!mask) FAIL(c, HR_ERR_INVALID, "null output");
    *mask = c->aov.mask;
    return HR_OK;
}

int hr_aov_readback(hr_ctx *c, int32_t plane, const float **rgba, int32_t *w, int32_t *h, uint64_t *passes)
{
    ENTER(c);
    if (!rgba) FAIL(c, HR_ERR_INVALID, "null output");
    int rc = aovCheckPlane(c, plane);
    if (rc) return rc;
    const size_t bytes = (size_t)c->W * c->H * 4 * sizeof(float);
    uint64_t n = 0;
    if (c->grp) {
        rc = groupAovAssemble(c, plane, &n);
    } else {
        rc = drainPipeline(c);
        n = c->nextResolveOrder - c->aov.zeroedAt;
    }
    if (rc == HR_OK) rc = growPinned(c, c->aov.pinned, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->aov.pinned.get(), c->aov.plane[plane], bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!c->grp) {
        rc = overflowCheck(c);
        if (rc) return rc;
    }
    *rgba = c->aov.pinned.get();
    if (w) *w = c->W;
    if (h) *h = c->H;
    if (passes) *passes = n;
    return HR_OK;
}

int hr_aov_copy(hr_ctx *c, int32_t plane, void *device_out, void *stream)
{
    ENTER(c);
    if (!device_out) FAIL(c, HR_ERR_INVALID, "null output");
    int rc = aovCheckPlane(c, plane);
    if (rc) return rc;
    rc = c->grp ? groupAovAssemble(c, plane, nullptr) : drainPipeline(c);
    if (rc) return rc;
    return copyOutOnStream(c, device_out, c->aov.plane[plane], (size_t)c->W * c->H * 4 * sizeof(float), stream); // (the next resolve or gather rewrites the plane: behind the copy)
}

} // extern "C"
