// hr_group.inl — a section of hr_core.hip (included at its end): context groups (include/hrcore_group.h).  N member contexts, member i =
// rank i of world N on device_ids[i], behind ONE hr_ctx handle; every hrcore.h entry point branches to the group* functions below at its top.
//
// Threads.  Every member has a host thread of its own, which makes every call on that member from its creation to its destruction: a
// member is never touched by two threads, and one member's hr_render_pass spinning on its device-written queue lengths (waitCounts)
// never stalls another.  The caller's thread posts jobs to the members' queues: calls that change state run on every member and wait
// for all of them; hr_render_pass posts and returns (a member's queue holds at most kGroupQueueDepth jobs, then the caller waits).  The
// first error of a member's job is kept and returned by the group's next call as "member i (device d): ...".
//
// Process-wide mutable state of the library, audited before members ran concurrently: the device counters of k_trace's tail profile
// (g_tailprof, HR_TAILPROF builds only — members on one device add into the same counters, so such a measurement is of the device, not
// of a member); getenv reads at context creation only (HR_TUNE and the HR_DEBUG_* flags go into the member's own hr_ctx::tune; nothing
// in the library sets the environment).  Everything else lives in the hr_ctx.
//
// Devices and ordering.  Members never wait on one another on the device.  Assembly: each member packs its owned pixels on its own stream
// (hr_frame_pack_owned: after the resolves enqueued so far, before the next one), a member on another device copies the packed bytes to a
// staging buffer on the first device (hipMemcpyPeerAsync: DMA over xGMI, 1/N of the frame), and records evPacked; the assembly stream
// waits for every member's evPacked and runs ONE k_gather_members over all members into the assembled frame, then records evGathered,
// which every member's next pack waits for (its packed buffer is read by that gather).  Peer access is enabled between every pair of
// distinct member devices that allows it.

struct GroupState {
    struct Member {
        hr_ctx *ctx = nullptr;   // written and used by the member's thread only
        int device = 0;
        Stream stream;  // the member context's stream (created by its thread, on its device, and reset there)
        Event evPacked; // its device: the member's packed pixels (and their copy to the first device) are complete
        std::thread thread;
        std::deque<std::function<int(hr_ctx *)>> jobs; // guarded by GroupState::mu
        int queued = 0;                                // jobs posted and not finished yet (guarded)
        int err = HR_OK;                               // first failure of a job since the group's last call reported one (guarded)
        std::string errMsg;
        // assembly (written by the member's job, read by the caller after waiting for it)
        DeviceBuf<float> packed;  // its device: owned pixels in pack order, slots x RGBA32F (reset by the member's thread)
        DeviceBuf<float> staging; // the first device: their copy (members on another device; caller's thread allocates it)
        uint64_t slots = 0;
        uint32_t passes = 0;      // complete passes in the last packed pixels
        bool idle = true;         // no pass of the member was pending or in flight when it last packed
    };
    int n = 0;
    Member m[HR_GROUP_MAX_MEMBERS];
    std::mutex mu;
    std::condition_variable cvJob, cvDone;
    bool stop = false;
    Event evGathered; // the first device: recorded on the assembly stream behind the last gather
    bool gathered = false;
};

// A member may have this many posted jobs outstanding: hr_render_pass posts one per pass, so the host runs at most a few of a small
// shard's batches (HR_BATCH_CAP passes) ahead of a member.
static const int kGroupQueueDepth = 3 * HR_BATCH_CAP;

static void groupWorker(GroupState *g, int i)
{
    GroupState::Member &M = g->m[i];
    hipSetDevice(M.device);
    std::unique_lock<std::mutex> lk(g->mu);
    for (;;) {
        g->cvJob.wait(lk, [&] { return g->stop || !M.jobs.empty(); });
        if (M.jobs.empty()) return; // (stop, with every posted job done)
        std::function<int(hr_ctx *)> job = std::move(M.jobs.front());
        M.jobs.pop_front();
        lk.unlock();
        const int rc = job(M.ctx);
        std::string msg;
        if (rc != HR_OK) msg = M.ctx && !M.ctx->err.empty() ? M.ctx->err : "status " + std::to_string(rc);
        lk.lock();
        if (rc != HR_OK && M.err == HR_OK) M.err = rc, M.errMsg = msg;
        --M.queued;
        g->cvDone.notify_all();
    }
}

static void groupPost(GroupState *g, int i, std::function<int(hr_ctx *)> job, int depth)
{
    std::unique_lock<std::mutex> lk(g->mu);
    g->cvDone.wait(lk, [&] { return g->m[i].queued < depth; });
    g->m[i].jobs.push_back(std::move(job));
    g->m[i].queued++;
    g->cvJob.notify_all();
}

// the lowest member's kept error -> the group's message (mu held); every member's is cleared
static int groupTakeErrorLocked(hr_ctx *c)
{
    GroupState *g = c->grp;
    int rc = HR_OK;
    for (int i = 0; i < g->n; ++i) {
        GroupState::Member &M = g->m[i];
        if (M.err != HR_OK && rc == HR_OK) rc = M.err, c->err = "member " + std::to_string(i) + " (device " + std::to_string(M.device) + "): " + M.errMsg;
        M.err = HR_OK, M.errMsg.clear();
    }
    return rc;
}
static int groupTakeError(hr_ctx *c)
{
    std::lock_guard<std::mutex> lk(c->grp->mu);
    return groupTakeErrorLocked(c);
}

// wait until member `only` (-1: every member) has run every job posted so far
static int groupWait(hr_ctx *c, int only = -1)
{
    GroupState *g = c->grp;
    std::unique_lock<std::mutex> lk(g->mu);
    g->cvDone.wait(lk, [&] {
        for (int i = 0; i < g->n; ++i)
            if ((only < 0 || i == only) && g->m[i].queued > 0) return false;
        return true;
    });
    return groupTakeErrorLocked(c);
}

// fn(member context, member index) on every member, in parallel; returns when all have run it
static int groupAll(hr_ctx *c, const std::function<int(hr_ctx *, int)> &fn)
{
    GroupState *g = c->grp;
    for (int i = 0; i < g->n; ++i) groupPost(g, i, [&fn, i](hr_ctx *m) { return fn(m, i); }, 1 << 30);
    return groupWait(c);
}

// fn on one member (the calls every member answers alike ask member 0)
static int groupOne(hr_ctx *c, int i, const std::function<int(hr_ctx *)> &fn)
{
    groupPost(c->grp, i, [&fn](hr_ctx *m) { return fn(m); }, 1 << 30);
    return groupWait(c, i);
}

// a call that returns an id: it must be the same on every member (they hold the same scene, built by the same calls)
static int groupAllId(hr_ctx *c, int32_t *out, const char *what, const std::function<int(hr_ctx *, int, int32_t *)> &fn)
{
    int32_t ids[HR_GROUP_MAX_MEMBERS];
    for (int32_t &v : ids) v = -1;
    const int rc = groupAll(c, [&](hr_ctx *m, int i) { return fn(m, i, &ids[i]); });
    if (rc) return rc;
    for (int i = 1; i < c->grp->n; ++i)
        if (ids[i] != ids[0])
            FAIL(c, HR_ERR_DEVICE, std::string("internal: ") + what + " returned id " + std::to_string(ids[i]) + " on member " + std::to_string(i) + " but " +
                                       std::to_string(ids[0]) + " on member 0: the members' scenes differ");
    if (out) *out = ids[0];
    return HR_OK;
}

static int groupUnsupported(hr_ctx *c, const char *what)
{
    FAIL(c, HR_ERR_UNSUPPORTED, std::string(what) + " is not supported on a context group (per-member counters: hr_group_member_stats)");
}

static int groupDestroy(hr_ctx *c)
{
    GroupState *g = c->grp;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream); // (the last gather reads the members' packed buffers)
    for (int i = 0; i < g->n; ++i)
        groupPost(g, i, [g, i](hr_ctx *m) {
            GroupState::Member &M = g->m[i];
            hipSetDevice(M.device);
            if (m) hr_ctx_destroy(m);
            M.ctx = nullptr;
            M.packed.reset(), M.evPacked.reset(), M.stream.reset(); // (on the member's thread, its device current)
            return HR_OK;
        }, 1 << 30);
    {
        std::unique_lock<std::mutex> lk(g->mu);
        g->cvDone.wait(lk, [&] {
            for (int i = 0; i < g->n; ++i)
                if (g->m[i].queued > 0) return false;
            return true;
        });
        g->stop = true;
        g->cvJob.notify_all();
    }
    for (int i = 0; i < g->n; ++i)
        if (g->m[i].thread.joinable()) g->m[i].thread.join();
    hipSetDevice(c->device); // (the first device: what the group itself holds lives there — staging, evGathered, the assembled frame)
    featuresDestroyed(c);
    delete g;
    delete c;
    return HR_OK;
}

static int groupSetStream(hr_ctx *c, void *stream)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)stream;
    return HR_OK;
}

static int groupResize(hr_ctx *c, int32_t w, int32_t h)
{
    if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 28)) FAIL(c, HR_ERR_INVALID, "bad frame size");
    GroupState *g = c->grp;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a gather in flight reads the buffers about to go)
    int rc = groupAll(c, [g, w, h](hr_ctx *m, int i) {
        GroupState::Member &M = g->m[i];
        int rc = hr_frame_resize(m, w, h);
        if (rc) return rc;
        M.packed.reset();
        M.slots = (uint64_t)m->frame.nOwnedTiles * (uint64_t)(m->tile * m->tile);
        if (M.slots) HIP_TRY(m, M.packed.alloc(M.slots * 4));
        return HR_OK;
    });
    if (rc) return rc;
    for (int i = 0; i < g->n; ++i) {
        GroupState::Member &M = g->m[i];
        M.staging.reset();
        if (M.device != c->device && M.slots) HIP_TRY(c, M.staging.alloc(M.slots * 4));
    }
    c->W = w, c->H = h;
    c->snapshotEpoch++;
    freeLagged(c->progFrame), freeLagged(c->progDisplay);
    c->fbInternal.reset();
    featuresFrameResized(c); // (the group's copy of the sample mask; the members' went with their frames)
    const size_t fbBytes = (size_t)w * h * 4 * sizeof(float);
    HIP_TRY(c, c->fbInternal.alloc((size_t)w * h * 4));
    HIP_TRY(c, hipMemsetAsync(c->fbInternal, 0, fbBytes, c->stream));
    if ((rc = growPinned(c, c->pinned, fbBytes))) return rc;
    FrameDev &f = c->frame; // the assembled frame: rank 0 of world 1
    f.W = w, f.H = h, f.rank = 0, f.world = 1, f.tile = c->tile;
    f.tilesX = (w + c->tile - 1) / c->tile, f.tilesY = (h + c->tile - 1) / c->tile;
    f.nOwnedTiles = f.tilesX * f.tilesY;
    f.fb = c->fbInternal;
    return aovAllocPlanes(c); // (the group's AOV planes, assembled like the frame)
}

// Every member packs the passes it has resolved (drain: after completing all it has been given), members on other devices copy their
// pack to the first device, and one gather on the assembly stream writes the assembled frame.  *passes: the fewest complete passes of a
// member that owns pixels; *idle: no member had a pass pending or in flight.
static int groupAssemble(hr_ctx *c, bool drain, uint32_t *passes, bool *idle)
{
    GroupState *g = c->grp;
    const int dev0 = c->device;
    const bool afterGather = g->gathered;
    const hipEvent_t evGathered = g->evGathered;
    int rc = groupAll(c, [&](hr_ctx *m, int i) {
        GroupState::Member &M = g->m[i];
        int rc = drain ? drainPipeline(m) : completeForSlowCaller(m);
        if (rc == HR_OK) rc = overflowCheck(m);
        if (rc) return rc;
        if (M.slots) {
            if (afterGather) HIP_TRY(m, hipStreamWaitEvent(m->stream, evGathered, 0)); // the last gather has read the buffer
            rc = hr_frame_pack_owned(m, M.packed, nullptr);
            if (rc) return rc;
            if (M.staging) HIP_TRY(m, hipMemcpyPeerAsync(M.staging, dev0, M.packed, M.device, M.slots * 16, m->stream));
        }
        HIP_TRY(m, hipEventRecord(M.evPacked, m->stream));
        M.passes = (uint32_t)(m->nextResolveOrder - m->resolvedAtClear);
        M.idle = m->pendingInject.empty() && occupiedSlots(m) == 0;
        return HR_OK;
    });
    if (rc) return rc;
    GatherList list{};
    list.n = g->n;
    uint32_t blocks = 0, fewest = 0;
    bool any = false, allIdle = true;
    for (int i = 0; i < g->n; ++i) {
        const GroupState::Member &M = g->m[i];
        list.blockStart[i] = blocks;
        list.packed[i] = M.staging ? M.staging : M.packed;
        blocks += (uint32_t)((M.slots + (uint64_t)gatherBlock() - 1) / (uint64_t)gatherBlock());
        HIP_TRY(c, hipStreamWaitEvent(c->stream, M.evPacked, 0));
        if (M.slots) fewest = any ? std::min(fewest, M.passes) : M.passes, any = true;
        allIdle = allIdle && M.idle;
    }
    list.blockStart[g->n] = blocks;
    launchGatherMembers(c->cfg(c->stream), c->frame, list, c->fbInternal);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(g->evGathered, c->stream));
    g->gathered = true;
    if (passes) *passes = fewest;
    if (idle) *idle = allIdle;
    return HR_OK;
}

static int groupReadback(hr_ctx *c, const float **rgba, int32_t *w, int32_t *h)
{
    if (c->W <= 0 || !rgba) FAIL(c, HR_ERR_INVALID, "no frame");
    int rc = groupAssemble(c, true, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->pinned.get(), c->fbInternal, (size_t)c->W * c->H * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *rgba = c->pinned.get();
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

static int groupReadbackProgressive(hr_ctx *c, const float **rgba, int32_t *w, int32_t *h, uint32_t *passesOut)
{
    if (c->W <= 0 || !rgba) FAIL(c, HR_ERR_INVALID, "no frame");
    const size_t bytes = (size_t)c->W * c->H * 4 * sizeof(float);
    uint32_t passes = 0;
    bool idle = true;
    int rc = groupAssemble(c, false, &passes, &idle);
    if (rc == HR_OK) rc = ensureLagged(c, c->progFrame, bytes, false);
    if (rc) return rc;
    const int k = beginLagged(c->progFrame);
    HIP_TRY(c, hipMemcpyAsync(c->progFrame.pinned[k], c->fbInternal, bytes, hipMemcpyDeviceToHost, c->stream));
    const void *out = nullptr;
    rc = finishLaggedAt(c, c->progFrame, k, 0, &out, passesOut, passes, idle);
    if (rc) return rc;
    *rgba = (const float *)out;
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

static int groupDisplayTo(hr_ctx *c, const hr_display_params *params, int32_t format, void *out, uint32_t *passes, bool *idle)
{
    if (!params || !out) FAIL(c, HR_ERR_INVALID, "null argument");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    const bool progressive = (format & HR_DISPLAY_PROGRESSIVE) != 0;
    format &= ~HR_DISPLAY_PROGRESSIVE;
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format");
    const int rc = groupAssemble(c, !progressive, passes, idle);
    if (rc) return rc;
    FrameDev fr = c->frame;
    fr.fb = c->fbInternal;
    launchDisplay(c->cfg(c->stream), fr, *params, format, out); // (world 1: every pixel is the group's)
    HIP_TRY(c, hipGetLastError());
    return HR_OK;
}

static int groupDisplay(hr_ctx *c, const hr_display_params *params, int32_t format, void *out, uint32_t *shown)
{
    uint32_t passes = 0;
    const int rc = groupDisplayTo(c, params, format, out, &passes, nullptr);
    if (rc == HR_OK && shown) *shown = passes;
    return rc;
}

static int groupDisplayReadback(hr_ctx *c, const hr_display_params *params, int32_t format, const void **pixels, int32_t *width, int32_t *height, uint32_t *shown)
{
    if (!pixels || !params) FAIL(c, HR_ERR_INVALID, "null argument");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    const size_t need = (size_t)c->W * c->H * 16;
    const size_t bytes = (size_t)c->W * c->H * displayPixelBytes(format & ~HR_DISPLAY_PROGRESSIVE);
    uint32_t passes = 0;
    bool idle = true;
    int rc = HR_OK;
    if (format & HR_DISPLAY_PROGRESSIVE) { // lagged, like a plain context's
        rc = ensureLagged(c, c->progDisplay, need, true);
        if (rc) return rc;
        const int k = beginLagged(c->progDisplay);
        rc = groupDisplayTo(c, params, format, c->progDisplay.dev[k], &passes, &idle);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->progDisplay.pinned[k], c->progDisplay.dev[k], bytes, hipMemcpyDeviceToHost, c->stream));
        int32_t key = format;
        for (size_t i = 0; i < sizeof(*params) / 4; ++i) key = key * 31 + ((const int32_t *)params)[i];
        rc = finishLaggedAt(c, c->progDisplay, k, key, pixels, shown, passes, idle);
    } else {
        if ((rc = growDisplay(c, need))) return rc;
        rc = groupDisplayTo(c, params, format, c->dDisplay, &passes, nullptr);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->pinnedDisplay.get(), c->dDisplay, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        *pixels = c->pinnedDisplay.get();
        if (shown) *shown = passes;
    }
    if (rc) return rc;
    if (width) *width = c->W;
    if (height) *height = c->H;
    return HR_OK;
}

static int groupDevicePtr(hr_ctx *c, void **deviceRgba)
{
    if (c->W <= 0 || !deviceRgba) FAIL(c, HR_ERR_INVALID, "no frame");
    const int rc = groupAssemble(c, true, nullptr, nullptr);
    if (rc) return rc;
    *deviceRgba = c->fbInternal; // (assembled on the assembly stream: work the caller puts there sees it)
    return HR_OK;
}

static int groupPassesResolved(hr_ctx *c, uint64_t *passes)
{
    if (!passes) FAIL(c, HR_ERR_INVALID, "null output");
    uint64_t n[HR_GROUP_MAX_MEMBERS];
    bool owns[HR_GROUP_MAX_MEMBERS];
    const int rc = groupAll(c, [&](hr_ctx *m, int i) {
        n[i] = m->nextResolveOrder - m->resolvedAtClear;
        owns[i] = m->frame.nOwnedTiles > 0;
        return HR_OK;
    });
    if (rc) return rc;
    bool any = false;
    *passes = 0;
    for (int i = 0; i < c->grp->n; ++i) // (a member without tiles resolves nothing: it does not hold the count down)
        if (owns[i]) *passes = any ? std::min(*passes, n[i]) : n[i], any = true;
    return HR_OK;
}

static int groupSync(hr_ctx *c, bool wait)
{
    const int rc = groupAll(c, [wait](hr_ctx *m, int) { return wait ? hr_synchronize(m) : hr_flush(m); });
    if (rc) return rc;
    if (wait) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HR_OK;
}

static int groupClear(hr_ctx *c)
{
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    const int rc = groupAll(c, [](hr_ctx *m, int) { return hr_clear(m); });
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->fbInternal, 0, (size_t)c->W * c->H * 4 * sizeof(float), c->stream));
    featuresFrameCleared(c); // (hr_clear has removed the members' sample masks: the group's copy goes too)
    c->snapshotEpoch++;
    return HR_OK;
}

static int groupRenderPass(hr_ctx *c, const hr_pass_params *pp)
{
    if (!pp) FAIL(c, HR_ERR_INVALID, "null params");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    const int rc = groupTakeError(c);
    if (rc) return rc;
    const hr_pass_params p = *pp;
    for (int i = 0; i < c->grp->n; ++i) groupPost(c->grp, i, [p](hr_ctx *m) { return hr_render_pass(m, &p); }, kGroupQueueDepth);
    return HR_OK;
}

static int groupStats(hr_ctx *c, hr_pass_stats *out)
{
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    hr_pass_stats part[HR_GROUP_MAX_MEMBERS];
    const int rc = groupAll(c, [&](hr_ctx *m, int i) { return hr_get_stats(m, &part[i]); });
    if (rc) return rc;
    std::memset(out, 0, sizeof(*out));
    for (int i = 0; i < c->grp->n; ++i) {
        const hr_pass_stats &s = part[i];
        out->ms = std::max(out->ms, s.ms);
        out->paths += s.paths, out->rays_closest += s.rays_closest, out->rays_any += s.rays_any, out->shaded_hits += s.shaded_hits;
        out->accumulates += s.accumulates, out->node_visits += s.node_visits, out->tri_tests += s.tri_tests;
        out->node_visits_any += s.node_visits_any, out->tri_tests_any += s.tri_tests_any;
    }
    return HR_OK;
}

// With a tree cache file, member 0 commits first (it writes the file if the scene's tree is not in it), then the others in parallel
// (they read it).  Should member 0 have failed to write the file, the others commit one after another: two members never write it at once.
static int groupCommit(hr_ctx *c)
{
    GroupState *g = c->grp;
    bool cached = false;
    int rc = groupOne(c, 0, [&](hr_ctx *m) {
        cached = !m->cachePath.empty();
        return hr_scene_commit(m);
    });
    if (rc || g->n == 1) return rc;
    bool fileThere = true;
    if (cached) rc = groupOne(c, 0, [&](hr_ctx *m) {
        FILE *f = fopen(m->cachePath.c_str(), "rb");
        fileThere = f != nullptr;
        if (f) fclose(f);
        return HR_OK;
    });
    if (rc) return rc;
    if (!cached || fileThere) {
        for (int i = 1; i < g->n; ++i) groupPost(g, i, [](hr_ctx *m) { return hr_scene_commit(m); }, 1 << 30);
        return groupWait(c);
    }
    for (int i = 1; i < g->n; ++i) {
        rc = groupOne(c, i, [](hr_ctx *m) { return hr_scene_commit(m); });
        if (rc) return rc;
    }
    return HR_OK;
}

static int groupMultiscatter(hr_ctx *c, float *out, hr_tex_id *outTex)
{
    // (the host copy comes from member 0; every member keeps its own LUT texture)
    return groupAllId(c, outTex, "hr_multiscatter_lut_generate",
                      [out, outTex](hr_ctx *m, int i, int32_t *id) { return hr_multiscatter_lut_generate(m, i == 0 ? out : nullptr, outTex ? id : nullptr); });
}

extern "C" {

uint32_t hr_group_api_version(void) { return HR_GROUP_API_VERSION; }

int hr_ctx_create_group(const hr_ctx_desc *desc, const int32_t *device_ids, int32_t n, hr_ctx **out)
{
    if (!out) return HR_ERR_INVALID;
    *out = nullptr;
    if (desc && (desc->rank != 0 || desc->world > 1)) return HR_ERR_INVALID; // (no group inside a tile shard)
    if (n < 0 || n > HR_GROUP_MAX_MEMBERS || (n > 0 && !device_ids)) return HR_ERR_INVALID;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0) return HR_ERR_DEVICE;
    std::vector<int> dev;
    if (n == 0 || !device_ids) {
        for (int d = 0; d < nDev && d < HR_GROUP_MAX_MEMBERS; ++d) dev.push_back(d);
    } else {
        for (int i = 0; i < n; ++i) {
            if (device_ids[i] < 0 || device_ids[i] >= nDev) return HR_ERR_INVALID;
            dev.push_back(device_ids[i]);
        }
    }
    const int tile = desc && desc->tile_size > 0 ? desc->tile_size : 32;
    if ((tile & 7) != 0) return HR_ERR_INVALID;
    // peer access between every pair of distinct member devices that allows it (torch or RCCL may have enabled it already)
    for (int a : dev)
        for (int b : dev) {
            int can = 0;
            if (a == b || hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) continue;
            if (hipSetDevice(a) != hipSuccess) return HR_ERR_DEVICE;
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) hipGetLastError(); // (clears the sticky status)
            else if (e != hipSuccess) return HR_ERR_DEVICE;
        }
    if (hipSetDevice(dev[0]) != hipSuccess) return HR_ERR_DEVICE;
    hr_ctx *c = new hr_ctx();
    c->device = dev[0];
    c->tile = tile;
    c->stream = desc ? (hipStream_t)desc->stream : nullptr;
    GroupState *g = new GroupState();
    c->grp = g;
    g->n = (int)dev.size();
    if (g->evGathered.create(hipEventDisableTiming) != hipSuccess) {
        groupDestroy(c);
        return HR_ERR_DEVICE;
    }
    hr_ctx_desc md{};
    if (desc) md = *desc;
    md.world = g->n;
    for (int i = 0; i < g->n; ++i) {
        g->m[i].device = dev[i];
        g->m[i].thread = std::thread(groupWorker, g, i);
        md.rank = i, md.device_id = dev[i];
        groupPost(g, i, [g, i, md](hr_ctx *) mutable { // (the member's own thread creates it)
            GroupState::Member &M = g->m[i];
            if (hipSetDevice(M.device) != hipSuccess || M.stream.create(hipStreamNonBlocking) != hipSuccess || M.evPacked.create(hipEventDisableTiming) != hipSuccess)
                return HR_ERR_DEVICE;
            md.stream = M.stream;
            return hr_ctx_create(&md, &M.ctx);
        }, 1 << 30);
    }
    const int rc = groupWait(c);
    if (rc) {
        groupDestroy(c);
        return rc;
    }
    *out = c;
    return HR_OK;
}

int hr_group_get_info(hr_ctx *c, hr_group_info *out)
{
    if (!c) return HR_ERR_INVALID;
    if (!c->grp) FAIL(c, HR_ERR_INVALID, "not a context group");
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    std::memset(out, 0, sizeof(*out));
    const GroupState *g = c->grp;
    out->n_members = g->n;
    for (int i = 0; i < g->n; ++i) out->device_ids[i] = g->m[i].device;
    const FrameDev &f = c->frame;
    for (int t = 0; c->W > 0 && t < f.tilesX * f.tilesY; ++t) {
        const int tx = t % f.tilesX, ty = t / f.tilesX;
        const int w = std::min(f.tile, f.W - tx * f.tile), h = std::min(f.tile, f.H - ty * f.tile);
        out->owned_pixels[t % g->n] += (uint64_t)w * (uint64_t)h;
    }
    return HR_OK;
}

int hr_group_member_stats(hr_ctx *c, int32_t member, hr_pass_stats *stats, hr_kernel_times *times)
{
    if (!c) return HR_ERR_INVALID;
    if (!c->grp) FAIL(c, HR_ERR_INVALID, "not a context group");
    if (member < 0 || member >= c->grp->n) FAIL(c, HR_ERR_INVALID, "no such member");
    return groupOne(c, member, [stats, times](hr_ctx *m) {
        int rc = stats ? hr_get_stats(m, stats) : HR_OK;
        if (rc == HR_OK && times) rc = hr_get_kernel_times(m, times);
        return rc;
    });
}

} // extern "C"
