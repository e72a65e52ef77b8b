// hr_core.hip — host side of libhrcore: the C-ABI of include/hrcore.h over the HIP kernels.
//
// Owns device memory (scene, BVH, tables, ray queues, accumulation buffer) and sequences the kernels of
// a pass.  There is no CPU rendering path in this library: without a usable HIP device every entry point
// that needs one fails with HR_ERR_DEVICE.
//
//   hr_ctx.h          the context (what the opaque handle points to), the error macros
//   hr_owned.h        the owning handles every device buffer, pinned buffer, event and stream is held through: the one place that frees them
//   hr_features.h     the state of the post-process features, one struct per feature with a release(); ResultCounters
//   hr_step_memory.h  the bytes a macro step takes from scratch and from the step arena, stated once (host-only, like hr_tune.h)
//   hr_core.hip       this file: context life cycle, frame, display, read-backs, statistics
//   hr_scene.inl      geometry ingest, commit (build / refit / tree cache), textures, materials, lights, sample tables
//   hr_pipeline.inl   ray memory, the macro step, batching and the packet selector, hr_render_pass, the step log
//   hr_group.inl      context groups (include/hrcore_group.h): member threads, the assembly of the members' tiles
//   hr_postprocess.inl  what the sections below share: the copy out on a caller's stream, "is the frame ready for a full-frame
//                     post-process?", and the four functions that say when each feature's state goes (planes gone, frame resized,
//                     frame cleared, context destroyed)
//   hr_aov.inl        the AOV planes (include/hrcore_aov.h);  hr_denoise.inl  the denoiser over them (include/hrcore_denoise.h)
//   hr_denoise_spatial.inl  the denoiser with a spatial variance estimate for pixels with few samples (include/hrcore_denoise_spatial.h)
//   hr_despeckle.inl  firefly suppression: the outlier clamp the denoiser can be run behind (include/hrcore_despeckle.h)
//   hr_mesh.inl       mesh preparation: smooth normals and tangent frames for a mesh without them (include/hrcore_mesh.h)
//   hr_deform.inl     deformable meshes: vertex updates in place, device posing, read-back (include/hrcore_deform.h)
//   hr_query.inl      ray queries: the caller's rays traced against the committed scene, with surface records (include/hrcore_query.h)
//   hr_motion.inl     motion reprojection: the history gathered where a moved or deformed surface was (include/hrcore_motion.h)
//   hr_adaptive.inl   the sample mask and the error estimate that builds it (include/hrcore_adaptive.h)
//   hr_history.inl    history reprojection across a camera change (include/hrcore_history.h)
//   hr_reproject.inl  its progressive form and the preview of unsampled pixels (include/hrcore_reproject.h)
//   hr_exposure.inl   auto-exposure: the luminance histogram, its reduce and the metered display (include/hrcore_exposure.h)
//   hr_metric.inl     the convergence metric: exact relative L2 against a reference, or predicted from the moments (include/hrcore_metric.h)
// (one translation unit: the .inl files are sections of this one, included below)
// The kernels it launches are units of their own (declared in hr_kernels.h): the render stages hr_raygen.hip, hr_trace.hip, hr_shade.hip and
// hr_frame.hip (resolve, shard exchange, display) over what they share in hr_wave.h; hr_build.hip (scene assembly, the tree) and hr_tables.hip (the table generators); one unit per post-process feature.
#include "hr_ctx.h"

static const int kTableRing = 4;
static int drainPipeline(hr_ctx *c);
static void featuresPlanesGone(hr_ctx *c), featuresFrameResized(hr_ctx *c), featuresFrameCleared(hr_ctx *c), featuresDestroyed(hr_ctx *c); // hr_postprocess.inl: when the features' state goes
// A kernel found a ray queue longer than its capacity (hr_wave.h: queueOverflow): rays were dropped, the frame is not the render
// that was asked for.  Sticky until hr_clear; every call that hands finished work to the caller reports it.
static int overflowCheck(hr_ctx *c)
{
    if (!c->hOverflow || c->hOverflow[0] == 0u) return HR_OK;
    static const char *kinds[] = {"?", "camera rays", "closest-hit queue (input)", "occlusion queue (input)", "closest-hit queue (emitted rays)", "occlusion queue (emitted rays)", "hit list"};
    const uint32_t kind = c->hOverflow[0];
    c->err = std::string("ray queue overflow: ") + kinds[kind < 7u ? kind : 0u] + " of table entry " + std::to_string(c->hOverflow[2]) + " in macro step " +
             std::to_string(c->hOverflow[1] ? c->hOverflow[1] - 1u : 0u) + " held " + std::to_string(c->hOverflow[3]) +
             " rays, more than the host provided for; rays were dropped (hr_clear resets the frame and this report)";
    return HR_ERR_DEVICE;
}
// finish every enqueued pass and wait for the device: required before anything the in-flight kernels read changes
static int quiesce(hr_ctx *c)
{
    int rc = drainPipeline(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, c->query.wait()); // (include/hrcore_query.h: a ray query in flight on a caller's stream reads the committed scene)
    return HR_OK;
}
#define QUIESCE(ctx)              \
    do {                          \
        int rc_ = quiesce(ctx);   \
        if (rc_) return rc_;      \
    } while (0)

static int occupiedSlots(const hr_ctx *c, int group = -1);
// Batching and the pass pipeline are driven by the passes that follow.  A caller that issues ONE pass per displayed frame (the viewer
// at its refresh rate) must not wait for a batch to fill, nor for ten more passes to push this one through its stages: when the oldest
// unfinished request is more than 4 ms old AND no group has work in flight on the device, everything requested is completed now
// (enqueued, not waited for).  A caller that issues passes faster than the device renders them never meets both conditions for long:
// its passes keep travelling in full batches through a full pipeline.  Called by the progressive (display) read-backs.
static int completeForSlowCaller(hr_ctx *c)
{
    if (c->oldestWaitingNs == 0 || (c->pendingInject.empty() && occupiedSlots(c) == 0)) return HR_OK;
    const unsigned long long now = (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    if (c->tune.slow <= 0 || now - c->oldestWaitingNs <= 1000000ull * (unsigned long long)c->tune.slow) return HR_OK; // (HR_TUNE slow=0: never, for tests of the lag itself)
    for (int g = 0; g < c->nGroups; ++g) {
        const hipError_t q = hipStreamQuery(c->groups[g].stream);
        if (q == hipErrorNotReady) return HR_OK; // work in flight: the pipeline is being fed
        HIP_TRY(c, q);                           // (anything else is a real error of an earlier launch)
    }
    return drainPipeline(c);
}
static void freeLagged(hr_ctx::Lagged &L)
{
    for (int k = 0; k < 3; ++k) L.pinned[k].reset(), L.dev[k].reset(), L.ev[k].reset(), L.pending[k] = false;
    L.bytes = 0;
}

static int ensureLagged(hr_ctx *c, hr_ctx::Lagged &L, size_t bytes, bool withDevice)
{
    if (L.bytes >= bytes && (!withDevice || L.dev[0])) return HR_OK;
    freeLagged(L);
    for (int k = 0; k < 3; ++k) {
        HIP_TRY(c, L.pinned[k].alloc(bytes));
        if (withDevice) HIP_TRY(c, L.dev[k].alloc(bytes));
        HIP_TRY(c, L.ev[k].create(hipEventDisableTiming));
    }
    L.bytes = bytes;
    return HR_OK;
}

// slot to fill now; afterwards `finishLagged` picks what to hand out
static int beginLagged(hr_ctx::Lagged &L) { return L.turn++ % 3; }
// (`passesNow`: complete passes in the snapshot just enqueued; `idle`: no pass is pending or in flight — a context group's are its members')
static int finishLaggedAt(hr_ctx *c, hr_ctx::Lagged &L, int k, int32_t format, const void **out, uint32_t *passes, uint32_t passesNow, bool idle)
{
    HIP_TRY(c, hipEventRecord(L.ev[k], c->stream));
    L.pending[k] = true, L.epoch[k] = c->snapshotEpoch, L.format[k] = format;
    L.passes[k] = passesNow;
    const int prev = (k + 2) % 3;
    // nothing in flight (e.g. right after a complete readback): the current snapshot is final, hand it out itself
    const int use = (!idle && L.pending[prev] && L.epoch[prev] == c->snapshotEpoch && L.format[prev] == format && L.passes[prev] > 0) ? prev : k;
    HIP_TRY(c, hipEventSynchronize(L.ev[use]));
    *out = L.pinned[use];
    if (passes) *passes = L.passes[use];
    return HR_OK;
}
static int finishLagged(hr_ctx *c, hr_ctx::Lagged &L, int k, int32_t format, const void **out, uint32_t *passes)
{
    return finishLaggedAt(c, L, k, format, out, passes, (uint32_t)(c->nextResolveOrder - c->resolvedAtClear), c->pendingInject.empty() && occupiedSlots(c) == 0);
}

static void freeQueues(hr_ctx *c)
{
    for (hr_ctx::PassSlot &ps : c->slots) ps = hr_ctx::PassSlot();
    for (hr_ctx::Group &G : c->groups) {
        G.arena[0] = hr_ctx::Group::Region(), G.arena[1] = hr_ctx::Group::Region(), G.scratch = hr_ctx::Group::Region();
        G.arenaHighWater = 0;
    }
    c->nSlotsAllocated = 0;
    c->queueCapacity = 0;
    c->budgetSeen.forget(); // (memory budget: back to the guarantee until the stages have been seen again)
}

// how many passes may be in flight: a slot holds a pass buffer (four partial sums once HR_ESTIMATOR_ALL_LIGHTS has been used); the rays
// live in the groups' step arenas, about 7 KB per owned pixel of the frame for both generations of a step's young passes (below)
static void slotBudget(hr_ctx *c)
{
    size_t freeB = 0, totalB = 0;
    c->maxSlots = kMaxSlots;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
        const size_t fbBytes = (size_t)c->W * c->H * 4 * sizeof(float);
        const size_t k = (c->allLightsUsed ? 4 : 1) + c->aov.framesPerSlot();
        const size_t perSlot = fbBytes * k + sizeof(Counters);
        const size_t fit = (freeB / 2) / perSlot; // at most half of the free device memory for pass slots
        c->maxSlots = fit < 1 ? 1 : (fit > (size_t)kMaxSlots ? kMaxSlots : (int)fit);
    }
}

// AOVs (include/hrcore_aov.h): the frame's planes of the enabled mask at the frame's size, zeroed on the ctx stream
static int aovAllocPlanes(hr_ctx *c)
{
    c->aov.freePlanes();
    featuresPlanesGone(c);
    c->aov.zeroedAt = c->nextResolveOrder;
    if (c->W <= 0) return HR_OK;
    const size_t bytes = (size_t)c->W * c->H * 4 * sizeof(float);
    const bool want[3] = {(c->aov.mask & HR_AOV_SURFACE) != 0, (c->aov.mask & HR_AOV_SURFACE) != 0, (c->aov.mask & HR_AOV_MOMENTS) != 0};
    for (int p = 0; p < 3; ++p) {
        if (!want[p]) continue;
        HIP_TRY(c, c->aov.plane[p].alloc(bytes / sizeof(float)));
        HIP_TRY(c, hipMemsetAsync(c->aov.plane[p], 0, bytes, c->stream));
    }
    return HR_OK;
}

// the one place that frees a tree (BuildResult is hr_kernels.h's, shared with the build unit: it stays raw)
static void freeTree(BuildResult &br)
{
    hipFree(br.nodes), hipFree(br.nodes32), hipFree(br.leafKeys), hipFree(br.tris), hipFree(br.nodeBox), hipFree(br.slotOfPrim);
    br = BuildResult{};
}
static void freeTree(hr_ctx *c)
{
    freeTree(c->tree);
    c->nodes = nullptr, c->tris = nullptr, c->treeTris = 0;
}

// Context groups (hr_group.inl, included at the end of this file): every entry point hands a group handle to one of these.
static int groupAll(hr_ctx *c, const std::function<int(hr_ctx *, int)> &fn);
static int groupOne(hr_ctx *c, int i, const std::function<int(hr_ctx *)> &fn);
static int groupAllId(hr_ctx *c, int32_t *out, const char *what, const std::function<int(hr_ctx *, int, int32_t *)> &fn);
static int groupUnsupported(hr_ctx *c, const char *what);
static int groupDestroy(hr_ctx *c);
static int groupSetStream(hr_ctx *c, void *stream);
static int groupResize(hr_ctx *c, int32_t w, int32_t h);
static int groupReadback(hr_ctx *c, const float **rgba, int32_t *w, int32_t *h);
static int groupReadbackProgressive(hr_ctx *c, const float **rgba, int32_t *w, int32_t *h, uint32_t *passes);
static int groupDisplay(hr_ctx *c, const hr_display_params *params, int32_t format, void *out, uint32_t *shown);
static int groupDisplayReadback(hr_ctx *c, const hr_display_params *params, int32_t format, const void **pixels, int32_t *width, int32_t *height, uint32_t *shown);
static int groupDevicePtr(hr_ctx *c, void **deviceRgba);
static int groupPassesResolved(hr_ctx *c, uint64_t *passes);
static int groupSync(hr_ctx *c, bool wait);
static int groupClear(hr_ctx *c);
static int groupRenderPass(hr_ctx *c, const hr_pass_params *pp);
static int groupStats(hr_ctx *c, hr_pass_stats *out);
static int groupCommit(hr_ctx *c);
static int groupMultiscatter(hr_ctx *c, float *out, hr_tex_id *outTex);

extern "C" {

uint32_t hr_abi_version(void) { return HR_ABI_VERSION; }

int hr_ctx_create(const hr_ctx_desc *desc, hr_ctx **out)
{
    if (!out) return HR_ERR_INVALID;
    *out = nullptr;
    Tune tune; // (before any HIP call: a malformed HR_TUNE never touches the device)
    std::string bad;
    const char *text = getenv("HR_TUNE");
    if (text && !parseTune(text, tune, bad)) return fprintf(stderr, "hr_ctx_create: HR_TUNE: %s\n", bad.c_str()), HR_ERR_INVALID;
    tune.debugPipe = getenv("HR_DEBUG_PIPE") != nullptr, tune.debugStepTimes = getenv("HR_DEBUG_STEPTIMES") != nullptr;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0) return HR_ERR_DEVICE;
    hr_ctx *c = new hr_ctx();
    c->tune = tune, c->traceBlocks = tune.blocks;
    if (desc) {
        c->device = desc->device_id;
        c->rank = desc->rank;
        c->world = desc->world > 0 ? desc->world : 1;
        c->tile = desc->tile_size > 0 ? desc->tile_size : 32;
        c->stream = (hipStream_t)desc->stream;
        c->memBudget = desc->memory_budget;
        c->collectStats = (desc->flags & HR_CTX_COLLECT_STATS) != 0;
        c->timeKernels = (desc->flags & HR_CTX_TIME_KERNELS) != 0;
    }
    if (c->device < 0 || c->device >= nDev || c->rank < 0 || c->rank >= c->world || (c->tile & 7) != 0) {
        delete c;
        return HR_ERR_INVALID;
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(c->device) != hipSuccess || hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
        delete c;
        return HR_ERR_DEVICE;
    }
    c->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // Memory the host READS WHILE A KERNEL THAT WRITES IT IS RUNNING (queue lengths, probe totals, the overflow report): coherent
    // (uncached on the device side, fine-grained) whatever HIP_HOST_COHERENT says — hipHostMallocDefault leaves that to the environment
    const unsigned kHostSpun = hipHostMallocCoherent | hipHostMallocMapped;
// (hr_ctx_create has no context to leave a message in: what was made so far goes with the context)
#define CREATE_TRY(expr)                \
    do {                                \
        if ((expr) != hipSuccess) {     \
            delete c;                   \
            return HR_ERR_DEVICE;       \
        }                               \
    } while (0)
    for (int g = 0; g < kMaxGroups; ++g) {
        hr_ctx::Group &G = c->groups[g];
        // Worker streams at the highest stream priority, created before anything else uses the device queues: HIP maps the
        // streams of one priority to a small pool of hardware queues, and two groups that land on the same queue do not
        // overlap at all — which happened as soon as the application had a few streams of its own (torch side stream, RCCL).
        // The high-priority pool is practically empty, so the groups get a hardware queue each.  (Creating them lazily, at
        // the first macro step, measurably loses overlap on half- and quarter-frame shards.)
        int least = 0, greatest = 0;
        CREATE_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        CREATE_TRY(G.stream.createWithPriority(hipStreamNonBlocking, c->tune.prio ? greatest : 0));
        CREATE_TRY(G.streamB.createWithPriority(hipStreamNonBlocking, c->tune.prio ? greatest : 0));
        CREATE_TRY(G.evFork.create(hipEventDisableTiming));
        CREATE_TRY(G.evJoin.create(hipEventDisableTiming));
        CREATE_TRY(G.dTables.alloc(kTableRing));
        CREATE_TRY(G.hTables.alloc(kTableRing));
        CREATE_TRY(G.hTables.devicePointer(&G.dTablesHost));
        CREATE_TRY(G.evUser.create(hipEventDisableTiming));
        for (Event &e : G.tableCopied) CREATE_TRY(e.create(hipEventDisableTiming));
        for (Event &e : G.statusEv) CREATE_TRY(e.create(hipEventDisableTiming));
        CREATE_TRY(G.hQCount.alloc((size_t)kTableRing * kMaxSlots * kMaxBounceSlots));
        CREATE_TRY(G.hCounts.alloc(kTableRing * kMaxSegs + 1, kHostSpun));
        CREATE_TRY(G.hSeq.alloc(kTableRing, kHostSpun));
        CREATE_TRY(G.hCounts.devicePointer(&G.dCounts));
        CREATE_TRY(G.hSeq.devicePointer(&G.dSeq));
        CREATE_TRY(G.hProbe.alloc(kTableRing * 8, kHostSpun));
        CREATE_TRY(G.hProbe.devicePointer(&G.dProbeHost));
        G.hCounts[kTableRing * kMaxSegs] = 0u; // (the last word: StepTable::hostCameraCount)
        for (int k = 0; k < kTableRing; ++k) G.hSeq[k] = 0ull, G.hProbe[8 * k] = 0ull, G.hProbe[8 * k + 1] = 0ull, G.hProbe[8 * k + 2] = 0ull, G.hProbe[8 * k + 3] = 0ull, G.hProbe[8 * k + 4] = 0ull;
        std::memset(G.statusOrder, 0, sizeof(G.statusOrder));
    }
    CREATE_TRY(c->hOverflow.alloc(4, kHostSpun));
    CREATE_TRY(c->hOverflow.devicePointer(&c->dOverflowHost));
    c->hOverflow[0] = c->hOverflow[1] = c->hOverflow[2] = c->hOverflow[3] = 0u;
    CREATE_TRY(c->dScene.alloc(1));
    CREATE_TRY(c->dStats.alloc(kStatSlots));
    CREATE_TRY(c->dScratch.alloc(6 * kBoundSlots));
    CREATE_TRY(c->dZero.alloc(64 / sizeof(uint32_t)));
    CREATE_TRY(c->selector.dProbe.alloc(64 / sizeof(unsigned long long)));
    CREATE_TRY(hipMemset(c->selector.dProbe, 0, 64));
    CREATE_TRY(c->selector.probeStream.create(hipStreamNonBlocking));
    CREATE_TRY(c->selector.evProbeA.create(hipEventDisableTiming));
    CREATE_TRY(c->selector.evProbeB.create(hipEventDisableTiming));
    CREATE_TRY(c->dCounters.alloc(kMaxSlots));
    CREATE_TRY(c->dStepLog.alloc(3 * kStepLogCap));
#undef CREATE_TRY
    hipMemset(c->dStats, 0, sizeof(Stats) * kStatSlots);
    hipMemset(c->dZero, 0, 64);
    *out = c;
    return HR_OK;
}

// What must happen in order happens here; then the context is deleted and every handle it holds frees what it owns.  The one invariant
// that replaces a list of frees: nothing may still be in flight when the members go, and the steps before the delete ensure that.
int hr_ctx_destroy(hr_ctx *c)
{
    if (!c) return HR_OK;
    if (c->grp) return groupDestroy(c);
    hipSetDevice(c->device);
    if (c->tune.debugPipe)
        fprintf(stderr, "hr_ctx %p: ray-memory growths %llu (last sizes summed %.1f MiB); queue-length waits %llu, of which %llu had to spin, %.2f ms in total\n", (void *)c,
                c->dbgGrowths, (double)c->dbgGrowBytes / 1048576.0, c->dbgWaits, c->dbgWaitSpun, (double)c->dbgWaitNs * 1e-6);
    drainPipeline(c);
    hipStreamSynchronize(c->stream);
    c->query.wait(); // (ray queries in flight on a caller's stream)
    if (c->selector.probeStream) hipStreamSynchronize(c->selector.probeStream);
    c->drainTimes();
    featuresDestroyed(c);
    freeTree(c); // (the two kept raw: the tree, and the bindings of deformable meshes)
    for (Geom &g : c->geoms) deformRelease(g);
    delete c;
    return HR_OK;
}

const char *hr_last_error(const hr_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

int hr_ctx_set_stream(hr_ctx *c, void *stream)
{
    ENTER(c);
    if (c->grp) return groupSetStream(c, stream);
    QUIESCE(c);
    c->stream = (hipStream_t)stream;
    return HR_OK;
}

// the frame geometry of `rank` of `world` (the ctx's own when they match its description)
static FrameDev frameOf(const hr_ctx *c, int32_t rank, int32_t world)
{
    FrameDev f = c->frame;
    f.rank = rank, f.world = world;
    const int nTiles = f.tilesX * f.tilesY;
    f.nOwnedTiles = nTiles > rank ? (nTiles - rank + world - 1) / world : 0;
    return f;
}

int hr_frame_packed_slots(hr_ctx *c, int32_t rank, int32_t world, uint64_t *n_slots)
{
    ENTER(c);
    if (c->grp) return groupUnsupported(c, "hr_frame_packed_slots");
    if (!n_slots || world <= 0 || rank < 0 || rank >= world) FAIL(c, HR_ERR_INVALID, "bad rank / world");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    *n_slots = (uint64_t)frameOf(c, rank, world).nOwnedTiles * (uint64_t)(c->tile * c->tile);
    return HR_OK;
}

int hr_frame_pack_owned(hr_ctx *c, void *device_out, void *stream)
{
    ENTER(c);
    if (c->grp) return groupUnsupported(c, "hr_frame_pack_owned");
    if (!device_out) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    FrameDev fr = c->frame;
    fr.fb = c->fb();
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (st != c->stream) { // the resolves enqueued so far run on the ctx stream: order the copy behind them
        if (!c->evPack) HIP_TRY(c, c->evPack.create(hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->evPack, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(st, c->evPack, 0));
    }
    launchPackOwned(c->cfg(st), fr, c->fb(), (float *)device_out, 0, nullptr);
    HIP_TRY(c, hipGetLastError());
    if (st != c->stream) { // ... and the next resolve (which rewrites the frame) behind the copy
        HIP_TRY(c, hipEventRecord(c->evPack, st));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evPack, 0));
    }
    return HR_OK;
}

int hr_frame_unpack(hr_ctx *c, int32_t src_rank, int32_t world, const void *device_packed, void *device_full_frame, void *stream)
{
    ENTER(c);
    if (c->grp) return groupUnsupported(c, "hr_frame_unpack");
    if (!device_packed || !device_full_frame) FAIL(c, HR_ERR_INVALID, "null argument");
    if (world <= 0 || src_rank < 0 || src_rank >= world) FAIL(c, HR_ERR_INVALID, "bad rank / world");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    launchPackOwned(c->cfg(stream ? (hipStream_t)stream : c->stream), frameOf(c, src_rank, world), nullptr, (float *)device_packed, 1,
                    (float *)device_full_frame);
    HIP_TRY(c, hipGetLastError());
    return HR_OK;
}

static size_t displayPixelBytes(int32_t format) { return format == HR_DISPLAY_RGBA8 ? 4 : 16; }
// the display read-backs' device staging and its pinned host copy, at least `need` bytes each; they only grow
static int growDisplay(hr_ctx *c, size_t need)
{
    HIP_TRY(c, c->dDisplay.reserve(need));
    return growPinned(c, c->pinnedDisplay, need);
}

int hr_display(hr_ctx *c, const hr_display_params *params, int32_t format, void *device_out, uint32_t *passes_shown)
{
    ENTER(c);
    if (c->grp) return groupDisplay(c, params, format, device_out, passes_shown);
    if (!params || !device_out) FAIL(c, HR_ERR_INVALID, "null argument");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    const bool progressive = (format & HR_DISPLAY_PROGRESSIVE) != 0;
    format &= ~HR_DISPLAY_PROGRESSIVE;
    if (format < HR_DISPLAY_RGBA8 || format > HR_DISPLAY_HDR_RGBA32F) FAIL(c, HR_ERR_INVALID, "unknown display format");
    if (!progressive) {
        int rc = drainPipeline(c);
        if (rc) return rc;
    }
    FrameDev fr = c->frame;
    fr.fb = c->fb();
    launchDisplay(c->cfg(c->stream), fr, *params, format, device_out);
    HIP_TRY(c, hipGetLastError());
    if (passes_shown) *passes_shown = (uint32_t)(c->nextResolveOrder - c->resolvedAtClear); // (the resolves enqueued before this kernel, same stream)
    return HR_OK;
}

int hr_frame_passes_resolved(hr_ctx *c, uint64_t *passes)
{
    ENTER(c);
    if (c->grp) return groupPassesResolved(c, passes);
    if (!passes) FAIL(c, HR_ERR_INVALID, "null output");
    *passes = c->nextResolveOrder - c->resolvedAtClear;
    return HR_OK;
}

int hr_display_readback(hr_ctx *c, const hr_display_params *params, int32_t format, const void **pixels, int32_t *width, int32_t *height, uint32_t *passes_shown)
{
    ENTER(c);
    if (c->grp) return groupDisplayReadback(c, params, format, pixels, width, height, passes_shown);
    if (!pixels) FAIL(c, HR_ERR_INVALID, "null output");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    {
        const int rc = overflowCheck(c);
        if (rc) return rc;
    }
    const size_t need = (size_t)c->W * c->H * 16;
    if (int rc = growDisplay(c, need)) return rc;
    if (format & HR_DISPLAY_PROGRESSIVE) { // lagged, like hr_readback_progressive
        int rc = completeForSlowCaller(c);
        if (rc) return rc;
        rc = ensureLagged(c, c->progDisplay, need, true);
        if (rc) return rc;
        const int k = beginLagged(c->progDisplay);
        rc = hr_display(c, params, format, c->progDisplay.dev[k], nullptr);
        if (rc) return rc;
        const size_t nb = (size_t)c->W * c->H * displayPixelBytes(format & ~HR_DISPLAY_PROGRESSIVE);
        HIP_TRY(c, hipMemcpyAsync(c->progDisplay.pinned[k], c->progDisplay.dev[k], nb, hipMemcpyDeviceToHost, c->stream));
        // the parameters are part of the snapshot's identity: a change of settings must not hand out an old image
        int32_t key = format;
        for (size_t i = 0; i < sizeof(*params) / 4; ++i) key = key * 31 + ((const int32_t *)params)[i];
        rc = finishLagged(c, c->progDisplay, k, key, pixels, passes_shown); // (the passes of the snapshot handed out, which may be the previous call's)
        if (rc) return rc;
        if (width) *width = c->W;
        if (height) *height = c->H;
        return HR_OK;
    }
    int rc = hr_display(c, params, format, c->dDisplay, passes_shown);
    if (rc) return rc;
    const size_t bytes = (size_t)c->W * c->H * displayPixelBytes(format & ~HR_DISPLAY_PROGRESSIVE);
    HIP_TRY(c, hipMemcpyAsync(c->pinnedDisplay.get(), c->dDisplay, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *pixels = c->pinnedDisplay.get();
    if (width) *width = c->W;
    if (height) *height = c->H;
    return HR_OK;
}

int hr_synchronize(hr_ctx *c)
{
    ENTER(c);
    if (c->grp) return groupSync(c, true);
    QUIESCE(c);
    return overflowCheck(c);
}

// ------------------------------------------------------------------------------------------ frame
int hr_frame_resize(hr_ctx *c, int32_t w, int32_t h)
{
    ENTER(c);
    if (c->grp) return groupResize(c, w, h);
    if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 28)) FAIL(c, HR_ERR_INVALID, "bad frame size");
    QUIESCE(c);
    c->W = w, c->H = h;
    c->snapshotEpoch++;
    c->selector.sceneOrSizeChanged(); // (another resolution)
    freeLagged(c->progFrame), freeLagged(c->progDisplay);
    c->fbInternal.reset();
    c->fbExternal = nullptr;
    featuresFrameResized(c); // (the sample mask goes with the frame it was made for, and so do a captured history and the progressive merge's examined bits)
    const size_t fbBytes = (size_t)w * h * 4 * sizeof(float);
    HIP_TRY(c, c->fbInternal.alloc((size_t)w * h * 4));
    HIP_TRY(c, hipMemsetAsync(c->fbInternal, 0, fbBytes, c->stream));
    c->frameZeroedAt = c->nextResolveOrder;
    if (int rc = growPinned(c, c->pinned, fbBytes)) return rc;
    FrameDev &f = c->frame;
    f.W = w, f.H = h, f.rank = c->rank, f.world = c->world, f.tile = c->tile;
    f.tilesX = (w + c->tile - 1) / c->tile, f.tilesY = (h + c->tile - 1) / c->tile;
    const int nTiles = f.tilesX * f.tilesY;
    f.nOwnedTiles = nTiles > c->rank ? (nTiles - c->rank + c->world - 1) / c->world : 0;
    // one path per owned pixel and pass: queue capacity = owned tiles x tile^2; pass slots are allocated on demand
    freeQueues(c);
    {
        const int rc = aovAllocPlanes(c);
        if (rc) return rc;
    }
    c->queueCapacity = (uint32_t)f.nOwnedTiles * (uint32_t)(c->tile * c->tile);
    // how many passes may be in flight: each slot holds two ray queues, an occlusion queue, hit records and a pass buffer
    slotBudget(c);
    {
        // Paths per macro step worth launching for.  A trace launch ends in a tail of a few long rays (0.5-0.7 ms whatever it
        // carries) and every pass costs depth + 2 dependent launches, so passes requested back to back are collected and injected
        // together: 9 passes of a 1080p frame per step measured 1715 against 1607 Mrays/s (128 passes) and 1488 against 1400
        // (20 passes) for one at a time on two pipeline groups (profiles/r2b_batch_sweep*.txt).  Round 3, with the small launches
        // dealt out statically and the shading stage split: 11-14 passes per step are another 3-4 % over 9 at 20 passes and 2 % at
        // 128 (profiles/r3n_batch_sweep.txt); 12 it is (120 pass buffers of a 1080p frame and the step arenas: ~21 GB of the 288; 53 GB before round 4 sized the queues by stage).  A caller that asks for
        // pixels after every pass (hr_readback) completes what is pending, so batching never delays a displayed frame.
        const long long target = 12ll * 1920ll * 1080ll;
        const long long own = c->queueCapacity ? c->queueCapacity : 1;
        long long b = (target + own - 1) / own;
        c->injectBatch = (int)(b < 1 ? 1 : (b > HR_BATCH_CAP ? HR_BATCH_CAP : b));
        if (c->tune.batch > 0) c->injectBatch = c->tune.batch;
        // Two pipeline groups (their steps alternate on two streams, so one group's trace tail and its shade / raygen run
        // under the other group's trace) pay off only while a launch carries little work: +11..14 % on a 1080p frame at one pass
        // per step; with several passes per step one group (five trace workgroups per CU) is as fast or faster (1697 vs 1696
        // Mrays/s at 8 passes per step) and needs half the pass slots.
        c->nGroups = c->tune.groups > 0 ? c->tune.groups : (c->injectBatch >= 4 || c->queueCapacity > 4200000u ? 1 : 2);
        c->nextGroup = 0;
        c->traceBlocks = c->tune.blocksSet ? c->tune.blocks : (c->nGroups > 1 ? 3 : 5);
        c->pendingInject.clear();
    }
    return HR_OK;
}

int hr_frame_bind_external(hr_ctx *c, void *deviceRgba)
{
    ENTER(c);
    if (c->grp) return groupUnsupported(c, "hr_frame_bind_external");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    QUIESCE(c);
    c->fbExternal = (float *)deviceRgba;
    c->snapshotEpoch++;
    return HR_OK;
}

int hr_frame_device_ptr(hr_ctx *c, void **deviceRgba)
{
    ENTER(c);
    if (c->grp) return groupDevicePtr(c, deviceRgba);
    if (c->W <= 0 || !deviceRgba) FAIL(c, HR_ERR_INVALID, "no frame");
    *deviceRgba = c->fb();
    return HR_OK;
}

// --------------------------------------------------------------------------------------- geometry
#include "hr_scene.inl"
#include "hr_pipeline.inl"

int hr_readback(hr_ctx *c, const float **rgba, int32_t *w, int32_t *h)
{
    ENTER(c);
    if (c->grp) return groupReadback(c, rgba, w, h);
    if (c->W <= 0 || !rgba) FAIL(c, HR_ERR_INVALID, "no frame");
    const size_t bytes = (size_t)c->W * c->H * 4 * sizeof(float);
    {
        int rc = drainPipeline(c);
        if (rc) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(c->pinned.get(), c->fb(), bytes, hipMemcpyDeviceToHost, c->stream));
    QUIESCE(c);
    {
        const int rc = overflowCheck(c);
        if (rc) return rc;
    }
    *rgba = c->pinned.get();
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

int hr_readback_progressive(hr_ctx *c, const float **rgba, int32_t *w, int32_t *h, uint32_t *passes)
{
    ENTER(c);
    if (c->grp) return groupReadbackProgressive(c, rgba, w, h, passes);
    if (c->W <= 0 || !rgba) FAIL(c, HR_ERR_INVALID, "no frame");
    const size_t bytes = (size_t)c->W * c->H * 4 * sizeof(float);
    int rc = completeForSlowCaller(c);
    if (rc == HR_OK) rc = overflowCheck(c);
    if (rc) return rc;
    // no drain: the resolves enqueued so far are ordered before this copy on the ctx stream
    rc = ensureLagged(c, c->progFrame, bytes, false);
    if (rc) return rc;
    const int k = beginLagged(c->progFrame);
    HIP_TRY(c, hipMemcpyAsync(c->progFrame.pinned[k], c->fb(), bytes, hipMemcpyDeviceToHost, c->stream));
    const void *out = nullptr;
    rc = finishLagged(c, c->progFrame, k, 0, &out, passes);
    if (rc) return rc;
    *rgba = (const float *)out;
    if (w) *w = c->W;
    if (h) *h = c->H;
    return HR_OK;
}

int hr_debug_trace(hr_ctx *c, int32_t n, const float *o, const float *d, const float *tmax, const int32_t *skip, int32_t anyHit, hr_hit *out)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_debug_trace(m, n, o, d, tmax, skip, anyHit, out); });
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    if (n <= 0 || !o || !d || !out) FAIL(c, HR_ERR_INVALID, "bad arguments");
    int rc = uploadScene(c);
    if (rc) return rc;
    DeviceBuf<float> dO, dD, dT;
    DeviceBuf<int> dS;
    DeviceBuf<hr_hit> dH;
    HIP_TRY(c, dO.alloc((size_t)n * 3));
    HIP_TRY(c, dD.alloc((size_t)n * 3));
    HIP_TRY(c, dH.alloc((size_t)n));
    HIP_TRY(c, hipMemcpy(dO, o, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dD, d, (size_t)n * 12, hipMemcpyHostToDevice));
    if (tmax) {
        HIP_TRY(c, dT.alloc((size_t)n));
        HIP_TRY(c, hipMemcpy(dT, tmax, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (skip) {
        HIP_TRY(c, dS.alloc((size_t)n));
        HIP_TRY(c, hipMemcpy(dS, skip, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    launchDebugTrace(c->cfg(c->stream), c->dScene, n, dO, dD, dT, dS, anyHit, dH);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dH, (size_t)n * sizeof(hr_hit), hipMemcpyDeviceToHost));
    return HR_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------ context groups
#include "hr_group.inl"

// ------------------------------------------------------------------------------------------ what the post-process sections share
#include "hr_postprocess.inl"

// ------------------------------------------------------------------------------------------ AOVs
#include "hr_aov.inl"

// ------------------------------------------------------------------------------------------ denoiser
#include "hr_denoise.inl"

// ------------------------------------------------------------------------------------------ adaptive sampling
#include "hr_adaptive.inl"

// ------------------------------------------------------------------------------------------ history reprojection
#include "hr_history.inl"

// ------------------------------------------------------------------------------------------ progressive merge and preview
#include "hr_reproject.inl"

// ------------------------------------------------------------------------------------------ denoiser with the spatial variance estimate
#include "hr_denoise_spatial.inl"

// ------------------------------------------------------------------------------------------ firefly suppression ahead of the denoiser
#include "hr_despeckle.inl"

// ------------------------------------------------------------------------------------------ auto-exposure
#include "hr_exposure.inl"

// ------------------------------------------------------------------------------------------ convergence metric
#include "hr_metric.inl"

// ------------------------------------------------------------------------------------------ mesh preparation
#include "hr_mesh.inl"

// ------------------------------------------------------------------------------------------ deformable meshes
#include "hr_deform.inl"

// ------------------------------------------------------------------------------------------ ray queries
#include "hr_query.inl"

// ------------------------------------------------------------------------------------------ motion reprojection
#include "hr_motion.inl"
