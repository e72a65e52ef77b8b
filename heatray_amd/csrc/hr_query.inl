// hr_query.inl — a section of hr_core.hip (included at its end, behind hr_deform.inl): the entry points of include/hrcore_query.h.  The
// kernels are in hr_query.hip, the arithmetic in hr_query.h.  Every refusal is decided on the host before anything is launched.
//
// Ordering.  A query reads what hr_scene_commit wrote (the tree, the triangles, the attributes), the scene block uploadScene wrote and
// the context's own table of mesh ids; it writes the caller's outputs and the context's counters.  It is enqueued on the caller's stream
// (null: the context's) behind an event recorded on the context's stream, where the two differ, and behind the previous query's evDone
// where THAT ran on another stream: the queries of a context run one after the other, so one set of counters serves them.  evDone is
// recorded behind every query (and behind the copy of its counters to pinned memory); QueryState::wait, called by quiesce and
// hr_ctx_destroy, is how a commit, an upload of the scene block and the destruction wait for queries in flight.  The pass pipeline's
// streams are never waited for, except by the scene block's upload where it is due (as for the first pass after a change).
//
// A group's handle owns no scene: member 0 serves every call.

static int queryScratch(hr_ctx *c, size_t bytes)
{
    QueryState &q = c->query;
    if (q.scratch.capacity() >= bytes) return HR_OK;
    HIP_TRY(c, q.wait()); // (the host calls are synchronous: nothing of theirs is in flight; a device-side query does not use the scratch)
    HIP_TRY(c, q.scratch.reserve(bytes));
    return HR_OK;
}

// what every query needs beside its rays: the scene block on the device, the table of mesh ids, the counters and the two events
static int queryPrepare(hr_ctx *c)
{
    QueryState &q = c->query;
    int rc = uploadScene(c);
    if (rc) return rc;
    if (!q.evOrder) HIP_TRY(c, q.evOrder.create(hipEventDisableTiming));
    if (!q.evDone) HIP_TRY(c, q.evDone.create(hipEventDisableTiming));
    HIP_TRY(c, q.counters.ensure(kQyCounterWords));
    if (q.geomsStale) { // (set by every commit, which has waited for the queries in flight)
        std::vector<QyGeom> t;
        uint32_t nTris = 0;
        for (size_t id = 0; id < c->geoms.size(); ++id) { // hr_scene_commit's list: the live meshes that have triangles, in id order
            const Geom &g = c->geoms[id];
            if (!g.alive || g.nTris() == 0) continue;
            t.push_back(QyGeom{nTris, (int32_t)id});
            nTris += g.nTris();
        }
        if (q.geoms.capacity() < t.size() || !q.geoms) {
            HIP_TRY(c, q.wait());
            HIP_TRY(c, q.geoms.reserve(t.size(), 16));
        }
        if (!t.empty()) HIP_TRY(c, hipMemcpy(q.geoms, t.data(), t.size() * sizeof(QyGeom), hipMemcpyHostToDevice));
        q.nGeoms = (int)t.size(), q.geomsStale = false;
    }
    return HR_OK;
}

struct QueryStrides {
    int32_t o, d, t, s;
};

// the desc as all three calls read it (pointers are not dereferenced here)
static int queryCheck(hr_ctx *c, const std::string &what, const hr_query_desc *d, bool devicePointers, QueryStrides *st)
{
    if (!d) FAIL(c, HR_ERR_INVALID, what + "null desc");
    if (d->n < 0) FAIL(c, HR_ERR_INVALID, what + "n = " + std::to_string(d->n) + " is negative");
    if (d->flags & ~HR_QUERY_ANY_HIT) FAIL(c, HR_ERR_INVALID, what + "unknown flags " + std::to_string(d->flags & ~HR_QUERY_ANY_HIT));
    for (int k = 0; k < 3; ++k)
        if (d->reserved[k]) FAIL(c, HR_ERR_INVALID, what + "reserved[" + std::to_string(k) + "] must be 0");
    if (!d->origins) FAIL(c, HR_ERR_INVALID, what + "null origins");
    if (!d->directions) FAIL(c, HR_ERR_INVALID, what + "null directions");
    if (!d->hits && !d->surfaces) FAIL(c, HR_ERR_INVALID, what + "no output: hits and surfaces are both null");
    if ((d->flags & HR_QUERY_ANY_HIT) && d->surfaces) FAIL(c, HR_ERR_INVALID, what + "surfaces with HR_QUERY_ANY_HIT: an occlusion query has no surface");
    const int32_t given[4] = {d->origin_stride, d->direction_stride, d->tmax_stride, d->skip_stride}, elem[4] = {12, 12, 4, 4};
    static const char *const name[4] = {"origin_stride", "direction_stride", "tmax_stride", "skip_stride"};
    int32_t out[4];
    for (int k = 0; k < 4; ++k) {
        if (given[k] != 0 && (given[k] % 4 != 0 || given[k] < elem[k]))
            FAIL(c, HR_ERR_INVALID, what + name[k] + " = " + std::to_string(given[k]) + " is not 0 or a multiple of 4 that is at least " + std::to_string(elem[k]));
        out[k] = given[k] ? given[k] : elem[k];
    }
    *st = QueryStrides{out[0], out[1], out[2], out[3]};
    if (d->tmin != d->tmin) FAIL(c, HR_ERR_INVALID, what + "tmin is NaN");
    if (devicePointers) {
        if ((uintptr_t)d->hits % 16 != 0) FAIL(c, HR_ERR_INVALID, what + "hits must be 16-byte aligned");
        if ((uintptr_t)d->surfaces % 16 != 0) FAIL(c, HR_ERR_INVALID, what + "surfaces must be 16-byte aligned");
        if ((uintptr_t)d->origins % 4 != 0 || (uintptr_t)d->directions % 4 != 0 || (uintptr_t)d->tmax % 4 != 0 || (uintptr_t)d->skip_prim % 4 != 0)
            FAIL(c, HR_ERR_INVALID, what + "the ray arrays must be 4-byte aligned");
    }
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    return HR_OK;
}

// Enqueues one query on `stream` (null: the context's): the counters zeroed, the kernel, the counters to pinned memory, evDone.
static int queryEnqueue(hr_ctx *c, QyArgs a, bool anyHit, void *stream)
{
    QueryState &q = c->query;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (st != c->stream) { // behind the last commit, the scene block and whatever query ran on the context's stream
        HIP_TRY(c, hipEventRecord(q.evOrder, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(st, q.evOrder, 0));
    }
    if (q.inFlight && q.lastStream != st) HIP_TRY(c, hipStreamWaitEvent(st, q.evDone, 0)); // (the previous query, on another stream: it owns the counters)
    a.scene = c->dScene, a.slotOfPrim = c->tree.slotOfPrim, a.geoms = q.geoms, a.nGeoms = q.nGeoms, a.counters = q.counters.dev;
    if (c->hScene.nTris == 0) a.slotOfPrim = nullptr; // (an empty scene has no tree: traverse returns at once)
    HIP_TRY(c, q.counters.zero(st));
    launchQueryTrace(st, a, anyHit);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, q.counters.fetch(st));
    HIP_TRY(c, hipEventRecord(q.evDone, st));
    q.inFlight = true, q.lastStream = st, q.lastRays = (uint64_t)a.n, q.done = true;
    return HR_OK;
}

static size_t queryAlign(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" {

uint32_t hr_query_api_version(void) { return HR_QUERY_API_VERSION; }

int hr_query_trace(hr_ctx *c, const hr_query_desc *d, void *stream)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_query_trace(m, d, stream); });
    QueryStrides s;
    int rc = queryCheck(c, "query_trace: ", d, true, &s);
    if (rc) return rc;
    if (d->n == 0) return HR_OK;
    rc = queryPrepare(c);
    if (rc) return rc;
    QyArgs a{};
    a.origins = (const char *)d->origins, a.directions = (const char *)d->directions, a.tmax = (const char *)d->tmax, a.skip = (const char *)d->skip_prim;
    a.oStride = s.o, a.dStride = s.d, a.tStride = s.t, a.sStride = s.s, a.n = d->n, a.tmin = d->tmin, a.hits = d->hits, a.surfaces = d->surfaces;
    return queryEnqueue(c, a, (d->flags & HR_QUERY_ANY_HIT) != 0, stream);
}

int hr_query_trace_host(hr_ctx *c, const hr_query_desc *d)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_query_trace_host(m, d); });
    QueryStrides s;
    int rc = queryCheck(c, "query_trace_host: ", d, false, &s);
    if (rc) return rc;
    if (d->n == 0) return HR_OK;
    rc = queryPrepare(c);
    if (rc) return rc;
    // ---- the scratch: every input as the caller laid it out (its stride kept), then the outputs
    const size_t n = (size_t)d->n;
    const size_t bO = (n - 1) * (size_t)s.o + 12, bD = (n - 1) * (size_t)s.d + 12, bT = d->tmax ? (n - 1) * (size_t)s.t + 4 : 0, bS = d->skip_prim ? (n - 1) * (size_t)s.s + 4 : 0;
    const size_t bH = d->hits ? n * sizeof(hr_hit) : 0, bF = d->surfaces ? n * sizeof(hr_query_surface) : 0;
    const size_t oO = 0, oD = oO + queryAlign(bO), oT = oD + queryAlign(bD), oS = oT + queryAlign(bT), oH = oS + queryAlign(bS), oF = oH + queryAlign(bH);
    rc = queryScratch(c, oF + queryAlign(bF));
    if (rc) return rc;
    char *base = c->query.scratch;
    HIP_TRY(c, hipMemcpyAsync(base + oO, d->origins, bO, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(base + oD, d->directions, bD, hipMemcpyHostToDevice, c->stream));
    if (bT) HIP_TRY(c, hipMemcpyAsync(base + oT, d->tmax, bT, hipMemcpyHostToDevice, c->stream));
    if (bS) HIP_TRY(c, hipMemcpyAsync(base + oS, d->skip_prim, bS, hipMemcpyHostToDevice, c->stream));
    QyArgs a{};
    a.origins = base + oO, a.directions = base + oD, a.tmax = bT ? base + oT : nullptr, a.skip = bS ? base + oS : nullptr;
    a.oStride = s.o, a.dStride = s.d, a.tStride = s.t, a.sStride = s.s, a.n = d->n, a.tmin = d->tmin;
    a.hits = bH ? (hr_hit *)(base + oH) : nullptr, a.surfaces = bF ? (hr_query_surface *)(base + oF) : nullptr;
    rc = queryEnqueue(c, a, (d->flags & HR_QUERY_ANY_HIT) != 0, nullptr);
    if (rc) return rc;
    if (bH) HIP_TRY(c, hipMemcpyAsync(d->hits, base + oH, bH, hipMemcpyDeviceToHost, c->stream));
    if (bF) HIP_TRY(c, hipMemcpyAsync(d->surfaces, base + oF, bF, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->query.inFlight = false; // (evDone was recorded on the stream just waited for)
    return HR_OK;
}

int hr_query_pixels(hr_ctx *c, const hr_pass_params *cam, int32_t n, const float *xy, hr_hit *hits, hr_query_surface *surfaces, float *raysOut)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_query_pixels(m, cam, n, xy, hits, surfaces, raysOut); });
    const std::string what = "query_pixels: ";
    if (!cam) FAIL(c, HR_ERR_INVALID, what + "null camera");
    if (n < 0) FAIL(c, HR_ERR_INVALID, what + "n = " + std::to_string(n) + " is negative");
    if (!xy) FAIL(c, HR_ERR_INVALID, what + "null pixels");
    if (!hits && !surfaces && !raysOut) FAIL(c, HR_ERR_INVALID, what + "no output: hits, surfaces and rays_out are all null");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, what + "no frame");
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    if (n == 0) return HR_OK;
    int rc = queryPrepare(c);
    if (rc) return rc;
    const size_t N = (size_t)n;
    const size_t bX = N * 8, bR = N * 24, bH = hits ? N * sizeof(hr_hit) : 0, bF = surfaces ? N * sizeof(hr_query_surface) : 0;
    const size_t oX = 0, oR = oX + queryAlign(bX), oH = oR + queryAlign(bR), oF = oH + queryAlign(bH);
    rc = queryScratch(c, oF + queryAlign(bF));
    if (rc) return rc;
    char *base = c->query.scratch;
    HIP_TRY(c, hipMemcpyAsync(base + oX, xy, bX, hipMemcpyHostToDevice, c->stream));
    QyCamera k{};
    std::memcpy(k.view, cam->view_matrix, sizeof(k.view));
    k.fovTan = cam->fov_tan, k.aspect = cam->aspect_ratio, k.focus = cam->focus_distance, k.W = (float)c->W, k.H = (float)c->H;
    launchQueryCamera(c->stream, k, n, (const float *)(base + oX), (float *)(base + oR));
    HIP_TRY(c, hipGetLastError());
    if (hits || surfaces) {
        QyArgs a{};
        a.origins = base + oR, a.directions = base + oR + 12, a.oStride = a.dStride = 24, a.tStride = a.sStride = 4, a.n = n, a.tmin = 0.0f;
        a.hits = bH ? (hr_hit *)(base + oH) : nullptr, a.surfaces = bF ? (hr_query_surface *)(base + oF) : nullptr;
        rc = queryEnqueue(c, a, false, nullptr);
        if (rc) return rc;
    }
    const bool traced = hits || surfaces;
    if (bH) HIP_TRY(c, hipMemcpyAsync(hits, base + oH, bH, hipMemcpyDeviceToHost, c->stream));
    if (bF) HIP_TRY(c, hipMemcpyAsync(surfaces, base + oF, bF, hipMemcpyDeviceToHost, c->stream));
    if (raysOut) HIP_TRY(c, hipMemcpyAsync(raysOut, base + oR, bR, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (traced) c->query.inFlight = false; // (evDone was recorded on the stream just waited for)
    return HR_OK;
}

int hr_query_last(hr_ctx *c, hr_query_result *out)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_query_last(m, out); });
    if (!out) FAIL(c, HR_ERR_INVALID, "query_last: null output");
    QueryState &q = c->query;
    if (!q.done) FAIL(c, HR_ERR_INVALID, "query_last: no query has run on this context");
    HIP_TRY(c, q.wait());
    unsigned long long packed = 0, hitsN = 0, invalidN = 0;
    for (int k = 0; k < kQySlots; ++k) {
        packed = q.counters.host[(size_t)k * kQySlotStride];
        hitsN += packed & 0xFFFFFFFFull, invalidN += packed >> 32;
    }
    *out = hr_query_result{};
    out->rays = q.lastRays, out->hits = hitsN, out->invalid = invalidN;
    return HR_OK;
}

} // extern "C"
