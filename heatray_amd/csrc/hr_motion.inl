// hr_motion.inl — a section of hr_core.hip (included at its end, behind hr_query.inl): the entry points of include/hrcore_motion.h.  The
// kernels are in hr_motion.hip, the per-pixel arithmetic and the cameras' arithmetic (mvCameras) in hr_motion.h; the parameter and frame
// checks are hr_history.inl's, the scene block and the table of committed meshes hr_query.inl's (queryPrepare).  Every refusal is decided
// on the host before anything is launched.
//
// Ordering.  Everything runs on the context's stream.  hr_scene_commit returns with its work complete, so a snapshot enqueued behind it
// reads the committed triangles; the next commit starts with quiesce, which waits for the context's stream and so for the snapshot.  A
// trace reads what a commit wrote, the snapshot and two small tables, and waits for the stream because its counters go back to the
// host; a merge runs behind drainPipeline exactly as hr_history_merge does (hr_history.inl, Ordering).
#include "hr_motion.h"

static int motionCheckCamera(hr_ctx *c, const char *what, const hr_pass_params *cam)
{
    if (!cam) FAIL(c, HR_ERR_INVALID, std::string(what) + ": null camera");
    bool finite = std::isfinite(cam->fov_tan) && std::isfinite(cam->aspect_ratio);
    for (float v : cam->view_matrix) finite = finite && std::isfinite(v);
    if (!finite) FAIL(c, HR_ERR_INVALID, std::string(what) + ": the camera (view_matrix, fov_tan, aspect_ratio) is not finite");
    return HR_OK;
}

// a plain context (history's refusals of a group and of a tile shard) and, where asked for, a frame
static int motionPlainContext(hr_ctx *c, const char *what, bool needFrame)
{
    if (!needFrame && !c->grp && c->world <= 1) return HR_OK;
    const FrameNeed need{0, what, "the gather", false, false, std::string(), std::string()};
    return frameKindReady(c, need);
}

// The trace for `camera` into the motion planes; the caller has checked the camera and the kind of context, and fetches the counters.
static int motionTraceEnqueue(hr_ctx *c, const char *what, const hr_pass_params *camera)
{
    MotionState &m = c->motion;
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    if (!m.have) FAIL(c, HR_ERR_INVALID, std::string(what) + ": no snapshot (hr_motion_snapshot; hr_motion_drop removes it)");
    int rc = queryPrepare(c);
    if (rc) return rc;
    // ---- current mesh -> its first triangle in the snapshot, in the order of the query's table (hr_scene_commit's list)
    std::vector<int32_t> remap;
    size_t at = 0; // (both lists are in id order: one walk)
    for (size_t id = 0; id < c->geoms.size(); ++id) {
        const Geom &g = c->geoms[id];
        if (!g.alive || g.nTris() == 0) continue;
        while (at < m.meshes.size() && m.meshes[at].id < (int32_t)id) ++at;
        const bool held = at < m.meshes.size() && m.meshes[at].id == (int32_t)id && m.meshes[at].count == g.nTris();
        remap.push_back(held ? (int32_t)m.meshes[at].first : -1);
    }
    if ((int)remap.size() != c->query.nGeoms) FAIL(c, HR_ERR_INVALID, std::string(what) + ": the meshes do not match the committed scene");
    HIP_TRY(c, m.remap.reserve(remap.size() + 1, 16));
    if (!remap.empty()) HIP_TRY(c, hipMemcpy(m.remap, remap.data(), remap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!m.planes) HIP_TRY(c, m.planes.alloc((size_t)c->W * c->H * kMotionPlaneBytesPerPixel / sizeof(float)));
    m.traced = false;
    HIP_TRY(c, m.result.ensure(kMotionTraceResultWords + kMotionMergeResultWords));
    HIP_TRY(c, m.result.zero(c->stream));
    MvTraceArgs a{};
    a.scene = c->dScene, a.geoms = c->query.geoms, a.nGeoms = c->query.nGeoms, a.remap = m.remap, a.snap = reinterpret_cast<const float4 *>(m.snap.get());
    a.W = c->W, a.H = c->H, a.aspect = camera->aspect_ratio, a.fov = camera->fov_tan;
    std::memcpy(a.view, camera->view_matrix, sizeof(a.view));
    a.planes = m.planes, a.result = m.result.dev;
    launchMotionTrace(c->stream, a);
    HIP_TRY(c, hipGetLastError());
    std::memcpy(m.view, camera->view_matrix, sizeof(m.view));
    m.fovTan = camera->fov_tan, m.aspect = camera->aspect_ratio, m.traced = true;
    return HR_OK;
}

// the old camera of the motion vectors (null: the captured history's) and the last trace's -> the two cameras
static int motionVectorCameras(hr_ctx *c, const hr_pass_params *oldCamera, MvCam *cam)
{
    const MotionState &m = c->motion;
    if (c->grp || !m.traced) FAIL(c, HR_ERR_INVALID, "motion vectors: no trace at this frame size (hr_motion_trace or hr_motion_merge; hr_frame_resize and hr_motion_drop remove it)");
    if (oldCamera) {
        const int rc = motionCheckCamera(c, "motion vectors", oldCamera);
        if (rc) return rc;
        *cam = mvCameras(oldCamera->view_matrix, oldCamera->aspect_ratio, oldCamera->fov_tan, m.view, m.aspect, m.fovTan);
    } else {
        if (!c->history.captured) FAIL(c, HR_ERR_INVALID, "motion vectors: no old camera and no captured history to take it from");
        *cam = mvCameras(c->history.view, c->history.aspect, c->history.fovTan, m.view, m.aspect, m.fovTan);
    }
    return HR_OK;
}

extern "C" {

uint32_t hr_motion_api_version(void) { return HR_MOTION_API_VERSION; }

void hr_motion_default_params(hr_history_params *p)
{
    if (!p) return;
    hr_history_default_params(p);
    p->normal_cos = 0.8f;
}

int hr_motion_snapshot(hr_ctx *c)
{
    ENTER(c);
    int rc = motionPlainContext(c, "motion snapshot", false);
    if (rc) return rc;
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    MotionState &m = c->motion;
    std::vector<MotionState::Mesh> meshes;
    uint32_t nTris = 0;
    for (size_t id = 0; id < c->geoms.size(); ++id) { // hr_scene_commit's list: the live meshes that have triangles, in id order
        const Geom &g = c->geoms[id];
        if (!g.alive || g.nTris() == 0) continue;
        meshes.push_back(MotionState::Mesh{(int32_t)id, nTris, g.nTris()});
        nTris += g.nTris();
    }
    if (nTris != (uint32_t)c->hScene.nTris) FAIL(c, HR_ERR_INVALID, "motion snapshot: the meshes do not match the committed scene");
    m.have = false;
    if (nTris) {
        HIP_TRY(c, m.snap.reserve((size_t)nTris * kMotionSnapshotFloatsPerTri));
        launchMotionSnapshot(c->stream, nTris, c->tree.tris, c->tree.slotOfPrim, m.snap);
        HIP_TRY(c, hipGetLastError());
    }
    m.meshes = std::move(meshes);
    m.nTris = nTris, m.have = true;
    return HR_OK;
}

int hr_motion_trace(hr_ctx *c, const hr_pass_params *camera, hr_motion_trace_result *out)
{
    ENTER(c);
    int rc = motionCheckCamera(c, "motion trace", camera);
    if (rc == HR_OK) rc = motionPlainContext(c, "motion trace", true);
    if (rc == HR_OK) rc = motionTraceEnqueue(c, "motion trace", camera);
    if (rc) return rc;
    MotionState &m = c->motion;
    HIP_TRY(c, m.result.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out) {
        *out = hr_motion_trace_result{};
        out->surface_pixels = m.result.host[0], out->sky_pixels = m.result.host[1], out->unmatched_pixels = m.result.host[2];
    }
    return HR_OK;
}

int hr_motion_merge(hr_ctx *c, const hr_pass_params *camera, const hr_history_params *params, hr_motion_result *out)
{
    ENTER(c);
    hr_history_params defaults, p;
    hr_motion_default_params(&defaults);
    int rc = historyCheckParams(c, params ? params : &defaults, &p);
    if (rc == HR_OK) rc = motionCheckCamera(c, "motion merge", camera);
    if (rc) return rc;
    uint32_t n = 0;
    rc = historyCheckFrame(c, "motion merge", &n);
    if (rc) return rc;
    MotionState &m = c->motion;
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    if (!m.have) FAIL(c, HR_ERR_INVALID, "motion merge: no snapshot (hr_motion_snapshot; hr_motion_drop removes it)");
    if (!c->history.captured) FAIL(c, HR_ERR_INVALID, "motion merge: no captured history (hr_history_capture; hr_frame_resize and hr_history_drop remove it)");
    if (c->history.merged)
        FAIL(c, HR_ERR_INVALID, "motion merge: a history has already been merged into this frame (one merge per hr_clear, of whatever kind: a second would count it twice)");
    rc = motionTraceEnqueue(c, "motion merge", camera);
    if (rc) return rc;
    const HsLaunch l = historyLaunch(c, camera, p);
    launchMotionMerge(c->stream, c->W, c->H, mvCameras(l.cam, c->history.view), l.P, m.planes, c->history.hist, c->fb(), c->aov.plane[HR_AOV_PLANE_ALBEDO], c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH],
                      c->aov.plane[HR_AOV_PLANE_MOMENTS], m.result.dev + kMotionTraceResultWords);
    HIP_TRY(c, hipGetLastError());
    c->history.merged = true; // (hr_history_merge and hr_reproject_merge refuse from here to the next hr_clear)
    c->snapshotEpoch++;       // (progressive snapshots taken before the merge are not handed out any more)
    HIP_TRY(c, m.result.fetch(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out) {
        *out = hr_motion_result{};
        const unsigned long long *h = m.result.host;
        out->surface_pixels = h[0], out->sky_pixels = h[1], out->unmatched_pixels = h[2];
        out->reused_pixels = h[3], out->rejected_pixels = h[4], out->history_samples = h[5];
        out->history_passes = c->history.passes, out->passes = n;
    }
    return HR_OK;
}

int hr_motion_vectors(hr_ctx *c, const hr_pass_params *oldCamera, float *deviceOut, void *stream)
{
    ENTER(c);
    if (!deviceOut) FAIL(c, HR_ERR_INVALID, "motion vectors: null output");
    if ((uintptr_t)deviceOut % 16 != 0) FAIL(c, HR_ERR_INVALID, "motion vectors: the output must be 16-byte aligned");
    MvCam cam;
    const int rc = motionVectorCameras(c, oldCamera, &cam);
    if (rc) return rc;
    MotionState &m = c->motion;
    const bool own = !stream || (hipStream_t)stream == c->stream;
    if (own) {
        launchMotionVectors(c->stream, c->W, c->H, cam, m.planes, deviceOut);
        HIP_TRY(c, hipGetLastError());
        return HR_OK;
    }
    if (!m.out) HIP_TRY(c, m.out.alloc((size_t)c->W * c->H * 4));
    launchMotionVectors(c->stream, c->W, c->H, cam, m.planes, m.out);
    HIP_TRY(c, hipGetLastError());
    return copyOutOnStream(c, deviceOut, m.out, (size_t)c->W * c->H * 16, stream);
}

int hr_motion_vectors_readback(hr_ctx *c, const hr_pass_params *oldCamera, float *hostOut)
{
    ENTER(c);
    if (!hostOut) FAIL(c, HR_ERR_INVALID, "motion vectors: null output");
    MvCam cam;
    int rc = motionVectorCameras(c, oldCamera, &cam);
    if (rc) return rc;
    MotionState &m = c->motion;
    const size_t bytes = (size_t)c->W * c->H * 16;
    if (!m.out) HIP_TRY(c, m.out.alloc(bytes / sizeof(float)));
    rc = growPinned(c, m.pinned, bytes);
    if (rc) return rc;
    launchMotionVectors(c->stream, c->W, c->H, cam, m.planes, m.out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(m.pinned.get(), m.out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(hostOut, m.pinned.get(), bytes);
    return HR_OK;
}

int hr_motion_readback(hr_ctx *c, float *hostOut)
{
    ENTER(c);
    if (!hostOut) FAIL(c, HR_ERR_INVALID, "motion readback: null output");
    MotionState &m = c->motion;
    if (c->grp || !m.traced) FAIL(c, HR_ERR_INVALID, "motion readback: no trace at this frame size (hr_motion_trace or hr_motion_merge; hr_frame_resize and hr_motion_drop remove it)");
    const size_t bytes = (size_t)c->W * c->H * kMotionPlaneBytesPerPixel;
    const int rc = growPinned(c, m.pinned, bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(m.pinned.get(), m.planes, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(hostOut, m.pinned.get(), bytes);
    return HR_OK;
}

int hr_motion_snapshot_readback(hr_ctx *c, float *hostOut)
{
    ENTER(c);
    if (!hostOut) FAIL(c, HR_ERR_INVALID, "motion snapshot readback: null output");
    MotionState &m = c->motion;
    if (c->grp || !m.have) FAIL(c, HR_ERR_INVALID, "motion snapshot readback: no snapshot (hr_motion_snapshot; hr_motion_drop removes it)");
    if (m.nTris) HIP_TRY(c, hipMemcpyAsync(hostOut, m.snap, (size_t)m.nTris * kMotionSnapshotFloatsPerTri * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HR_OK;
}

int hr_motion_drop(hr_ctx *c)
{
    ENTER(c);
    if (c->grp) return HR_OK; // (a group never holds one)
    MotionState &m = c->motion;
    const int rc = (m.snap || m.planes || m.out) ? quiesce(c) : HR_OK;
    if (rc) return rc;
    m.release();
    return HR_OK;
}

int hr_motion_info(hr_ctx *c, hr_motion_info_t *out)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "motion info: null output");
    *out = hr_motion_info_t{};
    if (c->grp) return HR_OK;
    const MotionState &m = c->motion;
    out->snapshot = m.have ? 1 : 0, out->traced = m.traced ? 1 : 0;
    out->triangles = m.have ? m.nTris : 0u, out->meshes = m.have ? (uint32_t)m.meshes.size() : 0u;
    out->bytes = (m.snap.capacity() + m.planes.capacity() + m.out.capacity()) * sizeof(float) + m.remap.capacity() * sizeof(int32_t);
    return HR_OK;
}

} // extern "C"
