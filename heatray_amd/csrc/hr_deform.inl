// hr_deform.inl — a section of hr_core.hip (included at its end, behind hr_mesh.inl): the entry points of include/hrcore_deform.h.  The
// kernels are in hr_deform.hip, the arithmetic in hr_deform.h.  Every refusal is decided on the host before anything is uploaded or
// launched, so a refused call leaves the mesh block as it was.
//
// Ordering: uploads (the staging ring hr_geom_add uses), the kernels and the copies back run on the context's stream.  A mesh block is
// read by hr_scene_commit alone (launchAssemble, and sceneKey with a tree cache), on that same stream and behind a quiesce of its own;
// passes in flight read the committed triangle arrays, never a block.  So nothing here waits for the pass pipeline: the calls order
// themselves against the next commit by the stream, and the scene counts as not committed until then.  The tight staging is the mesh
// scratch (meshScratch, hr_mesh.inl), which hr_mesh_prepare uses on the same stream.
//
// A group's handle owns no meshes: the public calls go to every member, whose checks answer alike; member 0 fills the result.

static const int kDfComps[6] = {3, 3, 2, 3, 3, 3};
static const char *const kDfAttrName[6] = {"positions", "normals", "uvs", "tangents", "bitangents", "colors"};

static Geom *deformGeom(hr_ctx *c, hr_geom_id id) { return (id < 0 || id >= (int)c->geoms.size() || !c->geoms[id].alive) ? nullptr : &c->geoms[id]; }

// params as both calls read them, against the mesh; the given attributes of an update (null for a pose)
static int deformCheckParams(hr_ctx *c, const std::string &what, const Geom &g, const hr_deform_params *in, const float *const given[6], hr_deform_params *p)
{
    if (in)
        *p = *in;
    else
        hr_deform_default_params(p);
    if (p->regenerate & ~(HR_DEFORM_NORMALS | HR_DEFORM_TANGENTS)) FAIL(c, HR_ERR_INVALID, what + "unknown regenerate " + std::to_string(p->regenerate));
    if ((p->regenerate & HR_DEFORM_TANGENTS) && !(p->regenerate & HR_DEFORM_NORMALS)) FAIL(c, HR_ERR_INVALID, what + "regenerate TANGENTS needs NORMALS");
    if (p->weight != HR_MESH_WEIGHT_ANGLE && p->weight != HR_MESH_WEIGHT_AREA && p->weight != HR_MESH_WEIGHT_UNIFORM)
        FAIL(c, HR_ERR_INVALID, what + "unknown weight " + std::to_string(p->weight));
    if (p->weld != 0 && p->weld != 1) FAIL(c, HR_ERR_INVALID, what + "weld = " + std::to_string(p->weld) + " is neither 0 nor 1");
    for (int k = 0; k < 5; ++k)
        if (p->reserved[k]) FAIL(c, HR_ERR_INVALID, what + "reserved[" + std::to_string(k) + "] must be 0");
    if ((p->regenerate & HR_DEFORM_NORMALS) && given && given[HR_GEOM_NORMALS]) FAIL(c, HR_ERR_INVALID, what + "normals are both given and regenerated");
    if ((p->regenerate & HR_DEFORM_TANGENTS) && given && (given[HR_GEOM_TANGENTS] || given[HR_GEOM_BITANGENTS]))
        FAIL(c, HR_ERR_INVALID, what + "tangents are both given and regenerated");
    if ((p->regenerate & HR_DEFORM_TANGENTS) && !(g.has[HR_GEOM_UVS] && g.has[HR_GEOM_TANGENTS] && g.has[HR_GEOM_BITANGENTS]))
        FAIL(c, HR_ERR_INVALID, what + "regenerate TANGENTS needs a mesh with uvs, tangents and bitangents");
    return HR_OK;
}

static float *deformSlot(const Geom &g, int a) { return reinterpret_cast<float *>(g.dBlock + g.off[a]); }

// tight arrays -> the block: attrs[k] of the mesh from tight[k], four per launch
static void deformScatter(hr_ctx *c, const Geom &g, const int *attrs, float *const *tight, int n)
{
    for (int at = 0; at < n; at += 4) {
        DfCopy s{};
        s.V = (uint32_t)g.nVerts;
        for (int k = at; k < n && k < at + 4; ++k, ++s.n)
            s.strided[s.n] = deformSlot(g, attrs[k]), s.tight[s.n] = tight[k], s.stride[s.n] = g.stride[attrs[k]], s.comps[s.n] = kDfComps[attrs[k]];
        launchDeformScatter(c->stream, s);
    }
}
static void deformGather(hr_ctx *c, const Geom &g, const int *attrs, float *const *tight, int n)
{
    for (int at = 0; at < n; at += 4) {
        DfCopy s{};
        s.V = (uint32_t)g.nVerts;
        for (int k = at; k < n && k < at + 4; ++k, ++s.n)
            s.strided[s.n] = deformSlot(g, attrs[k]), s.tight[s.n] = tight[k], s.stride[s.n] = g.stride[attrs[k]], s.comps[s.n] = kDfComps[attrs[k]];
        launchDeformGather(c->stream, s);
    }
}

// The scratch of one call on mesh g: with `regenerate` everything launchMeshPrepare needs (b.pos is where the new tight positions go in
// either case, b.idx the block's own indices), and `extraBytes` of staging behind it.
static int deformScratch(hr_ctx *c, const Geom &g, const hr_deform_params &p, size_t extraBytes, MsBufs *b, char **extra)
{
    const bool regen = p.regenerate != 0, tangents = (p.regenerate & HR_DEFORM_TANGENTS) != 0;
    const size_t V = (size_t)g.nVerts, T = regen ? (size_t)g.nTris() : 0;
    *b = MsBufs{};
    const int rc = meshScratch(c, V, T, 0, true, tangents, extraBytes, b, extra);
    if (rc) return rc;
    b->V = (uint32_t)V, b->T = (uint32_t)T, b->C = (uint32_t)(3 * T);
    b->strip = g.mode == HR_TRIANGLE_STRIP, b->weight = p.weight, b->weld = p.weld, b->want = p.regenerate;
    b->idx = reinterpret_cast<const uint32_t *>(g.dBlock + g.off[6]);
    return HR_OK;
}

// The regeneration: b.pos holds the new positions, the block everything else as the call leaves it.  Enqueues; the caller waits.
static int deformRegenerate(hr_ctx *c, const Geom &g, const hr_deform_params &p, const MsBufs &b)
{
    if (p.regenerate & HR_DEFORM_TANGENTS) {
        const int a[1] = {HR_GEOM_UVS};
        float *const t[1] = {const_cast<float *>(b.uv)};
        deformGather(c, g, a, t, 1);
    }
    HIP_TRY(c, c->meshPrep.counters.ensure(kMsCounterWords));
    HIP_TRY(c, c->meshPrep.counters.zero(c->stream));
    MsBufs bb = b;
    bb.counters = c->meshPrep.counters.dev;
    launchMeshPrepare(c->stream, bb);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->meshPrep.counters.fetch(c->stream));
    const int a[3] = {HR_GEOM_NORMALS, HR_GEOM_TANGENTS, HR_GEOM_BITANGENTS};
    float *const t[3] = {b.outN, b.outT, b.outB};
    deformScatter(c, g, a, t, (p.regenerate & HR_DEFORM_TANGENTS) ? 3 : 1);
    return HR_OK;
}

// after the caller's wait: the regeneration's counters (meshPrepareOn's lines)
static void deformMeshResult(hr_ctx *c, const Geom &g, hr_mesh_result *res)
{
    const unsigned long long *h = c->meshPrep.counters.host;
    *res = hr_mesh_result{};
    res->triangles = g.nTris(), res->degenerate_triangles = h[kMsDegenerate], res->degenerate_uv_triangles = h[kMsDegenerateUv];
    res->weld_groups = h[kMsGroups], res->unreferenced_vertices = h[kMsUnreferenced], res->cancelled_vertices = h[kMsCancelled];
    res->fallback_tangents = h[kMsFallback], res->max_valence = h[kMsMaxValence];
}

static bool deformAllFinite(const float *a, size_t n)
{
    float worst = 0.0f;
    bool nan = false;
    for (size_t i = 0; i < n; ++i) {
        const float m = std::fabs(a[i]);
        worst = m > worst ? m : worst;
        nan = nan || a[i] != a[i];
    }
    return !nan && worst <= 3.0e37f;
}

static void deformDone(hr_ctx *c, const hr_deform_result &r, hr_deform_result *out)
{
    c->deform.last = r, c->deform.done = true;
    if (out) *out = r;
}

extern "C" {

uint32_t hr_deform_api_version(void) { return HR_DEFORM_API_VERSION; }

void hr_deform_default_params(hr_deform_params *p)
{
    if (!p) return;
    *p = hr_deform_params{};
    p->regenerate = 0, p->weight = HR_MESH_WEIGHT_ANGLE, p->weld = 1;
}

int hr_geom_update(hr_ctx *c, hr_geom_id id, const hr_mesh_desc *d, const hr_deform_params *params, hr_deform_result *out)
{
    ENTER(c);
    if (c->grp) {
        hr_deform_result r{};
        const int rc = groupAll(c, [&](hr_ctx *m, int i) { return hr_geom_update(m, id, d, params, i == 0 ? &r : nullptr); });
        if (rc) return rc;
        deformDone(c, r, out);
        return HR_OK;
    }
    const std::string what = "geom_update: ";
    Geom *gp = deformGeom(c, id);
    if (!gp) FAIL(c, HR_ERR_INVALID, what + "bad geom id");
    const Geom &g = *gp;
    if (!d) FAIL(c, HR_ERR_INVALID, what + "null desc");
    if (!d->positions) FAIL(c, HR_ERR_INVALID, what + "null positions");
    if (d->n_vertices != g.nVerts) FAIL(c, HR_ERR_INVALID, what + "n_vertices = " + std::to_string(d->n_vertices) + " but the mesh has " + std::to_string(g.nVerts));
    const float *const src[6] = {d->positions, d->normals, d->uvs, d->tangents, d->bitangents, d->colors};
    const int32_t strideB[6] = {d->position_stride, d->normal_stride, d->uv_stride, d->tangent_stride, d->bitangent_stride, d->color_stride};
    for (int a = 0; a < 6; ++a) {
        if (!src[a]) continue;
        if (!g.has[a]) FAIL(c, HR_ERR_INVALID, what + "the mesh has no " + kDfAttrName[a]);
        if (strideB[a] != 0 && strideB[a] < kDfComps[a] * (int)sizeof(float)) FAIL(c, HR_ERR_INVALID, what + "attribute stride smaller than the attribute");
    }
    {
        const int sb = d->position_stride == 0 ? 12 : d->position_stride; // hr_geom_add's rule, word for word
        float worst = 0.0f;
        bool nan = false;
        for (int i = 0; i < d->n_vertices; ++i) {
            float q[3];
            std::memcpy(q, (const char *)d->positions + (size_t)i * (size_t)sb, 12);
            const float m = std::fmax(std::fabs(q[0]), std::fmax(std::fabs(q[1]), std::fabs(q[2])));
            worst = m > worst ? m : worst;
            nan = nan || q[0] != q[0] || q[1] != q[1] || q[2] != q[2];
        }
        if (nan || !(worst <= 3.0e37f)) FAIL(c, HR_ERR_INVALID, what + "vertex positions must be finite");
    }
    hr_deform_params p;
    int rc = deformCheckParams(c, what, g, params, src, &p);
    if (rc) return rc;
    // ---- the given attributes, tight, into the scratch: the positions where a regeneration reads them, the others behind
    const size_t V = (size_t)g.nVerts;
    size_t extraBytes = 0;
    for (int a = 1; a < 6; ++a) extraBytes += src[a] ? ((V * kDfComps[a] * 4 + 255) & ~(size_t)255) : 0;
    MsBufs b;
    char *extra = nullptr;
    rc = deformScratch(c, g, p, extraBytes, &b, &extra);
    if (rc) return rc;
    int attrs[6], n = 0;
    float *tight[6];
    std::vector<float> tmp;
    for (int a = 0; a < 6 && rc == HR_OK; ++a) {
        if (!src[a]) continue;
        float *dst = const_cast<float *>(b.pos);
        if (a > 0) dst = (float *)extra, extra += (V * kDfComps[a] * 4 + 255) & ~(size_t)255;
        rc = stagedUpload(c, (char *)dst, meshTight(src[a], strideB[a], kDfComps[a], (int)V, tmp), V * kDfComps[a] * 4);
        attrs[n] = a, tight[n] = dst, ++n;
    }
    if (rc) return rc;
    deformScatter(c, g, attrs, tight, n);
    if (p.regenerate) {
        rc = deformRegenerate(c, g, p, b);
        if (rc) return rc;
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the scratch and the caller's arrays are free again; a regeneration's counters are here)
    hr_deform_result r{};
    r.vertices = V, r.triangles = g.nTris(), r.regenerated = (uint32_t)p.regenerate, r.posed = 0;
    if (p.regenerate) deformMeshResult(c, g, &r.mesh);
    c->committed = false, c->transformDirty = true;
    deformDone(c, r, out);
    return HR_OK;
}

int hr_geom_get_attribute(hr_ctx *c, hr_geom_id id, int32_t attribute, float *out)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_geom_get_attribute(m, id, attribute, out); });
    const std::string what = "geom_get_attribute: ";
    Geom *gp = deformGeom(c, id);
    if (!gp) FAIL(c, HR_ERR_INVALID, what + "bad geom id");
    if (attribute < 0 || attribute > 5) FAIL(c, HR_ERR_INVALID, what + "unknown attribute " + std::to_string(attribute));
    if (!gp->has[attribute]) FAIL(c, HR_ERR_INVALID, what + "the mesh has no " + kDfAttrName[attribute]);
    if (!out) FAIL(c, HR_ERR_INVALID, what + "null output");
    hr_deform_params p;
    hr_deform_default_params(&p);
    MsBufs b;
    const int rc = deformScratch(c, *gp, p, 0, &b, nullptr);
    if (rc) return rc;
    const int a[1] = {attribute};
    float *const t[1] = {const_cast<float *>(b.pos)}; // (V x 12 bytes: room for any attribute)
    deformGather(c, *gp, a, t, 1);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, b.pos, (size_t)gp->nVerts * kDfComps[attribute] * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HR_OK;
}

int hr_deform_bind(hr_ctx *c, hr_geom_id id, const hr_deform_rig *rig)
{
    ENTER(c);
    if (c->grp) return groupAll(c, [&](hr_ctx *m, int) { return hr_deform_bind(m, id, rig); });
    const std::string what = "deform_bind: ";
    Geom *gp = deformGeom(c, id);
    if (!gp) FAIL(c, HR_ERR_INVALID, what + "bad geom id");
    Geom &g = *gp;
    if (!rig) FAIL(c, HR_ERR_INVALID, what + "null rig");
    const int K = rig->n_morph, J = rig->n_joints;
    if (K < 0 || K > HR_DEFORM_MAX_MORPH) FAIL(c, HR_ERR_INVALID, what + "n_morph = " + std::to_string(K) + " is outside 0 .. " + std::to_string(HR_DEFORM_MAX_MORPH));
    if (J < 0 || J > HR_DEFORM_MAX_JOINTS) FAIL(c, HR_ERR_INVALID, what + "n_joints = " + std::to_string(J) + " is outside 0 .. " + std::to_string(HR_DEFORM_MAX_JOINTS));
    if (K == 0 && J == 0) FAIL(c, HR_ERR_INVALID, what + "a rig needs morphs or joints");
    for (int k = 0; k < 6; ++k)
        if (rig->reserved[k]) FAIL(c, HR_ERR_INVALID, what + "reserved[" + std::to_string(k) + "] must be 0");
    if (K > 0 && !rig->morph_positions) FAIL(c, HR_ERR_INVALID, what + "null morph_positions");
    if (K == 0 && rig->morph_positions) FAIL(c, HR_ERR_INVALID, what + "morph_positions without morphs");
    if (K == 0 && rig->morph_normals) FAIL(c, HR_ERR_INVALID, what + "morph_normals without morphs");
    if (J > 0 && !rig->joints) FAIL(c, HR_ERR_INVALID, what + "null joints");
    if (J > 0 && !rig->weights) FAIL(c, HR_ERR_INVALID, what + "null weights");
    if (J == 0 && (rig->joints || rig->weights)) FAIL(c, HR_ERR_INVALID, what + "joints or weights without joints");
    const size_t V = (size_t)g.nVerts;
    if (J > 0) {
        uint32_t worst = 0;
        for (size_t i = 0; i < 4 * V; ++i) worst = rig->joints[i] > worst ? rig->joints[i] : worst;
        if (worst >= (uint32_t)J) FAIL(c, HR_ERR_INVALID, what + "joint index out of range");
        if (!deformAllFinite(rig->weights, 4 * V)) FAIL(c, HR_ERR_INVALID, what + "weights must be finite");
    }
    if (K > 0 && !(deformAllFinite(rig->morph_positions, (size_t)K * V * 3) && (!rig->morph_normals || deformAllFinite(rig->morph_normals, (size_t)K * V * 3))))
        FAIL(c, HR_ERR_INVALID, what + "morph deltas must be finite");
    // ---- one allocation, cut in 256-byte steps
    const bool frames = g.has[HR_GEOM_TANGENTS] && g.has[HR_GEOM_BITANGENTS], morphN = rig->morph_normals != nullptr;
    size_t total = 0;
    const auto reserve = [&](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t oP = reserve(V * 12), oN = reserve(V * 12), oT = reserve(frames ? V * 12 : 0), oB = reserve(frames ? V * 12 : 0);
    const size_t oDP = reserve((size_t)K * V * 12), oDN = reserve(morphN ? (size_t)K * V * 12 : 0);
    const size_t oJ = reserve(J > 0 ? V * 16 : 0), oW = reserve(J > 0 ? V * 16 : 0), oPose = reserve((size_t)HR_DEFORM_MAX_MORPH * 4 + (size_t)J * 64);
    char *dev = nullptr;
    HIP_TRY(c, hipMalloc((void **)&dev, total));
    deformRelease(g); // (a second bind replaces the first)
    DeformBinding *bd = new DeformBinding();
    bd->dev = dev, bd->nMorph = K, bd->nJoints = J;
    bd->restP = (float *)(dev + oP), bd->restN = (float *)(dev + oN);
    if (frames) bd->restT = (float *)(dev + oT), bd->restB = (float *)(dev + oB);
    if (K > 0) bd->dP = (float *)(dev + oDP);
    if (morphN) bd->dN = (float *)(dev + oDN);
    if (J > 0) bd->joints = (uint32_t *)(dev + oJ), bd->weights = (float *)(dev + oW);
    bd->pose = (float *)(dev + oPose);
    g.deform = bd;
    // ---- the rest pose out of the block, the rig from the host
    const int a[4] = {HR_GEOM_POSITIONS, HR_GEOM_NORMALS, HR_GEOM_TANGENTS, HR_GEOM_BITANGENTS};
    float *const t[4] = {bd->restP, bd->restN, bd->restT, bd->restB};
    deformGather(c, g, a, t, frames ? 4 : 2);
    int rc = HR_OK;
    if (K > 0) rc = stagedUpload(c, (char *)bd->dP, (const char *)rig->morph_positions, (size_t)K * V * 12);
    if (rc == HR_OK && morphN) rc = stagedUpload(c, (char *)bd->dN, (const char *)rig->morph_normals, (size_t)K * V * 12);
    if (rc == HR_OK && J > 0) rc = stagedUpload(c, (char *)bd->joints, (const char *)rig->joints, V * 16);
    if (rc == HR_OK && J > 0) rc = stagedUpload(c, (char *)bd->weights, (const char *)rig->weights, V * 16);
    if (rc == HR_OK && hipGetLastError() != hipSuccess) c->err = what + "launch failed", rc = HR_ERR_DEVICE;
    if (rc == HR_OK && hipStreamSynchronize(c->stream) != hipSuccess) c->err = what + "hipStreamSynchronize failed", rc = HR_ERR_DEVICE; // (the caller's arrays are free again)
    if (rc) deformRelease(g);
    return rc;
}

int hr_deform_unbind(hr_ctx *c, hr_geom_id id)
{
    ENTER(c);
    if (c->grp) return groupAll(c, [&](hr_ctx *m, int) { return hr_deform_unbind(m, id); });
    Geom *gp = deformGeom(c, id);
    if (!gp) FAIL(c, HR_ERR_INVALID, "deform_unbind: bad geom id");
    if (!gp->deform) FAIL(c, HR_ERR_INVALID, "deform_unbind: the mesh is not bound");
    deformRelease(*gp);
    return HR_OK;
}

int hr_deform_pose(hr_ctx *c, hr_geom_id id, const float *morphWeights, const float *jointMatrices, const hr_deform_params *params, hr_deform_result *out)
{
    ENTER(c);
    if (c->grp) {
        hr_deform_result r{};
        const int rc = groupAll(c, [&](hr_ctx *m, int i) { return hr_deform_pose(m, id, morphWeights, jointMatrices, params, i == 0 ? &r : nullptr); });
        if (rc) return rc;
        deformDone(c, r, out);
        return HR_OK;
    }
    const std::string what = "deform_pose: ";
    Geom *gp = deformGeom(c, id);
    if (!gp) FAIL(c, HR_ERR_INVALID, what + "bad geom id");
    const Geom &g = *gp;
    if (!g.deform) FAIL(c, HR_ERR_INVALID, what + "the mesh is not bound");
    const DeformBinding &bd = *g.deform;
    if (bd.nMorph > 0 && !morphWeights) FAIL(c, HR_ERR_INVALID, what + "null morph_weights");
    if (bd.nJoints > 0 && !jointMatrices) FAIL(c, HR_ERR_INVALID, what + "null joint_matrices");
    if (bd.nMorph > 0 && !deformAllFinite(morphWeights, (size_t)bd.nMorph)) FAIL(c, HR_ERR_INVALID, what + "morph weights must be finite");
    if (bd.nJoints > 0 && !deformAllFinite(jointMatrices, (size_t)bd.nJoints * 16)) FAIL(c, HR_ERR_INVALID, what + "joint matrices must be finite");
    hr_deform_params p;
    int rc = deformCheckParams(c, what, g, params, nullptr, &p);
    if (rc) return rc;
    const size_t V = (size_t)g.nVerts, arr = (V * 12 + 255) & ~(size_t)255;
    const bool frames = bd.restT != nullptr, writeN = bd.dN != nullptr || bd.nJoints > 0, writeTB = frames && bd.nJoints > 0;
    MsBufs b;
    char *extra = nullptr;
    rc = deformScratch(c, g, p, 3 * arr, &b, &extra);
    if (rc) return rc;
    // ---- this pose's weights and matrices
    std::vector<float> pose((size_t)HR_DEFORM_MAX_MORPH + (size_t)bd.nJoints * 16, 0.0f);
    for (int k = 0; k < bd.nMorph; ++k) pose[k] = morphWeights[k];
    if (bd.nJoints > 0) std::memcpy(&pose[HR_DEFORM_MAX_MORPH], jointMatrices, (size_t)bd.nJoints * 64);
    rc = stagedUpload(c, (char *)bd.pose, (const char *)pose.data(), pose.size() * 4);
    if (rc) return rc;
    HIP_TRY(c, c->deform.counters.ensure(kDfCounterWords));
    HIP_TRY(c, c->deform.counters.zero(c->stream));
    DfPoseArgs s{};
    s.restP = bd.restP, s.restN = bd.restN, s.restT = bd.restT, s.restB = bd.restB, s.dP = bd.dP, s.dN = bd.dN, s.weights = bd.weights, s.pose = bd.pose;
    s.joints = bd.joints;
    s.outP = const_cast<float *>(b.pos), s.outN = writeN ? (float *)extra : nullptr;
    s.outT = writeTB ? (float *)(extra + arr) : nullptr, s.outB = writeTB ? (float *)(extra + 2 * arr) : nullptr;
    s.V = (uint32_t)V, s.nMorph = bd.nMorph, s.nJoints = bd.nJoints, s.counters = c->deform.counters.dev;
    launchDeformPose(c->stream, s);
    HIP_TRY(c, c->deform.counters.fetch(c->stream));
    // ---- into the block: what the pose wrote, except what a regeneration replaces
    const bool regenN = (p.regenerate & HR_DEFORM_NORMALS) != 0, regenT = (p.regenerate & HR_DEFORM_TANGENTS) != 0;
    int attrs[4], n = 0;
    float *tight[4];
    attrs[n] = HR_GEOM_POSITIONS, tight[n] = s.outP, ++n;
    if (writeN && !regenN) attrs[n] = HR_GEOM_NORMALS, tight[n] = s.outN, ++n;
    if (writeTB && !regenT) {
        attrs[n] = HR_GEOM_TANGENTS, tight[n] = s.outT, ++n;
        attrs[n] = HR_GEOM_BITANGENTS, tight[n] = s.outB, ++n;
    }
    deformScatter(c, g, attrs, tight, n);
    if (p.regenerate) {
        rc = deformRegenerate(c, g, p, b);
        if (rc) return rc;
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hr_deform_result r{};
    r.vertices = V, r.triangles = g.nTris(), r.regenerated = (uint32_t)p.regenerate, r.posed = 1;
    r.rejected_vertices = c->deform.counters.host[0], r.kept_directions = c->deform.counters.host[1];
    if (p.regenerate) deformMeshResult(c, g, &r.mesh);
    c->committed = false, c->transformDirty = true;
    deformDone(c, r, out);
    return HR_OK;
}

int hr_deform_last(hr_ctx *c, hr_deform_result *out)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "deform_last: null output");
    if (!c->deform.done) FAIL(c, HR_ERR_INVALID, "deform_last: no mesh has been updated or posed on this context");
    *out = c->deform.last;
    return HR_OK;
}

} // extern "C"
