// hr_mesh.inl — a section of hr_core.hip (included at its end): the entry points of include/hrcore_mesh.h.  The kernels are in
// hr_mesh.hip, the arithmetic in hr_mesh.h.  Every refusal is decided on the host before anything is uploaded or launched: the kernels
// index the vertex arrays with the caller's indices unchecked.
//
// Ordering: uploads (the staging ring hr_geom_add uses), launches and the copies back run on the context's stream; ONE wait at the end
// covers the outputs and the counters.  Nothing of the scene or the frame is read or written, so the pass pipeline is left alone.

static const char *const kMeshWhat = "mesh_prepare: ";

// the checks, and the triangle count of the list
static int meshCheck(hr_ctx *c, const hr_mesh_desc *d, const hr_mesh_params *in, const float *nOut, const float *tOut, const float *bOut, hr_mesh_params *p, uint64_t *nTris)
{
    const std::string what = kMeshWhat;
    if (!d) FAIL(c, HR_ERR_INVALID, what + "null desc");
    if (in)
        *p = *in;
    else
        hr_mesh_default_params(p);
    if (p->weight != HR_MESH_WEIGHT_ANGLE && p->weight != HR_MESH_WEIGHT_AREA && p->weight != HR_MESH_WEIGHT_UNIFORM)
        FAIL(c, HR_ERR_INVALID, what + "unknown weight " + std::to_string(p->weight));
    if (p->weld != 0 && p->weld != 1) FAIL(c, HR_ERR_INVALID, what + "weld = " + std::to_string(p->weld) + " is neither 0 nor 1");
    if (p->want == 0) FAIL(c, HR_ERR_INVALID, what + "want = 0 asks for nothing");
    if (p->want & ~(HR_MESH_WANT_NORMALS | HR_MESH_WANT_TANGENTS)) FAIL(c, HR_ERR_INVALID, what + "unknown want " + std::to_string(p->want));
    for (int k = 0; k < 5; ++k)
        if (p->reserved[k]) FAIL(c, HR_ERR_INVALID, what + "reserved[" + std::to_string(k) + "] must be 0");
    const bool normals = (p->want & HR_MESH_WANT_NORMALS) != 0, tangents = (p->want & HR_MESH_WANT_TANGENTS) != 0;
    if (!d->positions) FAIL(c, HR_ERR_INVALID, what + "null positions");
    if (!d->indices) FAIL(c, HR_ERR_INVALID, what + "null indices");
    if (d->n_vertices <= 0) FAIL(c, HR_ERR_INVALID, what + "n_vertices = " + std::to_string(d->n_vertices) + " must be positive");
    if (d->n_indices < 0) FAIL(c, HR_ERR_INVALID, what + "n_indices = " + std::to_string(d->n_indices) + " is negative");
    if (d->mode != HR_TRIANGLES && d->mode != HR_TRIANGLE_STRIP) FAIL(c, HR_ERR_INVALID, what + "unsupported draw mode");
    if (normals && !nOut) FAIL(c, HR_ERR_INVALID, what + "normals are wanted and normals_out is null");
    if (tangents && !tOut) FAIL(c, HR_ERR_INVALID, what + "tangents are wanted and tangents_out is null");
    if (tangents && !bOut) FAIL(c, HR_ERR_INVALID, what + "tangents are wanted and bitangents_out is null");
    if (tangents && !d->uvs) FAIL(c, HR_ERR_INVALID, what + "tangents need uvs");
    if (tangents && !normals && !d->normals) FAIL(c, HR_ERR_INVALID, what + "tangents need normals: want them too, or give desc->normals");
    const struct {
        bool read;
        int32_t stride, comps;
    } attrs[3] = {{true, d->position_stride, 3}, {tangents, d->uv_stride, 2}, {tangents && !normals, d->normal_stride, 3}};
    for (const auto &a : attrs)
        if (a.read && a.stride != 0 && a.stride < a.comps * (int)sizeof(float)) FAIL(c, HR_ERR_INVALID, what + "attribute stride smaller than the attribute");
    {
        uint32_t worst = 0; // (a plain max reduction: vectorises)
        for (int i = 0; i < d->n_indices; ++i) worst = d->indices[i] > worst ? d->indices[i] : worst;
        if (d->n_indices > 0 && worst >= (uint32_t)d->n_vertices) FAIL(c, HR_ERR_INVALID, what + "index out of range");
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
    const uint64_t n = (uint64_t)d->n_indices;
    *nTris = d->mode == HR_TRIANGLE_STRIP ? (n >= 3 ? n - 2 : 0) : n / 3;
    if (3 * *nTris > 0xFFFFFFFFull) FAIL(c, HR_ERR_INVALID, what + "more than 2^32 - 1 corners");
    return HR_OK;
}

// an attribute as the kernels read it: tightly packed (the caller's array itself where it is, else re-packed into tmp)
static const char *meshTight(const float *src, int32_t strideB, int comps, int nVerts, std::vector<float> &tmp)
{
    const size_t sb = strideB == 0 ? (size_t)comps * sizeof(float) : (size_t)strideB;
    if (sb == (size_t)comps * sizeof(float)) return (const char *)src;
    tmp.resize((size_t)nVerts * comps);
    for (int i = 0; i < nVerts; ++i) std::memcpy(&tmp[(size_t)i * comps], (const char *)src + (size_t)i * sb, comps * sizeof(float));
    return (const char *)tmp.data();
}

// The scratch of one preparation of V vertices, T triangles and nIdx indices: one block cut in 256-byte steps, the context's own, grown
// only; b's pointers are set into it (b.idx too: a caller whose indices are on the device already passes nIdx = 0 and points b.idx at
// them).  `extraBytes` more are cut off behind it for the caller (hr_deform.inl's tight staging) and come back in *extra.
static int meshScratch(hr_ctx *c, size_t V, size_t T, size_t nIdx, bool normals, bool tangents, size_t extraBytes, MsBufs *out, char **extra)
{
    MsBufs &b = *out;
    const size_t C = 3 * T, S = C > V ? C : V;
    size_t total = 0;
    const auto reserve = [&](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t oPos = reserve(V * 12), oUv = reserve(tangents ? V * 8 : 0), oNrm = reserve(tangents && !normals ? V * 12 : 0), oIdx = reserve(nIdx * 4);
    const size_t oFlag = reserve(T), oCN = reserve(C * 12), oCT = reserve(tangents ? C * 12 : 0), oCB = reserve(tangents ? C * 12 : 0);
    const size_t oKA = reserve(S * 4), oKB = reserve(S * 4), oVA = reserve(S * 4), oVB = reserve(S * 4), oHist = reserve(meshSortBlocks(S) * 256 * 4);
    const size_t oBegin = reserve(V * 4), oEnd = reserve(V * 4), oFirst = reserve(V * 4);
    const size_t oS = reserve(V * 12), oTa = reserve(tangents ? V * 12 : 0), oBa = reserve(tangents ? V * 12 : 0);
    const size_t oPerm = reserve(V * 4), oGroupOf = reserve(V * 4), oStart = reserve((V + 1) * 4), oScan = reserve(V * 4), oNG = reserve(4);
    const size_t oGN = reserve(V * 12), oGC = reserve(V);
    const size_t oOutN = reserve(normals ? V * 12 : 0), oOutT = reserve(tangents ? V * 12 : 0), oOutB = reserve(tangents ? V * 12 : 0);
    const size_t oExtra = reserve(extraBytes);
    if (c->meshPrep.scratch.capacity() < total) {
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // (an earlier call's kernels have been waited for; the ring's copies too)
        HIP_TRY(c, c->meshPrep.scratch.reserve(total));
    }
    char *base = c->meshPrep.scratch;
    const auto F32 = [&](size_t o) { return (float *)(base + o); };
    const auto U32 = [&](size_t o) { return (uint32_t *)(base + o); };
    b.pos = F32(oPos), b.uv = tangents ? F32(oUv) : nullptr, b.nrmIn = tangents && !normals ? F32(oNrm) : nullptr, b.idx = U32(oIdx);
    b.tflag = (uint8_t *)(base + oFlag), b.cN = F32(oCN), b.cT = F32(oCT), b.cB = F32(oCB);
    b.keysA = U32(oKA), b.keysB = U32(oKB), b.valsA = U32(oVA), b.valsB = U32(oVB), b.blockHist = U32(oHist);
    b.vBegin = U32(oBegin), b.vEnd = U32(oEnd), b.vFirst = U32(oFirst), b.vS = F32(oS), b.vTa = F32(oTa), b.vBa = F32(oBa);
    b.perm = U32(oPerm), b.groupOf = U32(oGroupOf), b.groupStart = U32(oStart), b.scan = U32(oScan), b.nGroups = U32(oNG);
    b.gN = F32(oGN), b.gClass = (uint8_t *)(base + oGC), b.outN = F32(oOutN), b.outT = F32(oOutT), b.outB = F32(oOutB);
    if (extra) *extra = base + oExtra;
    return HR_OK;
}

// the device part, on a context that is no group; the inputs have passed meshCheck
static int meshPrepareOn(hr_ctx *c, const hr_mesh_desc *d, const hr_mesh_params &p, uint64_t nTris, float *nOut, float *tOut, float *bOut, hr_mesh_result *res)
{
    HIP_TRY(c, hipSetDevice(c->device)); // (a group's member: the call arrives on its thread)
    const bool normals = (p.want & HR_MESH_WANT_NORMALS) != 0, tangents = (p.want & HR_MESH_WANT_TANGENTS) != 0;
    const size_t V = (size_t)d->n_vertices, T = (size_t)nTris, C = 3 * T, nIdx = (size_t)d->n_indices;
    MsBufs b{};
    b.V = (uint32_t)V, b.T = (uint32_t)T, b.C = (uint32_t)C;
    b.strip = d->mode == HR_TRIANGLE_STRIP, b.weight = p.weight, b.weld = p.weld, b.want = p.want;
    // ---- the scratch
    const int src = meshScratch(c, V, T, nIdx, normals, tangents, 0, &b, nullptr);
    if (src) return src;
    float *const posAt = const_cast<float *>(b.pos), *const uvAt = const_cast<float *>(b.uv), *const nrmAt = const_cast<float *>(b.nrmIn);
    uint32_t *const idxAt = const_cast<uint32_t *>(b.idx);
    // ---- uploads
    std::vector<float> tmp;
    int rc = stagedUpload(c, (char *)posAt, meshTight(d->positions, d->position_stride, 3, (int)V, tmp), V * 12);
    if (rc == HR_OK && tangents) rc = stagedUpload(c, (char *)uvAt, meshTight(d->uvs, d->uv_stride, 2, (int)V, tmp), V * 8);
    if (rc == HR_OK && tangents && !normals) rc = stagedUpload(c, (char *)nrmAt, meshTight(d->normals, d->normal_stride, 3, (int)V, tmp), V * 12);
    if (rc == HR_OK && nIdx) rc = stagedUpload(c, (char *)idxAt, (const char *)d->indices, nIdx * 4);
    if (rc) return rc;
    // ---- the kernels, the copies back, one wait
    HIP_TRY(c, c->meshPrep.counters.ensure(kMsCounterWords));
    HIP_TRY(c, c->meshPrep.counters.zero(c->stream));
    b.counters = c->meshPrep.counters.dev;
    launchMeshPrepare(c->stream, b);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->meshPrep.counters.fetch(c->stream));
    if (normals) HIP_TRY(c, hipMemcpyAsync(nOut, b.outN, V * 12, hipMemcpyDeviceToHost, c->stream));
    if (tangents) {
        HIP_TRY(c, hipMemcpyAsync(tOut, b.outT, V * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bOut, b.outB, V * 12, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long *h = c->meshPrep.counters.host;
    *res = hr_mesh_result{};
    res->triangles = nTris, res->degenerate_triangles = h[kMsDegenerate], res->degenerate_uv_triangles = h[kMsDegenerateUv];
    res->weld_groups = normals ? h[kMsGroups] : 0, res->unreferenced_vertices = h[kMsUnreferenced], res->cancelled_vertices = h[kMsCancelled];
    res->fallback_tangents = h[kMsFallback], res->max_valence = h[kMsMaxValence];
    return HR_OK;
}

extern "C" {

uint32_t hr_mesh_api_version(void) { return HR_MESH_API_VERSION; }

void hr_mesh_default_params(hr_mesh_params *p)
{
    if (!p) return;
    *p = hr_mesh_params{};
    p->weight = HR_MESH_WEIGHT_ANGLE, p->weld = 1, p->want = HR_MESH_WANT_NORMALS;
}

int hr_mesh_prepare(hr_ctx *c, const hr_mesh_desc *desc, const hr_mesh_params *params, float *normals_out, float *tangents_out, float *bitangents_out, hr_mesh_result *out)
{
    ENTER(c);
    hr_mesh_params p;
    uint64_t nTris = 0;
    int rc = meshCheck(c, desc, params, normals_out, tangents_out, bitangents_out, &p, &nTris);
    if (rc) return rc;
    hr_mesh_result r{};
    if (c->grp) // (every member would answer alike: the first one does)
        rc = groupOne(c, 0, [&](hr_ctx *m) { return meshPrepareOn(m, desc, p, nTris, normals_out, tangents_out, bitangents_out, &r); });
    else
        rc = meshPrepareOn(c, desc, p, nTris, normals_out, tangents_out, bitangents_out, &r);
    if (rc) return rc;
    c->meshPrep.last = r, c->meshPrep.prepared = true;
    if (out) *out = r;
    return HR_OK;
}

int hr_mesh_last(hr_ctx *c, hr_mesh_result *out)
{
    ENTER(c);
    if (!out) FAIL(c, HR_ERR_INVALID, "mesh_last: null output");
    if (!c->meshPrep.prepared) FAIL(c, HR_ERR_INVALID, "mesh_last: no mesh has been prepared on this context");
    *out = c->meshPrep.last;
    return HR_OK;
}

} // extern "C"
