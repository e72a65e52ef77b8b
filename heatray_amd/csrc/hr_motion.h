// hr_motion.h — the per-pixel arithmetic of motion reprojection (include/hrcore_motion.h states the contract these lines implement).
// Pure float32 functions with no memory of their own, so that the kernels in hr_motion.hip and the CPU test (tests/host/motion_cpu.cpp,
// against heatray_amd/motion.py) compile the same lines.  HsCam, HsParams, hsRayX / hsRayY, hsProject, hsCount, the HS_* answers and the
// gather itself (hsGather with this feature's normal test, hsApply) come from hr_history.h; v3, dot, cross, msValid and msNormalize from
// hr_mesh.h, dfDir (the contract's dir) from hr_deform.h.
#pragma once
#include "hr_history.h"
#include "hr_deform.h"

namespace hr {

// the two cameras of a merge or of the motion vectors: hsCameras' numbers and the old camera's eye
struct MvCam {
    HsCam hs;
    float eyeOld[3];
};

inline MvCam mvCameras(const HsCam &hs, const float *vOld) { return MvCam{hs, {vOld[12], vOld[13], vOld[14]}}; }

inline MvCam mvCameras(const float *vOld, float aspectOld, float fovOld, const float *vNew, float aspectNew, float fovNew)
{
    return mvCameras(hsCameras(vOld, aspectOld, fovOld, vNew, aspectNew, fovNew), vOld);
}

// the ray through the centre of pixel (x, y): o = eye(V), d = normalize(dir(V, ray(x, y; aspect, fov)))
template <class PF> HRN void mvCameraRay(PF V, float aspect, float fov, int x, int y, float Wf, float Hf, v3 &o, v3 &d)
{
    const v3 c(hsRayX(x, Wf, aspect, fov), hsRayY(y, Hf, fov), -1.0f);
    o = v3(V[12], V[13], V[14]);
    d = msNormalize(dfDir(V, c));
}

HRN void mvMiss(dn4 &Mv0, dn4 &Mv1)
{
    Mv0 = dn4{0.0f, 0.0f, 0.0f, 0.0f};
    Mv1 = dn4{0.0f, 0.0f, 0.0f, __builtin_inff()};
}

// the world-space hit point and its depth along the camera's axis n2 = col_2(V)
HRN v3 mvHitPoint(v3 o, v3 d, float t, v3 n2, float &depth)
{
    const v3 Pw = o + d * t;
    depth = -dot(n2, Pw - o);
    return Pw;
}

// a hit on a mesh the snapshot does not hold
HRN void mvUnmatched(v3 Pw, float depth, dn4 &Mv0, dn4 &Mv1)
{
    Mv0 = dn4{Pw.x, Pw.y, Pw.z, -1.0f};
    Mv1 = dn4{0.0f, 0.0f, 0.0f, depth};
}

// a hit at (u, v) of a triangle whose previous pose is (p0, e1, e2)
HRN void mvMatched(v3 p0, v3 e1, v3 e2, float u, float v, float depth, dn4 &Mv0, dn4 &Mv1)
{
    const v3 Q = (p0 + e1 * u) + e2 * v;
    const v3 Gn = cross(e1, e2);
    const v3 Ng = msValid(dot(Gn, Gn)) ? msNormalize(Gn) : v3(0.0f);
    Mv0 = dn4{Q.x, Q.y, Q.z, 1.0f};
    Mv1 = dn4{Ng.x, Ng.y, Ng.z, depth};
}

// The place pixel (x, y) of the new view gathers from: q = the surface point (Mv0.w == 1) or the sky direction (Mv0.w == 0) in the old
// camera's space (Mv0.w == -1 has no such place: its callers decide that; what is computed for it is not used).
HRN void mvOldSpace(const MvCam &cam, const dn4 &Mv0, int x, int y, float Wf, float Hf, float q[3])
{
    const HsCam &h = cam.hs;
    if (Mv0.w == 1.0f) {
        const float rx = Mv0.x - cam.eyeOld[0], ry = Mv0.y - cam.eyeOld[1], rz = Mv0.z - cam.eyeOld[2];
        for (int i = 0; i < 3; ++i) q[i] = HS_DOT(h.O[3 * i], h.O[3 * i + 1], h.O[3 * i + 2], rx, ry, rz);
    } else {
        const float cx = hsRayX(x, Wf, h.aspectNew, h.fovNew), cy = hsRayY(y, Hf, h.fovNew), cz = -1.0f;
        for (int i = 0; i < 3; ++i) q[i] = (h.R[3 * i] * cx + h.R[3 * i + 1] * cy) + h.R[3 * i + 2] * cz;
    }
}

// Merge at the pixel (x, y) of the new view with the motion planes' values Mv0, Mv1: F, A, G, M are updated in place when the answer is
// HS_REUSED (*nhOut = the samples taken over), and left alone otherwise.  The place it gathers from is the traced one (mvOldSpace), the
// normal the previous pose's geometric one, which may face either way: hsGather tests |dot| for it.
template <class S>
HRN int mvMerge(const S &s, const MvCam &cam, const HsParams &P, const dn4 &Mv0, const dn4 &Mv1, int x, int y, int W, int H, dn4 &F, dn4 &A, dn4 &G, dn4 &M, float *nhOut)
{
    const HsCam &hc = cam.hs;
    const float n = F.w;
    const bool sampled = n > 0.0f;
    const float cov = A.w / n;
    const bool surf = sampled && Mv0.w == 1.0f && cov >= 0.5f;
    const bool sky = sampled && Mv0.w == 0.0f && cov < 0.5f;
    bool ok = surf || sky;
    const float Wf = (float)W, Hf = (float)H;
    float q[3], Nq[3] = {0.0f, 0.0f, 0.0f};
    mvOldSpace(cam, Mv0, x, y, Wf, Hf, q);
    const float Ng[3] = {Mv1.x, Mv1.y, Mv1.z};
    if (surf) {
        const float dmean = G.w / A.w;
        ok = ok && abs_(Mv1.w - dmean) <= P.planeTol * dmean;
        for (int i = 0; i < 3; ++i) Nq[i] = HS_DOT(hc.O[3 * i], hc.O[3 * i + 1], hc.O[3 * i + 2], Ng[0], Ng[1], Ng[2]);
    }
    HsSums sums;
    if (!hsGather<true, true>(s, hc, P, ok, surf, q, Ng, Nq, W, H, sums)) return sampled ? HS_REJECTED : HS_UNSAMPLED;
    *nhOut = hsApply(sums, P, n, F, A, G, M);
    return HS_REUSED;
}

// the motion vector of pixel (x, y)
HRN dn4 mvVector(const MvCam &cam, const dn4 &Mv0, int x, int y, int W, int H)
{
    const float Wf = (float)W, Hf = (float)H;
    float q[3];
    mvOldSpace(cam, Mv0, x, y, Wf, Hf, q);
    float z, sx, sy;
    hsProject(cam.hs, q, Wf, Hf, z, sx, sy);
    if (Mv0.w == -1.0f || !(z > 0.0f)) return dn4{0.0f, 0.0f, 0.0f, Mv0.w};
    return dn4{sx - ((float)x + 0.5f), sy - ((float)y + 0.5f), z, Mv0.w};
}

} // namespace hr
