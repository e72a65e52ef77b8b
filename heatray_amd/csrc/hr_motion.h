// hr_motion.h — the per-pixel arithmetic of motion reprojection (include/hrcore_motion.h states the contract these lines implement).
// Pure float32 functions with no memory of their own, so that the kernels in hr_motion.hip and the CPU test (tests/host/motion_cpu.cpp,
// against heatray_amd/motion.py) compile the same lines.  HsCam, HsParams, hsRayX / hsRayY, hsFinite, hsCount and the HS_* answers come
// from hr_history.h; v3, dot, cross, msValid and msNormalize from hr_mesh.h, dfDir (the contract's dir) from hr_deform.h.  The tap loop
// is hsMerge's, stated again with this feature's normal test: k_history_merge's registers are pinned by a test and stay as they are.
#pragma once
#include "hr_history.h"
#include "hr_deform.h"

namespace hr {

// the two cameras of a merge or of the motion vectors: hsCameras' numbers and the old camera's eye
struct MvCam {
    HsCam hs;
    float eyeOld[3];
};

inline MvCam mvCameras(const float *vOld, float aspectOld, float fovOld, const float *vNew, float aspectNew, float fovNew)
{
    MvCam c;
    c.hs = hsCameras(vOld, aspectOld, fovOld, vNew, aspectNew, fovNew);
    c.eyeOld[0] = vOld[12], c.eyeOld[1] = vOld[13], c.eyeOld[2] = vOld[14];
    return c;
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
// HS_REUSED (*nhOut = the samples taken over), and left alone otherwise.  Like hsMerge, written without a branch around any load.
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
    const float z = -q[2];
    ok = ok && z > 0.0f;
    const float sx = (((q[0] / z) / hc.axOld + 1.0f) * 0.5f) * Wf;
    const float sy = (((q[1] / z) / hc.fovOld + 1.0f) * 0.5f) * Hf;
    ok = ok && (sx >= -1.0f && sx <= Wf + 1.0f && sy >= -1.0f && sy <= Hf + 1.0f);
    const float fx = ok ? sx - 0.5f : 0.0f, fy = ok ? sy - 0.5f : 0.0f; // (a position that is not ok may be NaN: no integer is made of it)
    const float x0f = floor_(fx), y0f = floor_(fy);
    const float wx = fx - x0f, wy = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float tol = P.planeTol * z;
    float wsum = 0.0f, ns = 0.0f, hs[3] = {0.0f, 0.0f, 0.0f}, ms[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
        const float w = ((k & 1) ? wx : 1.0f - wx) * ((k >> 1) ? wy : 1.0f - wy);
        const bool inside = tx >= 0 && tx < W && ty >= 0 && ty < H;
        const int ux = tx < 0 ? 0 : (tx >= W ? W - 1 : tx), uy = ty < 0 ? 0 : (ty >= H ? H - 1 : ty);
        const int i = uy * W + ux;
        const dn4 h0 = s.h0(i), h1 = s.h1(i), h2 = s.h2(i);
        bool use = ok && inside && h0.w > 0.0f && (hsFinite(h2.w) == surf);
        if (surf) {
            const float nd = abs_(HS_DOT(Ng[0], Ng[1], Ng[2], h2.x, h2.y, h2.z));
            const float px = h2.w * hsRayX(ux, Wf, hc.aspectOld, hc.fovOld), py = h2.w * hsRayY(uy, Hf, hc.fovOld), pz = h2.w * -1.0f;
            const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
            const float pd = abs_(HS_DOT(Nq[0], Nq[1], Nq[2], dx, dy, dz));
            use = use && nd >= P.normalCos && pd <= tol;
        }
        wsum = use ? wsum + w : wsum;
        hs[0] = use ? hs[0] + w * h0.x : hs[0], hs[1] = use ? hs[1] + w * h0.y : hs[1], hs[2] = use ? hs[2] + w * h0.z : hs[2];
        ms[0] = use ? ms[0] + w * h1.x : ms[0], ms[1] = use ? ms[1] + w * h1.y : ms[1], ms[2] = use ? ms[2] + w * h1.z : ms[2];
        ns = use ? ns + w * h0.w : ns;
    }
    ok = ok && !(wsum < P.minWeight);
    if (!ok) return sampled ? HS_REJECTED : HS_UNSAMPLED;
    const float nh = floor_(fmin_(ns / wsum, P.maxHistory));
    const float h[3] = {hs[0] / wsum, hs[1] / wsum, hs[2] / wsum}, m2[3] = {ms[0] / wsum, ms[1] / wsum, ms[2] / wsum};
    F.x = F.x + h[0] * nh, F.y = F.y + h[1] * nh, F.z = F.z + h[2] * nh, F.w = F.w + nh;
    M.x = M.x + m2[0] * nh, M.y = M.y + m2[1] * nh, M.z = M.z + m2[2] * nh, M.w = M.w + nh;
    A.x = A.x + (A.x / n) * nh, A.y = A.y + (A.y / n) * nh, A.z = A.z + (A.z / n) * nh, A.w = A.w + (A.w / n) * nh;
    G.x = G.x + (G.x / n) * nh, G.y = G.y + (G.y / n) * nh, G.z = G.z + (G.z / n) * nh, G.w = G.w + (G.w / n) * nh;
    *nhOut = nh;
    return HS_REUSED;
}

// the motion vector of pixel (x, y)
HRN dn4 mvVector(const MvCam &cam, const dn4 &Mv0, int x, int y, int W, int H)
{
    const HsCam &hc = cam.hs;
    const float Wf = (float)W, Hf = (float)H;
    float q[3];
    mvOldSpace(cam, Mv0, x, y, Wf, Hf, q);
    const float z = -q[2];
    const float sx = (((q[0] / z) / hc.axOld + 1.0f) * 0.5f) * Wf;
    const float sy = (((q[1] / z) / hc.fovOld + 1.0f) * 0.5f) * Hf;
    if (Mv0.w == -1.0f || !(z > 0.0f)) return dn4{0.0f, 0.0f, 0.0f, Mv0.w};
    return dn4{sx - ((float)x + 0.5f), sy - ((float)y + 0.5f), z, Mv0.w};
}

} // namespace hr
