// hr_history.h — the per-pixel arithmetic of history reprojection (include/hrcore_history.h states the contract these lines implement).
// Pure float32 functions over a history source, no memory of their own, so that the kernels in hr_history.hip and the CPU test
// (tests/host/history_cpu.cpp, against heatray_amd/history.py) compile the same lines.  dn4 and the host's sqrt_ / floor_ / abs_ come
// from hr_denoise.h.  hsCameras is host code on both sides: hr_history.inl calls it once per merge.  hsGather and hsApply are the one
// statement of the gather from the history: hr_reproject.h's preview and hr_motion.h's merge call them with their own place-finding.
#pragma once
#include "hr_denoise.h"

#ifndef HRD
namespace hr {
inline float fmin_(float x, float y) { return (y < x) ? y : x; }
} // namespace hr
#endif

namespace hr {

// what a merge knows about its two cameras: R = Rold^T Rnew and t = Rold^T (eye_new - eye_old) take a point of the new camera's space to
// the old one's, O = Rold^T (row i = column i of the old view matrix) takes a world-space normal there
struct HsCam {
    float R[9], O[9], t[3];
    float aspectNew, fovNew, aspectOld, fovOld, axOld; // axOld = aspectOld * fovOld
};

struct HsParams {
    float maxHistory, normalCos, planeTol, minWeight; // max_history as a float: sample counts are the frame's alpha
};

#define HS_DOT(ax, ay, az, bx, by, bz) (((ax) * (bx) + (ay) * (by)) + (az) * (bz))

// view matrices: camera -> world, column-major (hr_pass_params::view_matrix)
inline HsCam hsCameras(const float *vOld, float aspectOld, float fovOld, const float *vNew, float aspectNew, float fovNew)
{
    HsCam c;
    const float e[3] = {vNew[12] - vOld[12], vNew[13] - vOld[13], vNew[14] - vOld[14]};
    for (int i = 0; i < 3; ++i) {
        const float *o = vOld + 4 * i;
        for (int j = 0; j < 3; ++j) {
            const float *n = vNew + 4 * j;
            c.R[3 * i + j] = HS_DOT(o[0], o[1], o[2], n[0], n[1], n[2]);
        }
        c.O[3 * i + 0] = o[0], c.O[3 * i + 1] = o[1], c.O[3 * i + 2] = o[2];
        c.t[i] = HS_DOT(o[0], o[1], o[2], e[0], e[1], e[2]);
    }
    c.aspectNew = aspectNew, c.fovNew = fovNew, c.aspectOld = aspectOld, c.fovOld = fovOld;
    c.axOld = aspectOld * fovOld;
    return c;
}

HRN bool hsFinite(float v) { return abs_(v) < __builtin_inff(); }

// the camera-space direction through the centre of pixel (x, y), z = -1 (generatePrimary without the jitter and the normalisation)
HRN float hsRayX(int x, float Wf, float aspect, float fov) { return ((2.0f * (((float)x + 0.5f) / Wf) - 1.0f) * aspect) * fov; }
HRN float hsRayY(int y, float Hf, float fov) { return (2.0f * (((float)y + 0.5f) / Hf) - 1.0f) * fov; }

// Capture: frame F and the planes A (ALBEDO), G (NORMAL_DEPTH), M (MOMENTS) of one pixel -> its history
//   H0 = mean colour, samples;  H1 = mean second moment, coverage;  H2 = unit world-space normal, mean depth (+inf: sky)
HRN void hsCapture(const dn4 &F, const dn4 &A, const dn4 &G, const dn4 &M, dn4 &H0, dn4 &H1, dn4 &H2)
{
    const float n = F.w;
    if (!(n > 0.0f)) {
        H0 = H1 = H2 = dn4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    H0 = dn4{F.x / n, F.y / n, F.z / n, n};
    const float cov = A.w / n;
    H1 = dn4{M.x / n, M.y / n, M.z / n, cov};
    H2 = dn4{0.0f, 0.0f, 0.0f, __builtin_inff()};
    if (cov >= 0.5f) {
        const float l2 = HS_DOT(G.x, G.y, G.z, G.x, G.y, G.z);
        if (l2 > 0.0f) {
            const float l = sqrt_(l2);
            H2.x = G.x / l, H2.y = G.y / l, H2.z = G.z / l;
        }
        H2.w = G.w / A.w;
    }
}

// A history source S gives the three values of the pixel with index i = y * W + x: S.h0(i), S.h1(i), S.h2(i); the function below asks only
// for pixels inside the image.

enum { HS_UNSAMPLED = 0, HS_REJECTED = 1, HS_REUSED = 2 };

// The sums of a gather over the four taps: the weights that counted, and the history's colour, second moment and samples under them
struct HsSums {
    float wsum, ns, hs[3], ms[3];
};

// a point q of the old camera's space -> its depth z and its place (sx, sy) in the old view, in pixels (z <= 0: the place means nothing)
HRN void hsProject(const HsCam &cam, const float q[3], float Wf, float Hf, float &z, float &sx, float &sy)
{
    z = -q[2];
    sx = (((q[0] / z) / cam.axOld + 1.0f) * 0.5f) * Wf;
    sy = (((q[1] / z) / cam.fovOld + 1.0f) * 0.5f) * Hf;
}

// The gather every consumer of the history shares (hsMerge, rpPreviewFromGuide in hr_reproject.h, mvMerge in hr_motion.h): the history
// around the point q of the old camera's space, for a pixel of the class `surf` whose unit normal is N in world space and Nq in the old
// camera's (both unused for sky), `ok` being what the caller has decided so far.  Projection, border test, bilinear split, four taps with
// their class, normal (ABS_NORMAL: either winding) and plane tests, the minimum-weight test: the answer is whether the sums count.
// Written without a branch around any load: a pixel that has already lost its history, and a tap outside the image, read the pixel
// their coordinates clamp to and decide afterwards, so that the loads are issued together (the denoiser's lesson:
// profiles/denoise_taps_ab.txt).  The sums skip a tap that does not count by a select.  Without MOMENTS no H1 is read (eight float4, not
// twelve) and ms and ns stay 0.
template <bool MOMENTS, bool ABS_NORMAL, class S>
HRN bool hsGather(const S &s, const HsCam &cam, const HsParams &P, bool ok, bool surf, const float q[3], const float N[3], const float Nq[3], int W, int H, HsSums &sums)
{
    const float Wf = (float)W, Hf = (float)H;
    float z, sx, sy;
    hsProject(cam, q, Wf, Hf, z, sx, sy);
    ok = ok && z > 0.0f;
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
        const dn4 h0 = s.h0(i), h2 = s.h2(i);
        dn4 h1{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (MOMENTS) h1 = s.h1(i);
        bool use = ok && inside && h0.w > 0.0f && (hsFinite(h2.w) == surf);
        if (surf) {
            const float cosN = HS_DOT(N[0], N[1], N[2], h2.x, h2.y, h2.z), nd = ABS_NORMAL ? abs_(cosN) : cosN;
            const float px = h2.w * hsRayX(ux, Wf, cam.aspectOld, cam.fovOld), py = h2.w * hsRayY(uy, Hf, cam.fovOld), pz = h2.w * -1.0f;
            const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
            const float pd = abs_(HS_DOT(Nq[0], Nq[1], Nq[2], dx, dy, dz));
            use = use && nd >= P.normalCos && pd <= tol;
        }
        wsum = use ? wsum + w : wsum;
        hs[0] = use ? hs[0] + w * h0.x : hs[0], hs[1] = use ? hs[1] + w * h0.y : hs[1], hs[2] = use ? hs[2] + w * h0.z : hs[2];
        if constexpr (MOMENTS) {
            ms[0] = use ? ms[0] + w * h1.x : ms[0], ms[1] = use ? ms[1] + w * h1.y : ms[1], ms[2] = use ? ms[2] + w * h1.z : ms[2];
            ns = use ? ns + w * h0.w : ns;
        }
    }
    sums = HsSums{wsum, ns, {hs[0], hs[1], hs[2]}, {ms[0], ms[1], ms[2]}};
    return ok && !(wsum < P.minWeight);
}

// The sums of a gather that counts -> nh history samples added to the n the pixel has, in the frame and its three planes; returns nh
HRN float hsApply(const HsSums &sums, const HsParams &P, float n, dn4 &F, dn4 &A, dn4 &G, dn4 &M)
{
    const float wsum = sums.wsum;
    const float nh = floor_(fmin_(sums.ns / wsum, P.maxHistory));
    const float h[3] = {sums.hs[0] / wsum, sums.hs[1] / wsum, sums.hs[2] / wsum}, m2[3] = {sums.ms[0] / wsum, sums.ms[1] / wsum, sums.ms[2] / wsum};
    F.x = F.x + h[0] * nh, F.y = F.y + h[1] * nh, F.z = F.z + h[2] * nh, F.w = F.w + nh;
    M.x = M.x + m2[0] * nh, M.y = M.y + m2[1] * nh, M.z = M.z + m2[2] * nh, M.w = M.w + nh;
    A.x = A.x + (A.x / n) * nh, A.y = A.y + (A.y / n) * nh, A.z = A.z + (A.z / n) * nh, A.w = A.w + (A.w / n) * nh;
    G.x = G.x + (G.x / n) * nh, G.y = G.y + (G.y / n) * nh, G.z = G.z + (G.z / n) * nh, G.w = G.w + (G.w / n) * nh;
    return nh;
}

// Merge at the pixel (x, y) of the new view: F, A, G, M are updated in place when the answer is HS_REUSED (*nhOut = the samples taken
// over), and left alone otherwise.  The place it gathers from is the pixel's own mean depth along its centre ray, or that ray's
// direction for sky.
template <class S> HRN int hsMerge(const S &s, const HsCam &cam, const HsParams &P, int x, int y, int W, int H, dn4 &F, dn4 &A, dn4 &G, dn4 &M, float *nhOut)
{
    const float n = F.w;
    const bool sampled = n > 0.0f;
    const bool surf = sampled && (A.w / n >= 0.5f);
    const float Wf = (float)W, Hf = (float)H;
    const float cx = hsRayX(x, Wf, cam.aspectNew, cam.fovNew), cy = hsRayY(y, Hf, cam.fovNew), cz = -1.0f;
    float q[3], N[3] = {0.0f, 0.0f, 0.0f}, Nq[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 3; ++i) q[i] = (cam.R[3 * i] * cx + cam.R[3 * i + 1] * cy) + cam.R[3 * i + 2] * cz;
    if (surf) {
        const float d = G.w / A.w;
        const float l2 = HS_DOT(G.x, G.y, G.z, G.x, G.y, G.z);
        if (l2 > 0.0f) {
            const float l = sqrt_(l2);
            N[0] = G.x / l, N[1] = G.y / l, N[2] = G.z / l;
        }
        for (int i = 0; i < 3; ++i) {
            q[i] = d * q[i] + cam.t[i];
            Nq[i] = HS_DOT(cam.O[3 * i], cam.O[3 * i + 1], cam.O[3 * i + 2], N[0], N[1], N[2]);
        }
    }
    HsSums sums;
    if (!hsGather<true, false>(s, cam, P, sampled, surf, q, N, Nq, W, H, sums)) return sampled ? HS_REJECTED : HS_UNSAMPLED;
    *nhOut = hsApply(sums, P, n, F, A, G, M);
    return HS_REUSED;
}

// the samples a reused pixel took over as an integer (a NaN count — a history whose alpha is not finite — counts as none)
HRN uint32_t hsCount(float nh) { return nh >= 0.0f ? (uint32_t)nh : 0u; }

} // namespace hr
