// hr_denoise.h — the per-pixel arithmetic of the denoiser (include/hrcore_denoise.h states the contract these lines implement).
// Pure float32 functions over a pixel source, no memory of their own, so that the kernels in hr_denoise.hip (global memory or an LDS
// tile behind the source) and the CPU test (tests/host/denoise_cpu.cpp, against heatray_amd/denoise.py) compile the same lines.
#pragma once
#include <stdint.h>

#ifdef HRD
#define HRN HRD
#else
// The host build has no hr_math.h (it needs the HIP runtime): the five functions used below, in the same lines.
#include <string.h>
#define HRN inline
namespace hr {
inline float fmax_(float x, float y) { return (x < y) ? y : x; }
inline float sqrt_(float x) { return __builtin_sqrtf(x); }
inline float floor_(float x) { return __builtin_floorf(x); }
inline float abs_(float x) { return __builtin_fabsf(x); }
inline float exp_(float xx)
{
    if (xx > 88.0f) return __builtin_inff();
    if (!(xx >= -87.0f)) return (xx != xx) ? xx : 0.0f;
    float x = xx;
    float z = floor_(1.44269504088896341f * x + 0.5f);
    x = x - z * 0.693359375f;
    x = x - z * -2.12194440e-4f;
    int n = (int)z;
    z = x * x;
    z = (((((1.9875691500e-4f * x + 1.3981999507e-3f) * x + 8.3334519073e-3f) * x + 4.1665795894e-2f) * x + 1.6666665459e-1f) * x + 5.0000001201e-1f) * z + x + 1.0f;
    const uint32_t bits = (uint32_t)(n + 127) << 23;
    float s;
    memcpy(&s, &bits, 4);
    return z * s;
}
} // namespace hr
#endif

namespace hr {

struct alignas(16) dn4 {
    float x, y, z, w;
};

struct DnParams {
    int32_t iterations, normalPower;
    float sigmaL, sigmaZ;
};

HRN float dnLum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// Prepare: frame F and the planes A (ALBEDO), G (NORMAL_DEPTH), M (MOMENTS) of one pixel -> its working values
//   cv = demodulated colour, luminance variance of the mean;  nd = unit normal, mean depth;  ac = effective albedo, coverage (-1: invalid)
HRN void dnPrepare(const dn4 &F, const dn4 &A, const dn4 &G, const dn4 &M, dn4 &cv, dn4 &nd, dn4 &ac)
{
    const float n = F.w;
    if (!(n > 0.0f)) {
        cv = dn4{0.0f, 0.0f, 0.0f, 0.0f}, nd = dn4{0.0f, 0.0f, 0.0f, 0.0f}, ac = dn4{0.0f, 0.0f, 0.0f, -1.0f};
        return;
    }
    const float hits = A.w, miss = n - hits;
    const float c[3] = {F.x / n, F.y / n, F.z / n};
    const float a[3] = {fmax_((A.x + miss) / n, 0.01f), fmax_((A.y + miss) / n, 0.01f), fmax_((A.z + miss) / n, 0.01f)};
    float v = 0.0f;
    if (n >= 2.0f) {
        const float m[3] = {M.x, M.y, M.z};
        float vc[3];
        for (int k = 0; k < 3; ++k) {
            float e = m[k] - (n * c[k]) * c[k];
            e = e > 0.0f ? e : 0.0f;
            vc[k] = ((e / (n - 1.0f)) / n) / (a[k] * a[k]);
        }
        v = dnLum(vc[0], vc[1], vc[2]);
    }
    cv = dn4{c[0] / a[0], c[1] / a[1], c[2] / a[2], v};
    const float l2 = (G.x * G.x + G.y * G.y) + G.z * G.z;
    nd = dn4{0.0f, 0.0f, 0.0f, 0.0f};
    if (hits > 0.0f) {
        if (l2 > 0.0f) {
            const float l = sqrt_(l2);
            nd.x = G.x / l, nd.y = G.y / l, nd.z = G.z / l;
        }
        nd.w = G.w / hits;
    }
    ac = dn4{a[0], a[1], a[2], hits / n};
}

// A pixel source S gives the working values of the pixel (x, y) of the image: S.cv(x, y), S.nd(x, y), S.cov(x, y); the functions below ask
// only for pixels inside the image.

// do two pixels look at one side of a surface (or both at none)?  Only then does one lend the other its variance or its depth.
HRN bool dnFacing(const dn4 &np, float covp, const dn4 &nq, float covq)
{
    return (covp == 0.0f && covq == 0.0f) || (np.x * nq.x + np.y * nq.y) + np.z * nq.z > 0.0f;
}

// the depth gradient of a pixel: the largest depth difference to a direct neighbour with a surface facing the same way
template <class S> HRN float dnGradient(const S &s, int x, int y, int W, int H)
{
    if (!(s.cov(x, y) > 0.0f)) return 0.0f;
    const dn4 np = s.nd(x, y);
    const float z = np.w;
    float g = 0.0f;
    const int ox[4] = {-1, 1, 0, 0}, oy[4] = {0, 0, -1, 1};
    for (int k = 0; k < 4; ++k) {
        const int qx = x + ox[k], qy = y + oy[k];
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const float covq = s.cov(qx, qy);
        if (!(covq > 0.0f)) continue;
        const dn4 nq = s.nd(qx, qy);
        if (!dnFacing(np, 1.0f, nq, covq)) continue;
        g = fmax_(g, abs_(z - nq.w));
    }
    return g;
}

// One a-trous iteration at a valid pixel: the new colour and variance.  Written without a branch around any load: a tap outside the image
// reads the pixel its coordinates clamp to and weighs nothing, so the compiler can issue the loads of many taps before it waits for the
// first (with a `continue` per tap every tap waited for its own loads in turn: 2.5 x slower from global memory,
// profiles/denoise_taps_ab.txt).  The sums skip a tap that weighs 0 exactly as the contract says: by a select.
template <class S> HRN dn4 dnFilter(const S &s, int x, int y, int W, int H, int step, const DnParams &P, float grad)
{
    const dn4 cp = s.cv(x, y), np = s.nd(x, y);
    const float covp = s.cov(x, y);
    float gv = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        const bool iny = qy >= 0 && qy < H;
        const int cy = iny ? qy : y;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            const bool inx = qx >= 0 && qx < W;
            const int cx = inx ? qx : x;
            const float covq = s.cov(cx, cy);
            const float vq = s.cv(cx, cy).w;
            bool ok = iny && inx && !(covq < 0.0f);
            if (dx != 0 || dy != 0) ok = ok && dnFacing(np, covp, s.nd(cx, cy), covq);
            const float g = (dy ? 0.25f : 0.5f) * (dx ? 0.25f : 0.5f);
            gv = ok ? gv + g * vq : gv;
            gs = ok ? gs + g : gs;
        }
    }
    const float sl = P.sigmaL * sqrt_(gv / gs) + 1e-6f;
    const float zs = (P.sigmaZ * (grad * (float)step) + 1e-3f * abs_(np.w)) + 1e-30f;
    const float lp = dnLum(cp.x, cp.y, cp.z);
    float S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, V = 0.0f, Wt = 0.0f;
#pragma unroll 1 // (a row of five taps in flight at a time: all 25 cost 190 VGPRs and the occupancy that hides what latency remains)
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * step;
        const bool iny = qy >= 0 && qy < H;
        const int cy = iny ? qy : y;
        const float kj = j == 0 ? 0.375f : ((j == 1 || j == -1) ? 0.25f : 0.0625f);
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * step;
            const bool inx = qx >= 0 && qx < W;
            const int cx = inx ? qx : x;
            const float k = kj * (i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f));
            const float covq = s.cov(cx, cy);
            const dn4 cq = s.cv(cx, cy);
            float w = k;
            if (i != 0 || j != 0) {
                const dn4 nq = s.nd(cx, cy);
                float wn = fmax_((np.x * nq.x + np.y * nq.y) + np.z * nq.z, 0.0f);
                for (int r = 0; r < P.normalPower; ++r) wn = wn * wn;
                wn = (covp == 0.0f && covq == 0.0f) ? 1.0f : wn;
                const float wc = fmax_(1.0f - 4.0f * abs_(covp - covq), 0.0f);
                const float we = exp_(-(abs_(np.w - nq.w) / zs + abs_(lp - dnLum(cq.x, cq.y, cq.z)) / sl));
                w = ((k * wn) * wc) * we;
            }
            const bool use = iny && inx && !(covq < 0.0f) && w > 0.0f;
            S0 = use ? S0 + w * cq.x : S0, S1 = use ? S1 + w * cq.y : S1, S2 = use ? S2 + w * cq.z : S2;
            V = use ? V + (w * w) * cq.w : V;
            Wt = use ? Wt + w : Wt;
        }
    }
    return dn4{S0 / Wt, S1 / Wt, S2 / Wt, V / (Wt * Wt)};
}

// Finish: the working colour back under its albedo, as a one-sample accumulation buffer
HRN dn4 dnFinish(const dn4 &cv, const dn4 &ac)
{
    if (ac.w < 0.0f) return dn4{0.0f, 0.0f, 0.0f, 0.0f};
    return dn4{cv.x * ac.x, cv.y * ac.y, cv.z * ac.z, 1.0f};
}

} // namespace hr
