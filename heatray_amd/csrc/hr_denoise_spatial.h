// hr_denoise_spatial.h — the per-pixel arithmetic of the spatial variance estimate (include/hrcore_denoise_spatial.h states the contract
// these lines implement).  A pure float32 function over a pixel source, like dnFilter of hr_denoise.h, so that the kernel in
// hr_denoise_spatial.hip (an LDS tile behind the source) and the CPU test (tests/host/denoise_spatial_cpu.cpp, against
// heatray_amd/denoise_spatial.py) compile the same lines.
#pragma once
#include "hr_denoise.h"

namespace hr {

struct DsParams {
    int32_t below, minTaps, normalPower;
    float sigmaZ;
};

enum { DS_KEPT = 0, DS_ESTIMATED = 1, DS_STARVED = 2 };

static constexpr int kDsRadius = 3; // the window: (2 * kDsRadius + 1)^2 taps

// is a valid pixel with n samples a spatial pixel?
HRN bool dsSpatial(float n, const DsParams &P) { return n < (float)P.below; }

// A pixel source S gives, for a pixel (x, y) inside the image: S.nd(x, y) = unit normal and depth, S.lum(x, y) = the luminance of its
// demodulated colour, S.alum(x, y) = the luminance of its effective albedo, S.n(x, y) = its samples, S.cov(x, y) = its coverage
// (< 0: invalid).

struct DsTap {
    float w, n, l; // the tap's weight (0: it does not count), samples and luminance
};
struct DsResult {
    int status; // DS_ESTIMATED or DS_STARVED
    float v;    // the pixel's variance after the estimate
};

// the tap (dx, dy) of p as the pixel (cx, cy) gives it; `ok`: the tap is inside the image
template <class S> HRN DsTap dsTap(const S &s, int cx, int cy, int dx, int dy, bool ok, const dn4 &np, float covp, float lap, float grad, const DsParams &P)
{
    const float covq = s.cov(cx, cy);
    const dn4 q = s.nd(cx, cy);
    const float nq = s.n(cx, cy), lq = s.lum(cx, cy), laq = s.alum(cx, cy);
    float wn = fmax_((np.x * q.x + np.y * q.y) + np.z * q.z, 0.0f);
    for (int r = 0; r < P.normalPower; ++r) wn = wn * wn;
    wn = (covp == 0.0f && covq == 0.0f) ? 1.0f : wn;
    const float wc = fmax_(1.0f - 4.0f * abs_(covp - covq), 0.0f);
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const float r = (float)(ax > ay ? ax : ay);
    const float zs = (P.sigmaZ * (grad * r) + 1e-3f * abs_(np.w)) + 1e-30f;
    const float wz = exp_(-(abs_(np.w - q.w) / zs));
    const float wa = fmax_(1.0f - 4.0f * abs_(lap - laq), 0.0f);
    float w = ((wn * wc) * wz) * wa;
    w = (dx == 0 && dy == 0) ? 1.0f : w;
    return DsTap{(ok && !(covq < 0.0f) && w > 0.0f) ? w : 0.0f, nq, lq};
}

// The estimate at a valid spatial pixel with the prepared variance v.  Written without a branch around a load, like
// dnFilter: a tap outside the image reads the pixel its coordinates clamp to and does not count.  The second pass computes every weight
// again (the same lines on the same values: the same bits) instead of keeping 49 of them in registers.
template <class S> HRN DsResult dsEstimate(const S &s, int x, int y, int W, int H, const DsParams &P, float grad, float v)
{
    const dn4 np = s.nd(x, y);
    const float covp = s.cov(x, y), n = s.n(x, y), lap = s.alum(x, y);
    float W0 = 0.0f, Wn = 0.0f, L = 0.0f;
    int K = 0;
#pragma unroll 1
    for (int dy = -kDsRadius; dy <= kDsRadius; ++dy) {
        const int qy = y + dy;
        const bool iny = qy >= 0 && qy < H;
        const int cy = iny ? qy : y;
#pragma unroll
        for (int dx = -kDsRadius; dx <= kDsRadius; ++dx) {
            const int qx = x + dx;
            const bool inx = qx >= 0 && qx < W;
            const int cx = inx ? qx : x;
            const DsTap t = dsTap(s, cx, cy, dx, dy, iny && inx, np, covp, lap, grad, P);
            const bool use = t.w > 0.0f;
            const float u = t.w * t.n;
            W0 = use ? W0 + t.w : W0, Wn = use ? Wn + u : Wn, L = use ? L + u * t.l : L;
            K = use ? K + 1 : K;
        }
    }
    const float mu = L / Wn;
    float E = 0.0f;
#pragma unroll 1
    for (int dy = -kDsRadius; dy <= kDsRadius; ++dy) {
        const int qy = y + dy;
        const bool iny = qy >= 0 && qy < H;
        const int cy = iny ? qy : y;
#pragma unroll
        for (int dx = -kDsRadius; dx <= kDsRadius; ++dx) {
            const int qx = x + dx;
            const bool inx = qx >= 0 && qx < W;
            const int cx = inx ? qx : x;
            const DsTap t = dsTap(s, cx, cy, dx, dy, iny && inx, np, covp, lap, grad, P);
            const float u = t.w * t.n, e = t.l - mu;
            E = t.w > 0.0f ? E + u * (e * e) : E;
        }
    }
    if (K < P.minTaps) return DsResult{DS_STARVED, v};
    const float kf = (float)K;
    const float s2 = (E / W0) * (kf / (kf - 1.0f));
    return DsResult{DS_ESTIMATED, fmax_(v, s2 / n)};
}

} // namespace hr
