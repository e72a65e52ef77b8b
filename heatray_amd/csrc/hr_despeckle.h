// hr_despeckle.h — the per-pixel arithmetic of firefly suppression (include/hrcore_despeckle.h states the contract these lines
// implement).  Pure float32 functions over a pixel source, like dnFilter of hr_denoise.h, so that the kernel in hr_despeckle.hip (an LDS
// tile behind the source) and the CPU test (tests/host/despeckle_cpu.cpp, against heatray_amd/despeckle.py) compile the same lines.
#pragma once
#include "hr_denoise.h"

namespace hr {

struct DkParams {
    int32_t rank, minTaps;
    float ratio, sigmas, floor;
};

// what became of a pixel; the counters of hr_despeckle_result count DK_PASSED .. DK_STARVED as valid
enum { DK_EMPTY = 0, DK_NONFINITE = 1, DK_PASSED = 2, DK_CLAMPED = 3, DK_KEPT = 4, DK_STARVED = 5 };

static constexpr int kDkRadius = 2; // the window: (2 * kDkRadius + 1)^2 - 1 taps

// the luminance of a pixel that is nobody's tap: no finite luminance equals it, and it is greater than none
HRN float dkNoTap() { return -__builtin_inff(); }
// (a comparison: false for a NaN and for both infinities)
HRN bool dkFinite(float x) { return abs_(x) <= 3.40282346638528859812e38f; }

// the class of a frame pixel (DK_EMPTY, DK_NONFINITE, or DK_PASSED for a VALID one) and l = its mean's luminance, dkNoTap() unless VALID
HRN int dkClass(const dn4 &F, float &l)
{
    l = dkNoTap();
    const float n = F.w;
    if (!(n > 0.0f)) return DK_EMPTY;
    const float lc = dnLum(F.x / n, F.y / n, F.z / n);
    if (!(dkFinite(lc) && dkFinite(n))) return DK_NONFINITE;
    l = lc;
    return DK_PASSED;
}

// A pixel source S gives S.lum(x, y) for a pixel inside the image: dkClass's l of that pixel.

// The pixel (x, y) with the frame's F in f and the moments' M in m: its status, and f and m as the outputs hold them.  Written
// without a branch around a tap's read, like dnFilter: a tap outside the image reads the pixel its coordinates clamp to and does not
// count.  The four largest luminances so far stay in order by compares and selects only: nothing here can round.
template <class S> HRN int dkPixel(const S &s, int x, int y, int W, int H, const DkParams &P, dn4 &f, dn4 &m)
{
    float l;
    const int cls = dkClass(f, l);
    if (cls == DK_NONFINITE) f = dn4{0.0f, 0.0f, 0.0f, 0.0f}, m = dn4{0.0f, 0.0f, 0.0f, 0.0f};
    if (cls != DK_PASSED) return cls;
    float t0 = dkNoTap(), t1 = t0, t2 = t0, t3 = t0;
    int K = 0;
#pragma unroll 1 // (a row of five taps in flight at a time: all 24 at once cost 77 VGPRs, and with them two of the eight waves per SIMD)
    for (int dy = -kDkRadius; dy <= kDkRadius; ++dy) {
        const int qy = y + dy;
        const bool iny = qy >= 0 && qy < H;
        const int cy = iny ? qy : y;
#pragma unroll
        for (int dx = -kDkRadius; dx <= kDkRadius; ++dx) {
            const int qx = x + dx;
            const bool inx = qx >= 0 && qx < W;
            const int cx = inx ? qx : x;
            const float lq = s.lum(cx, cy);
            float v = (iny && inx && (dx != 0 || dy != 0)) ? lq : dkNoTap(); // (the centre is read like a tap outside the image: it does not count)
            K = v > dkNoTap() ? K + 1 : K;
            bool up = v > t0;
            float d = up ? t0 : v;
            t0 = up ? v : t0;
            up = d > t1, v = up ? t1 : d, t1 = up ? d : t1;
            up = v > t2, d = up ? t2 : v, t2 = up ? v : t2;
            t3 = d > t3 ? d : t3;
        }
    }
    if (K < P.minTaps) return DK_STARVED;
    const float R = P.rank == 1 ? t0 : (P.rank == 2 ? t1 : (P.rank == 3 ? t2 : t3));
    const float T = fmax_(P.ratio * R + P.floor, 0.0f);
    const float ex = l - T;
    if (!(ex > 0.0f)) return DK_PASSED;
    const float n = f.w;
    if (n >= 2.0f) {
        const float c[3] = {f.x / n, f.y / n, f.z / n}, mk[3] = {m.x, m.y, m.z};
        float vc[3];
        for (int k = 0; k < 3; ++k) {
            float e = mk[k] - (n * c[k]) * c[k];
            e = e > 0.0f ? e : 0.0f;
            vc[k] = (e / (n - 1.0f)) / n;
        }
        const float v = dnLum(vc[0], vc[1], vc[2]);
        if (ex * ex > (P.sigmas * P.sigmas) * v) return DK_KEPT;
    }
    const float sc = T / l, s2 = sc * sc;
    f = dn4{f.x * sc, f.y * sc, f.z * sc, f.w};
    m = dn4{m.x * s2, m.y * s2, m.z * s2, m.w};
    return DK_CLAMPED;
}

} // namespace hr
