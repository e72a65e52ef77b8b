// hr_adaptive.h — the per-pixel arithmetic of adaptive sampling (include/hrcore_adaptive.h states the contract these lines implement).
// Pure float32 functions, no memory of their own, so that the kernels in hr_adaptive.hip and the CPU test (tests/host/adaptive_cpu.cpp,
// against heatray_amd/adaptive.py) compile the same lines.  dn4, dnLum and the host's fmax_ / sqrt_ come from hr_denoise.h.
#pragma once
#include "hr_denoise.h"

namespace hr {

// the error of one pixel from its frame value F and its MOMENTS value M: the standard deviation of the mean's luminance, relative to the
// mean's luminance (absolute below `floor`); +inf while the pixel has fewer than minSamples samples (min_samples as a float: sample
// counts are the frame's alpha)
HRN float adError(const dn4 &F, const dn4 &M, float floor, float minSamples)
{
    const float n = F.w;
    if (!(n > 0.0f)) return __builtin_inff();
    if (n < minSamples) return __builtin_inff();
    const float c[3] = {F.x / n, F.y / n, F.z / n};
    const float m[3] = {M.x, M.y, M.z};
    float vc[3];
    for (int k = 0; k < 3; ++k) {
        float e = m[k] - (n * c[k]) * c[k];
        e = e > 0.0f ? e : 0.0f;
        vc[k] = (e / (n - 1.0f)) / n;
    }
    const float v = dnLum(vc[0], vc[1], vc[2]);
    return sqrt_(v) / fmax_(dnLum(c[0], c[1], c[2]), floor);
}

HRN bool adUnconverged(float err, float threshold) { return err > threshold; }

// a finite error as an ordered integer (errors are not negative), 0 for +inf and NaN: what max_error is the maximum of
HRN uint32_t adFiniteBits(float err)
{
    uint32_t b;
    __builtin_memcpy(&b, &err, 4);
    return (b & 0x7fffffffu) < 0x7f800000u ? (b & 0x7fffffffu) : 0u;
}

} // namespace hr
