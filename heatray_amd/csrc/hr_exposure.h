// hr_exposure.h — the arithmetic of auto-exposure (include/hrcore_exposure.h states the contract these lines implement): the class of one
// pixel, the ordered reduce of the 256 bins and the inverse of the piecewise-linear log.  Pure functions, no memory of their own, so
// that the kernels in hr_exposure.hip and the CPU test (tests/host/exposure_cpu.cpp, against heatray_amd/exposure.py) compile the same
// lines.  dn4, dnLum and the host's fmax_ come from hr_denoise.h.
#pragma once
#include "hr_denoise.h"

#ifndef HRD
namespace hr {
inline float fmin_(float x, float y) { return (y < x) ? y : x; }
} // namespace hr
#endif

namespace hr {

static constexpr int kExBins = 256;
// what exClass answers beside a bin, and where the words of a metering lie (unsigned long long each): the bins, the four class
// counters in this order, then what the reduce writes
enum { kExBelow = 256, kExAbove = 257, kExNonfinite = 258, kExInvalid = 259 };
enum { kExWordScale = 260, kExWordTarget, kExWordLavg, kExWordPosition, kExWordCounted, kExWordUsed, kExWordFlags, kExWords };
enum { kExEmpty = 1u, kExClampedLow = 2u, kExClampedHigh = 4u, kExAdapted = 8u }; // HR_EXPOSURE_*

struct ExParams {
    float key;
    int32_t lowPermille, highPermille;
    float minScale, maxScale, adapt;
};

struct ExWindow { // half-open, in pixels; the whole image: 0 0 W H
    int32_t x0, y0, x1, y1;
};

struct ExReduced {
    float scale, target, lavg;
    uint32_t position, flags;
    unsigned long long counted, used;
};

HRN uint32_t exBits(float v)
{
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}
HRN float exFromBits(uint32_t b)
{
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

// the bin of one pixel of an accumulation-format image, 0 .. 255, or the class that counts it instead
HRN int exClass(const dn4 &p)
{
    const float a = p.w;
    if (!(a > 0.0f)) return kExInvalid;
    const float L = dnLum(p.x / a, p.y / a, p.z / a);
    const uint32_t b = exBits(L);
    if ((b & 0x7f800000u) == 0x7f800000u) return kExNonfinite;
    if (b >> 31) return kExBelow;
    const int k = (int)(b >> 20) - 888;
    return k < 0 ? kExBelow : (k > 255 ? kExAbove : k);
}

// the luminance at position q (1/4096 octave above 2^-16, q < 2^17): the inverse of exClass's map
HRN float exLuminanceAt(uint32_t q) { return exFromBits((((q >> 12) - 16u + 127u) << 23) | ((q & 4095u) << 11)); }

// The ordered pass over the bins in three pieces, so that one lane (exReduce below: the CPU test, the reference's shape) and a workgroup
// with a scan (k_exposure_reduce) compute the same integers from the same lines.
// the percentile bounds of N counted pixels: [lo, hi) in sorted order
HRN void exBounds(unsigned long long N, const ExParams &P, unsigned long long &lo, unsigned long long &hi)
{
    lo = N * (unsigned long long)P.lowPermille / 1000ull;
    hi = N * (unsigned long long)P.highPermille / 1000ull;
    if (hi <= lo) hi = lo + 1;
}

// bin k's term of T: used_k * (2k + 1), with C the count before the bin and h the bin's
HRN unsigned long long exTerm(int k, unsigned long long C, unsigned long long h, unsigned long long lo, unsigned long long hi)
{
    const unsigned long long end = C + h;
    const unsigned long long to = end < hi ? end : hi, from = C > lo ? C : lo;
    return to > from ? (to - from) * (unsigned long long)(2 * k + 1) : 0ull;
}

// N and T -> the result.  hasState / prev: the adaptation state before; returns whether there is one after, *next its scale.
HRN bool exFinish(unsigned long long N, unsigned long long T, const ExParams &P, bool hasState, float prev, ExReduced &r, float *next)
{
    r = ExReduced{};
    r.counted = N;
    if (N == 0) {
        r.flags = kExEmpty;
        r.target = r.scale = hasState ? prev : 1.0f;
        *next = prev;
        return hasState;
    }
    unsigned long long lo, hi;
    exBounds(N, P, lo, hi);
    const unsigned long long U = hi - lo;
    r.used = U;
    r.position = (uint32_t)((T << 8) / U);
    r.lavg = exLuminanceAt(r.position);
    const float t = P.key / r.lavg;
    const float floored = fmax_(t, P.minScale);
    r.target = fmin_(floored, P.maxScale);
    if (t < P.minScale) r.flags |= kExClampedLow;
    if (P.maxScale < floored) r.flags |= kExClampedHigh;
    if (hasState && P.adapt < 1.0f) {
        r.scale = prev + (r.target - prev) * P.adapt;
        r.flags |= kExAdapted;
    } else {
        r.scale = r.target;
    }
    *next = r.scale;
    return true;
}

HRN bool exReduce(const unsigned long long *hist, const ExParams &P, bool hasState, float prev, ExReduced &r, float *next)
{
    unsigned long long N = 0, lo = 0, hi = 0, C = 0, T = 0;
    for (int k = 0; k < kExBins; ++k) N += hist[k];
    exBounds(N, P, lo, hi);
    for (int k = 0; k < kExBins; ++k) {
        T += exTerm(k, C, hist[k], lo, hi);
        C += hist[k];
    }
    return exFinish(N, T, P, hasState, prev, r, next);
}

} // namespace hr
