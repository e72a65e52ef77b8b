// hr_metric.h — the arithmetic of the convergence metric (include/hrcore_metric.h states the contract these lines implement): the terms
// of one pixel for both kinds, the bin of a term, and the fold of 256 bins into the one correctly rounded double of their exact sum.
// Pure functions, no memory of their own, so that the kernels in hr_metric.hip, the host section hr_metric.inl (the fold) and the CPU
// test (tests/host/metric_cpu.cpp, against heatray_amd/metric.py) compile the same lines.  dn4 and dnLum come from hr_denoise.h.
#pragma once
#include "hr_denoise.h"

namespace hr {

static constexpr int kMtBins = 256;
enum { kMtCompare = 0, kMtEstimate = 1 }; // HR_METRIC_COMPARE / HR_METRIC_ESTIMATE
// what mtCompare and mtEstimate answer: the pixel's class
enum { kMtCounted = 0, kMtNonfinite = 1, kMtSkipped = 2 };
// where the words of a measurement lie (unsigned long long each): the bins of NUM, the bins of DEN, the four counters in this order,
// the bits of max_abs
enum { kMtWordNum = 0, kMtWordDen = 256, kMtWordCounted = 512, kMtWordDiffering, kMtWordNonfinite, kMtWordSkipped, kMtWordMaxAbs, kMtWords };
enum { kMtEmpty = 1u, kMtZeroDenominator = 2u }; // HR_METRIC_*

struct MtWindow { // half-open, in pixels; the whole image: 0 0 W H
    int32_t x0, y0, x1, y1;
};

HRN uint32_t mtBits(float v)
{
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}
HRN bool mtFinite(float v) { return (mtBits(v) & 0x7f800000u) != 0x7f800000u; }

// ---- the terms of one pixel.  x[] goes to NUM, y[] to DEN, and only when the answer is kMtCounted.
// Compare: I and R are the pixel in the image and in the reference (accumulation format); three terms each.  differing: d != 0 in some
// channel; maxAbs: the bits of the largest |d| (non-negative floats order as their bits do).
HRN int mtCompare(const dn4 &I, const dn4 &R, float x[3], float y[3], bool &differing, uint32_t &maxAbs)
{
    const bool hasI = I.w > 0.0f, hasR = R.w > 0.0f;
    const float cI[3] = {hasI ? I.x / I.w : 0.0f, hasI ? I.y / I.w : 0.0f, hasI ? I.z / I.w : 0.0f};
    const float cR[3] = {hasR ? R.x / R.w : 0.0f, hasR ? R.y / R.w : 0.0f, hasR ? R.z / R.w : 0.0f};
    bool finite = true;
    differing = false, maxAbs = 0u;
    for (int k = 0; k < 3; ++k) {
        const float d = cI[k] - cR[k];
        x[k] = d * d, y[k] = cR[k] * cR[k];
        finite = finite && mtFinite(x[k]) && mtFinite(y[k]);
        differing = differing || d != 0.0f;
        const uint32_t a = mtBits(d) & 0x7fffffffu;
        maxAbs = a > maxAbs ? a : maxAbs;
    }
    return finite ? kMtCounted : kMtNonfinite;
}

// Estimate: F and M are the pixel in the frame and in the MOMENTS plane; one term each: the variance of the mean's luminance and the
// square of the mean's luminance (the lines of adError in hr_adaptive.h up to its square root)
HRN int mtEstimate(const dn4 &F, const dn4 &M, float &x, float &y)
{
    const float n = F.w;
    x = y = 0.0f;
    if (!(n >= 2.0f)) return kMtSkipped;
    const float c[3] = {F.x / n, F.y / n, F.z / n};
    const float m[3] = {M.x, M.y, M.z};
    float vc[3];
    for (int k = 0; k < 3; ++k) {
        float e = m[k] - (n * c[k]) * c[k];
        e = e > 0.0f ? e : 0.0f;
        vc[k] = (e / (n - 1.0f)) / n;
    }
    const float l = dnLum(c[0], c[1], c[2]);
    x = dnLum(vc[0], vc[1], vc[2]), y = l * l;
    return mtFinite(x) && mtFinite(y) ? kMtCounted : kMtNonfinite;
}

// ---- a finite non-negative term t -> bins[mtBin(t)] += mtMantissa(t): the term is mantissa * 2^(max(bin, 1) - 150), exactly
HRN uint32_t mtBin(float t) { return (mtBits(t) >> 23) & 0xffu; } // (a term has no sign bit; 255 is Inf and NaN, which are no terms)
HRN uint32_t mtMantissa(float t)
{
    const uint32_t b = mtBits(t);
    return (b & 0x7fffffu) | ((b & 0x7f800000u) ? 0x800000u : 0u);
}

// ---- the fold (host): S = sum of bins[e] * 2^(max(e, 1) - 1), an integer in units of 2^-149 of fewer than 320 bits, kept in 32-bit
// limbs (least significant first); the result is S * 2^-149 rounded once to binary64, to nearest, ties to even
static constexpr int kMtLimbs = 11; // 352 bits: bins below 2^64 shifted by at most 253

// w += v * 2^(32 * at): v is any 64-bit value
inline void mtLimbsAdd(uint32_t *w, int at, unsigned long long v)
{
    for (int k = at; v != 0ull && k < kMtLimbs; ++k) {
        const unsigned long long t = (unsigned long long)w[k] + (v & 0xffffffffull);
        w[k] = (uint32_t)t;
        v = (v >> 32) + (t >> 32);
    }
}

inline uint32_t mtLimbsBit(const uint32_t *w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }

inline double mtFold(const unsigned long long *bins)
{
    uint32_t w[kMtLimbs] = {};
    for (int e = 0; e < kMtBins; ++e) {
        if (bins[e] == 0ull) continue;
        const int s = (e > 1 ? e : 1) - 1, q = s >> 5, r = s & 31; // (r <= 31: a 32-bit half shifted by it stays inside 64 bits)
        mtLimbsAdd(w, q, (bins[e] & 0xffffffffull) << r);
        mtLimbsAdd(w, q + 1, (bins[e] >> 32) << r);
    }
    int p = kMtLimbs * 32 - 1; // the highest set bit
    while (p >= 0 && !mtLimbsBit(w, p)) --p;
    if (p < 0) return 0.0;
    unsigned long long mant = 0ull; // the top 53 bits (all of S when it has no more)
    const int low = p > 52 ? p - 52 : 0;
    for (int i = p; i >= low; --i) mant = (mant << 1) | mtLimbsBit(w, i);
    if (low > 0) {
        bool sticky = false;
        for (int i = low - 2; i >= 0 && !sticky; --i) sticky = mtLimbsBit(w, i) != 0u;
        if (mtLimbsBit(w, low - 1) && (sticky || (mant & 1ull))) mant += 1ull; // (2^53 when it carries all the way: still exact below)
    }
    // mant * 2^(low - 149), mant <= 2^53 and the product a normal binary64: exact.  The power of two is built from its bits.
    const unsigned long long scaleBits = (unsigned long long)(low - 149 + 1023) << 52;
    double scale;
    __builtin_memcpy(&scale, &scaleBits, 8);
    return (double)mant * scale;
}

// the words of a measurement -> what the result says beside the counters
struct MtFolded {
    double num, den, value, mse;
    uint32_t flags;
};

inline MtFolded mtFinish(const unsigned long long *words, uint32_t kind)
{
    MtFolded r{mtFold(words + kMtWordNum), mtFold(words + kMtWordDen), 0.0, 0.0, 0u};
    const unsigned long long counted = words[kMtWordCounted];
    if (r.den == 0.0) {
        r.flags |= kMtZeroDenominator;
        r.value = r.num == 0.0 ? 0.0 : (double)__builtin_inff();
    } else {
        r.value = __builtin_sqrt(r.num / r.den);
    }
    if (counted == 0ull) {
        r.flags |= kMtEmpty;
        r.value = r.mse = 0.0;
    } else {
        r.mse = r.num / (double)(kind == (uint32_t)kMtCompare ? 3ull * counted : counted);
    }
    return r;
}

} // namespace hr
