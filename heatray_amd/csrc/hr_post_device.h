// hr_post_device.h — what the kernels of the post-process features (hr_history.hip, hr_reproject.hip, hr_denoise_spatial.hip,
// hr_adaptive.hip, hr_despeckle.hip) share.  Device code only.  The workgroup counters: a kernel counts per wave (waveCount, waveSum), lane 0 of each wave
// adds into `sRed` in LDS under the kernel's own rule for what it adds, and wgCountersFlush sends the workgroup's totals on: integer
// atomics, a result does not depend on their order.
#pragma once
#include "hr_math.h"    // HRD, G
#include "hr_denoise.h" // dn4
#include "hr_wave_sum.h" // waveSum (shared with the render stages)

namespace hr {

// lanes of the wave for which `p` holds; the same number in every lane
HRD uint32_t waveCount(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// (no barrier: the caller has one between this and the first add)
template <int N> HRD void wgCountersZero(uint32_t *sRed)
{
    if (threadIdx.x < (uint32_t)N) sRed[threadIdx.x] = 0u;
}

// after the waves' adds: the first N words of sRed -> result[0 .. N)
template <int N> HRD void wgCountersFlush(const uint32_t *sRed, unsigned long long *result)
{
    __syncthreads();
    if (threadIdx.x < (uint32_t)N && sRed[threadIdx.x]) atomicAdd(&result[threadIdx.x], (unsigned long long)sRed[threadIdx.x]);
}

// The history as hsMerge and rpPreviewFromGuide read it: three planes of W x H float4 one after the other (H0, H1, H2)
struct HsPlanes {
    const dn4 *p0, *p1, *p2;
    HRD HsPlanes(const dn4 *hist, size_t n) : p0(hist), p1(hist + n), p2(hist + 2 * n) {}
    HRD dn4 h0(int i) const { return G(p0)[i]; }
    HRD dn4 h1(int i) const { return G(p1)[i]; }
    HRD dn4 h2(int i) const { return G(p2)[i]; }
};

} // namespace hr
