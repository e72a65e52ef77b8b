// hr_post_device.h — what the kernels of the post-process features share.  Device code only, but for the grid that goes with the tile.
//   The workgroup counters (hr_history.hip, hr_reproject.hip, hr_motion.hip, hr_denoise_spatial.hip, hr_adaptive.hip, hr_despeckle.hip,
//     hr_exposure.hip, hr_metric.hip, hr_mesh.hip, hr_deform.hip): a kernel counts per wave (waveCount, waveSum), lane 0 of each wave adds into `sRed` in LDS
//     under the kernel's own rule for what it adds, and wgCountersFlush sends the workgroup's totals on: integer atomics, a result does
//     not depend on their order.
//   The 32 x 8 tile of one lane per pixel (k_history_merge, k_reproject_merge, k_reproject_preview, k_motion_trace, k_motion_merge):
//     kPostTileW / kPostTileH, postTileOrigin, postTilePixel, postTileGrid.
//   The history's planes as hsGather reads them (the three merges and the preview): HsPlanes.
//   The tail of a merge (k_history_merge, k_reproject_merge, k_motion_merge): mergeTail.
#pragma once
#include "hr_math.h"    // HRD, G
#include "hr_history.h" // dn4 (hr_denoise.h), hsCount
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

// The pixels of a workgroup: four waves of 8 x 8 side by side.  A row of a wave's own pixels is one 128-byte line per float4 plane.
static constexpr int kPostTileW = 32, kPostTileH = 8;

// the image position of the workgroup's first pixel (a one-dimensional grid: no bound on the image's height)
HRD void postTileOrigin(int W, int &x0, int &y0)
{
    const uint32_t tilesX = (uint32_t)(W + kPostTileW - 1) / (uint32_t)kPostTileW;
    x0 = (int)(blockIdx.x % tilesX) * kPostTileW, y0 = (int)(blockIdx.x / tilesX) * kPostTileH;
}

// the pixel of this lane, and whether it lies inside the image: lane = (y & 7) * 8 + (x & 7) within the wave's 8 x 8 block
HRD bool postTilePixel(int W, int H, int &x, int &y)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    postTileOrigin(W, x, y);
    x += (int)(wave * 8u + (lane & 7u)), y += (int)(lane >> 3);
    return x < W && y < H;
}

inline dim3 postTileGrid(int W, int H) { return dim3(((W + kPostTileW - 1) / kPostTileW) * ((H + kPostTileH - 1) / kPostTileH)); }

// The history as hsGather reads it: three planes of W x H float4 one after the other (H0, H1, H2)
struct HsPlanes {
    const dn4 *p0, *p1, *p2;
    HRD HsPlanes(const dn4 *hist, size_t n) : p0(hist), p1(hist + n), p2(hist + 2 * n) {}
    HRD dn4 h0(int i) const { return G(p0)[i]; }
    HRD dn4 h1(int i) const { return G(p1)[i]; }
    HRD dn4 h2(int i) const { return G(p2)[i]; }
};

// The tail of a merge at pixel i: where history was taken over the four updated float4 go back, and the wave's {reused pixels, rejected
// pixels, samples taken over} are added to sRed[0 .. 3) (behind wgCountersZero and a barrier; a sum of zero is added like any other).
HRD void mergeTail(bool reused, bool rejected, float nh, int i, const dn4 &F, const dn4 &A, const dn4 &Gn, const dn4 &M, dn4 *frame, dn4 *albedo, dn4 *normalDepth,
                   dn4 *moments, uint32_t *sRed)
{
    if (reused) G(frame)[i] = F, G(albedo)[i] = A, G(normalDepth)[i] = Gn, G(moments)[i] = M;
    const uint32_t samples = waveSum(reused ? hsCount(nh) : 0u); // (at most 65536 per pixel: a workgroup's sum fits 32 bits)
    const uint32_t nReused = waveCount(reused), nRejected = waveCount(rejected);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(&sRed[0], nReused), atomicAdd(&sRed[1], nRejected), atomicAdd(&sRed[2], samples);
}

} // namespace hr
