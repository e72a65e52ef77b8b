// hr_history.hip — the kernels of history reprojection (include/hrcore_history.h is the contract, hr_history.h the per-pixel arithmetic,
// hr_history.inl the entry points).  A translation unit of its own: nothing here touches the register budgets of the render stages (hr_raygen.hip, hr_trace.hip, hr_shade.hip).
//
// The history lives on the device as three planes of W x H float4 one after the other: H0, H1, H2.
//
//   k_history_capture  one lane per pixel: the frame's and the three planes' float4 in (64 B, coalesced), three float4 out (48 B): a
//                      streaming kernel
//   k_history_merge    one lane per pixel, a wave = an 8 x 8 block of pixels, a workgroup four of them side by side (32 x 8): a row of a
//                      wave's own pixels is one 128-byte line per plane, and the wave's four-tap footprints (which a camera change
//                      moves together) overlap in a handful of lines.  Own pixel 4 x 16 B in and, where history was taken over,
//                      4 x 16 B out; 12 gathered float4 of history, every load issued before the first decision.  The counters: the
//                      wave's ballots and a shuffle sum of the samples taken over, reduced in LDS (hr_post_device.h), one integer
//                      atomic per workgroup and counter: the result does not depend on the order workgroups finish in.
// No scratch, no float atomics.
#include "hr_math.h"
#include "hr_history.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

__global__ __launch_bounds__(256) void k_history_capture(int n, const dn4 *__restrict__ frame, const dn4 *__restrict__ albedo, const dn4 *__restrict__ normalDepth,
                                                         const dn4 *__restrict__ moments, dn4 *__restrict__ hist)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    dn4 H0, H1, H2;
    hsCapture(G(frame)[i], G(albedo)[i], G(normalDepth)[i], G(moments)[i], H0, H1, H2);
    G(hist)[i] = H0, G(hist)[(size_t)n + i] = H1, G(hist)[2 * (size_t)n + i] = H2;
}

// result: {reused pixels, rejected pixels, samples taken over}, zeroed by the caller
__global__ __launch_bounds__(256) void k_history_merge(int W, int H, HsCam cam, HsParams P, const dn4 *__restrict__ hist, dn4 *__restrict__ frame, dn4 *__restrict__ albedo,
                                                       dn4 *__restrict__ normalDepth, dn4 *__restrict__ moments, unsigned long long *__restrict__ result)
{
    __shared__ uint32_t sRed[3];
    wgCountersZero<3>(sRed);
    __syncthreads();
    int x, y;
    const bool in = postTilePixel(W, H, x, y);
    const int i = in ? y * W + x : 0; // (a lane outside the image reads pixel 0 and writes nothing)
    dn4 F = G(frame)[i], A = G(albedo)[i], Gn = G(normalDepth)[i], M = G(moments)[i];
    const HsPlanes src(hist, (size_t)W * (size_t)H);
    float nh = 0.0f;
    const int st = hsMerge(src, cam, P, in ? x : 0, in ? y : 0, W, H, F, A, Gn, M, &nh);
    mergeTail(in && st == HS_REUSED, in && st == HS_REJECTED, nh, i, F, A, Gn, M, frame, albedo, normalDepth, moments, sRed);
    wgCountersFlush<3>(sRed, result);
}

void launchHistoryCapture(hipStream_t st, int W, int H, const float *frame, const float *albedo, const float *normalDepth, const float *moments, float *hist)
{
    const int n = W * H;
    hipLaunchKernelGGL(k_history_capture, dim3((n + 255) / 256), dim3(256), 0, st, n, reinterpret_cast<const dn4 *>(frame), reinterpret_cast<const dn4 *>(albedo),
                       reinterpret_cast<const dn4 *>(normalDepth), reinterpret_cast<const dn4 *>(moments), reinterpret_cast<dn4 *>(hist));
}

void launchHistoryMerge(hipStream_t st, int W, int H, const HsCam &cam, const HsParams &P, const float *hist, float *frame, float *albedo, float *normalDepth, float *moments,
                        unsigned long long *result)
{
    hipLaunchKernelGGL(k_history_merge, postTileGrid(W, H), dim3(256), 0, st, W, H, cam, P, reinterpret_cast<const dn4 *>(hist), reinterpret_cast<dn4 *>(frame),
                       reinterpret_cast<dn4 *>(albedo), reinterpret_cast<dn4 *>(normalDepth), reinterpret_cast<dn4 *>(moments), result);
}

} // namespace hr
