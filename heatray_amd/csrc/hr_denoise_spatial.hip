// hr_denoise_spatial.hip — the kernel of the spatial variance estimate (include/hrcore_denoise_spatial.h is the contract,
// hr_denoise_spatial.h the per-pixel arithmetic, hr_denoise_spatial.inl the entry points).  A translation unit of its own: nothing here
// touches the register budgets of hr_denoise.hip.
//
//   k_spatial_variance   one thread per pixel, 16 x 16 pixels per workgroup.  It reads the prepared planes and writes cv[1] = the colour of
//                        cv[0] with the variance after the estimate: the a-trous iterations then start from cv[1].  No word is read by
//                        one workgroup and written by another.
//                        A workgroup first votes on its own pixels' sample counts: with no spatial pixel among them it copies its cv
//                        through and is done (from `below` passes on the whole launch is this streaming copy).  Otherwise it stages its
//                        tile and a halo of 3 (22 x 22 entries) in LDS once: unit normal + depth as float4 (ds_read_b128),
//                        and lum(d), lum(a), n and cov as floats: 32 B per entry, 15488 B (a row of 22 entries: a wave's four rows of 16 lanes
//                        overlap in six banks of 32, a two-way conflict the taps' arithmetic hides).  Both tap
//                        passes of dsEstimate read LDS; both luminances are computed once per entry.
//                        The counters: ballots, summed in LDS, one 64-bit integer atomic per workgroup and counter (hr_post_device.h).
// No scratch, no float atomics.
#include "hr_math.h"
#include "hr_denoise_spatial.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kDsTile = 16;                       // workgroup: kDsTile x kDsTile pixels, one thread each
static constexpr int kDsSide = kDsTile + 2 * kDsRadius;  // 22
static constexpr int kDsEntries = kDsSide * kDsSide;     // 484

#if defined(__HIP_DEVICE_COMPILE__)
#define HR_LDS __attribute__((address_space(3))) // (a plain pointer into LDS is generic to the compiler: flat loads)
#else
#define HR_LDS
#endif
struct DsTile {
    const HR_LDS dn4 *nds;
    const HR_LDS float *ls, *las, *ns, *covs;
    int x0, y0; // image coordinates of the tile entry (0, 0)
    HRD int at(int x, int y) const { return (y - y0) * kDsSide + (x - x0); }
    HRD dn4 nd(int x, int y) const { return nds[at(x, y)]; }
    HRD float lum(int x, int y) const { return ls[at(x, y)]; }
    HRD float alum(int x, int y) const { return las[at(x, y)]; }
    HRD float n(int x, int y) const { return ns[at(x, y)]; }
    HRD float cov(int x, int y) const { return covs[at(x, y)]; }
};

// result: {spatial pixels, estimated pixels, starved pixels}, zeroed by the caller
__global__ __launch_bounds__(256) void k_spatial_variance(int W, int H, DsParams P, const dn4 *__restrict__ frame, const dn4 *__restrict__ cvIn, const dn4 *__restrict__ nd,
                                                          const dn4 *__restrict__ ac, const float *__restrict__ grad, dn4 *__restrict__ cvOut,
                                                          unsigned long long *__restrict__ result)
{
    __shared__ dn4 sNd[kDsEntries];
    __shared__ float sLum[kDsEntries];
    __shared__ float sAlum[kDsEntries];
    __shared__ float sN[kDsEntries];
    __shared__ float sCov[kDsEntries];
    __shared__ uint32_t sRed[4]; // spatial, estimated, starved pixels of the workgroup; [3]: does it have a spatial pixel at all
    wgCountersZero<4>(sRed);
    const uint32_t lane = threadIdx.x & 63u;
    const int x = (int)(blockIdx.x * kDsTile + (threadIdx.x & (kDsTile - 1))), y = (int)(blockIdx.y * kDsTile + threadIdx.x / kDsTile);
    const bool in = x < W && y < H;
    const int i = in ? y * W + x : 0; // (a lane outside the image reads pixel 0 and writes nothing)
    const float n = G(frame)[i].w;
    const dn4 c = G(cvIn)[i];
    const bool spatial = in && n > 0.0f && dsSpatial(n, P);
    __syncthreads();
    const uint32_t nSpatial = waveCount(spatial);
    if (lane == 0u && nSpatial) atomicAdd(&sRed[0], nSpatial), sRed[3] = 1u;
    __syncthreads();
    if (sRed[3] == 0u) { // (the same word for every lane of the workgroup: nobody waits at a barrier below)
        if (in) G(cvOut)[i] = c;
        return;
    }
    const int x0 = (int)(blockIdx.x * kDsTile) - kDsRadius, y0 = (int)(blockIdx.y * kDsTile) - kDsRadius;
    for (int e = (int)threadIdx.x; e < kDsEntries; e += 256) {
        const int gx = x0 + e % kDsSide, gy = y0 + e / kDsSide;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float l = 0.0f, la = 0.0f, nq = 0.0f, cov = -1.0f; // (outside the image: nobody's tap; dsEstimate does not ask for it anyway)
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const int q = gy * W + gx;
            const float4 d = G(reinterpret_cast<const float4 *>(cvIn))[q];
            const dn4 a = G(ac)[q];
            g = G(reinterpret_cast<const float4 *>(nd))[q], cov = a.w, nq = G(frame)[q].w;
            l = dnLum(d.x, d.y, d.z), la = dnLum(a.x, a.y, a.z);
        }
        reinterpret_cast<float4 *>(sNd)[e] = g, sLum[e] = l, sAlum[e] = la, sN[e] = nq, sCov[e] = cov;
    }
    __syncthreads();
    int st = DS_KEPT;
    float v = c.w; // (c itself stays as loaded: a dn4 changed in one field is copied through a private array, which the compiler puts in LDS)
    if (spatial) {
        const DsTile s{(const HR_LDS dn4 *)sNd, (const HR_LDS float *)sLum, (const HR_LDS float *)sAlum, (const HR_LDS float *)sN, (const HR_LDS float *)sCov, x0, y0};
        const DsResult r = dsEstimate(s, x, y, W, H, P, G(grad)[i], v);
        st = r.status, v = r.v;
    }
    if (in) G(cvOut)[i] = dn4{c.x, c.y, c.z, v};
    const uint32_t nEstimated = waveCount(st == DS_ESTIMATED), nStarved = waveCount(st == DS_STARVED);
    if (lane == 0u) atomicAdd(&sRed[1], nEstimated), atomicAdd(&sRed[2], nStarved);
    wgCountersFlush<3>(sRed, result); // (sRed[3] is the vote, no counter)
}

static inline const dn4 *P4(const float *p) { return reinterpret_cast<const dn4 *>(p); }

void launchDenoiseSpatial(hipStream_t st, int W, int H, const float *frame, const DenoiseBufs &b, const hr_denoise_params &p, const hr_denoise_spatial_params &sp,
                          unsigned long long *result)
{
    const DsParams P{sp.below, sp.min_taps, p.normal_power, p.sigma_z};
    const dim3 grid((W + kDsTile - 1) / kDsTile, (H + kDsTile - 1) / kDsTile);
    hipLaunchKernelGGL(k_spatial_variance, grid, dim3(256), 0, st, W, H, P, P4(frame), P4(b.cv[0]), P4(b.nd), P4(b.ac), b.grad, reinterpret_cast<dn4 *>(b.cv[1]), result);
}

} // namespace hr
