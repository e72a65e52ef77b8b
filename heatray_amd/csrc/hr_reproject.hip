// hr_reproject.hip — the kernels of the progressive history merge and the preview (include/hrcore_reproject.h is the contract,
// hr_reproject.h the per-pixel arithmetic, hr_reproject.inl the entry points).  A translation unit of its own: nothing here touches the
// register budgets of hr_history.hip or the render stages (hr_raygen.hip, hr_trace.hip, hr_shade.hip).
//
//   k_reproject_merge    k_history_merge's shape: one lane per pixel, a wave = an 8 x 8 block of pixels, a workgroup four of them side by
//                        side (32 x 8).  The examined bits are one 64-bit word per 8 x 8 block, bit = the lane: a wave reads its word
//                        with one load, and one lane writes it back from a __ballot.  A wave without a pixel to examine (every sampled
//                        pixel of its block examined already, or none sampled yet) leaves before any plane or history load: that branch
//                        is wave-uniform.  Otherwise hsMerge: all twelve history loads at clamped addresses before the first decision.
//   k_reproject_preview  a workgroup stages the guide records (rpGuide: class, unit normal, mean depth) of its 32 x 8 tile and a halo of
//                        2 in LDS, 36 x 12 entries, each normalised and divided once; an unsampled lane walks the 24 offsets there
//                        and stops at the first hit; the four taps' H0 and H2, eight float4, are issued together.  A wave whose pixels
//                        all have samples writes their means and reads no history.
// The counters of both (hr_post_device.h): ballots (and a shuffle sum of the samples taken over), reduced in LDS, one integer atomic per
// workgroup and counter: a result does not depend on the order workgroups finish in.  No scratch, no float atomics, plain vector stores.
#include "hr_math.h"
#include "hr_reproject.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kRpHaloW = kPostTileW + 2 * RP_GUIDE_REACH, kRpHaloH = kPostTileH + 2 * RP_GUIDE_REACH; // 36 x 12 staged guide records

// result: {reused pixels, rejected pixels, samples taken over, pending pixels, examined pixels}, zeroed by the caller
__global__ __launch_bounds__(256) void k_reproject_merge(int W, int H, HsCam cam, HsParams P, const dn4 *__restrict__ hist, dn4 *__restrict__ frame, dn4 *__restrict__ albedo,
                                                         dn4 *__restrict__ normalDepth, dn4 *__restrict__ moments, unsigned long long *__restrict__ examined,
                                                         unsigned long long *__restrict__ result)
{
    __shared__ uint32_t sRed[5];
    wgCountersZero<5>(sRed);
    __syncthreads();
    const uint32_t blocksX = (uint32_t)(W + 7) / 8u;
    const uint32_t lane = threadIdx.x & 63u;
    int x, y;
    const bool in = postTilePixel(W, H, x, y);
    const uint32_t blockX = (uint32_t)x >> 3, blockY = (uint32_t)y >> 3; // the wave's 8 x 8 block
    const int i = in ? y * W + x : 0; // (a lane outside the image reads pixel 0 and writes nothing)
    const bool hasWord = blockX < blocksX; // (the last workgroup of a row may hold waves that lie outside the image altogether)
    const size_t wordAt = (size_t)blockY * blocksX + blockX;
    const unsigned long long word = hasWord ? G(examined)[wordAt] : 0ull;
    dn4 F = G(frame)[i];
    const bool todo = in && !((word >> lane) & 1ull) && F.w > 0.0f;
    const unsigned long long todoMask = __ballot(todo);
    if (todoMask) { // wave-uniform
        dn4 A = G(albedo)[i], Gn = G(normalDepth)[i], M = G(moments)[i];
        const HsPlanes src(hist, (size_t)W * (size_t)H);
        float nh = 0.0f;
        const int st = hsMerge(src, cam, P, in ? x : 0, in ? y : 0, W, H, F, A, Gn, M, &nh);
        mergeTail(todo && st == HS_REUSED, todo && st == HS_REJECTED, nh, i, F, A, Gn, M, frame, albedo, normalDepth, moments, sRed);
        if (lane == 0u) G(examined)[wordAt] = word | todoMask; // (todoMask != 0 implies hasWord)
    }
    const unsigned long long now = word | todoMask;
    const uint32_t nExamined = (uint32_t)__popcll(now), nPending = (uint32_t)__popcll(__ballot(in) & ~now); // (bit masks in hand: no waveCount)
    if (lane == 0u) atomicAdd(&sRed[3], nPending), atomicAdd(&sRed[4], nExamined);
    wgCountersFlush<5>(sRed, result);
}

// the workgroup's staged guide records behind rpFindGuide's source
struct RpTileGuides {
    const dn4 *rec_;
    const unsigned char *cls_;
    int x0, y0; // the image position of entry (0, 0)
    HRD int at(int gx, int gy) const { return (gy - y0) * kRpHaloW + (gx - x0); }
    HRD int cls(int gx, int gy) const { return (int)cls_[at(gx, gy)]; }
    HRD dn4 rec(int gx, int gy) const { return rec_[at(gx, gy)]; }
};

// result: {own pixels, previewed pixels, empty pixels}, zeroed by the caller
__global__ __launch_bounds__(256) void k_reproject_preview(int W, int H, HsCam cam, HsParams P, const dn4 *__restrict__ hist, const dn4 *__restrict__ frame,
                                                           const dn4 *__restrict__ albedo, const dn4 *__restrict__ normalDepth, dn4 *__restrict__ out,
                                                           unsigned long long *__restrict__ result)
{
    __shared__ dn4 sRec[kRpHaloW * kRpHaloH];
    __shared__ unsigned char sCls[kRpHaloW * kRpHaloH];
    __shared__ uint32_t sRed[3];
    wgCountersZero<3>(sRed); // (the barrier behind the staging loop comes before the first add)
    int tx0, ty0;
    postTileOrigin(W, tx0, ty0);
    for (int e = (int)threadIdx.x; e < kRpHaloW * kRpHaloH; e += 256) {
        const int gx = tx0 - RP_GUIDE_REACH + e % kRpHaloW, gy = ty0 - RP_GUIDE_REACH + e / kRpHaloW;
        const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const int gi = inside ? gy * W + gx : 0;
        const dn4 Fg = G(frame)[gi], A = G(albedo)[gi], Gn = G(normalDepth)[gi];
        dn4 rec;
        const int cls = rpGuide(inside ? Fg.w : 0.0f, A, Gn, rec);
        sRec[e] = rec, sCls[e] = (unsigned char)cls;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    int x, y;
    const bool in = postTilePixel(W, H, x, y);
    const int i = in ? y * W + x : 0;
    const dn4 F = G(frame)[i];
    const bool own = in && F.w > 0.0f, needs = in && !own;
    dn4 px = own ? rpOwn(F) : dn4{0.0f, 0.0f, 0.0f, 0.0f};
    bool previewed = false;
    if (__ballot(needs)) { // wave-uniform: a wave whose pixels all have samples reads no history
        const RpTileGuides guides{sRec, sCls, tx0 - RP_GUIDE_REACH, ty0 - RP_GUIDE_REACH};
        int gx = 0, gy = 0, cls = RP_GUIDE_NONE;
        dn4 rec{0.0f, 0.0f, 0.0f, 0.0f};
        if (needs) cls = rpFindGuide(guides, x, y, W, H, gx, gy, rec);
        const HsPlanes src(hist, (size_t)W * (size_t)H);
        dn4 pv;
        const int st = rpPreviewFromGuide(src, cam, P, in ? x : 0, in ? y : 0, W, H, cls, gx, gy, rec, pv);
        previewed = needs && st == RP_PREVIEWED;
        if (previewed) px = pv;
    }
    if (in) G(out)[i] = px;
    const uint32_t nOwn = waveCount(own), nPrev = waveCount(previewed), nEmpty = waveCount(needs && !previewed);
    if (lane == 0u) {
        if (nOwn) atomicAdd(&sRed[0], nOwn);
        if (nPrev) atomicAdd(&sRed[1], nPrev);
        if (nEmpty) atomicAdd(&sRed[2], nEmpty);
    }
    wgCountersFlush<3>(sRed, result);
}

void launchReprojectMerge(hipStream_t st, int W, int H, const HsCam &cam, const HsParams &P, const float *hist, float *frame, float *albedo, float *normalDepth, float *moments,
                          unsigned long long *examined, unsigned long long *result)
{
    hipLaunchKernelGGL(k_reproject_merge, postTileGrid(W, H), dim3(256), 0, st, W, H, cam, P, reinterpret_cast<const dn4 *>(hist), reinterpret_cast<dn4 *>(frame),
                       reinterpret_cast<dn4 *>(albedo), reinterpret_cast<dn4 *>(normalDepth), reinterpret_cast<dn4 *>(moments), examined, result);
}

void launchReprojectPreview(hipStream_t st, int W, int H, const HsCam &cam, const HsParams &P, const float *hist, const float *frame, const float *albedo,
                            const float *normalDepth, float *out, unsigned long long *result)
{
    hipLaunchKernelGGL(k_reproject_preview, postTileGrid(W, H), dim3(256), 0, st, W, H, cam, P, reinterpret_cast<const dn4 *>(hist), reinterpret_cast<const dn4 *>(frame),
                       reinterpret_cast<const dn4 *>(albedo), reinterpret_cast<const dn4 *>(normalDepth), reinterpret_cast<dn4 *>(out), result);
}

} // namespace hr
