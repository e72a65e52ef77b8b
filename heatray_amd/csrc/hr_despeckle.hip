// hr_despeckle.hip — the kernel of firefly suppression (include/hrcore_despeckle.h is the contract, hr_despeckle.h the per-pixel
// arithmetic, hr_despeckle.inl the entry points).  A translation unit of its own: nothing here touches another kernel's register budget.
//
//   k_despeckle   one thread per pixel, 16 x 16 pixels per workgroup (four waves), workgroups numbered row by row in a one-dimensional
//                 grid.  A thread reads its pixel of the frame and of the moments once (two coalesced 16-byte loads), classifies it and
//                 puts its luminance (dkClass: -inf for a pixel that is nobody's tap) into a 20 x 20 float tile in LDS; the first 144
//                 threads also read one pixel each of the two-pixel halo around the tile (the frame only: 16 bytes) and do the same.
//                 The halo's load has no branch around it: a thread without a halo entry, or whose entry lies outside the image,
//                 reads its own pixel again and stores -inf or nothing.  The 24 taps of dkPixel then read LDS (a row of 20 floats:
//                 the two 16-lane rows of a half wave overlap in four banks of 32, a two-way conflict on a quarter of the reads).  Both outputs
//                 are written once per pixel, the moments only when the caller gave a plane for them.
//                 The five counters: ballots, summed in LDS, one 64-bit integer atomic per workgroup and non-zero counter
//                 (hr_post_device.h), into one of 64 copies of the counters by the workgroup's index: every workgroup has valid
//                 pixels to report, and the 8100 atomics of a 1080p frame on one word took 104 us by themselves (profiles/despeckle_time.txt).
// No scratch, no float atomics.  Traffic: 32 B read + 32 B written per pixel, and the halo's 9 B per pixel, which neighbouring
// workgroups have just read.
#include "hr_math.h"
#include "hr_despeckle.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kDkTile = 16;                      // workgroup: kDkTile x kDkTile pixels, one thread each
static constexpr int kDkSide = kDkTile + 2 * kDkRadius; // 20
static constexpr int kDkEntries = kDkSide * kDkSide;    // 400
static constexpr int kDkHalo = kDkEntries - kDkTile * kDkTile; // 144: two rows of 20 below, two above, two columns of 16 on either side

#if defined(__HIP_DEVICE_COMPILE__)
#define HR_LDS __attribute__((address_space(3))) // (a plain pointer into LDS is generic to the compiler: flat loads)
#else
#define HR_LDS
#endif
struct DkTile {
    const HR_LDS float *ls;
    int x0, y0; // image coordinates of the tile entry (0, 0)
    HRD float lum(int x, int y) const { return ls[(y - y0) * kDkSide + (x - x0)]; }
};

// result: kDespeckleSlots copies of {valid, clamped, kept, starved, nonfinite pixels} (hr_kernels.h), zeroed by the caller; tilesX: workgroups per row of tiles
__global__ __launch_bounds__(256) void k_despeckle(int W, int H, int tilesX, DkParams P, const dn4 *__restrict__ frame, const dn4 *__restrict__ moments,
                                                   dn4 *__restrict__ out, dn4 *__restrict__ momentsOut, unsigned long long *__restrict__ result)
{
    __shared__ float sLum[kDkEntries];
    __shared__ uint32_t sRed[kDespeckleCounters];
    wgCountersZero<kDespeckleCounters>(sRed);
    const int tid = (int)threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const int bx = (int)(blockIdx.x % (uint32_t)tilesX), by = (int)(blockIdx.x / (uint32_t)tilesX);
    const int tx = tid & (kDkTile - 1), ty = tid / kDkTile;
    const int x = bx * kDkTile + tx, y = by * kDkTile + ty;
    const bool in = x < W && y < H;
    const int i = in ? y * W + x : 0; // (a lane outside the image reads pixel 0 and writes nothing)
    dn4 f = G(frame)[i], m = G(moments)[i];
    const int x0 = bx * kDkTile - kDkRadius, y0 = by * kDkTile - kDkRadius;
    // the halo entry of this thread, if it has one: entries 0 .. 79 are the two rows below and the two above, 80 .. 143 the columns beside
    const bool hasHalo = tid < kDkHalo;
    int hx, hy;
    if (tid < 4 * kDkSide) {
        const int row = tid / kDkSide;
        hx = tid % kDkSide, hy = row < kDkRadius ? row : row + kDkTile;
    } else {
        const int k = tid - 4 * kDkSide, col = k & 3;
        hx = col < kDkRadius ? col : col + kDkTile, hy = kDkRadius + (k >> 2);
    }
    const int gx = x0 + hx, gy = y0 + hy;
    const bool hin = hasHalo && gx >= 0 && gx < W && gy >= 0 && gy < H;
    const dn4 fh = G(frame)[hin ? gy * W + gx : i];
    float l, lh;
    dkClass(f, l);
    dkClass(fh, lh);
    sLum[(ty + kDkRadius) * kDkSide + tx + kDkRadius] = in ? l : dkNoTap();
    if (hasHalo) sLum[hy * kDkSide + hx] = hin ? lh : dkNoTap();
    __syncthreads();
    const DkTile s{(const HR_LDS float *)sLum, x0, y0};
    const int st = in ? dkPixel(s, x, y, W, H, P, f, m) : DK_EMPTY;
    if (in) {
        G(out)[i] = f;
        if (momentsOut) G(momentsOut)[i] = m;
    }
    const uint32_t nValid = waveCount(st >= DK_PASSED), nClamped = waveCount(st == DK_CLAMPED), nKept = waveCount(st == DK_KEPT),
                   nStarved = waveCount(st == DK_STARVED), nNonfinite = waveCount(st == DK_NONFINITE);
    if (lane == 0u) {
        if (nValid) atomicAdd(&sRed[0], nValid);
        if (nClamped) atomicAdd(&sRed[1], nClamped);
        if (nKept) atomicAdd(&sRed[2], nKept);
        if (nStarved) atomicAdd(&sRed[3], nStarved);
        if (nNonfinite) atomicAdd(&sRed[4], nNonfinite);
    }
    wgCountersFlush<kDespeckleCounters>(sRed, result + (blockIdx.x % (uint32_t)kDespeckleSlots) * (uint32_t)kDespeckleSlotStride);
}

static inline const dn4 *P4(const float *p) { return reinterpret_cast<const dn4 *>(p); }
static inline dn4 *P4(float *p) { return reinterpret_cast<dn4 *>(p); }

void launchDespeckle(hipStream_t st, int W, int H, const float *frame, const float *moments, const hr_despeckle_params &p, float *out, float *momentsOut,
                     unsigned long long *result)
{
    const DkParams P{p.rank, p.min_taps, p.ratio, p.sigmas, p.floor};
    const int tilesX = (W + kDkTile - 1) / kDkTile, tilesY = (H + kDkTile - 1) / kDkTile;
    hipLaunchKernelGGL(k_despeckle, dim3((uint32_t)tilesX * (uint32_t)tilesY), dim3(256), 0, st, W, H, tilesX, P, P4(frame), P4(moments), P4(out), P4(momentsOut), result);
}

} // namespace hr
