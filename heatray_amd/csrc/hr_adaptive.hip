// hr_adaptive.hip — the kernels of adaptive sampling (include/hrcore_adaptive.h is the contract, hr_adaptive.h the per-pixel arithmetic,
// hr_adaptive.inl the entry points).  A translation unit of its own: nothing here touches the register budgets of the render stages (hr_raygen.hip, hr_trace.hip, hr_shade.hip).
//
// The sample mask lives on the device as row-major 32-bit words, (W + 31) / 32 per row, bit (x & 31) of word (x >> 5) of row y = pixel
// (x, y); bits beyond W are 0.  cameraLane (hr_raygen.hip) reads it: a wave of k_raygen covers an 8 x 8 block, eight words.
//
//   k_adaptive_error   one lane per pixel: the frame's and the MOMENTS plane's float4 (32 B, coalesced) -> the pixel's error (4 B)
//   k_adaptive_mask    a workgroup owns a tile of 64 x 16 pixels: it stages the unconverged flags of the tile and a halo of `radius`
//                      as bytes in LDS, takes the separable maximum (rows, then columns) and writes the mask one bit per pixel: a
//                      wave's 64 decisions of one row gathered with __ballot, the two words stored by lanes 0 and 32.  The counts
//                      (popcounts of the ballots, hr_post_device.h) and the largest finite error (as an ordered integer) are reduced in
//                      LDS and go to the result block with one atomic each per workgroup: integer adds and a maximum, so the result does
//                      not depend on the order workgroups finish in.
//   k_mask_pack / k_mask_unpack   the byte form of hr_sample_mask_set / _get <-> the words (the same ballot)
// No scratch, no float atomics.
#include "hr_math.h"
#include "hr_adaptive.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kAdTileW = 64, kAdTileH = 16;           // pixels of a workgroup of k_adaptive_mask: a wave is 64 pixels of a row
static constexpr int kAdHalo = HR_ADAPTIVE_MAX_RADIUS;       // the LDS tile is laid out for the largest radius
static constexpr int kAdSideW = kAdTileW + 2 * kAdHalo, kAdSideH = kAdTileH + 2 * kAdHalo;

HRD int maskWordsPerRow(int W) { return (W + 31) >> 5; }

__global__ __launch_bounds__(256) void k_adaptive_error(int n, float floor, float minSamples, const dn4 *__restrict__ frame, const dn4 *__restrict__ moments,
                                                        float *__restrict__ err)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    G(err)[i] = adError(G(frame)[i], G(moments)[i], floor, minSamples);
}

// the 64 decisions of one row segment -> its two mask words (the second only where the image reaches it)
HRD void storeMaskWords(uint32_t *words, int W, int x0, int y, unsigned long long bits, uint32_t lane)
{
    uint32_t *row = words + (size_t)y * maskWordsPerRow(W) + (x0 >> 5);
    if (lane == 0u) G(row)[0] = (uint32_t)bits;
    if (lane == 32u && x0 + 32 < W) G(row)[1] = (uint32_t)(bits >> 32);
}

// result: {unconverged pixels, active pixels, bits of the largest finite error, 0}, zeroed by the caller
__global__ __launch_bounds__(256) void k_adaptive_mask(int W, int H, int radius, float threshold, const float *__restrict__ err, uint32_t *__restrict__ words,
                                                       uint32_t *__restrict__ result)
{
    __shared__ uint8_t sU[kAdSideH * kAdSideW]; // unconverged, tile + halo
    __shared__ uint8_t sR[kAdSideH * kAdTileW]; // ... its maximum along the rows
    __shared__ uint32_t sRed[4];
    const int tilesX = (W + kAdTileW - 1) / kAdTileW; // (a one-dimensional grid: no bound on the image's height)
    const int x0 = (int)(blockIdx.x % (uint32_t)tilesX) * kAdTileW, y0 = (int)(blockIdx.x / (uint32_t)tilesX) * kAdTileH;
    wgCountersZero<4>(sRed);
    for (int e = (int)threadIdx.x; e < kAdSideH * kAdSideW; e += 256) {
        const int lx = e % kAdSideW - kAdHalo, ly = e / kAdSideW - kAdHalo; // relative to the tile
        const int gx = x0 + lx, gy = y0 + ly;
        bool u = false; // (outside the image, or further out than the radius reaches: nobody's neighbour)
        if (gx >= 0 && gx < W && gy >= 0 && gy < H && lx >= -radius && lx < kAdTileW + radius && ly >= -radius && ly < kAdTileH + radius)
            u = adUnconverged(G(err)[gy * W + gx], threshold);
        sU[e] = u ? 1 : 0;
    }
    __syncthreads();
    for (int e = (int)threadIdx.x; e < kAdSideH * kAdTileW; e += 256) {
        const int r = e / kAdTileW, x = e % kAdTileW;
        uint32_t m = 0u;
        for (int dx = -radius; dx <= radius; ++dx) m |= sU[r * kAdSideW + x + kAdHalo + dx];
        sR[e] = (uint8_t)m;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int gx = x0 + (int)lane;
    const bool inX = gx < W;
    uint32_t nUnc = 0u, nAct = 0u, maxBits = 0u;
    for (int j = 0; j < kAdTileH / 4; ++j) {
        const int ly = (int)wave * (kAdTileH / 4) + j, gy = y0 + ly; // (the same for the whole wave)
        if (gy >= H) break;
        uint32_t m = 0u;
        for (int dy = -radius; dy <= radius; ++dy) m |= sR[(ly + kAdHalo + dy) * kAdTileW + (int)lane];
        const bool on = inX && m != 0u;
        const bool unc = inX && sU[(ly + kAdHalo) * kAdSideW + (int)lane + kAdHalo] != 0;
        if (inX) {
            const uint32_t b = adFiniteBits(G(err)[gy * W + gx]);
            maxBits = b > maxBits ? b : maxBits;
        }
        const unsigned long long bits = __ballot(on);
        nAct += (uint32_t)__popcll(bits);
        nUnc += waveCount(unc);
        storeMaskWords(words, W, x0, gy, bits, lane);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)maxBits, o);
        maxBits = other > maxBits ? other : maxBits;
    }
    if (lane == 0u) { // (the counts are the wave's already: every lane holds the ballots' popcounts)
        atomicAdd(&sRed[0], nUnc), atomicAdd(&sRed[1], nAct), atomicMax(&sRed[2], maxBits);
    }
    __syncthreads();
    if (threadIdx.x == 0u) { // (32-bit words and a maximum among them: not wgCountersFlush's form)
        if (sRed[0]) atomicAdd(&result[0], sRed[0]);
        if (sRed[1]) atomicAdd(&result[1], sRed[1]);
        if (sRed[2]) atomicMax(&result[2], sRed[2]);
    }
}

// W x H bytes (non-zero = sampled) -> mask words: a wave is 64 pixels of one row, a workgroup four rows
__global__ __launch_bounds__(256) void k_mask_pack(int W, int H, const uint8_t *__restrict__ bytes, uint32_t *__restrict__ words)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t segsX = (uint32_t)(W + 63) >> 6;
    const int x0 = (int)(blockIdx.x % segsX) * 64, gx = x0 + (int)lane, gy = (int)((blockIdx.x / segsX) * 4u + wave);
    if (gy >= H) return;
    const bool on = gx < W && G(bytes)[(size_t)gy * W + gx] != 0;
    storeMaskWords(words, W, x0, gy, __ballot(on), lane);
}

__global__ __launch_bounds__(256) void k_mask_unpack(int W, int H, const uint32_t *__restrict__ words, uint8_t *__restrict__ bytes)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= W * H) return;
    const int x = i % W, y = i / W;
    G(bytes)[i] = (uint8_t)((G(words)[(size_t)y * maskWordsPerRow(W) + (x >> 5)] >> (x & 31)) & 1u);
}

size_t sampleMaskWords(int W, int H) { return (size_t)((W + 31) >> 5) * (size_t)H; }

void launchAdaptiveError(hipStream_t st, int W, int H, const float *frame, const float *moments, const hr_adaptive_params &p, float *err)
{
    const int n = W * H;
    hipLaunchKernelGGL(k_adaptive_error, dim3((n + 255) / 256), dim3(256), 0, st, n, p.floor, (float)p.min_samples, reinterpret_cast<const dn4 *>(frame),
                       reinterpret_cast<const dn4 *>(moments), err);
}

void launchAdaptiveMask(hipStream_t st, int W, int H, const float *err, const hr_adaptive_params &p, uint32_t *words, uint32_t *result)
{
    const dim3 grid(((W + kAdTileW - 1) / kAdTileW) * ((H + kAdTileH - 1) / kAdTileH));
    hipLaunchKernelGGL(k_adaptive_mask, grid, dim3(256), 0, st, W, H, p.radius, p.threshold, err, words, result);
}

void launchMaskPack(hipStream_t st, int W, int H, const uint8_t *bytes, uint32_t *words)
{
    hipLaunchKernelGGL(k_mask_pack, dim3(((W + 63) / 64) * ((H + 3) / 4)), dim3(256), 0, st, W, H, bytes, words);
}

void launchMaskUnpack(hipStream_t st, int W, int H, const uint32_t *words, uint8_t *bytes)
{
    const int n = W * H;
    hipLaunchKernelGGL(k_mask_unpack, dim3((n + 255) / 256), dim3(256), 0, st, W, H, words, bytes);
}

} // namespace hr
