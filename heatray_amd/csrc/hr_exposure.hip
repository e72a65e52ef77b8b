// hr_exposure.hip — the kernels of auto-exposure (include/hrcore_exposure.h is the contract, hr_exposure.h the arithmetic, hr_exposure.inl
// the entry points).  A translation unit of its own: nothing here touches the register budgets of the render stages (hr_raygen.hip, hr_trace.hip, hr_shade.hip).
//
// The first post-process that is a reduction and not a per-pixel map.  What makes it reproducible is that everything summed across lanes,
// waves and workgroups is an integer: the sums do not depend on the order the adds arrive in, and the one ordered pass (the reduce) is
// a scan of integers.
//
//   k_exposure_hist     wave64, 256 threads, a grid-stride loop under a capped grid: float4 loads of 1 KB per wave instruction,
//                       coalesced, four of them in flight per lane and step -> the pixel's bin or class (hr_exposure.h).  The workgroup's histogram is 256 x u32 in
//                       LDS, fed by non-returning LDS adds; the four class counters are ballots' popcounts (hr_post_device.h).  At the
//                       end every non-zero bin goes on with one 64-bit integer atomic.  The window is a row and a column test per pixel.
//   k_exposure_reduce   one workgroup, thread k holds bin k: a scan in LDS gives the counts before the bins, hr_exposure.h's exTerm every
//                       bin's share of T, lane 0 finishes (exFinish); writes the result words (the scale word among them) and the
//                       adaptation state.  The same integers as the one-lane loop (exReduce) the CPU test runs.
//   k_exposure_display  k_display's body (hr_frame.hip) behind one multiply per channel by the scale word: displayFragment unchanged.
// No scratch, no float atomics.
#include "hr_math.h"
#include "hr_exposure.h"
#include "hr_kernels.h"
#include "hr_display.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kExBlock = 256;
typedef float ExF4 __attribute__((ext_vector_type(4))); // (a pixel read as one vector: one 16-byte load, where dn4's four members may be loaded apart)
// The grid's cap, then the loop strides.  Every workgroup ends with up to 256 global atomics on the same 2 KB: at 8 workgroups per CU
// they took a third of the kernel's time on a rendered 1080p frame, so few workgroups, each with kExUnroll loads per lane in flight.
static constexpr int kExBlocksPerCU = 2, kExUnroll = 4;

// the workgroup's sum of v, in every thread (integers: the order is no concern); sBuf is free before and after
HRD unsigned long long exBlockSum(unsigned long long *sBuf, unsigned long long v)
{
    __syncthreads();
    sBuf[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = kExBlock / 2; o > 0u; o >>= 1) {
        if (threadIdx.x < o) sBuf[threadIdx.x] += sBuf[threadIdx.x + o];
        __syncthreads();
    }
    return sBuf[0];
}

__global__ __launch_bounds__(kExBlock) void k_exposure_hist(const dn4 *__restrict__ image, uint32_t n, int W, ExWindow win, unsigned long long *__restrict__ words)
{
    __shared__ uint32_t sBins[kExBins];
    __shared__ uint32_t sRed[4];
    sBins[threadIdx.x] = 0u;
    wgCountersZero<4>(sRed);
    __syncthreads();
    uint32_t nBelow = 0u, nAbove = 0u, nNonfinite = 0u, nInvalid = 0u; // the wave's: every lane holds the ballots' popcounts
    const uint32_t step = (uint32_t)(kExBlock * kExUnroll), stride = gridDim.x * step;
    for (uint32_t base = blockIdx.x * step; base < n; base += stride) { // (the same trip count in every lane: the ballots are whole waves')
        ExF4 v[kExUnroll];
        bool in[kExUnroll]; // inside the image and the window
#pragma unroll
        for (int u = 0; u < kExUnroll; ++u) { // the step's loads first: kExUnroll x 1 KB per wave in flight
            const uint32_t i = base + (uint32_t)(u * kExBlock) + threadIdx.x, at = i < n ? i : n - 1u;
            const int x = (int)(at % (uint32_t)W), y = (int)(at / (uint32_t)W);
            in[u] = i < n && x >= win.x0 && x < win.x1 && y >= win.y0 && y < win.y1;
            v[u] = G(reinterpret_cast<const ExF4 *>(image))[at]; // (unconditional, at a pixel of the image: nothing stands between the four loads)
        }
#pragma unroll
        for (int u = 0; u < kExUnroll; ++u) {
            const int cls = in[u] ? exClass(dn4{v[u].x, v[u].y, v[u].z, v[u].w}) : -1;
            if (cls >= 0 && cls < kExBins) atomicAdd(&sBins[cls], 1u);
            nBelow += waveCount(cls == kExBelow), nAbove += waveCount(cls == kExAbove);
            nNonfinite += waveCount(cls == kExNonfinite), nInvalid += waveCount(cls == kExInvalid);
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (nBelow) atomicAdd(&sRed[0], nBelow);
        if (nAbove) atomicAdd(&sRed[1], nAbove);
        if (nNonfinite) atomicAdd(&sRed[2], nNonfinite);
        if (nInvalid) atomicAdd(&sRed[3], nInvalid);
    }
    wgCountersFlush<4>(sRed, words + kExBelow); // (its barrier is the one the bins need too)
    const uint32_t mine = sBins[threadIdx.x];
    if (mine) atomicAdd(&words[threadIdx.x], (unsigned long long)mine);
}

// One workgroup, thread k holds bin k: the counts before the bins by a scan in LDS, every bin's term of T, their sum, and lane 0
// finishes.  state: {1 when there is an adaptation state, its scale's bits}
__global__ __launch_bounds__(kExBlock) void k_exposure_reduce(ExParams P, unsigned long long *__restrict__ words, uint32_t *__restrict__ state)
{
    __shared__ unsigned long long sBuf[kExBins];
    const unsigned long long h = G(words)[threadIdx.x];
    sBuf[threadIdx.x] = h;
    __syncthreads();
    for (uint32_t o = 1u; o < (uint32_t)kExBins; o <<= 1) { // the inclusive scan
        const unsigned long long before = threadIdx.x >= o ? sBuf[threadIdx.x - o] : 0ull;
        __syncthreads();
        sBuf[threadIdx.x] += before;
        __syncthreads();
    }
    const unsigned long long C = sBuf[threadIdx.x] - h, N = sBuf[kExBins - 1];
    unsigned long long lo, hi;
    exBounds(N, P, lo, hi);
    const unsigned long long T = exBlockSum(sBuf, exTerm((int)threadIdx.x, C, h, lo, hi));
    if (threadIdx.x != 0u) return;
    const bool hasState = G(state)[0] != 0u;
    const float prev = exFromBits(G(state)[1]);
    ExReduced r;
    float next = 0.0f;
    const bool has = exFinish(N, T, P, hasState, prev, r, &next);
    G(words)[kExWordScale] = exBits(r.scale), G(words)[kExWordTarget] = exBits(r.target), G(words)[kExWordLavg] = exBits(r.lavg);
    G(words)[kExWordPosition] = r.position, G(words)[kExWordCounted] = r.counted, G(words)[kExWordUsed] = r.used, G(words)[kExWordFlags] = r.flags;
    if (has) G(state)[0] = 1u, G(state)[1] = exBits(next);
}

// hr_frame.hip's k_display over the image whose rgb is multiplied by the metered scale: one thread per pixel, row-major
__global__ __launch_bounds__(kExBlock) void k_exposure_display(FrameDev fr, hr_display_params P, int format, const unsigned long long *__restrict__ words, void *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kExBlock + threadIdx.x;
    if (i >= (uint32_t)(fr.W * fr.H)) return;
    const int x = (int)(i % (uint32_t)fr.W), y = (int)(i / (uint32_t)fr.W);
    const bool owned = (((y / fr.tile) * fr.tilesX + (x / fr.tile)) % fr.world) == fr.rank;
    const float scale = exFromBits((uint32_t)G(words)[kExWordScale]);
    float4 px = reinterpret_cast<const float4 *>(fr.fb)[i];
    px.x = px.x * scale, px.y = px.y * scale, px.z = px.z * scale;
    if (format == HR_DISPLAY_HDR_RGBA32F) {
        float4 o = make_float4(0.0f, 0.0f, 0.0f, owned ? px.w : 0.0f);
        if (owned && px.w != 0.0f) {
            const float divisor = 1.0f / px.w;
            o.x = px.x * divisor, o.y = px.y * divisor, o.z = px.z * divisor;
        }
        reinterpret_cast<float4 *>(out)[i] = o;
        return;
    }
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (owned) displayFragment(px, ((float)x + 0.5f) / (float)fr.W, ((float)y + 0.5f) / (float)fr.H, P, c);
    if (format == HR_DISPLAY_RGBA32F)
        reinterpret_cast<float4 *>(out)[i] = make_float4(c[0], c[1], c[2], owned ? 1.0f : 0.0f);
    else
        reinterpret_cast<uint32_t *>(out)[i] = owned ? (toByte(c[0]) | (toByte(c[1]) << 8) | (toByte(c[2]) << 16) | 0xFF000000u) : 0u;
}

void launchExposureMeter(hipStream_t st, int numCUs, int W, int H, const float *image, const ExWindow &win, const ExParams &P, unsigned long long *words, uint32_t *state)
{
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    if (n == 0u) return;
    const uint32_t step = (uint32_t)(kExBlock * kExUnroll), want = (n + step - 1u) / step, cap = (uint32_t)(numCUs > 0 ? numCUs : 1) * (uint32_t)kExBlocksPerCU;
    hipLaunchKernelGGL(k_exposure_hist, dim3(want < cap ? want : cap), dim3(kExBlock), 0, st, reinterpret_cast<const dn4 *>(image), n, W, win, words);
    hipLaunchKernelGGL(k_exposure_reduce, dim3(1), dim3(kExBlock), 0, st, P, words, state);
}

void launchExposureDisplay(hipStream_t st, const FrameDev &fr, const hr_display_params &P, int format, const unsigned long long *words, void *out)
{
    const int n = fr.W * fr.H;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_exposure_display, dim3((n + kExBlock - 1) / kExBlock), dim3(kExBlock), 0, st, fr, P, format, words, out);
}

} // namespace hr
