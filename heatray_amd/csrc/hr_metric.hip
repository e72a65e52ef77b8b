// hr_metric.hip — the kernel of the convergence metric (include/hrcore_metric.h is the contract, hr_metric.h the arithmetic, hr_metric.inl
// the entry points).  A translation unit of its own: nothing here touches the register budgets of the render stages.
//
// A sum of floats as an ordered reduction: a term is never added as a float.  Its 24-bit mantissa goes into the 64-bit integer bin of
// its exponent (hr_metric.h: mtBin, mtMantissa), so everything summed across lanes, waves and workgroups is an integer and the bins
// hold the exact sum whatever the arrival order; the host folds them (mtFold).
//
//   k_metric_accumulate<KIND>  wave64, 256 threads, a grid-stride loop under a capped grid (k_exposure_hist's shape): float4 loads of
//                       both images (compare: the image and the reference; estimate: the frame and the MOMENTS plane), coalesced,
//                       kMtUnroll of each in flight per lane and step -> the pixel's terms or class (hr_metric.h).  The workgroup's
//                       two sets of 256 x u64 bins are in LDS, kMtCopies lane-striped words per bin (16 KB), fed by non-returning
//                       64-bit LDS adds; the class counters are ballots' popcounts (hr_post_device.h), the largest |d| an integer
//                       maximum.  At the end the copies are summed and every non-zero bin and counter goes on with one 64-bit integer
//                       atomic.  The window is a row and a column test per pixel.
// No scratch, no float atomics.
#include "hr_math.h"
#include "hr_metric.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kMtBlock = 256;
typedef float MtF4 __attribute__((ext_vector_type(4))); // (a pixel read as one vector: one 16-byte load)
// the grid's cap and the loads in flight per lane and image, as k_exposure_hist settled them: every workgroup ends with up to 512 global
// atomics on the same 4 KB of words, so few workgroups, each with long loops
static constexpr int kMtBlocksPerCU = 2, kMtUnroll = 4;

// kMtCopies words per bin: a lane adds to copy (lane % kMtCopies), and the flush sums the copies: the same integers reach the bin.  With
// one word per bin, 64 lanes whose terms share an exponent (a flat region, a constant reference) queue on one LDS word: the flat pair
// took 51 us against 29 us for noise at 1080p; with 2 copies 33 us, with 4 and with 8 both take 28 us (profiles/metric_cost.txt).
static constexpr int kMtCopies = 4;

// a counted pixel's term -> the workgroup's bins (a zero adds nothing: it is not sent)
HRD void mtAddTerm(unsigned long long *sBins, float t)
{
    const uint32_t m = mtMantissa(t);
    if (m) atomicAdd(&sBins[mtBin(t) * (uint32_t)kMtCopies + (threadIdx.x & (uint32_t)(kMtCopies - 1))], (unsigned long long)m);
}

template <int KIND>
__global__ __launch_bounds__(kMtBlock) void k_metric_accumulate(const dn4 *__restrict__ image, const dn4 *__restrict__ other, uint32_t n, int W, MtWindow win,
                                                                 unsigned long long *__restrict__ words)
{
    __shared__ unsigned long long sBins[2 * kMtBins * kMtCopies]; // NUM, then DEN; kMtCopies words per bin, a lane adds to copy lane % kMtCopies
    __shared__ uint32_t sRed[5];                      // counted, differing, nonfinite, skipped (the words' order); the bits of max_abs
#pragma unroll
    for (int k = 0; k < 2 * kMtCopies; ++k) sBins[threadIdx.x + k * kMtBlock] = 0ull;
    wgCountersZero<5>(sRed);
    __syncthreads();
    uint32_t nCounted = 0u, nDiffering = 0u, nNonfinite = 0u, nSkipped = 0u; // the wave's: every lane holds the ballots' popcounts
    uint32_t laneMax = 0u;                                                     // this lane's
    const uint32_t step = (uint32_t)(kMtBlock * kMtUnroll), stride = gridDim.x * step;
    for (uint32_t base = blockIdx.x * step; base < n; base += stride) { // (the same trip count in every lane: the ballots are whole waves')
        MtF4 a[kMtUnroll], b[kMtUnroll];
        bool in[kMtUnroll]; // inside the image and the window
#pragma unroll
        for (int u = 0; u < kMtUnroll; ++u) { // the step's loads first: 2 x kMtUnroll x 1 KB per wave in flight
            const uint32_t i = base + (uint32_t)(u * kMtBlock) + threadIdx.x, at = i < n ? i : n - 1u;
            const int x = (int)(at % (uint32_t)W), y = (int)(at / (uint32_t)W);
            in[u] = i < n && x >= win.x0 && x < win.x1 && y >= win.y0 && y < win.y1;
            a[u] = G(reinterpret_cast<const MtF4 *>(image))[at]; // (unconditional, at a pixel of the image: nothing stands between the loads)
            b[u] = G(reinterpret_cast<const MtF4 *>(other))[at];
        }
#pragma unroll
        for (int u = 0; u < kMtUnroll; ++u) {
            const dn4 pa{a[u].x, a[u].y, a[u].z, a[u].w}, pb{b[u].x, b[u].y, b[u].z, b[u].w};
            int cls = -1;
            if (KIND == kMtCompare) {
                float x[3], y[3];
                bool differing = false;
                uint32_t maxAbs = 0u;
                if (in[u]) cls = mtCompare(pa, pb, x, y, differing, maxAbs);
                if (cls == kMtCounted) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) mtAddTerm(sBins, x[k]), mtAddTerm(sBins + kMtBins * kMtCopies, y[k]);
                    laneMax = maxAbs > laneMax ? maxAbs : laneMax;
                }
                nDiffering += waveCount(cls == kMtCounted && differing);
            } else {
                float x = 0.0f, y = 0.0f;
                if (in[u]) cls = mtEstimate(pa, pb, x, y);
                if (cls == kMtCounted) mtAddTerm(sBins, x), mtAddTerm(sBins + kMtBins * kMtCopies, y);
                nSkipped += waveCount(cls == kMtSkipped);
            }
            nCounted += waveCount(cls == kMtCounted), nNonfinite += waveCount(cls == kMtNonfinite);
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (nCounted) atomicAdd(&sRed[0], nCounted);
        if (nDiffering) atomicAdd(&sRed[1], nDiffering);
        if (nNonfinite) atomicAdd(&sRed[2], nNonfinite);
        if (nSkipped) atomicAdd(&sRed[3], nSkipped);
    }
    if (laneMax) atomicMax(&sRed[4], laneMax);
    wgCountersFlush<4>(sRed, words + kMtWordCounted); // (its barrier is the one the bins and the maximum need too)
    if (threadIdx.x == 0u && sRed[4]) atomicMax(&words[kMtWordMaxAbs], (unsigned long long)sRed[4]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        unsigned long long mine = 0ull;
#pragma unroll
        for (int k = 0; k < kMtCopies; ++k) mine += sBins[(threadIdx.x + h * kMtBlock) * kMtCopies + k];
        if (mine) atomicAdd(&words[threadIdx.x + h * kMtBlock], mine);
    }
}

void launchMetricAccumulate(hipStream_t st, int numCUs, int W, int H, int kind, const float *image, const float *other, const MtWindow &win, unsigned long long *words)
{
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    if (n == 0u) return;
    const uint32_t step = (uint32_t)(kMtBlock * kMtUnroll), want = (n + step - 1u) / step, cap = (uint32_t)(numCUs > 0 ? numCUs : 1) * (uint32_t)kMtBlocksPerCU;
    const dim3 grid(want < cap ? want : cap), block(kMtBlock);
    const dn4 *a = reinterpret_cast<const dn4 *>(image), *b = reinterpret_cast<const dn4 *>(other);
    if (kind == kMtCompare)
        hipLaunchKernelGGL(k_metric_accumulate<kMtCompare>, grid, block, 0, st, a, b, n, W, win, words);
    else
        hipLaunchKernelGGL(k_metric_accumulate<kMtEstimate>, grid, block, 0, st, a, b, n, W, win, words);
}

} // namespace hr
