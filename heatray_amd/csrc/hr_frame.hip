// hr_frame.hip — the kernels of a macro step that are not a stage of a path: the injected passes' counters back to zero, the step table's
// way to the device, the resolve of finished passes into the frame (with and without AOVs), the shard exchange of context groups, display.
#include "hr_kernels.h"
#include "hr_display.h"
#include "hr_shade.h"
#include "hr_trace.h"
#include "hr_packet_interval.h"
#include "hr_wave.h"

namespace hr {

// one workgroup per injected pass: its Counters block (a few hundred words) back to zero
__global__ __launch_bounds__(256) void k_zero_counters(CounterList list)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(list.ctr[blockIdx.x]);
    for (uint32_t i = threadIdx.x; i < sizeof(Counters) / 4; i += 256) w[i] = 0u;
}
// The step table comes to the device by a kernel that reads its pinned host entry (hr_core.hip: Group::hTables), 16 bytes per thread
__global__ __launch_bounds__(256) void k_fetch_table(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}
void launchFetchTable(hipStream_t stream, const void *hostMapped, void *dst, size_t bytes)
{
    const uint32_t n16 = (uint32_t)((bytes + 15) / 16);
    hipLaunchKernelGGL(k_fetch_table, dim3((n16 + 255u) / 256u), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(hostMapped), reinterpret_cast<uint4 *>(dst), n16);
}
void launchZeroCounters(const LaunchCfg &cfg, const CounterList &list)
{
    if (list.n > 0) hipLaunchKernelGGL(k_zero_counters, dim3(list.n), dim3(256), 0, cfg.stream, list);
}

// ------------------------------------------------------------------------------------------ resolve
// The finished passes' samples are added one after the other, in pass order (float addition order is part of the contract)
__global__ __launch_bounds__(kBlock) void k_resolve(FrameDev fr, PassBufList bufs)
{
    int x = 0, y = 0;
    if (!ownedPixel(fr, blockIdx.x * kBlock + threadIdx.x, x, y)) return;
    const uint32_t pixel = (uint32_t)(y * fr.W + x);
    float4 a = reinterpret_cast<float4 *>(fr.fb)[pixel];
    for (int k = 0; k < bufs.n; ++k) {
        float4 s = reinterpret_cast<const float4 *>(bufs.buf[k])[pixel];
        if (bufs.bufB[k]) { // HR_ESTIMATOR_ALL_LIGHTS: the pass's four partial sums meet here, in order, then the sample joins the frame
            const size_t framePixels = (size_t)(bufs.bufB[k] - bufs.buf[k]) >> 2;
            for (int j = 1; j <= 3; ++j) {
                const float4 t = reinterpret_cast<const float4 *>(bufs.buf[k])[pixel + j * framePixels];
                s.x = s.x + t.x, s.y = s.y + t.y, s.z = s.z + t.z;
            }
        }
        a.x = a.x + s.x, a.y = a.y + s.y, a.z = a.z + s.z, a.w = a.w + s.w;
    }
    reinterpret_cast<float4 *>(fr.fb)[pixel] = a;
}

// The same with AOVs enabled (include/hrcore_aov.h): every pass is also folded into the frame's AOV planes, in the same order, and its
// own AOV planes are zeroed for the slot's next pass (so ray generation never clears them).  k_resolve stays the kernel without AOVs.
__global__ __launch_bounds__(kBlock) void k_resolve_aov(FrameDev fr, PassBufList bufs, AovList aov)
{
    int x = 0, y = 0;
    if (!ownedPixel(fr, blockIdx.x * kBlock + threadIdx.x, x, y)) return;
    const uint32_t pixel = (uint32_t)(y * fr.W + x);
    float4 a = reinterpret_cast<float4 *>(fr.fb)[pixel];
    float4 m = aov.moments ? reinterpret_cast<float4 *>(aov.moments)[pixel] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 al = aov.albedo ? reinterpret_cast<float4 *>(aov.albedo)[pixel] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 nd = aov.normalDepth ? reinterpret_cast<float4 *>(aov.normalDepth)[pixel] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < bufs.n; ++k) {
        float4 s = reinterpret_cast<const float4 *>(bufs.buf[k])[pixel];
        if (bufs.bufB[k]) {
            const size_t pixelsB = (size_t)(bufs.bufB[k] - bufs.buf[k]) >> 2;
            for (int j = 1; j <= 3; ++j) {
                const float4 t = reinterpret_cast<const float4 *>(bufs.buf[k])[pixel + j * pixelsB];
                s.x = s.x + t.x, s.y = s.y + t.y, s.z = s.z + t.z;
            }
        }
        a.x = a.x + s.x, a.y = a.y + s.y, a.z = a.z + s.z, a.w = a.w + s.w;
        const float sx = s.x * s.x, sy = s.y * s.y, sz = s.z * s.z; // (-ffp-contract=off: rounded, then added)
        m.x = m.x + sx, m.y = m.y + sy, m.z = m.z + sz, m.w = m.w + s.w;
        if (aov.pass[k]) { // (a pass's planes are interleaved: albedo and normal-depth of a pixel are 32 consecutive bytes)
            float4 *p = reinterpret_cast<float4 *>(aov.pass[k]) + 2 * (size_t)pixel;
            const float4 pa = p[0], pn = p[1];
            al.x = al.x + pa.x, al.y = al.y + pa.y, al.z = al.z + pa.z, al.w = al.w + pa.w;
            nd.x = nd.x + pn.x, nd.y = nd.y + pn.y, nd.z = nd.z + pn.z, nd.w = nd.w + pn.w;
            p[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            p[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    reinterpret_cast<float4 *>(fr.fb)[pixel] = a;
    if (aov.moments) reinterpret_cast<float4 *>(aov.moments)[pixel] = m;
    if (aov.albedo) reinterpret_cast<float4 *>(aov.albedo)[pixel] = al;
    if (aov.normalDepth) reinterpret_cast<float4 *>(aov.normalDepth)[pixel] = nd;
}

// ----------------------------------------------------------------------------------- shard exchange
// dense copy of a rank's pixels, in ownedPixel order (coalesced 8x8 blocks); `unpack` is the inverse into a full frame
__global__ __launch_bounds__(kBlock) void k_pack_owned(FrameDev fr, const float4 *__restrict__ frame, float4 *__restrict__ packed, int unpack,
                                                       float4 *__restrict__ full)
{
    const uint32_t gid = blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (uint32_t)(fr.nOwnedTiles * fr.tile * fr.tile)) return;
    int x = 0, y = 0;
    const bool in = ownedPixel(fr, gid, x, y);
    const uint32_t pixel = (uint32_t)(y * fr.W + x);
    if (unpack) {
        if (in) full[pixel] = packed[gid];
    } else {
        packed[gid] = in ? frame[pixel] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

void launchPackOwned(const LaunchCfg &cfg, const FrameDev &fr, const float *frame, float *packed, int unpack, float *full)
{
    const int threads = fr.nOwnedTiles * fr.tile * fr.tile;
    if (threads <= 0) return;
    hipLaunchKernelGGL(k_pack_owned, dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, cfg.stream, fr, reinterpret_cast<const float4 *>(frame),
                       reinterpret_cast<float4 *>(packed), unpack, reinterpret_cast<float4 *>(full));
}

// Context groups: every member's packed tiles -> the full frame on the group's first device, in one launch.  The member of a workgroup
// is found by comparing its index with the members' first workgroups — unrolled over constant indices, so the list stays in the
// kernel-argument segment (scalar loads) instead of being copied to scratch for a dynamic index.  A wave reads 64 consecutive
// 16-byte slots and writes one 8x8-pixel block (8 rows of 128 contiguous bytes), as k_pack_owned does the other way round.
// Copies only: the assembled frame is the members' bits.
__global__ __launch_bounds__(kBlock) void k_gather_members(FrameDev fr, GatherList list, float4 *__restrict__ full)
{
    const uint32_t b = blockIdx.x;
    int m = 0;
    uint32_t first = 0;
    const float *src = list.packed[0];
#pragma unroll
    for (int k = 1; k < HR_GROUP_MAX_MEMBERS; ++k)
        if (k < list.n && b >= list.blockStart[k]) m = k, first = list.blockStart[k], src = list.packed[k];
    const int nTiles = fr.tilesX * fr.tilesY;
    fr.rank = m, fr.world = list.n;
    fr.nOwnedTiles = nTiles > m ? (nTiles - m + list.n - 1) / list.n : 0;
    const uint32_t gid = (b - first) * kBlock + threadIdx.x;
    int x = 0, y = 0;
    if (!ownedPixel(fr, gid, x, y)) return; // past the member's slots (padding) or outside a cropped edge tile
    full[(uint32_t)(y * fr.W + x)] = reinterpret_cast<const float4 *>(src)[gid];
}

int gatherBlock() { return kBlock; }

void launchGatherMembers(const LaunchCfg &cfg, const FrameDev &fr, const GatherList &list, float *full)
{
    if (list.n <= 0 || list.n > HR_GROUP_MAX_MEMBERS || list.blockStart[list.n] == 0u) return;
    hipLaunchKernelGGL(k_gather_members, dim3(list.blockStart[list.n]), dim3(kBlock), 0, cfg.stream, fr, list, reinterpret_cast<float4 *>(full));
}

// ------------------------------------------------------------------------------------------ display
// displayGL.frag on the accumulation buffer: one thread per pixel, row-major (coalesced 16-byte reads, 4- or 16-byte writes)
__global__ __launch_bounds__(kBlock) void k_display(FrameDev fr, hr_display_params P, int format, void *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)(fr.W * fr.H)) return;
    const int x = (int)(i % (uint32_t)fr.W), y = (int)(i / (uint32_t)fr.W);
    const bool owned = (((y / fr.tile) * fr.tilesX + (x / fr.tile)) % fr.world) == fr.rank;
    const float4 px = reinterpret_cast<const float4 *>(fr.fb)[i];
    if (format == HR_DISPLAY_HDR_RGBA32F) { // saveScreenshot's HDR path (HeatrayRenderer.cpp:1633-1645)
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

void launchResolve(const LaunchCfg &cfg, const FrameDev &fr, const PassBufList &bufs)
{
    const int threads = ownedThreads(fr);
    if (threads <= 0 || bufs.n <= 0) return;
    hipLaunchKernelGGL(k_resolve, dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, cfg.stream, fr, bufs);
}

void launchResolveAov(const LaunchCfg &cfg, const FrameDev &fr, const PassBufList &bufs, const AovList &aov)
{
    const int threads = ownedThreads(fr);
    if (threads <= 0 || bufs.n <= 0) return;
    hipLaunchKernelGGL(k_resolve_aov, dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, cfg.stream, fr, bufs, aov);
}

void launchDisplay(const LaunchCfg &cfg, const FrameDev &fr, const hr_display_params &P, int format, void *out)
{
    const int n = fr.W * fr.H;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_display, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, cfg.stream, fr, P, format, out);
}

} // namespace hr
