// hr_motion.hip — the kernels of motion reprojection (include/hrcore_motion.h is the contract, hr_motion.h the per-pixel arithmetic,
// hr_motion.inl the entry points).  A translation unit of its own: nothing of the render's kernels is touched, and the traversal is the
// render's (traverse<false, false> of hr_trace.h, the hit rule of DESIGN.md §4).
//
//   k_motion_snapshot  one lane per triangle in prim order: the first 36 bytes of its Tri (p0, e1, e2), found through slotOfPrim, as
//                      three 16-byte loads and three 16-byte stores (48 B per triangle, the last 12 zero).
//   k_motion_trace     one lane per pixel, a wave = an 8 x 8 block of pixels, a workgroup four of them side by side (32 x 8) like
//                      k_history_merge: the pixel-centre rays of a block walk the same part of the tree.  The camera ray is made in
//                      registers, traverse keeps its deferred-child stack in LDS ([wave][kStackLDS][64], 16 KiB per workgroup), and
//                      the resolve is FUSED behind the walk, when its registers are dead, as k_query_trace<false, true> fuses the
//                      surface record: the mesh by the binary search over the first triangles, the snapshot's triangle by the
//                      host's table from mesh to snapshot offset, three 16-byte loads, TWO 16-byte stores.  The three counters are
//                      reduced per wave (ballots), then per workgroup in the FIRST WORDS OF THE STACK, which every wave has finished
//                      with behind a barrier: no LDS beyond traverse's, one integer atomic per workgroup and counter.
//   k_motion_merge     k_history_merge's shape.  Own pixel 6 x 16 B in (the two motion planes, the frame, the three AOV planes) and,
//                      where history was taken over, 4 x 16 B out; 12 gathered float4 of history, every load issued before the first
//                      decision.  Counters as k_history_merge.
//   k_motion_vectors   one lane per pixel, one float4 in, one out: a streaming kernel.
// No float atomics; no scratch beyond traverse's overflow stack.
// Bounds: a pixel index is < W * H by the `in` guard (a lane outside reads pixel 0 and writes nothing); a prim read from a HitRec is
// < nTris (traverse reports only prims it read from the committed triangles); the mesh index is < nGeoms (nGeoms >= 1 whenever there is a
// triangle to hit); a snapshot offset is first + lt with lt < the mesh's count, and the host enters `first` only for a snapshot mesh of
// exactly that count.
#include "hr_math.h"
#include "hr_kernels.h"
#include "hr_trace.h"
#include "hr_query.h"
#include "hr_motion.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kMvWaves = 4;

__global__ __launch_bounds__(256) void k_motion_snapshot(uint32_t nTris, const Tri *__restrict__ tris, const uint32_t *__restrict__ slotOfPrim, float4 *__restrict__ out)
{
    const uint32_t prim = blockIdx.x * 256u + threadIdx.x;
    if (prim >= nTris) return;
    const HR_GLOBAL Tri &tr = G(tris)[G(slotOfPrim)[prim]];
    const float4 p = tr.p, q = tr.q, r = tr.r;
    HR_GLOBAL float4 *o = G(out) + 3 * (size_t)prim;
    o[0] = p, o[1] = q, o[2] = make_float4(r.x, 0.0f, 0.0f, 0.0f);
}

// result: {surface, sky, unmatched pixels}, zeroed by the caller
__global__ __launch_bounds__(256) void k_motion_trace(MvTraceArgs a)
{
    __shared__ int stack[kMvWaves][kStackLDS][64];
    const SceneDev &S = *a.scene;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int *stackLane = &stack[wave][0][lane];
    int x, y;
    const bool in = postTilePixel(a.W, a.H, x, y);
    const float *V = (const float *)a.view;
    v3 o, d;
    mvCameraRay(V, a.aspect, a.fov, in ? x : 0, in ? y : 0, (float)a.W, (float)a.H, o, d);
    const bool valid = in && qyRayValid(o, d, __builtin_inff()); // (the screen of include/hrcore_query.h, before the walk)
    HitRec h;
    h.prim = kMissPrim, h.t = h.u = h.v = 0.0f;
    uint32_t nv = 0, nt = 0;
    if (valid) traverse<false, false>(S, o, d, 0.0f, __builtin_inff(), 0xFFFFFFFFu, stackLane, h, nv, nt);
    const bool hit = valid && h.prim != kMissPrim;
    dn4 Mv0, Mv1;
    mvMiss(Mv0, Mv1);
    bool matched = false;
    if (hit) {
        const uint32_t prim = h.prim & 0x7FFFFFFFu;
        float depth;
        const v3 Pw = mvHitPoint(o, d, h.t, v3(V[8], V[9], V[10]), depth);
        int lo = 0, hi = a.nGeoms - 1; // last mesh whose first triangle is <= prim (k_assemble's search)
        while (lo < hi) {
            const int m = (lo + hi + 1) >> 1;
            if (G(a.geoms)[m].triOffset <= prim)
                lo = m;
            else
                hi = m - 1;
        }
        const int32_t first = G(a.remap)[lo];
        matched = first >= 0;
        if (matched) {
            const HR_GLOBAL float4 *t = G(a.snap) + 3 * ((size_t)first + (size_t)(prim - G(a.geoms)[lo].triOffset));
            const float4 tp = t[0], tq = t[1], tr = t[2];
            mvMatched(v3(tp.x, tp.y, tp.z), v3(tp.w, tq.x, tq.y), v3(tq.z, tq.w, tr.x), h.u, h.v, depth, Mv0, Mv1);
        } else {
            mvUnmatched(Pw, depth, Mv0, Mv1);
        }
    }
    if (in) {
        const size_t i = (size_t)y * (size_t)a.W + (size_t)x;
        HR_GLOBAL dn4 *out = G(reinterpret_cast<dn4 *>(a.planes));
        out[i] = Mv0, out[(size_t)a.W * (size_t)a.H + i] = Mv1;
    }
    const uint32_t nSurface = waveCount(hit && matched), nSky = waveCount(in && !hit), nUnmatched = waveCount(hit && !matched);
    __syncthreads(); // (every wave's walk is over: the stack's first words serve as the workgroup's counters)
    uint32_t *sRed = reinterpret_cast<uint32_t *>(&stack[0][0][0]);
    wgCountersZero<3>(sRed);
    __syncthreads();
    if (lane == 0u) atomicAdd(&sRed[0], nSurface), atomicAdd(&sRed[1], nSky), atomicAdd(&sRed[2], nUnmatched);
    wgCountersFlush<3>(sRed, a.result);
}

// result: {reused pixels, rejected pixels, samples taken over}, zeroed by the caller
__global__ __launch_bounds__(256) void k_motion_merge(int W, int H, MvCam cam, HsParams P, const dn4 *__restrict__ mv, const dn4 *__restrict__ hist, dn4 *__restrict__ frame,
                                                      dn4 *__restrict__ albedo, dn4 *__restrict__ normalDepth, dn4 *__restrict__ moments, unsigned long long *__restrict__ result)
{
    __shared__ uint32_t sRed[3];
    wgCountersZero<3>(sRed);
    __syncthreads();
    int x, y;
    const bool in = postTilePixel(W, H, x, y);
    const size_t n = (size_t)W * (size_t)H;
    const int i = in ? y * W + x : 0; // (a lane outside the image reads pixel 0 and writes nothing)
    const dn4 Mv0 = G(mv)[i], Mv1 = G(mv)[n + i];
    dn4 F = G(frame)[i], A = G(albedo)[i], Gn = G(normalDepth)[i], M = G(moments)[i];
    const HsPlanes src(hist, n);
    float nh = 0.0f;
    const int st = mvMerge(src, cam, P, Mv0, Mv1, in ? x : 0, in ? y : 0, W, H, F, A, Gn, M, &nh);
    mergeTail(in && st == HS_REUSED, in && st == HS_REJECTED, nh, i, F, A, Gn, M, frame, albedo, normalDepth, moments, sRed);
    wgCountersFlush<3>(sRed, result);
}

__global__ __launch_bounds__(256) void k_motion_vectors(int W, int H, MvCam cam, const dn4 *__restrict__ mv, dn4 *__restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= W * H) return;
    G(out)[i] = mvVector(cam, G(mv)[i], i % W, i / W, W, H);
}

// ------------------------------------------------------------------------------------------ host
void launchMotionSnapshot(hipStream_t st, uint32_t nTris, const Tri *tris, const uint32_t *slotOfPrim, float *out)
{
    if (nTris) hipLaunchKernelGGL(k_motion_snapshot, dim3((nTris + 255u) / 256u), dim3(256), 0, st, nTris, tris, slotOfPrim, reinterpret_cast<float4 *>(out));
}

void launchMotionTrace(hipStream_t st, const MvTraceArgs &a) { hipLaunchKernelGGL(k_motion_trace, postTileGrid(a.W, a.H), dim3(256), 0, st, a); }

void launchMotionMerge(hipStream_t st, int W, int H, const MvCam &cam, const HsParams &P, const float *mv, const float *hist, float *frame, float *albedo, float *normalDepth,
                       float *moments, unsigned long long *result)
{
    hipLaunchKernelGGL(k_motion_merge, postTileGrid(W, H), dim3(256), 0, st, W, H, cam, P, reinterpret_cast<const dn4 *>(mv), reinterpret_cast<const dn4 *>(hist),
                       reinterpret_cast<dn4 *>(frame), reinterpret_cast<dn4 *>(albedo), reinterpret_cast<dn4 *>(normalDepth), reinterpret_cast<dn4 *>(moments), result);
}

void launchMotionVectors(hipStream_t st, int W, int H, const MvCam &cam, const float *mv, float *out)
{
    hipLaunchKernelGGL(k_motion_vectors, dim3((W * H + 255) / 256), dim3(256), 0, st, W, H, cam, reinterpret_cast<const dn4 *>(mv), reinterpret_cast<dn4 *>(out));
}

} // namespace hr
