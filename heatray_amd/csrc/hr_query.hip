// hr_query.hip — the kernels of ray queries (include/hrcore_query.h is the contract, hr_query.h the per-ray arithmetic, hr_query.inl
// the entry points).  A translation unit of its own: nothing of the render's kernels is touched, and the traversal is the render's
// (traverse<ANY, false> of hr_trace.h, the hit rule of DESIGN.md §4).
//
//   k_query_trace<ANY, SURF>   one ray per lane in the order given, 256-thread workgroups, the deferred-child stack in LDS as traverse
//                        expects it ([wave][kStackLDS][64], 16 KiB per workgroup).  Rays are read through the caller's byte strides.
//                        The invalid-ray screen (qyRayValid) runs BEFORE traverse: a lane with an invalid ray idles, so no input
//                        reaches the walk that the walk was not reasoned about.  hr_hit goes out as ONE 16-byte store per lane.
//                        <false, true> also writes the surface record, FUSED behind traverse, when the walk's registers are dead:
//                        TriAttr[prim] and tris[slotOfPrim[prim]] are the values k_assemble stored (nothing is transformed twice), the
//                        mesh is found by the binary search over the first triangles that k_assemble does, and the record goes out as
//                        FOUR 16-byte stores.  Fused, not a second kernel over a HitRec scratch: the compiler gives the fused kernel
//                        71 VGPRs, 656 bytes of scratch (traverse's overflow stack) and the same 16 KiB of LDS, no more than
//                        k_debug_trace (72 / 656 / 16 KiB); the split was 72 + a second kernel of 44 that reads the ray and
//                        the HitRec again ("Ray queries").
//   k_query_camera       one lane per pixel query: qyCameraRay, 24 bytes out.
//
// Counters: hits and invalid rays are summed per wave (waveSum) and sent on with ONE 64-bit atomic per wave (hits | invalid << 32) into
// one of kQySlots copies, each on a cache line of its own; a wave with nothing to report sends nothing.  No LDS beyond the stack.
// Bounds: every index is < n by the guard at the top of each kernel; a prim read from a HitRec is < nTris (traverse reports only prims it
// read from the committed triangles); the byte offsets are size_t.
#include "hr_kernels.h"
#include "hr_trace.h"
#include "hr_wave_sum.h"
#include "hr_query.h"

namespace hr {

static constexpr int kQyBlock = 256;
static constexpr int kQyWaves = kQyBlock / 64;

HRD v3 qyLoad3(const char *base, int i, int32_t stride)
{
    const HR_GLOBAL float *p = (const HR_GLOBAL float *)G(base + (size_t)i * (size_t)stride);
    return v3(p[0], p[1], p[2]);
}

// the surface record of ray i: a miss or an invalid ray is geom = -1 and every other byte 0
HRD void qyStoreSurface(const QyArgs &a, const SceneDev &S, int i, v3 ro, v3 rd, const HitRec &h, bool hit)
{
    HR_GLOBAL uint4 *out = G(reinterpret_cast<uint4 *>(a.surfaces + i));
    if (!hit) {
        out[0] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
        out[1] = out[2] = out[3] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t prim = h.prim & 0x7FFFFFFFu;
    const HR_GLOBAL TriAttr &at = G(S.attrs)[prim];
    const Tri &tr = S.tris[a.slotOfPrim ? G(a.slotOfPrim)[prim] : prim];
    const float4 tp = tr.p, tq = tr.q, trr = tr.r;
    const v3 e1(tp.w, tq.x, tq.y), e2(tq.z, tq.w, trr.x);
    const uint32_t mf = at.matflags;
    const QySurface s = qySurface((const HR_GLOBAL float *)at.n, (const HR_GLOBAL float *)at.uv, mf >> 24, e1, e2, ro, rd, h.t, h.u, h.v, (h.prim >> 31) != 0u);
    int lo = 0, hi = a.nGeoms - 1; // last mesh whose first triangle is <= prim (k_assemble's search)
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (G(a.geoms)[m].triOffset <= prim)
            lo = m;
        else
            hi = m - 1;
    }
    const QyGeom g = G(a.geoms)[lo];
    out[0] = make_uint4((uint32_t)g.id, mf & kMatMask, prim - g.triOffset, s.flags);
    out[1] = make_uint4(__float_as_uint(s.position.x), __float_as_uint(s.position.y), __float_as_uint(s.position.z), __float_as_uint(s.normal.x));
    out[2] = make_uint4(__float_as_uint(s.normal.y), __float_as_uint(s.normal.z), __float_as_uint(s.geometric.x), __float_as_uint(s.geometric.y));
    out[3] = make_uint4(__float_as_uint(s.geometric.z), __float_as_uint(s.uv[0]), __float_as_uint(s.uv[1]), 0u);
}

template <bool ANY, bool SURF> __global__ __launch_bounds__(kQyBlock) void k_query_trace(QyArgs a)
{
    __shared__ int stack[kQyWaves][kStackLDS][64];
    const SceneDev &S = *a.scene;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int *stackLane = &stack[wave][0][lane];
    const int i = blockIdx.x * kQyBlock + threadIdx.x;
    const bool live = i < a.n;
    v3 ro(0.0f), rd(0.0f);
    float tm = __builtin_inff();
    uint32_t sk = 0xFFFFFFFFu;
    bool valid = false;
    if (live) {
        ro = qyLoad3(a.origins, i, a.oStride), rd = qyLoad3(a.directions, i, a.dStride);
        if (a.tmax) tm = *(const HR_GLOBAL float *)G(a.tmax + (size_t)i * (size_t)a.tStride);
        if (a.skip) sk = (uint32_t) * (const HR_GLOBAL int32_t *)G(a.skip + (size_t)i * (size_t)a.sStride); // (a negative entry equals no prim)
        valid = qyRayValid(ro, rd, tm);
    }
    const float tmin = a.tmin > 0.0f ? a.tmin : (a.tmin < 0.0f ? S.rayEps : 0.0f); // (the slab test wants tmin >= +0)
    HitRec h;
    h.prim = kMissPrim, h.t = h.u = h.v = 0.0f;
    uint32_t nv = 0, nt = 0;
    if (valid) traverse<ANY, false>(S, ro, rd, tmin, tm, sk, stackLane, h, nv, nt);
    const bool hit = valid && h.prim != kMissPrim;
    if (live && a.hits) {
        int4 r;
        r.x = !valid ? HR_QUERY_INVALID_RAY : (ANY ? (hit ? 0 : -1) : (hit ? (int)(h.prim & 0x7FFFFFFFu) : -1));
        r.y = (!ANY && hit) ? (int)__float_as_uint(h.t) : 0, r.z = (!ANY && hit) ? (int)__float_as_uint(h.u) : 0, r.w = (!ANY && hit) ? (int)__float_as_uint(h.v) : 0;
        *(HR_GLOBAL int4 *)G(reinterpret_cast<int4 *>(a.hits + i)) = r;
    }
    if (SURF && live) qyStoreSurface(a, S, i, ro, rd, h, hit);
    const uint32_t nHit = waveSum(hit ? 1u : 0u), nInvalid = waveSum((live && !valid) ? 1u : 0u);
    if (lane == 0 && (nHit | nInvalid))
        atomicAdd(&a.counters[(size_t)(blockIdx.x & (uint32_t)(kQySlots - 1)) * kQySlotStride], (unsigned long long)nHit | ((unsigned long long)nInvalid << 32));
}

__global__ __launch_bounds__(kQyBlock) void k_query_camera(QyCamera cam, int n, const float *__restrict__ xy, float *__restrict__ rays)
{
    const int i = blockIdx.x * kQyBlock + threadIdx.x;
    if (i >= n) return;
    v3 o, d;
    qyCameraRay((const float *)cam.view, cam.fovTan, cam.aspect, cam.focus, cam.W, cam.H, G(xy)[2 * (size_t)i], G(xy)[2 * (size_t)i + 1], o, d);
    HR_GLOBAL float *r = G(rays) + 6 * (size_t)i;
    r[0] = o.x, r[1] = o.y, r[2] = o.z, r[3] = d.x, r[4] = d.y, r[5] = d.z;
}

// ------------------------------------------------------------------------------------------ host
static uint32_t qyGrid(int n) { return ((uint32_t)n + (uint32_t)kQyBlock - 1u) / (uint32_t)kQyBlock; }

void launchQueryTrace(hipStream_t st, const QyArgs &a, bool anyHit)
{
    if (a.n <= 0) return;
    const dim3 grid(qyGrid(a.n)), block(kQyBlock);
    if (anyHit)
        hipLaunchKernelGGL((k_query_trace<true, false>), grid, block, 0, st, a);
    else if (a.surfaces)
        hipLaunchKernelGGL((k_query_trace<false, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_query_trace<false, false>), grid, block, 0, st, a);
}

void launchQueryCamera(hipStream_t st, const QyCamera &cam, int n, const float *xy, float *rays)
{
    if (n > 0) hipLaunchKernelGGL(k_query_camera, dim3(qyGrid(n)), dim3(kQyBlock), 0, st, cam, n, xy, rays);
}

} // namespace hr
