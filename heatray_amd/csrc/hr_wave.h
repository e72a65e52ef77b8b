// hr_wave.h — what more than one unit of the render stages (hr_frame.hip, hr_raygen.hip, hr_trace.hip, hr_shade.hip) uses: the workgroup
// size of the plain kernels, wave- and block-level queue compaction, the queue guards, the ray record's packing and the tile shard's
// pixel order.  Device code, and ownedThreads: the launchers' side of ownedPixel (hr_frame.hip, hr_raygen.hip).
#pragma once
#include "hr_kernels.h"
#include "hr_shade.h"       // Ray, packCone
#include "hr_wave_sum.h"    // waveSum

namespace hr {

static const int kBlock = 256;

HRD uint32_t laneId() { return threadIdx.x & 63u; }

// Wave-level compaction: lanes with `want` get consecutive slots from *counter (one atomic per wave).
HRD uint32_t waveReserve(bool want, uint32_t *counter)
{
    const unsigned long long mask = __ballot(want);
    if (mask == 0ull) return 0;
    const uint32_t lane = laneId();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// Block-level compaction: one global atomic per workgroup.  Every thread of the block must call it.
// `scratch` is 2 + (blockDim/64) words of LDS.
HRD uint32_t blockReserve(bool want, uint32_t *counter, uint32_t *scratch)
{
    const uint32_t lane = laneId(), wave = threadIdx.x >> 6, nWaves = blockDim.x >> 6;
    const unsigned long long mask = __ballot(want);
    if (lane == 0) scratch[2 + wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < nWaves; ++w) {
            const uint32_t c = scratch[2 + w];
            scratch[2 + w] = tot; // exclusive prefix
            tot += c;
        }
        scratch[0] = tot ? atomicAdd(counter, tot) : 0u;
    }
    __syncthreads();
    const uint32_t slot = scratch[0] + scratch[2 + wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads(); // scratch may be reused by the next call
    return slot;
}

// ---- queue guards.  Queue capacities are upper bounds the host derives (hr_core.hip::macroStep); should one ever be wrong, the append
// that does not fit is DROPPED and the reader sees the counter clamped, and the first such event is reported to pinned host memory
// (kind of queue, step, table entry, count): the next hr_flush / hr_readback / hr_synchronize fails with HR_ERR_DEVICE naming it — instead
// of a write past the end of an arena (round 4 met one as a memory fault while the packet kernel's partial count served as a bound).
enum OverflowKind : uint32_t { OVF_CAMERA = 1, OVF_CLOSEST_IN = 2, OVF_OCCLUSION_IN = 3, OVF_CLOSEST_OUT = 4, OVF_OCCLUSION_OUT = 5, OVF_HIT_LIST = 6 };
// (inline: the library is built without relocatable device code, so every unit that calls it carries its own copy.  used: in a unit
// whose callers all report the same kind the compiler would otherwise fold the argument into its copy and change the callers.  The price
// is a fourth copy, 22 instructions nobody calls, in hr_frame.hip.)
__device__ __attribute__((noinline, used)) inline void queueOverflow(const StepTable *tbl, uint32_t kind, uint32_t seg, uint32_t count)
{
    uint32_t *h = tbl->hostOverflow;
    if (!h || __hip_atomic_load(&h[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return; // (the FIRST report stays: what follows from it — a clamped reader downstream — would only hide it)
    __hip_atomic_store(&h[1], (uint32_t)tbl->seqValue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&h[2], seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&h[3], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&h[0], kind, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
HRD uint32_t closestCap(const SegDev &sg) { return sg.qinCap < sg.hitCap ? sg.qinCap : sg.hitCap; } // (hits and the hit list are as long as the step's bound)
HRD uint32_t closestCount(const SegDev &sg) // rays of the closest-hit queue that are really there
{
    const uint32_t n = *sg.qCountIn, cap = closestCap(sg);
    return n < cap ? n : cap;
}
HRD uint32_t occlusionCount(const SegDev &sg)
{
    const uint32_t n = *sg.sCountIn;
    return n < sg.sInCap ? n : sg.sInCap;
}

HRD uint32_t packMeta(const Ray &r)
{
    return (uint32_t)(r.sequenceID & 0xFF) | ((uint32_t)(r.depth & 0xFFFF) << 8) | ((uint32_t)r.missKind << 24) | ((uint32_t)r.missIdx << 27);
}

// Bits 30-31 of the meta word are free (every reader masks its fields): bit 30 is kMetaAovFirst, set by the shading kernels of HR_AOV_SURFACE
// on a pass-through continuation of a path that has not met its first visible surface yet (a camera ray is one by its depth 0)
static const uint32_t kMetaAovFirst = 1u << 30;
HRD void storeRay(const RayQueue &q, uint32_t slot, const Ray &r, uint32_t pixel, uint32_t srcPrim, uint32_t metaBits = 0u)
{
    G(q.A)[slot] = make_float4(r.o.x, r.o.y, r.o.z, r.maxT);
    G(q.B)[slot] = make_float4(r.d.x, r.d.y, r.d.z, r.extraT);
    G(q.C)[slot] = make_float4(r.weight.x, r.weight.y, r.weight.z, __uint_as_float(pixel));
    G(q.D)[slot] = make_int4((int)(packMeta(r) | metaBits), r.sequenceIndexOffset, (int)srcPrim, (int)packCone(r.coneW, r.coneG));
}

// pixel of thread `gid` in this context's tile shard: tiles in round-robin order, 8x8-pixel blocks inside
// a tile so that one wave covers a compact screen patch
HRD bool ownedPixel(const FrameDev &fr, uint32_t gid, int &x, int &y)
{
    const uint32_t perTile = (uint32_t)(fr.tile * fr.tile);
    const uint32_t tileSlot = gid / perTile, within = gid % perTile;
    if (tileSlot >= (uint32_t)fr.nOwnedTiles) return false;
    const int tileId = fr.rank + (int)tileSlot * fr.world;
    const int tx = tileId % fr.tilesX, ty = tileId / fr.tilesX;
    const int blk = (int)(within >> 6), l = (int)(within & 63u), bpr = fr.tile >> 3;
    x = tx * fr.tile + (blk % bpr) * 8 + (l & 7);
    y = ty * fr.tile + (blk / bpr) * 8 + (l >> 3);
    return x < fr.W && y < fr.H;
}

// threads of a launch with one thread per pixel of this context's tile shard (ownedPixel's gid)
static int ownedThreads(const FrameDev &fr) { return fr.nOwnedTiles * fr.tile * fr.tile; }

} // namespace hr
